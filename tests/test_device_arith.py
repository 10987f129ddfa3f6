"""Device self-test of the arithmetic every kernel is built from, on edge
operands (tpst_selftest_field / tpst_selftest_curve, csrc/selftest.hip):

  field.h   Fq / Fr  mul, sqr (the device-only product scanning with its
            p_0 = 1 shortcut: the lo == 0 arm is taken once per 2^32 columns
            on random data), add, sub, neg, to_mont, from_mont;
  field29.h the ceil-carry products mul / sqr / mul_sum / mul_sub, add, sub,
            cneg, p_minus, to_std's quotient estimate, from_std, pack377 /
            unpack377 (alignbit on the device);
  Fq2       the lane product and square, and pair_fq2.h's product / is_zero / eq;
  curve.h   add_affine, add, dbl, dbl_affine, sub_affine, to_affine on Xyzz<Fq>,
            Xyzz<Fq29> (load_acc / store_acc and the packed load_pk / store_pk),
            Xyzz<Fq2>, Xyzz<Fq2x29> (acc_field.h, the G2 tail kernels' field),
            the Fq2P pair form of the G2 accumulation;
  coop.h    the 4-lane add_affine_quad / add_quad / dbl_quad of the MSM tail
            and the fixed-base tables, on Xyzz<Fq29> (both codecs) and
            Xyzz<Fq2x29>, with their own P == Q and P == -Q branches;
  glv.h     glv_split.

Every comparison is exact equality against Python integers; the operands and
expectations are tests/arith_vectors.py's, which tests/test_selftest_ops.py
proves on the host.  Constructed classes (reduction word m_k == 0, P == Q in
a scaled representation, ...) assert their defining property where they are
built, from integers alone, before the device is called."""
import numpy as np
import pytest

import arith_vectors as V
from testudo_amd import engine as E
from testudo_amd.engine import TpstError

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("family", ["fq", "fr", "fq29", "fq2", "fq2p"])
def test_field_ops(ctx, family):
    for c in V.field_cases()[family]:
        got = ctx.selftest_field(c.op, c.a, c.b)
        bad = np.nonzero((got != c.exp).any(axis=1))[0]
        assert not len(bad), (c.name, len(bad), [hex(v) for v in c.inputs[bad[0]]],
                              [hex(int(w)) for w in got[bad[0]]])


def test_to_std_agrees_with_its_product_form(ctx):
    """to_std (floating-point quotient estimate) against to_std_mul (one
    Montgomery product) on the device, word for word"""
    by = {c.name: c for c in V.field_cases()["fq29"]}
    c = by["fq29.to_std"]
    assert np.array_equal(ctx.selftest_field(c.op, c.a, c.b), ctx.selftest_field(by["fq29.to_std_mul"].op, c.a, c.b))


@pytest.mark.parametrize("form", list(V.CURVE_FORMS))
def test_curve_ops(ctx, form):
    grp, (mont, unmont) = V.CURVE_FORMS[form]
    cs = V.curve_set(grp)
    for cop in V.CURVE_FORM_OPS[form]:
        p, q = cs.operands(cop, mont)
        cs.check(cop, ctx.selftest_curve(V.curve_op(form, cop), p, q), unmont, form)


@pytest.mark.parametrize("form,lane", [("coop_fq29_acc", "fq"), ("coop_fq29_pk", "fq29_pk"), ("coop_fq2_acc", "fq2"),
                                       ("pair", "fq2"), ("fq2_acc", "fq2"), ("fq29_acc", "fq")])
def test_cooperative_forms_equal_the_lane_form(ctx, form, lane):
    """coop.h / pair_fq2.h / Fq29 / Fq2x29 results on the same inputs, after
    the lane form's to_affine, are the lane form's word for word (`lane`
    reads the same words: field.h's, or the packed ones)"""
    grp, (mont, _) = V.CURVE_FORMS[form]
    assert V.CURVE_FORMS[lane] == V.CURVE_FORMS[form]
    cs = V.curve_set(grp)
    aff = V.curve_op(lane, "to_affine")
    for cop in V.CURVE_FORM_OPS[form]:
        if cop == "to_affine":
            continue
        p, q = cs.operands(cop, mont)
        a = ctx.selftest_curve(aff, ctx.selftest_curve(V.curve_op(form, cop), p, q), q)
        b = ctx.selftest_curve(aff, ctx.selftest_curve(V.curve_op(lane, cop), p, q), q)
        assert np.array_equal(a, b), (form, cop)


def test_glv_split(ctx):
    ks = V.glv_scalars()
    lam, r = V.LAMBDA, V.R_SCALAR
    out = V.ints(ctx.selftest_curve(E.SELFTEST_GLV_SPLIT, V.words(ks, 8)), 4)
    for k, (k1, k2) in zip(ks, out):
        assert (k1 + k2 * lam) % r == k and k1 < 1 << 127 and k2 < 1 << 127, hex(k)
        assert (k1, k2) == (k % lam, k // lam), hex(k)


def test_selftest_bad_arguments_are_errors(ctx):
    a = np.zeros((1, 24), dtype=np.uint32)
    x = np.zeros((1, 96), dtype=np.uint32)
    for op in (-1, 7, 31, 32 + 7, 64 + 14, 96 + 2, 128 + 3, 160, 1 << 20):
        with pytest.raises(TpstError):
            ctx.check(ctx.lib.tpst_selftest_field(ctx.h, op, 1, E._u32ptr(a), E._u32ptr(a), E._u32ptr(a.copy())),
                      "field")
    for op in (-1, 6, 15, 4 * 16 + 3, 4 * 16 + 5, 5 * 16 + 4, 6 * 16 + 5, 7 * 16 + 1, 8 * 16 + 3, 9 * 16 + 5, 10 * 16,
               1 << 20):
        with pytest.raises(TpstError):
            ctx.check(ctx.lib.tpst_selftest_curve(ctx.h, op, 1, E._u32ptr(x), E._u32ptr(x), E._u32ptr(x.copy())),
                      "curve")
    o = E._u32ptr(x.copy())
    assert ctx.lib.tpst_selftest_field(ctx.h, 0, 0, E._u32ptr(a), E._u32ptr(a), o) != 0   # n == 0
    assert ctx.lib.tpst_selftest_field(ctx.h, 0, 1, None, E._u32ptr(a), o) != 0
    assert ctx.lib.tpst_selftest_field(ctx.h, 0, 1, E._u32ptr(a), None, o) != 0
    assert ctx.lib.tpst_selftest_field(ctx.h, 0, 1, E._u32ptr(a), E._u32ptr(a), None) != 0
    assert ctx.lib.tpst_selftest_curve(ctx.h, 0, 0, E._u32ptr(x), E._u32ptr(x), o) != 0
    assert ctx.lib.tpst_selftest_curve(ctx.h, 0, 1, None, E._u32ptr(x), o) != 0
    assert ctx.lib.tpst_selftest_curve(ctx.h, 0, 1, E._u32ptr(x), None, o) != 0
    assert ctx.lib.tpst_selftest_curve(ctx.h, 0, 1, E._u32ptr(x), E._u32ptr(x), None) != 0
    assert ctx.lib.tpst_selftest_field(None, 0, 1, E._u32ptr(a), E._u32ptr(a), o) != 0
    # and the context still works
    assert ctx.selftest_field(E.SELFTEST_FIELD["fq.add"], a[:, :12], a[:, :12]).shape == (1, 12)
