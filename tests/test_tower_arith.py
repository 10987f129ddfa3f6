"""Device self-test of the pairing's two Fq12 engines on edge operands
(tpst_selftest_tower, csrc/selftest.hip):

  rns_engine.h   load / load_res, every single Fq12 stage, store / store_res,
                 the inversion rc_inv, the final exponentiation (gt_prod_final)
                 and G2Prepared (g2_prepare_batch): the red64 / red32 folds,
                 both base extensions of mont(), the negk - y negation,
                 residue(), to_fq_wave's alpha and reduce16p's quotient estimate;
  wave_tower.h   the live op set (F12_MUL, CYC_SQR, FROB1, FROB2, CONJ), the
                 inversion fe_inv and gt_pow_wave: form()'s 64-bit limbs,
                 reduce_wide's quotient estimate, stage_mul's unreduced operand.

Every comparison is exact equality against Python integers.  Operands and
expectations are tests/tower_vectors.py's (coefficients 0, 1, p-1, ...; extreme
field.h words; products of exactly 1, -1 and 0; slot integers at k p, k p +- 1,
16 p - 1 and at residues 0 / m - 1 of every channel; forms at their weight
bound; structured inputs of the composites), which tests/test_tower_vectors.py
proves on the host; under the RES codec the expectation is the bit-exact output
of tools/gen_rns_ops.py's model of the engine."""
import numpy as np
import pytest

import tower_vectors as V
from testudo_amd import engine as E
from testudo_amd.engine import TpstError

pytestmark = pytest.mark.gpu

RNS_OPS = V.RNS_STAGES + ("inv",)
WAVE_OPS = V.WAVE_STAGES + ("inv",)
CASES = ([("rns", "fq", op) for op in RNS_OPS + ("final_exp",)] + [("rns", "res", op) for op in RNS_OPS] +
         [("rns", "fq->res", "pass"), ("rns", "res->fq", "pass")] + [("wave", "fq", op) for op in WAVE_OPS])


def _hex(vals):
    return [hex(int(v)) for v in vals]


def _check(c, got):
    """exact equality, reporting the first bad element: op, class name, index, inputs, device words"""
    assert got.shape == c.exp.shape, (c.name, got.shape, c.exp.shape)
    res = c.exp.shape[1] == 384
    live = V.res_live if res else (lambda x: x)
    bad = np.nonzero((live(got) != live(c.exp)).any(axis=1))[0]
    if len(bad):
        i = int(bad[0])
        per = 32 if res else 12
        diff = (got[i] != c.exp[i]).reshape(12, per)[:, :31 if res else 12].any(axis=1)
        k = int(np.nonzero(diff)[0][0])
        raise AssertionError("%s: %d of %d elements differ; first: class %r index %d coefficient %d\n inputs %s\n"
                             " device %s\n expect %s" % (c.name, len(bad), len(got), c.names[i], i, k,
                                                         _hex(c.inputs[i]), _hex(got[i, per * k:per * k + per]),
                                                         _hex(c.exp[i, per * k:per * k + per])))


def _case(engine, codec, op):
    if op == "pass":
        return V.pass_cases()[0 if codec == "fq->res" else 1]
    return V.fq_case(engine, op) if codec == "fq" else V.res_case(op)


@pytest.mark.parametrize("engine,codec,op", CASES)
def test_tower_ops(ctx, engine, codec, op):
    c = _case(engine, codec, op)
    _check(c, ctx.selftest_tower(c.op, c.a, c.b))


def test_odd_and_single_element_counts(ctx):
    """n = 1, 2, 3: the RNS engine's lone element of the last workgroup"""
    c = V.fq_case("rns", "f12_mul")
    for n in (1, 2, 3):
        got = ctx.selftest_tower(c.op, c.a[-n:], c.b[-n:])
        assert np.array_equal(got, c.exp[-n:]), n
    r = V.res_case("f12_sqr")
    for n in (1, 3):
        assert np.array_equal(V.res_live(ctx.selftest_tower(r.op, r.a[:n])), V.res_live(r.exp[:n])), n


@pytest.mark.parametrize("op", ["f12_mul", "cyc_sqr", "frob1", "frob2", "conj", "inv"])
def test_engines_agree_word_for_word(ctx, op):
    """the RNS and the wave engine on the same FQ inputs (the wave engine's
    operands, which include its form maximisers)"""
    c = V.fq_case("wave", op)
    r = ctx.selftest_tower(E.selftest_tower_op("rns", op), c.a, c.b)
    w = ctx.selftest_tower(c.op, c.a, c.b)
    bad = np.nonzero((r != w).any(axis=1))[0]
    assert not len(bad), (op, len(bad), c.names[bad[0]], _hex(c.inputs[bad[0]]), _hex(r[bad[0]]), _hex(w[bad[0]]))


@pytest.mark.parametrize("n", [1, 2, 3, 13])
def test_g2_prepare(ctx, n):
    """g2_prepare_batch (k_g2_prepare_rns + k_rns_to_fq) against the oracle's
    G2Prepared: n = 1, 3, 13 leave a lone chain in the last workgroup"""
    pts = V.g2_points()
    pts = pts[:n] if n > 3 else pts[3 - n:3] if n < 3 else pts[:3]
    exp = V.g2_expected([p for _, p in pts])
    got = ctx.selftest_tower(E.selftest_tower_op("rns", "g2_prepare"), V.g2_words([p for _, p in pts]))
    got = got.reshape(69, n, 72).transpose(1, 0, 2)  # coefficient-major on the device
    for i, (nm, p) in enumerate(pts):
        bad = np.nonzero((got[i] != exp[i]).any(axis=1))[0]
        assert not len(bad), (nm, "line", int(bad[0]), _hex(p[0] + p[1]), _hex(got[i, bad[0]]), _hex(exp[i, bad[0]]))


def test_gt_pow(ctx):
    vs = V.gt_pow_vectors()
    a = V.fq_words([base for _, base, _, _, _ in vs])
    d = np.array([dg for _, _, dg, _, _ in vs], dtype=np.uint64).view(np.uint32).reshape(len(vs), 8)
    out, ok = ctx.selftest_tower(E.selftest_tower_op("wave", "gt_pow"), a, d)
    exp = V.fq_words([e for _, _, _, _, e in vs])
    for i, (nm, base, dg, member, _) in enumerate(vs):
        assert int(ok[i]) == member, (nm, _hex(base), int(ok[i]))
        assert np.array_equal(out[i], exp[i]), (nm, _hex(base), _hex(dg), _hex(out[i]), _hex(exp[i]))


def test_selftest_tower_bad_arguments_are_errors(ctx):
    a = np.zeros((2, 384), dtype=np.uint32)
    o = np.zeros((2, 69 * 72), dtype=np.uint32)
    bad = [-1, 13, 63, 9 | 1 << 6, 9 | 1 << 7, 10 | 1 << 6, 10 | 3 << 6, 11, 1 << 8 | 1, 1 << 8 | 5, 1 << 8 | 7,
           1 << 8 | 9, 1 << 8 | 10, 1 << 8 | 12, 1 << 8 | 1 << 6, 1 << 8 | 1 << 7 | 8, 2 << 8, 1 << 20]
    for op in bad:
        assert not E.selftest_tower_valid(op), op
        with pytest.raises(TpstError):
            ctx.check(ctx.lib.tpst_selftest_tower(ctx.h, op, 1, E._u32ptr(a), E._u32ptr(a), E._u32ptr(o)), "tower")
    mul = E.selftest_tower_op("rns", "f12_mul")
    sqr = E.selftest_tower_op("wave", "cyc_sqr")
    pw = E.selftest_tower_op("wave", "gt_pow")
    assert ctx.lib.tpst_selftest_tower(ctx.h, mul, 0, E._u32ptr(a), E._u32ptr(a), E._u32ptr(o)) != 0   # n == 0
    assert ctx.lib.tpst_selftest_tower(ctx.h, mul, (1 << 16) + 1, E._u32ptr(a), E._u32ptr(a), E._u32ptr(o)) != 0
    assert ctx.lib.tpst_selftest_tower(ctx.h, mul, 1, None, E._u32ptr(a), E._u32ptr(o)) != 0
    assert ctx.lib.tpst_selftest_tower(ctx.h, mul, 1, E._u32ptr(a), None, E._u32ptr(o)) != 0
    assert ctx.lib.tpst_selftest_tower(ctx.h, pw, 1, E._u32ptr(a), None, E._u32ptr(o)) != 0
    assert ctx.lib.tpst_selftest_tower(ctx.h, mul, 1, E._u32ptr(a), E._u32ptr(a), None) != 0
    assert ctx.lib.tpst_selftest_tower(ctx.h, sqr, 1, None, None, E._u32ptr(o)) != 0
    assert ctx.lib.tpst_selftest_tower(None, mul, 1, E._u32ptr(a), E._u32ptr(a), E._u32ptr(o)) != 0
    # a unary op takes a null b, and the context still works
    assert ctx.lib.tpst_selftest_tower(ctx.h, sqr, 1, E._u32ptr(a), None, E._u32ptr(o)) == 0
    c = V.fq_case("rns", "copy")
    assert np.array_equal(ctx.selftest_tower(c.op, c.a[:2]), c.exp[:2])
