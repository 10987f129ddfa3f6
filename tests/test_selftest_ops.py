"""csrc/selftest_ops.h (the per-element dispatch behind tpst_selftest_field /
tpst_selftest_curve) run on the host with g++, on exactly the operands and
expected values of tests/test_device_arith.py (tests/arith_vectors.py).  The
host Montgomery product of field.h is a different algorithm from the device
one, so this proves the vectors, the word layouts and the Python expectations;
the GPU test then has the device code as its only unknown.  The 4-lane
(coop.h), pair, Fq2x29 and glv_split forms exist only on the device and take
the same operands."""
import os
import struct
import subprocess

import numpy as np
import pytest

import arith_vectors as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("stops") / "test_selftest_ops")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "testudo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_selftest_ops.cpp"), "-o", out], check=True)
    return out


def _run(exe, kind, op, a, b, wo):
    inp = struct.pack("<iii", kind, op, len(a)) + a.tobytes() + b.tobytes()
    r = subprocess.run([exe], input=inp, capture_output=True, check=True)
    return np.frombuffer(r.stdout, dtype=np.uint32).reshape(len(a), wo)


@pytest.mark.parametrize("family", ["fq", "fr", "fq29", "fq2"])
def test_host_field_dispatch(exe, family):
    for c in V.field_cases()[family]:
        got = _run(exe, 0, c.op, c.a, c.b, c.exp.shape[1])
        bad = np.nonzero((got != c.exp).any(axis=1))[0]
        assert not len(bad), (c.name, len(bad), [hex(v) for v in c.inputs[bad[0]]])


@pytest.mark.parametrize("form", V.LANE_FORMS)
def test_host_curve_dispatch(exe, form):
    grp, (mont, unmont) = V.CURVE_FORMS[form]
    cs = V.curve_set(grp)
    for cop in V.CURVE_FORM_OPS[form]:
        p, q = cs.operands(cop, mont)
        cs.check(cop, _run(exe, 1, V.curve_op(form, cop), p, q, p.shape[1]), unmont, form)


def test_device_only_ops_are_refused_by_the_host_dispatch(exe):
    z = np.zeros((1, 96), dtype=np.uint32)
    for kind, op in ((0, 128), (1, V.curve_op("pair", "add")), (1, V.curve_op("coop_fq29_acc", "dbl")),
                     (1, V.curve_op("fq2_acc", "add")), (0, 7), (1, 6)):
        r = subprocess.run([exe], input=struct.pack("<iii", kind, op, 1) + z.tobytes() * 2, capture_output=True)
        assert r.returncode == 2, (kind, op)


def test_python_op_tables_match_the_header(exe):
    """testudo_amd/engine.py restates csrc/selftest_ops.h's op numbers and word
    counts; the header's values are read through the compiled dispatch"""
    from testudo_amd import engine as E
    N = 256
    r = subprocess.run([exe], input=struct.pack("<iii", 2, 0, N), capture_output=True, check=True)
    tab = np.frombuffer(r.stdout, dtype=np.int32).reshape(N, 5)
    field_ops = set(E.SELFTEST_FIELD.values())
    curve_ops = {V.curve_op(f, c) for f, cops in V.CURVE_FORM_OPS.items() for c in cops} | {E.SELFTEST_GLV_SPLIT}
    assert set(V.CURVE_FORM_OPS) | {"glv"} == set(E.SELFTEST_CURVE_FORMS)
    for op in range(N):
        fv, fi, fo, cv, cw = (int(x) for x in tab[op])
        assert bool(fv) == (op in field_ops), op
        assert bool(cv) == (op in curve_ops), op
        if fv:
            assert E.selftest_field_words(op) == (fi, fo), op
        if cv:
            assert E.selftest_curve_words(op) == cw, op


def test_constructed_classes_are_populated():
    """every constructed class produced operands (the defining property of each
    is asserted where it is built, arith_vectors.py)"""
    V.field_cases()
    V.curve_set("g1")
    V.curve_set("g2")
    V.glv_scalars()
    for F in (V.FQ, V.FR, V.F29):
        for cols in V.mk0_columns(F):
            assert V.COUNTS["%s.mul.m_k=0 cols=%s" % (F.name, cols)] >= 1
        assert V.COUNTS["%s.sqr.m_0=0" % F.name] >= 2
        for k in range(1, F.n):
            assert V.COUNTS["%s.sqr.m_k=0 col=%d" % (F.name, k)] >= 1
    for cols in V.mk0_columns(V.F29):
        for nm in ("mul_sum", "mul_sub", "mul_sum4", "mul_sub4", "mul_sub4 d=0"):
            assert V.COUNTS["fq29.%s.m_k=0 cols=%s" % (nm, cols)] >= 1
    assert V.COUNTS["fq29.to_std 128 Y within 128 of q p"] == 254
    assert V.COUNTS["g1 curve edge pairs with ZZ != 1"] >= 40 and V.COUNTS["g2 curve edge pairs with ZZ != 1"] >= 14
    assert V.COUNTS["glv scalars m lambda + {-1,0,1}"] >= 10
    print("\n".join("%-48s %d" % kv for kv in sorted(V.COUNTS.items())))
