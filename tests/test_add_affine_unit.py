"""curve.h's chain-start mixed add (add_affine_unit, the `unit` form of
add_affine: p infinity or ZZ = ZZZ = 1) on the host: the same four XYZZ
coordinates, word for word, as add_affine over Fq and Fq29
(tests/cpp/test_add_affine_unit.cpp), and through the self-test dispatch of
csrc/selftest_ops.h in every lane form, against Python integers.  The
operands are chain_start_vectors.py's."""
import os
import struct
import subprocess

import numpy as np
import pytest

import arith_vectors as V
import chain_start_vectors as CS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("unit") / "test_add_affine_unit")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "testudo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_add_affine_unit.cpp"), "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def dispatch(tmp_path_factory):
    return CS.build_host_dispatch(str(tmp_path_factory.mktemp("unitd") / "test_selftest_ops"))


def test_unit_form_equals_add_affine_fq_and_fq29(exe):
    us, p, q, _ = CS.form_operands("fq")
    r = subprocess.run([exe], input=struct.pack("<i", len(p)) + p.tobytes() + q.tobytes(), capture_output=True,
                       text=False)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert r.stdout.decode().strip() == "pairs %d fq_bad 0 fq29_bad 0" % len(p)
    assert len(p) >= us.cs.n_edge + 500


def test_operands_outside_the_contract_are_refused(exe):
    """the comparison program checks ZZ = ZZZ = 1 itself (status 3)"""
    cs = V.curve_set("g1")
    p, q = cs.operands("add_affine", V.CURVE_FORMS["fq"][1][0])
    i = next(i for i, c in enumerate(cs.p) if c[2] not in (V.G1.F.zero, V.G1.F.one))
    r = subprocess.run([exe], input=struct.pack("<i", 1) + p[i:i + 1].tobytes() + q[i:i + 1].tobytes(),
                       capture_output=True)
    assert r.returncode == 3


@pytest.mark.parametrize("form", V.LANE_FORMS)
def test_host_dispatch_unit_forms(dispatch, form):
    us, p, q, unmont = CS.form_operands(form)
    got = CS.host_curve(dispatch, CS.unit_op(form), p, q)
    us.check(got, unmont, form + " unit")
    full = CS.host_curve(dispatch, V.curve_op(form, "add_affine"), p, q)
    bad = np.nonzero((got != full).any(axis=1))[0]
    assert not len(bad), (form, len(bad), us.cs.tags[bad[0]])


def test_unit_ops_lie_past_the_op_table(dispatch):
    """the chain-start forms are numbered from form 16 up (ops >= 256) and only
    add_affine exists in them"""
    from testudo_amd import engine as E
    z = np.zeros((1, 96), dtype=np.uint32)
    for form in E.SELFTEST_CURVE_UNIT_FORMS:
        op = CS.unit_op(form)
        assert op >= 256 and E.selftest_curve_words(op) == E.selftest_curve_words(V.curve_op(form, "add_affine"))
        for bad in (op + 1, op + 5):
            r = subprocess.run([dispatch], input=struct.pack("<iii", 1, bad, 1) + z.tobytes() * 2, capture_output=True)
            assert r.returncode == 2, bad
    r = subprocess.run([dispatch], input=struct.pack("<iii", 1, (16 + 4) * 16, 1) + z.tobytes() * 2, capture_output=True)
    assert r.returncode == 2
