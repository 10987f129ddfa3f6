"""CPU checks of the degenerate sqrt-PST cases (tests/degenerate_vectors.py)
before the device is compared with the reference on them:

* the two restatements -- oracle/py/pst.py (first principles) and oracle/cpu
  (arkworks-shaped C++) -- agree on every proof element at n = 4, down to the
  transcript-dependent values, and both verify;
* every case keeps its class properties under the C++ oracle (infinity
  commitments at the zero rows, T = 1, infinity U / final_a / pst_proof,
  infinities in comms_u and ones in comms_t) and its proof verifies;
* the host wire format (csrc/serialize.hip, no device) writes the degenerate
  proofs byte for byte like oracle/py/serialize.py, with infinity as
  bytes(47) + 0x40, and reads them back to the same arrays.
"""
import numpy as np
import pytest

import bls377 as O
import degenerate_vectors as V
import orc
import pst as P
import serialize as OS
from testudo_amd.encoding import g1_array, g1_from_array, g2_array, g2_from_array, gt_array, gt_from_array

INF_G1 = bytes(47) + b"\x40"
INF_G2 = bytes(95) + b"\x40"


def _gt(f):
    return gt_array(O.fq12_to_tower(f))


def _pair(xs, k):
    return (xs[2 * k], xs[2 * k + 1])


@pytest.mark.parametrize("case", ["zero", "const", "b_boolean", "one_row"])
def test_python_and_cpp_oracles_agree_n4(case):
    n = 4
    ref = V.reference(case, n)
    Zi = [V.fr_int(z) for z in ref["Z"]]
    pti = [V.fr_int(x) for x in ref["pt"]]
    srs = P.SRS((n + 1) // 2, V.SEED_SRS)
    pl = P.Polynomial(Zi)
    assert pl.eval(pti) == V.fr_int(ref["v"])
    comms, T = pl.commit(srs)
    assert np.array_equal(g1_array(comms), ref["comms"])
    assert np.array_equal(_gt(T), ref["T"])
    U, pst_proof, mipp = pl.open(P.PoseidonTranscript(), comms, srs, pti, T)
    pr = ref["pr"]
    assert np.array_equal(g1_array([U])[0], pr["U"])
    assert np.array_equal(g2_array(pst_proof), pr["pst_proof"])
    assert np.array_equal(g1_array([p for pair in mipp["comms_u"] for p in pair]), pr["comms_u"].reshape(-1, 12))
    assert np.array_equal(np.stack([_gt(t) for pair in mipp["comms_t"] for t in pair]), pr["comms_t"].reshape(-1, 72))
    assert np.array_equal(g1_array([mipp["final_a"]])[0], pr["final_a"])
    assert np.array_equal(g2_array([mipp["final_h"]])[0], pr["final_h"])
    assert np.array_equal(g1_array(mipp["pst_proof_h"]), pr["pst_proof_h"])
    assert P.Polynomial.verify(P.PoseidonTranscript(), srs, U, pti, pl.eval(pti), pst_proof, mipp, T)
    assert orc.pst_verify(V.oracle_srs((n + 1) // 2), n, ref["pt"], ref["v"], pr, ref["T"])
    V.check_class(case, n, ref["Z"], ref["v"], ref["comms"], ref["T"], pr)


@pytest.mark.parametrize("case,n", V.GRID)
def test_class_properties_under_cpp_oracle(case, n):
    ref = V.reference(case, n)
    V.check_class(case, n, ref["Z"], ref["v"], ref["comms"], ref["T"], ref["pr"])
    assert orc.pst_verify(V.oracle_srs((n + 1) // 2), n, ref["pt"], ref["v"], ref["pr"], ref["T"])
    bad = V.fr(V.fr_int(ref["v"]) + 1)
    assert not orc.pst_verify(V.oracle_srs((n + 1) // 2), n, ref["pt"], bad, ref["pr"], ref["T"])


def test_point_cases_are_what_they_say():
    """the degenerate points, coordinate by coordinate (a = point[:m_row], b = point[m_row:])"""
    for n in (6, 7):
        m_col, m_row, C = V.dims(n)
        ptr = [V.fr_int(x) for x in V.inputs("const", n)[1]]
        for case, a, b in (("b_boolean", ptr[:m_row], [t % 2 for t in range(m_col)]),
                           ("a_boolean", [1 - t % 2 for t in range(m_row)], ptr[m_row:]),
                           ("point_0", [0] * m_row, [0] * m_col), ("point_1", [1] * m_row, [1] * m_col),
                           ("point_max", [O.R - 1] * m_row, [O.R - 1] * m_col)):
            Z, pt = V.inputs(case, n)
            assert [V.fr_int(x) for x in pt] == a + b, (case, n)
            assert np.array_equal(Z, V.inputs("b_boolean", n)[0])
        # chi(b) of a boolean b is the unit vector at unit_row
        for case in ("b_boolean", "point_0", "point_1"):
            b = [V.fr_int(x) for x in V.inputs(case, n)[1][m_row:]]
            chi = [P.get_chi_i(b, i) for i in range(C)]
            assert chi == [int(i == V.unit_row(case, n)) for i in range(C)], (case, n)


def test_point_valid_on_zero_coordinates():
    """tpst_g1_check / tpst_g2_check (the verifier's point_valid, host code): the
    all-zero encoding is infinity and valid; x = 0 with y != 0 is a point like
    any other -- (0, 2) is off the curve, (0, +-1) is on y^2 = x^3 + 1 but has
    order 3"""
    from testudo_amd import _lib
    lib = _lib.load()

    def chk(a, g2=False):
        a = np.ascontiguousarray(a, dtype=np.uint64)
        return (lib.tpst_g2_check if g2 else lib.tpst_g1_check)(a.ctypes.data_as(_lib._u64p)) == 0

    assert chk(np.zeros(12, dtype=np.uint64)) and chk(np.zeros(24, dtype=np.uint64), g2=True)
    assert O.g1_on_curve((0, 1)) and not O.g1_in_subgroup((0, 1)) and not O.g1_on_curve((0, 2))
    for y in (1, 2, O.P - 1):
        assert not chk(g1_array([(0, y)])[0]), y
        assert not chk(g2_array([((0, 0), (y, 0))])[0], g2=True), y
        assert not chk(g2_array([((0, 0), (0, y))])[0], g2=True), y
    assert not chk(g1_array([(1, 0)])[0])  # y = 0, x != 0: not infinity either


@pytest.mark.parametrize("case", ["zero", "const", "two_rows"])
def test_wire_format_of_degenerate_proofs(case):
    from testudo_amd import serialize as S
    from testudo_amd.sqrt_pst import MippProof
    n = 6
    m_col, m_row, C = V.dims(n)
    pr = V.reference(case, n)["pr"]
    mipp = MippProof(comms_t=pr["comms_t"], comms_u=pr["comms_u"], final_a=pr["final_a"], final_h=pr["final_h"],
                     pst_proof_h=pr["pst_proof_h"])
    b_pst, b_mipp = S.ser_pst_proof(pr["pst_proof"], mipp), S.ser_mipp_proof(pr["pst_proof"], mipp)
    cu = g1_from_array(pr["comms_u"])
    ct = [gt_from_array(t) for t in pr["comms_t"].reshape(-1, 72)]  # tower order, as the wire has it
    assert b_pst == OS.ser_pst_proof(g2_from_array(pr["pst_proof"]))
    assert b_mipp == OS.ser_mipp_proof([_pair(ct, k) for k in range(m_col)], [_pair(cu, k) for k in range(m_col)],
                                       g1_from_array(pr["final_a"])[0], g2_from_array(pr["final_h"])[0],
                                       g1_from_array(pr["pst_proof_h"]))
    assert len(b_pst) == 8 + 96 * m_row
    assert len(b_mipp) == 8 + 1152 * m_col + 8 + 96 * m_col + 48 + 96 + 8 + 48 * m_col
    # the infinity encodings are on the wire where the class says they are
    g2s = [b_pst[8 + 96 * i:8 + 96 * (i + 1)] for i in range(m_row)]
    u0 = 8 + 1152 * m_col + 8
    g1s = [b_mipp[u0 + 48 * i:u0 + 48 * (i + 1)] for i in range(2 * m_col)]
    fa = b_mipp[u0 + 96 * m_col:u0 + 96 * m_col + 48]
    assert [g == INF_G2 for g in g2s] == list(V.is_inf(pr["pst_proof"], 24))
    assert [g == INF_G1 for g in g1s] == list(V.is_inf(pr["comms_u"], 12))
    assert (fa == INF_G1) == (case == "zero")
    if case in ("zero", "const"):
        assert g2s == [INF_G2] * m_row
    if case == "zero":
        assert g1s == [INF_G1] * (2 * m_col)
        one = (1).to_bytes(48, "little") + bytes(48 * 11)
        assert b_mipp[8:8 + 1152 * m_col] == one * (2 * m_col)
    else:
        assert (INF_G1 in g1s) == (case == "two_rows")
    pst2, mipp2 = S.de_open_proof(b_pst, b_mipp)
    assert np.array_equal(pst2, pr["pst_proof"])
    for f in ("comms_t", "comms_u", "final_a", "final_h", "pst_proof_h"):
        assert np.array_equal(getattr(mipp2, f), pr[f]), f

