"""CPU tests of the combined opening's definition (tests/pst_combine_ref.py):
the host-only tpst_pst_combine_challenge against its restatement over the
oracle's sponge, word for word, and the linearity the whole feature rests on,
on the oracle at n = 4, B = 2 (one size: the Python pairing is slow)."""
import ctypes as C

import numpy as np
import pytest

import bls377 as O
import golden_io as G
import pst as P
import pst_combine_ref as CR
from testudo_amd.encoding import fr_array, gt_array, limbs_to_int

R = O.R


def _golden_gts():
    """five GT values of the n = 4 fixture: T and the four comms_t entries (oracle Fq12)"""
    d = G.load("sqrt_pst_n4.json")
    towers = [G.gt(d["T"])] + [G.gt(t) for pair in d["comms_t"] for t in pair]
    return d, [O.fq12_from_tower(t) for t in towers]


def _gt_limbs(f):
    return gt_array(O.fq12_to_tower(f)).reshape(72)


@pytest.mark.parametrize("B", [1, 2, 5])
def test_combine_challenge_matches_oracle_sponge(B):
    """weights, the sponge state and the next challenge of the library's host call equal the restatement"""
    from testudo_amd.sqrt_pst import PoseidonTranscript, combine_challenge
    d, gts = _golden_gts()
    point = [G.i(x) for x in d["point"]]
    vs, _ = P.fr_stream(0xC0B1 + B, B)
    vs[0] = R - 1
    # both transcripts start mid-protocol: something absorbed, one challenge squeezed
    ref = P.PoseidonTranscript()
    ref.append_gt(gts[4])
    ref.challenge_scalar()
    lib = PoseidonTranscript()
    lib.append_gt(_gt_limbs(gts[4]))
    lib.challenge_scalar()
    want = CR.combine_challenge(ref, point, gts[:B], vs)
    got = combine_challenge(lib, fr_array(point), [_gt_limbs(f) for f in gts[:B]], fr_array(vs))
    assert got.shape == (B, 4)
    assert [limbs_to_int(x) for x in got] == want
    assert want[0] == 1 and (B == 1 or want[1] not in (0, 1))
    assert [limbs_to_int(x) for x in lib.state().reshape(3, 6)] == ref.sponge.state
    assert limbs_to_int(lib.challenge_scalar()) == ref.challenge_scalar()


def test_combine_challenge_misuse():
    """host only, no context: null arguments, B out of range, a value or coordinate >= r -> TPST_E_ARG,
    and the transcript is left as it was"""
    from testudo_amd import _lib
    from testudo_amd.encoding import ptr
    from testudo_amd.sqrt_pst import PoseidonTranscript, _ptr_array
    lib = _lib.load()
    d, gts = _golden_gts()
    point = fr_array([G.i(x) for x in d["point"]])
    T = [_gt_limbs(gts[0])]
    v = fr_array([5])
    w = np.zeros((1, 4), dtype=np.uint64)
    tr = PoseidonTranscript()
    before = bytes(tr.t)
    call = lambda *a: lib.tpst_pst_combine_challenge(*a)  # noqa: E731
    assert call(None, 4, ptr(point), _ptr_array(T), ptr(v), 1, ptr(w)) == -1
    assert call(C.byref(tr.t), 4, None, _ptr_array(T), ptr(v), 1, ptr(w)) == -1
    assert call(C.byref(tr.t), 4, ptr(point), _ptr_array(T), ptr(v), 0, ptr(w)) == -1
    assert call(C.byref(tr.t), 4, ptr(point), _ptr_array(T), ptr(v), 257, ptr(w)) == -1
    assert call(C.byref(tr.t), 4, ptr(point), _ptr_array(T), ptr(fr_array([R])), 1, ptr(w)) == -1
    bad_point = point.copy()
    bad_point[2] = fr_array([R + 1])[0]
    assert call(C.byref(tr.t), 4, ptr(bad_point), _ptr_array(T), ptr(v), 1, ptr(w)) == -1
    assert bytes(tr.t) == before
    assert call(C.byref(tr.t), 4, ptr(point), _ptr_array(T), ptr(v), 1, ptr(w)) == 0
    assert bytes(tr.t) != before and limbs_to_int(w[0]) == 1


def test_linearity_on_the_oracle_n4_b2():
    """n = 4, B = 2: the commitment of Z* is the row-wise combination of the two commitments and
    prod T_j^(w_j); its value is sum w_j v_j; the oracle verifier accepts the oracle opening of Z* with
    (T*, v*) formed from the parts alone"""
    srs = P.SRS(2)
    Z0, k = P.fr_stream(0xC0B2, 16)
    Z1, k = P.fr_stream(0xC0B2, 16, k)
    point, _ = P.fr_stream(0xC0B2, 4, k)
    p0, p1 = P.Polynomial(Z0), P.Polynomial(Z1)
    (c0, T0), (c1, T1) = p0.commit(srs), p1.commit(srs)
    vs = [p0.eval(point), p1.eval(point)]
    w = CR.combine_challenge(P.PoseidonTranscript(), point, [T0, T1], vs)
    comms, T, v, (U, pst_proof, mipp), _ = CR.parent_path(srs, [Z0, Z1], w, point)
    assert CR.combine_rows([c0, c1], w) == comms
    Tc, vc = CR.combine_T([T0, T1], w), CR.combine_v(vs, w)
    assert Tc == T and vc == v
    assert P.Polynomial.verify(P.PoseidonTranscript(), srs, U, point, vc, pst_proof, mipp, Tc)
    assert not P.Polynomial.verify(P.PoseidonTranscript(), srs, U, point, CR.combine_v([vs[0], vs[1] + 1], w),
                                   pst_proof, mipp, Tc)
