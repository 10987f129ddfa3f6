"""CPU tests of the host verifier of the grand-product argument
(tpst_prodcircuit_verify through libtpst.so) against the restatement
tests/product_tree_ref.py: no GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import product_tree_ref as T
from testudo_amd import _lib
from testudo_amd import product_tree as PT
from testudo_amd.encoding import fr_array, limbs_to_int, ptr
from testudo_amd.hyrax import FrTranscript

R = T.R
SHAPES = [(1, 1, 0), (2, 1, 0), (2, 2, 2), (3, 3, 2), (5, 2, 4)]
E_ARG, E_VERIFY = -1, -5


@functools.lru_cache(maxsize=None)
def _case(ell, P, D):
    polys, dotps, _whole = T.random_inputs(ell, P, D, 8000 + 100 * ell + 10 * P + D)
    return T.run(polys, dotps)


def _ints(a):
    return [limbs_to_int(x) for x in np.asarray(a).reshape(-1, 4)]


def _state(tr):
    st, sq, idx = tr.state()
    return [limbs_to_int(x) for x in st], sq, idx


def _proof(v, ell, P, D, flat=None):
    flat = T.flatten(v["proof"], ell, P, D) if flat is None else flat
    return PT.ProductCircuitProof.unpack(fr_array(flat), ell, P, D)


def _raw_verify(ell, P, D, cp, cd, flat, tr=None, null=None):
    """the C call itself -> rc; `null`: the name of one argument passed as NULL"""
    lib = _lib.load()
    t = tr or FrTranscript()
    a = {"cp": fr_array(cp), "cd": fr_array(cd) if len(cd) else None, "proof": fr_array(flat),
         "out": np.zeros((max(P, 1), 4), dtype=np.uint64), "dout": np.zeros((3 * max(D, 2), 4), dtype=np.uint64),
         "rand": np.zeros((max(ell, 1), 4), dtype=np.uint64)}
    p = {k: (None if v is None or k == null else ptr(v)) for k, v in a.items()}
    return lib.tpst_prodcircuit_verify(ell, P, D, p["cp"], p["cd"], p["proof"], None if null == "tr" else C.byref(t.t),
                                       p["out"], p["dout"], p["rand"])


@pytest.mark.parametrize("ell,P,D", SHAPES)
def test_verify_accepts_the_restatement(ell, P, D):
    v = _case(ell, P, D)
    assert PT.proof_len(ell, P, D) == T.proof_len(ell, P, D)
    pr = _proof(v, ell, P, D)
    assert _ints(pr.pack()) == T.flatten(v["proof"], ell, P, D)  # pack / unpack round trip
    tr = FrTranscript()
    res = PT.verify(fr_array(v["claims_prod"]), fr_array(v["claims_dotp"]), pr, tr)
    assert res is not False
    claims, claims_dotp, rand = res
    assert _ints(claims) == v["claims_out"]
    assert _ints(claims_dotp) == v["claims_dotp_out"]
    assert _ints(rand) == v["rand"]
    assert _state(tr) == v["transcript_end"]


def test_verify_chains_on_a_used_transcript():
    ell, P, D = 3, 3, 2
    polys, dotps, _ = T.random_inputs(ell, P, D, 8100)
    circuits = [T.product_circuit(p) for p in polys]
    rt, tr = T.Transcript(), FrTranscript()
    rt.append_scalar(12345)
    tr.append_scalar(fr_array([12345])[0])
    assert rt.challenge() == limbs_to_int(tr.challenge_scalar())
    proof, rand = T.prove(circuits, dotps, rt)
    cp, cd = [T.circuit_evaluate(c) for c in circuits], [T.dotp_evaluate(*d) for d in dotps]
    res = PT.verify(fr_array(cp), fr_array(cd), PT.ProductCircuitProof.unpack(
        fr_array(T.flatten(proof, ell, P, D)), ell, P, D), tr)
    assert res is not False and _ints(res[2]) == rand and _state(tr) == rt.state()


@pytest.mark.parametrize("ell,P,D", [(3, 3, 2), (5, 2, 4)])
def test_tampering_returns_verify_error(ell, P, D):
    v = _case(ell, P, D)
    flat = T.flatten(v["proof"], ell, P, D)
    cp, cd = v["claims_prod"], v["claims_dotp"]
    assert _raw_verify(ell, P, D, cp, cd, flat) == 0
    npoly = 4 * (ell * (ell - 1) // 2)
    # every round coefficient, every left / right claim, every dot-product claim
    for k in range(len(flat)):
        bad = list(flat)
        bad[k] = (bad[k] + 1) % R
        tr = FrTranscript()
        before = _state(tr)
        assert _raw_verify(ell, P, D, cp, cd, bad, tr) == E_VERIFY, k
        assert _state(tr) == before  # a rejected proof leaves the transcript alone
    assert npoly + 2 * ell * P + 3 * D == len(flat)
    for k in range(P):
        bad = list(cp)
        bad[k] = (bad[k] + 1) % R
        assert _raw_verify(ell, P, D, bad, cd, flat) == E_VERIFY
    for k in range(D):
        bad = list(cd)
        bad[k] = (bad[k] + 1) % R
        assert _raw_verify(ell, P, D, cp, bad, flat) == E_VERIFY
    # the Python surface reports a rejection as False
    bad = list(flat)
    bad[0] = (bad[0] + 1) % R
    assert PT.verify(fr_array(cp), fr_array(cd), _proof(v, ell, P, D, bad), FrTranscript()) is False


def test_non_canonical_values_return_verify_error():
    ell, P, D = 3, 3, 2
    v = _case(ell, P, D)
    flat = T.flatten(v["proof"], ell, P, D)
    cp, cd = v["claims_prod"], v["claims_dotp"]
    npoly = 4 * (ell * (ell - 1) // 2)
    # one position in each proof field: round polynomials, left, right, the three dot-product vectors
    for k in (0, npoly - 1, npoly, npoly + ell * P, npoly + 2 * ell * P, npoly + 2 * ell * P + D,
              npoly + 2 * ell * P + 2 * D, len(flat) - 1):
        for val in (flat[k] + R, R, 2**256 - 1):
            bad = list(flat)
            bad[k] = val
            assert _raw_verify(ell, P, D, cp, cd, bad) == E_VERIFY, (k, val)
    bad = list(cp)
    bad[1] += R
    assert _raw_verify(ell, P, D, bad, cd, flat) == E_VERIFY
    bad = list(cd)
    bad[0] += R
    assert _raw_verify(ell, P, D, cp, bad, flat) == E_VERIFY


def test_bad_arguments_return_arg_error():
    ell, P, D = 3, 3, 2
    v = _case(ell, P, D)
    flat = T.flatten(v["proof"], ell, P, D)
    cp, cd = v["claims_prod"], v["claims_dotp"]
    for null in ("cp", "cd", "proof", "tr", "out", "dout", "rand"):
        assert _raw_verify(ell, P, D, cp, cd, flat, null=null) == E_ARG, null
    assert _raw_verify(0, P, D, cp, cd, flat) == E_ARG       # ell = 0
    assert _raw_verify(31, P, D, cp, cd, flat) == E_ARG
    assert _raw_verify(ell, 0, D, cp, cd, flat) == E_ARG
    assert _raw_verify(ell, P, 1, cp, cd, flat) == E_ARG     # odd D
    assert _raw_verify(ell, P, 3, cp, cd + [0, 0], flat + [0] * 3) == E_ARG
    lib = _lib.load()
    assert lib.tpst_prodcircuit_proof_len(0, 1, 0) == 0 and lib.tpst_prodcircuit_proof_len(3, 2, 1) == 0
    assert lib.tpst_prodcircuit_proof_len(1, 1, 0) == 2
    # a transcript state no sponge can be in
    tr = FrTranscript()
    tr.t.index = 3
    assert _raw_verify(ell, P, D, cp, cd, flat, tr) == E_ARG
    # D == 0: the dot-product pointers may be NULL
    v0 = _case(2, 1, 0)
    assert _raw_verify(2, 1, 0, v0["claims_prod"], [], T.flatten(v0["proof"], 2, 1, 0), null="dout") == 0
