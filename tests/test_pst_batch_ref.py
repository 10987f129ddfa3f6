"""CPU tests of the batch verifier's combined equation as tests/pst_batch_ref.py
restates it over oracle/py: B = 2 at n = 4 (m_col = m_row = 2), the golden proof
and a second proof the oracle makes of another polynomial at another point.  The
two proofs and their single verdicts are computed once."""
import random

import pytest

import bls377 as O
import golden_io as G
import pst as P
import pst_batch_ref as B

R = O.R
_STATE = {}


def _golden_item(d):
    gt = lambda t: O.fq12_from_tower(G.gt(t))  # noqa: E731  (the files hold arkworks' tower order)
    mipp = {"comms_t": [(gt(a), gt(b)) for a, b in d["comms_t"]],
            "comms_u": [(G.g1(a), G.g1(b)) for a, b in d["comms_u"]],
            "final_a": G.g1(d["final_a"]), "final_h": G.g2(d["final_h"]),
            "pst_proof_h": [G.g1(x) for x in d["pst_proof_h"]]}
    return {"U": G.g1(d["U"]), "point": [G.i(x) for x in d["point"]], "v": G.i(d["eval"]),
            "pst_proof": [G.g2(x) for x in d["pst_proof"]], "mipp": mipp, "T": gt(d["T"]),
            "tr": P.PoseidonTranscript}


def state():
    """(srs, [golden item, oracle-made item], rho) -- built once"""
    if not _STATE:
        d = G.load("sqrt_pst_n4.json")
        srs = P.SRS(d["srs_nv"], d["srs_seed"])
        assert srs.g == G.g1(d["srs"]["g"])
        Z, k = P.fr_stream(0xBA7C4, 16)
        pt, _ = P.fr_stream(0xBA7C4, 4, k)
        pl = P.Polynomial(Z)
        v = pl.eval(pt)
        comms, T = pl.commit(srs)
        U, pst_proof, mipp = pl.open(P.PoseidonTranscript(), comms, srs, pt, T)
        second = {"U": U, "point": pt, "v": v, "pst_proof": pst_proof, "mipp": mipp, "T": T,
                  "tr": P.PoseidonTranscript}
        rng = random.Random(0x2B0)
        rho = [tuple(rng.getrandbits(128) | 1 for _ in range(4)) for _ in range(2)]
        _STATE.update(srs=srs, items=[_golden_item(d), second], rho=rho)
    return _STATE["srs"], _STATE["items"], _STATE["rho"]


def _with(it, **kw):
    out = dict(it)
    out.update(kw)
    return out


def _mipp_with(it, **kw):
    mp = dict(it["mipp"])
    mp.update(kw)
    return _with(it, mipp=mp)


def test_valid_batch_accepted():
    srs, items, rho = state()
    assert all(B.single_accepts(srs, it) for it in items)
    assert B.batch_accepts(srs, items, rho)
    assert B.batch_accepts(srs, items[:1], rho[:1])


TAMPERS = {
    "v + 1": lambda a, b: _with(a, v=(a["v"] + 1) % R),
    "other T": lambda a, b: _with(a, T=b["T"]),
    "other U": lambda a, b: _with(a, U=b["U"]),
    "comms_t[0] swapped": lambda a, b: _mipp_with(a, comms_t=[a["mipp"]["comms_t"][0][::-1]] + a["mipp"]["comms_t"][1:]),
    "comms_u[0] swapped": lambda a, b: _mipp_with(a, comms_u=[a["mipp"]["comms_u"][0][::-1]] + a["mipp"]["comms_u"][1:]),
    "other final_a": lambda a, b: _mipp_with(a, final_a=b["mipp"]["final_a"]),
    "other final_h": lambda a, b: _mipp_with(a, final_h=b["mipp"]["final_h"]),
    "other pst_proof[0]": lambda a, b: _with(a, pst_proof=[b["pst_proof"][0]] + a["pst_proof"][1:]),
    "other pst_proof_h[0]": lambda a, b: _mipp_with(a, pst_proof_h=[b["mipp"]["pst_proof_h"][0]] + a["mipp"]["pst_proof_h"][1:]),
    "point[0] + 1": lambda a, b: _with(a, point=[(a["point"][0] + 1) % R] + a["point"][1:]),
    "point[3] + 1": lambda a, b: _with(a, point=a["point"][:3] + [(a["point"][3] + 1) % R]),
}


@pytest.mark.parametrize("name", sorted(TAMPERS))
def test_single_field_tamper_rejected(name):
    """one field of the second item changed: the item alone is rejected (Polynomial.verify), the batch that
    holds it is rejected, and the batch of the untouched item alone is what test_valid_batch_accepted accepts"""
    srs, items, rho = state()
    bad = TAMPERS[name](items[1], items[0])
    assert not B.single_accepts(srs, bad)
    assert not B.batch_accepts(srs, [items[0], bad], rho)
    assert not B.batch_accepts(srs, [bad], rho[1:])


def test_cancelling_pair_needs_distinct_multipliers():
    """T_a delta and T_b / delta with delta = e(g, h): each item alone is invalid, their (A) errors cancel in
    an unweighted product.  Distinct rho_T reject the pair; equal rho_T accept it -- the reason the multipliers
    must be drawn at random after the proofs are fixed."""
    srs, items, rho = state()
    delta = O.pairing(srs.g, srs.h)
    a = _with(items[0], T=O.f12_mul(items[0]["T"], delta))
    b = _with(items[1], T=O.f12_mul(items[1]["T"], O.f12_inv(delta)))
    assert not B.single_accepts(srs, a) and not B.single_accepts(srs, b)
    assert rho[0][0] != rho[1][0]
    assert not B.batch_accepts(srs, [a, b], rho)
    same = [rho[0], (rho[0][0],) + rho[1][1:]]
    assert B.batch_accepts(srs, [a, b], same)
