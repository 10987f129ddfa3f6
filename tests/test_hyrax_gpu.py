"""GPU tests of the Hyrax evaluation proofs (csrc/hyrax.hip): PolyEvalProof /
DotProductProofLog prove and verify on the device, bit-exact against the
first-principles restatement tests/hyrax_ref.py (which folds G literally) and
the fixture tests/golden/hyrax_eval.json."""
import functools
import random

import numpy as np
import pytest

import bls377 as O
import hyrax_ref as H
import orc
from testudo_amd.encoding import fr_array, g1_array, g1_from_array, limbs_to_int

pytestmark = pytest.mark.gpu

R = O.R
BOUND_TILE = 64  # csrc/hyrax.hip HB_TJ: rows j per block of the bound kernel


def _proof_arrays(p):
    from testudo_amd.hyrax import DotProductProof
    k = len(p["L"])
    return DotProductProof(L=g1_array(p["L"]).reshape(k, 12), R=g1_array(p["R"]).reshape(k, 12),
                           delta=g1_array([p["delta"]])[0], beta=g1_array([p["beta"]])[0],
                           z1=fr_array([p["z1"]])[0], z2=fr_array([p["z2"]])[0])


def _proof_dict(pr):
    return {"L": g1_from_array(pr.L) if len(pr.L) else [], "R": g1_from_array(pr.R) if len(pr.R) else [],
            "delta": g1_from_array(pr.delta)[0], "beta": g1_from_array(pr.beta)[0], "z1": limbs_to_int(pr.z1),
            "z2": limbs_to_int(pr.z2)}


def _state(tr):
    st, sq, idx = tr.state()
    return [limbs_to_int(x) for x in st], sq, idx


def _ref_gens(hg):
    return g1_from_array(hg.gens.G), g1_from_array(hg.gens.h)[0], g1_from_array(hg.Q)[0]


_GENS = {}


def _gens(ctx, ell):
    from testudo_amd.hyrax import HyraxGens
    if ell not in _GENS:
        _GENS[ell] = HyraxGens.setup(ctx, ell, b"hyrax_eval")
    return _GENS[ell]


def _inputs(ell, blinded, seed=0):
    rng = random.Random(1000 * ell + (7 if blinded else 0) + seed)
    fr = lambda: rng.randrange(1, R)  # noqa: E731
    lv = ell // 2
    Z = [fr() for _ in range(1 << ell)]
    r = [fr() for _ in range(ell)]
    blinds = [fr() for _ in range(1 << lv)] if blinded else None
    blind_Zr = fr() if blinded else None
    rnd = [fr() for _ in range(3 + 4 * (ell - lv))]
    return Z, r, blinds, blind_Zr, rnd


@functools.lru_cache(maxsize=None)
def _reference(ell, blinded, gens_key):
    """the restatement's proof for _inputs(ell, blinded), computed once"""
    gens = _REF_GENS[gens_key]
    Z, r, blinds, blind_Zr, rnd = _inputs(ell, blinded)
    msm = H.py_msm if ell <= 4 else H.orc_msm
    Zr = H.evaluate(Z, r)
    tr = H.Transcript()
    proof, C_Zr = H.eval_prove(Z, blinds, r, Zr, blind_Zr, gens, tr, rnd, msm)
    comm = H.commit_rows(Z, blinds or [0] * (1 << (ell // 2)), gens, msm)
    return Zr, proof, C_Zr, comm, tr.state()


_REF_GENS = {}


def _device_z(ctx, Z):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(Z).view(np.int64)).to(torch.device("cuda", ctx.device))
    ctx.torch_to_lib()
    return d


# ---------------------------------------------------------------- bit-exact --
@pytest.mark.parametrize("blinded", [False, True])
@pytest.mark.parametrize("ell", [1, 2, 3, 4, 7, 10])
def test_eval_prove_bit_exact_vs_restatement(ctx, ell, blinded):
    """every L_k, R_k, delta, beta, z1, z2, C_Zr' and the transcript's end state,
    from host Z and from a device buffer, zero and nonzero blinds"""
    from testudo_amd.hyrax import FrTranscript, eval_prove, eval_verify
    hg = _gens(ctx, ell)
    _REF_GENS[ell] = _ref_gens(hg)
    if ell <= 4:
        assert _REF_GENS[ell] == H.setup_gens(ell, b"hyrax_eval")
    Z, r, blinds, blind_Zr, rnd = _inputs(ell, blinded)
    Zr, ref, C_ref, comm, end = _reference(ell, blinded, ell)
    Za, ra, rnda = fr_array(Z), fr_array(r), fr_array(rnd)
    bl = None if blinds is None else fr_array(blinds)
    bz = None if blind_Zr is None else fr_array([blind_Zr])[0]
    tr = FrTranscript()
    proof, C_Zr = eval_prove(hg, Za, ra, fr_array([Zr])[0], rnda, tr, blinds=bl, blind_Zr=bz)
    assert proof.rounds is None and len(proof.L) == ell - ell // 2
    assert _proof_dict(proof) == ref
    assert g1_from_array(C_Zr)[0] == C_ref
    assert _state(tr) == end
    d_Z = _device_z(ctx, Za)
    tr2 = FrTranscript()
    proof2, C2 = eval_prove(hg, d_Z.data_ptr(), ra, fr_array([Zr])[0], rnda, tr2, blinds=bl, blind_Zr=bz, ell=ell)
    assert _proof_dict(proof2) == ref and np.array_equal(C2, C_Zr) and _state(tr2) == end
    vt = FrTranscript()
    assert eval_verify(hg, ra, C_Zr, g1_array(comm), vt, proof)
    assert _state(vt) == end


def test_eval_prove_matches_fixture(ctx):
    import golden_io as G
    from testudo_amd.engine import dense_commit
    from testudo_amd.hyrax import FrTranscript, HyraxGens, dense_evaluate, eval_prove, eval_verify
    for d in G.load("hyrax_eval.json")["cases"]:
        c = H.load_case(d)
        hg = HyraxGens.setup(ctx, c["ell"], c["label"])
        assert _ref_gens(hg) == c["gens"]
        Z, r = fr_array(c["Z"]), fr_array(c["r"])
        assert limbs_to_int(dense_evaluate(ctx, Z, r)) == c["Zr"]
        comm = dense_commit(hg.gens, Z, fr_array(c["blinds"]))
        assert g1_from_array(comm) == c["comm"]
        tr = FrTranscript()
        proof, C_Zr = eval_prove(hg, Z, r, fr_array([c["Zr"]])[0], fr_array(c["rnd"]), tr,
                                 blinds=fr_array(c["blinds"]), blind_Zr=fr_array([c["blind_Zr"]])[0])
        assert _proof_dict(proof) == c["proof"]
        assert g1_from_array(C_Zr)[0] == c["C_Zr"]
        assert _state(tr) == c["transcript_end"]
        assert eval_verify(hg, r, C_Zr, comm, FrTranscript(), _proof_arrays(c["proof"]))
        hg.close()


# ---------------------------------------------------------- dot product ----
@pytest.mark.parametrize("n", [1, 2, 64])
def test_dotprod_random_a(ctx, n):
    """tpst_dotprod_*: a is any vector, not an eq table; n = 1 has zero rounds"""
    from testudo_amd.hyrax import FrTranscript, HyraxGens, dotprod_prove, dotprod_verify
    rng = random.Random(50 + n)
    fr = lambda: rng.randrange(1, R)  # noqa: E731
    hg = HyraxGens.new(ctx, n, b"dotprod")
    gens = _ref_gens(hg)
    lg = n.bit_length() - 1
    x, a = [fr() for _ in range(n)], [fr() for _ in range(n)]
    y, bx, by = H.inner(x, a), fr(), fr()
    rnd = [fr() for _ in range(3 + 4 * lg)]
    rt = H.Transcript()
    ref, Cx_ref, Cy_ref = H.dotprod_prove(gens, rt, x, bx, a, y, by, rnd, H.orc_msm)
    tr = FrTranscript()
    proof, Cx, Cy = dotprod_prove(hg, fr_array(x), fr_array([bx])[0], fr_array(a), fr_array([y])[0],
                                  fr_array([by])[0], fr_array(rnd), tr)
    assert len(proof.L) == lg
    assert _proof_dict(proof) == ref
    assert g1_from_array(Cx)[0] == Cx_ref and g1_from_array(Cy)[0] == Cy_ref
    assert _state(tr) == rt.state()
    vt = FrTranscript()
    assert dotprod_verify(hg, fr_array(a), Cx, Cy, vt, proof)
    assert _state(vt) == rt.state()
    a2 = list(a)
    a2[n - 1] = (a2[n - 1] + 1) % R
    assert not dotprod_verify(hg, fr_array(a2), Cx, Cy, FrTranscript(), proof)
    hg.close()


def test_dotprod_all_zero(ctx):
    """x = 0, zero blinds, rnd = 0: every point is infinity and every scalar row
    of the K1 launches is zero; it must prove and verify"""
    from testudo_amd.hyrax import FrTranscript, HyraxGens, dotprod_prove, dotprod_verify
    n, lg = 16, 4
    rng = random.Random(60)
    hg = HyraxGens.new(ctx, n, b"dotprod")
    a = [rng.randrange(1, R) for _ in range(n)]
    zero = np.zeros(4, dtype=np.uint64)
    rnd = np.zeros((3 + 4 * lg, 4), dtype=np.uint64)
    rt = H.Transcript()
    ref, Cx_ref, Cy_ref = H.dotprod_prove(_ref_gens(hg), rt, [0] * n, 0, a, 0, 0, [0] * (3 + 4 * lg))
    assert Cx_ref is None and Cy_ref is None and all(p is None for p in ref["L"] + ref["R"])
    tr = FrTranscript()
    proof, Cx, Cy = dotprod_prove(hg, np.zeros((n, 4), dtype=np.uint64), zero, fr_array(a), zero, zero, rnd, tr)
    assert not Cx.any() and not Cy.any() and not proof.L.any() and not proof.R.any()
    assert _proof_dict(proof) == ref and _state(tr) == rt.state()
    assert dotprod_verify(hg, fr_array(a), Cx, Cy, FrTranscript(), proof)
    hg.close()


# ------------------------------------------------------- bound: split pass --
def test_bound_split_shape(ctx):
    """ell = 14: L_size = 128 rows exceed the bound kernel's per-block tile of
    BOUND_TILE = 64 rows, so two blocks share every column and the partial-sum
    pass adds them.  Cx = commit(LZ, LZ_blind) is the first point the transcript
    absorbs (any difference changes every challenge); it is also checked as
    MSM(comm, L), which the verifier computes."""
    from testudo_amd.engine import dense_commit
    from testudo_amd.hyrax import FrTranscript, dense_evaluate, eval_prove, eval_verify
    ell = 14
    assert (1 << (ell // 2)) > BOUND_TILE
    hg = _gens(ctx, ell)
    gens = _ref_gens(hg)
    Za, _ = orc.fr_stream(1400, 1 << ell)
    Z = [limbs_to_int(z) for z in Za]
    _, r, blinds, blind_Zr, rnd = _inputs(ell, True)
    Zr = H.evaluate(Z, r)
    assert limbs_to_int(dense_evaluate(ctx, Za, fr_array(r))) == Zr
    L, _Rv = H.factored_evals(r)
    LZ, LZ_blind = H.bound(Z, L), H.inner(blinds, L)
    Cx_ref = H.orc_msm(gens[0] + [gens[1]], LZ + [LZ_blind])
    rt = H.Transcript()
    ref, C_ref = H.eval_prove(Z, blinds, r, Zr, blind_Zr, gens, rt, rnd, H.orc_msm)
    tr = FrTranscript()
    proof, C_Zr = eval_prove(hg, Za, fr_array(r), fr_array([Zr])[0], fr_array(rnd), tr, blinds=fr_array(blinds),
                             blind_Zr=fr_array([blind_Zr])[0])
    assert _proof_dict(proof) == ref and g1_from_array(C_Zr)[0] == C_ref and _state(tr) == rt.state()
    comm = dense_commit(hg.gens, Za, fr_array(blinds))
    assert g1_from_array(ctx.g1_msm(comm, fr_array(L)))[0] == Cx_ref
    assert eval_verify(hg, fr_array(r), C_Zr, comm, FrTranscript(), proof)


# -------------------------------------------------------- self-consistency --
def test_dense_evaluate_vs_python(ctx):
    from testudo_amd.hyrax import dense_evaluate
    ell = 10
    Z, r, _, _, _ = _inputs(ell, False, seed=3)
    assert limbs_to_int(dense_evaluate(ctx, fr_array(Z), fr_array(r))) == H.evaluate(Z, r)


def test_self_consistency_ell20(ctx):
    """R = 1024, the size of the reference's check_dotproductproof_log:
    dense_commit -> dense_evaluate -> prove -> verify -> verify_plain"""
    from testudo_amd.engine import dense_commit
    from testudo_amd.hyrax import FrTranscript, dense_evaluate, eval_prove, eval_verify, eval_verify_plain
    ell = 20
    hg = _gens(ctx, ell)
    assert hg.n == 1024
    Z, k = orc.fr_stream(2000, 1 << ell)
    r, k = orc.fr_stream(2000, ell, k)
    rnd, _ = orc.fr_stream(2000, 3 + 4 * 10, k)
    comm = dense_commit(hg.gens, Z)
    Zr = dense_evaluate(ctx, Z, r)
    pt, vt, vp = FrTranscript(), FrTranscript(), FrTranscript()
    proof, C_Zr = eval_prove(hg, Z, r, Zr, rnd, pt)
    assert len(proof.L) == 10
    assert eval_verify(hg, r, C_Zr, comm, vt, proof)
    assert eval_verify_plain(hg, r, Zr, comm, vp, proof)
    assert _state(vt) == _state(pt) == _state(vp)
    bad = Zr.copy()
    bad[0] ^= 1
    assert not eval_verify_plain(hg, r, bad, comm, FrTranscript(), proof)


# --------------------------------------------------------------- rejections --
def _non_subgroup_point():
    from serialize import _fq_sqrt
    x = 5
    while True:
        y = _fq_sqrt((x ** 3 + 1) % O.P)
        if y is not None and not O.g1_in_subgroup((x, y)):
            return (x, y)
        x += 1


def test_rejections(ctx):
    """every rejection is a return code: False (TPST_E_VERIFY) for what a verifier
    must refuse, TpstError for misuse (TPST_E_ARG / TPST_E_STATE)"""
    import dataclasses

    from testudo_amd import Gens, TpstError
    from testudo_amd.engine import dense_commit
    from testudo_amd.hyrax import (DotProductProof, FrTranscript, HyraxGens, eval_prove, eval_verify,
                                   eval_verify_plain)
    ell = 6
    hg = _gens(ctx, ell)
    Z, r, _, _, rnd = _inputs(ell, False, seed=9)
    Za, ra = fr_array(Z), fr_array(r)
    Zr = fr_array([H.evaluate(Z, r)])[0]
    comm = dense_commit(hg.gens, Za)
    proof, C_Zr = eval_prove(hg, Za, ra, Zr, fr_array(rnd), FrTranscript())
    ok = lambda p, r_=ra, c=comm, C=C_Zr: eval_verify(hg, r_, C, c, FrTranscript(), p)  # noqa: E731
    assert ok(proof)
    assert eval_verify_plain(hg, ra, Zr, comm, FrTranscript(), proof)
    other = g1_array([O.g1_mul(O.G1_GEN, 777)])[0]

    def with_(**kw):
        p = dataclasses.replace(proof, L=proof.L.copy(), R=proof.R.copy())
        for k, v in kw.items():
            if k in ("L", "R"):
                getattr(p, k)[v[0]] = v[1]
            else:
                setattr(p, k, v)
        return p

    z1p = fr_array([(limbs_to_int(proof.z1) + 1) % R])[0]
    z2p = fr_array([(limbs_to_int(proof.z2) + 1) % R])[0]
    for p in (with_(L=(0, other)), with_(L=(2, other)), with_(R=(0, other)), with_(R=(2, other)),
              with_(L=(1, proof.R[1])), with_(delta=other), with_(beta=other), with_(z1=z1p), with_(z2=z2p),
              with_(delta=np.zeros(12, dtype=np.uint64))):
        assert not ok(p)
    r2 = ra.copy()
    r2[3] = fr_array([(limbs_to_int(r2[3]) + 1) % R])[0]
    assert not ok(proof, r_=r2)
    comm2 = comm.copy()
    comm2[5] = other
    assert not ok(proof, c=comm2)
    assert not ok(proof, C=other)
    Zr2 = fr_array([(limbs_to_int(Zr) + 1) % R])[0]
    assert not eval_verify_plain(hg, ra, Zr2, comm, FrTranscript(), proof)
    # malformed elements: z1 >= r, an off-curve L[0], a non-subgroup delta, a
    # non-canonical coordinate, a malformed commitment row
    assert not ok(with_(z1=fr_array([R])[0]))
    off = proof.L[0].copy()
    off[6] ^= 1
    assert not ok(with_(L=(0, off)))
    ns = g1_array([_non_subgroup_point()])[0]
    assert not ok(with_(delta=ns))
    shifted = proof.beta.copy()
    xi = limbs_to_int(shifted[:6]) + O.P
    shifted[:6] = [(xi >> (64 * i)) & (2**64 - 1) for i in range(6)]
    assert not ok(with_(beta=shifted))
    comm3 = comm.copy()
    comm3[0] = ns
    assert not ok(proof, c=comm3)
    assert not ok(proof, C=ns)
    # rounds off by one
    assert not ok(dataclasses.replace(proof, rounds=len(proof.L) + 1))
    assert not ok(dataclasses.replace(proof, rounds=len(proof.L) - 1))
    assert not ok(DotProductProof(L=proof.L[:-1], R=proof.R[:-1], delta=proof.delta, beta=proof.beta, z1=proof.z1,
                                  z2=proof.z2))
    # misuse: generators of another size, generators without h, values >= r
    small = HyraxGens.setup(ctx, ell - 2, b"hyrax_eval")
    with pytest.raises(TpstError):
        eval_verify(small, ra, C_Zr, comm, FrTranscript(), proof)
    with pytest.raises(TpstError):
        eval_prove(small, Za, ra, Zr, fr_array(rnd), FrTranscript())
    noh = HyraxGens(ctx, Gens(ctx, hg.gens.G), hg.Q)
    with pytest.raises(TpstError):
        eval_verify(noh, ra, C_Zr, comm, FrTranscript(), proof)
    with pytest.raises(TpstError):
        eval_prove(noh, Za, ra, Zr, fr_array(rnd), FrTranscript())
    rbad = ra.copy()
    rbad[0] = fr_array([R])[0]
    with pytest.raises(TpstError):
        eval_verify(hg, rbad, C_Zr, comm, FrTranscript(), proof)
    rndbad = fr_array(rnd)
    rndbad[-1] = fr_array([R])[0]  # an unused pair is still range-checked
    with pytest.raises(TpstError):
        eval_prove(hg, Za, ra, Zr, rndbad, FrTranscript())
    small.close()
    assert ok(proof)  # the context still works after every refusal
