"""CPU tests of the Hyrax evaluation proof's restatement (tests/hyrax_ref.py)
and of the host Fr transcript of libtpst (tpst_transcript_fr_*): no GPU."""
import random

import numpy as np
import pytest

import bls377 as O
import hyrax_ref as H

R = O.R


@pytest.fixture(scope="module")
def cases():
    import golden_io as G
    return [H.load_case(d) for d in G.load("hyrax_eval.json")["cases"]]


def _case(ell, seed, blinded=True):
    rng = random.Random(seed)
    fr = lambda: rng.randrange(1, R)  # noqa: E731
    gens = H.setup_gens(ell, b"hyrax_ref_test")
    Rn = len(gens[0])
    Z = [fr() for _ in range(1 << ell)]
    r = [fr() for _ in range(ell)]
    blinds = [fr() for _ in range(1 << (ell // 2))] if blinded else None
    blind_Zr = fr() if blinded else 0
    rnd = [fr() for _ in range(3 + 4 * (Rn.bit_length() - 1))]
    return gens, Z, r, blinds, blind_Zr, rnd


def test_restatement_reproduces_fixture(cases):
    assert [c["ell"] for c in cases] == [3, 4]
    for c in cases:
        assert c["gens"] == H.setup_gens(c["ell"], c["label"])
        assert c["Zr"] == H.evaluate(c["Z"], c["r"])
        assert c["comm"] == H.commit_rows(c["Z"], c["blinds"], c["gens"])
        tr = H.Transcript()
        proof, C_Zr = H.eval_prove(c["Z"], c["blinds"], c["r"], c["Zr"], c["blind_Zr"], c["gens"], tr, c["rnd"])
        assert proof == c["proof"] and C_Zr == c["C_Zr"]
        assert tr.state() == c["transcript_end"]
        vt = H.Transcript()
        assert H.eval_verify(c["gens"], vt, c["r"], C_Zr, c["comm"], proof)
        assert vt.state() == c["transcript_end"]


@pytest.mark.parametrize("ell", [1, 2, 3, 4, 5, 6])
def test_prove_verify_accepts(ell):
    gens, Z, r, blinds, blind_Zr, rnd = _case(ell, 100 + ell, blinded=ell % 2 == 0)
    Zr = H.evaluate(Z, r)
    bl = blinds if blinds is not None else [0] * (1 << (ell // 2))
    comm = H.commit_rows(Z, bl, gens)
    proof, C_Zr = H.eval_prove(Z, blinds, r, Zr, blind_Zr, gens, H.Transcript(), rnd)
    assert len(proof["L"]) == ell - ell // 2
    assert H.eval_verify(gens, H.Transcript(), r, C_Zr, comm, proof)
    if not blind_Zr:
        assert H.eval_verify_plain(gens, H.Transcript(), r, Zr, comm, proof)
        assert not H.eval_verify_plain(gens, H.Transcript(), r, (Zr + 1) % R, comm, proof)


def test_wrong_value_and_tampered_fields_rejected():
    ell = 4
    gens, Z, r, blinds, blind_Zr, rnd = _case(ell, 200)
    Zr = H.evaluate(Z, r)
    comm = H.commit_rows(Z, blinds, gens)
    # a proof of a wrong evaluation does not verify
    bad, C_bad = H.eval_prove(Z, blinds, r, (Zr + 1) % R, blind_Zr, gens, H.Transcript(), rnd)
    assert not H.eval_verify(gens, H.Transcript(), r, C_bad, comm, bad)
    proof, C_Zr = H.eval_prove(Z, blinds, r, Zr, blind_Zr, gens, H.Transcript(), rnd)
    assert H.eval_verify(gens, H.Transcript(), r, C_Zr, comm, proof)
    other = O.g1_mul(O.G1_GEN, 12345)

    def tampered(**kw):
        p = dict(proof)
        p["L"], p["R"] = list(proof["L"]), list(proof["R"])
        for k, v in kw.items():
            if k in ("L", "R"):
                p[k][v[0]] = v[1]
            else:
                p[k] = v
        return p

    for p in (tampered(L=(0, other)), tampered(L=(1, other)), tampered(R=(0, other)), tampered(R=(1, other)),
              tampered(delta=other), tampered(beta=other), tampered(z1=(proof["z1"] + 1) % R),
              tampered(z2=(proof["z2"] + 1) % R)):
        assert not H.eval_verify(gens, H.Transcript(), r, C_Zr, comm, p)
    assert not H.eval_verify(gens, H.Transcript(), r, other, comm, proof)
    r2 = list(r)
    r2[1] = (r2[1] + 1) % R
    assert not H.eval_verify(gens, H.Transcript(), r2, C_Zr, comm, proof)
    comm2 = list(comm)
    comm2[2] = other
    assert not H.eval_verify(gens, H.Transcript(), r, C_Zr, comm2, proof)
    # one round short: n != 2^lg_n (bullet.rs:175)
    assert not H.eval_verify(gens, H.Transcript(), r, C_Zr, comm, dict(proof, L=proof["L"][:1], R=proof["R"][:1]))


@pytest.mark.parametrize("n", [1, 2, 8, 16])
def test_msm_by_s_is_the_folded_generator(n):
    """MSM(G, s) with verification_scalars' s equals the literally folded G[0]
    (bullet.rs:129 against :205-215) -- the identity the device's fixed-G
    schedule rests on: its weights w_final are this s."""
    rng = random.Random(300 + n)
    fr = lambda: rng.randrange(1, R)  # noqa: E731
    G, h, Q = H.dotprod_gens(n, b"fold")
    lg = n.bit_length() - 1
    tr = H.Transcript()
    Ls, Rs, _gam, _a, _b, g_hat, _bf = H.bullet_prove(tr, Q, G, h, [fr() for _ in range(n)], [fr() for _ in range(n)],
                                                      fr(), [(fr(), fr()) for _ in range(2 * lg)])
    _usq, _uisq, s = H.verification_scalars(Ls, Rs, n, H.Transcript())
    assert H.py_msm(G, s) == g_hat
    # the weight recurrence of the device schedule: w_{k+1}[2t] = w_k[t] / u, w_{k+1}[2t+1] = w_k[t] u
    vt, w = H.Transcript(), [1]
    for L, Rp in zip(Ls, Rs):
        vt.append_point(L)
        vt.append_point(Rp)
        u = vt.challenge()
        ui = pow(u, -1, R)
        w = [v for x in w for v in (x * ui % R, x * u % R)]
    assert w == s


def _limbs(v, n=4):
    return np.array([(v >> (64 * i)) & (2**64 - 1) for i in range(n)], dtype=np.uint64)


def test_fr_transcript_matches_sponge():
    """tpst_transcript_fr_* (host library only) against gens.FrSponge on a mixed
    flow: scalars, a point, the infinity point, bytes, squeezes between absorbs."""
    from testudo_amd.encoding import fr_array, g1_array, limbs_to_int
    from testudo_amd.hyrax import FrTranscript
    rng = random.Random(400)
    fr = lambda: rng.randrange(R)  # noqa: E731
    ref, tr = H.Transcript(), FrTranscript()

    def same():
        st, sq, idx = tr.state()
        assert ([limbs_to_int(x) for x in st], sq, idx) == ref.state()

    same()
    s0 = fr()
    ref.append_scalar(s0)
    tr.append_scalar(_limbs(s0))
    same()
    assert limbs_to_int(tr.challenge_scalar()) == ref.challenge()
    pt = O.g1_mul(O.G1_GEN, 0xABCDEF)
    ref.append_point(pt)
    tr.append_point(g1_array([pt])[0])
    same()
    vec = [fr() for _ in range(5)] + [0, R - 1]
    ref.append_scalars(vec)
    tr.append_scalars(fr_array(vec))
    same()
    assert limbs_to_int(tr.challenge_scalar()) == ref.challenge()
    assert limbs_to_int(tr.challenge_scalar()) == ref.challenge()
    assert limbs_to_int(tr.challenge_scalar()) == ref.challenge()  # third squeeze: a permutation in squeeze mode
    ref.append_point(None)
    tr.append_point(np.zeros(12, dtype=np.uint64))
    same()
    for data in (b"", b"testudo", bytes(range(31)), bytes(range(70))):
        ref.append_bytes(data)
        tr.append_bytes(data)
        same()
    assert limbs_to_int(tr.challenge_scalar()) == ref.challenge()
    same()
    # non-canonical input: a return code, the state untouched
    before = tr.state()
    with pytest.raises(ValueError):
        tr.append_scalar(_limbs(R))
    with pytest.raises(ValueError):
        tr.append_scalars(fr_array([1, R + 5]))
    bad = g1_array([pt])[0]
    bad[:6] = _limbs(pt[0] + O.P, 6)
    with pytest.raises(ValueError):
        tr.append_point(bad)
    after = tr.state()
    assert np.array_equal(before[0], after[0]) and before[1:] == after[1:]
