"""TEST INFRASTRUCTURE ONLY -- never imported by the product path.

First-principles restatement of the Hyrax evaluation proof: BulletReductionProof
(nizk/bullet.rs), DotProductProofLog (nizk/mod.rs) and PolyEvalProof
(dense_mlpoly.rs:473-575) over PoseidonTranscript<Fr> (poseidon_transcript.rs),
the checker of csrc/hyrax.hip.  Built on the oracle's curve arithmetic
(oracle/py/bls377.py), its Poseidon<Fr> sponge and generators (gens.py) and the
wire format (serialize.py) by import only.  G is folded literally every round,
as the reference does (bullet.rs:129); the device never folds it.

Points are affine tuples or None, scalars Python ints.  Every routine takes an
``msm(points, scalars) -> point`` callable (default: the pure-Python one), so
larger shapes can use the C++ oracle (``orc_msm``).

``python tests/hyrax_ref.py`` rewrites tests/golden/hyrax_eval.json.
Parity with arkworks is unpinned (no Rust toolchain): the restatement and the
verification equation pin the device code.
"""
from __future__ import annotations

import json
import os
import random
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.join(_ROOT, "oracle", "py"), os.path.join(_ROOT, "oracle", "cpu")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import bls377 as O  # noqa: E402
from gens import FrSponge, multi_commit_gens  # noqa: E402
from serialize import ser_g1  # noqa: E402

R = O.R


def orc_msm(points, scalars):
    """msm callable over the C++ CPU oracle."""
    import orc
    from testudo_amd.encoding import fr_array, g1_array, g1_from_array
    if not points:
        return None
    return g1_from_array(orc.g1_msm(g1_array(points), fr_array([s % R for s in scalars])))[0]


def py_msm(points, scalars):
    return O.g1_msm(list(points), [s % R for s in scalars])


# ------------------------------------------------------------ transcript --
class Transcript:
    """PoseidonTranscript<Fr> over poseidon_params() (poseidon_transcript.rs:38-47)."""

    def __init__(self):
        self.sp = FrSponge()

    def append_scalar(self, s):  # :73-75, a native absorb
        self.sp.absorb_elems([s % R])

    def append_scalars(self, v):  # append_scalar_vector :88-96
        for s in v:
            self.append_scalar(s)

    def append_point(self, p):  # :77-86, Compress::Yes bytes absorbed as Vec<u8>
        self.sp.absorb_bytes(ser_g1(p))

    def append_bytes(self, b):  # :69-71
        self.sp.absorb_bytes(bytes(b))

    def challenge(self):  # :30-32 squeeze_field_elements(1)
        return self.sp.squeeze_native(1)[0]

    def state(self):
        return list(self.sp.state), 1 if self.sp.mode == "squeeze" else 0, self.sp.idx


# ------------------------------------------------------------------ gens --
def setup_gens(num_vars, label):
    """PolyCommitmentGens::setup(num_vars, label).gens (dense_mlpoly.rs:185-187)."""
    return dotprod_gens(1 << (num_vars - num_vars // 2), label)


def dotprod_gens(n, label):
    """DotProductProofGens::new (nizk/mod.rs:25-28): MultiCommitGens::new(n + 1)
    split at n -> (G[0..n), h, Q = G[n])."""
    G, h = multi_commit_gens(n + 1, label)
    return G[:n], h, G[n]


def eq_evals(r):
    """EqPolynomial::evals (dense_mlpoly.rs:231-250), MSB-first."""
    ev = [1]
    for rj in r:
        ev = [v for e in ev for v in ((e * (1 - rj)) % R, (e * rj) % R)]
    return ev


def factored_evals(r):
    """compute_factored_evals (dense_mlpoly.rs:256-264)."""
    lv = len(r) // 2
    return eq_evals(r[:lv]), eq_evals(r[lv:])


def inner(a, b):
    return sum(x * y for x, y in zip(a, b)) % R


def commit_rows(Z, blinds, gens, msm=py_msm):
    """DensePolynomial::commit_inner (dense_mlpoly.rs:314-329)."""
    G, h, _ = gens
    Rn = len(Z) // len(blinds)
    return [msm(G + [h], Z[Rn * i:Rn * (i + 1)] + [blinds[i]]) for i in range(len(blinds))]


# ---------------------------------------------------------------- bullet --
def bullet_prove(tr, Q, G, H, a, b, blind, blinds_vec, msm=py_msm):
    """BulletReductionProof::prove (bullet.rs:36-152) ->
    (L_vec, R_vec, Gamma_hat, a_hat, b_hat, g_hat, blind_fin)."""
    G, a, b = list(G), [x % R for x in a], [x % R for x in b]
    n = len(G)
    assert n & (n - 1) == 0 and len(a) == n and len(b) == n
    assert len(blinds_vec) == 2 * (n.bit_length() - 1)  # bullet.rs:69
    Ls, Rs, it, blind_fin = [], [], iter(blinds_vec), blind % R
    while n != 1:
        n //= 2
        aL, aR, bL, bR, GL, GR = a[:n], a[n:], b[:n], b[n:], G[:n], G[n:]
        cL, cR = inner(aL, bR), inner(aR, bL)
        blL, blR = next(it)
        L = msm(GR + [Q, H], aL + [cL, blL])
        Rp = msm(GL + [Q, H], aR + [cR, blR])
        tr.append_point(L)
        tr.append_point(Rp)
        u = tr.challenge()
        ui = pow(u, -1, R)
        a = [(aL[i] * u + ui * aR[i]) % R for i in range(n)]
        b = [(bL[i] * ui + u * bR[i]) % R for i in range(n)]
        G = [O.g1_add(O.g1_mul(GL[i], ui), O.g1_mul(GR[i], u)) for i in range(n)]  # folded literally
        blind_fin = (blind_fin + u * u * blL + ui * ui * blR) % R
        Ls.append(L)
        Rs.append(Rp)
    Gamma_hat = msm([G[0], Q, H], [a[0], a[0] * b[0] % R, blind_fin])
    return Ls, Rs, Gamma_hat, a[0], b[0], G[0], blind_fin


def verification_scalars(Ls, Rs, n, tr):
    """bullet.rs:157-218 -> (u_sq, u_inv_sq, s) or None."""
    lg = len(Ls)
    if lg >= 32 or n != 1 << lg:
        return None
    ch = []
    for L, Rp in zip(Ls, Rs):
        tr.append_point(L)
        tr.append_point(Rp)
        ch.append(tr.challenge())
    if any(c == 0 for c in ch):
        return None
    inv = [pow(c, -1, R) for c in ch]
    allinv = 1
    for c in ch:
        allinv = allinv * c % R
    allinv = pow(allinv, -1, R)
    usq, uisq = [c * c % R for c in ch], [c * c % R for c in inv]
    s = [allinv]
    for i in range(1, n):
        lg_i = i.bit_length() - 1
        s.append(s[i - (1 << lg_i)] * usq[(lg - 1) - lg_i] % R)
    return usq, uisq, s


def bullet_verify(Ls, Rs, n, a, tr, Gamma, Gs, msm=py_msm):
    """bullet.rs:224-260 -> (G_hat, Gamma_hat, a_hat) or None."""
    vs = verification_scalars(Ls, Rs, n, tr)
    if vs is None:
        return None
    usq, uisq, s = vs
    return msm(list(Gs), s), msm(list(Ls) + list(Rs) + [Gamma], usq + uisq + [1]), inner(a, s)


# ------------------------------------------------------------ dot product --
def split_rnd(rnd, n):
    """the reference's draws in order (nizk/mod.rs:61-73): d, r_delta, r_beta,
    then 2 log2(n) pairs."""
    lg = n.bit_length() - 1
    assert len(rnd) == 3 + 4 * lg
    return rnd[0], rnd[1], rnd[2], [(rnd[3 + 2 * k], rnd[4 + 2 * k]) for k in range(2 * lg)]


def dotprod_prove(gens, tr, x, blind_x, a, y, blind_y, rnd, msm=py_msm):
    """DotProductProofLog::prove (nizk/mod.rs:45-125) -> (proof dict, Cx, Cy)."""
    G, h, Q = gens
    n = len(x)
    assert len(a) == n and len(G) == n
    d, r_delta, r_beta, blinds_vec = split_rnd(rnd, n)
    Cx = msm(G + [h], list(x) + [blind_x])
    tr.append_point(Cx)
    Cy = msm([Q, h], [y, blind_y])
    tr.append_point(Cy)
    tr.append_scalars(a)
    blind_Gamma = (blind_x + blind_y) % R
    Ls, Rs, _gam, x_hat, a_hat, g_hat, rhat = bullet_prove(tr, Q, G, h, x, a, blind_Gamma, blinds_vec, msm)
    y_hat = x_hat * a_hat % R
    delta = msm([g_hat, h], [d, r_delta])
    tr.append_point(delta)
    beta = msm([Q, h], [d, r_beta])
    tr.append_point(beta)
    c = tr.challenge()
    z1 = (d + c * y_hat) % R
    z2 = (a_hat * (c * rhat + r_beta) + r_delta) % R
    return {"L": Ls, "R": Rs, "delta": delta, "beta": beta, "z1": z1, "z2": z2}, Cx, Cy


def dotprod_verify(gens, tr, a, Cx, Cy, proof, msm=py_msm):
    """DotProductProofLog::verify (nizk/mod.rs:127-179) -> bool."""
    G, h, Q = gens
    n = len(G)
    assert len(a) == n
    tr.append_point(Cx)
    tr.append_point(Cy)
    tr.append_scalars(a)
    Gamma = O.g1_add(Cx, Cy)
    res = bullet_verify(proof["L"], proof["R"], n, a, tr, Gamma, G, msm)
    if res is None:
        return False
    g_hat, Gamma_hat, a_hat = res
    tr.append_point(proof["delta"])
    tr.append_point(proof["beta"])
    c = tr.challenge()
    lhs = O.g1_add(O.g1_mul(O.g1_add(O.g1_mul(Gamma_hat, c), proof["beta"]), a_hat), proof["delta"])
    rhs = O.g1_add(O.g1_mul(O.g1_add(g_hat, O.g1_mul(Q, a_hat)), proof["z1"]), O.g1_mul(h, proof["z2"]))
    return lhs == rhs


# ---------------------------------------------------------- PolyEvalProof --
def bound(Z, L):
    """DensePolynomial::bound (dense_mlpoly.rs:379-387)."""
    Rn = len(Z) // len(L)
    return [sum(L[j] * Z[j * Rn + i] for j in range(len(L))) % R for i in range(Rn)]


def evaluate(Z, r):
    """DensePolynomial::evaluate (dense_mlpoly.rs:408-414)."""
    return inner(Z, eq_evals(r))


def eval_prove(Z, blinds, r, Zr, blind_Zr, gens, tr, rnd, msm=py_msm):
    """PolyEvalProof::prove (dense_mlpoly.rs:482-534) -> (proof, C_Zr')."""
    L, Rv = factored_evals(r)
    assert len(Z) == 1 << len(r)
    blinds = [0] * len(L) if blinds is None else blinds
    assert len(blinds) == len(L)
    LZ = bound(Z, L)
    LZ_blind = inner(blinds, L)
    proof, _C_LR, C_Zr = dotprod_prove(gens, tr, LZ, LZ_blind, Rv, Zr, blind_Zr or 0, rnd, msm)
    return proof, C_Zr


def eval_verify(gens, tr, r, C_Zr, comm, proof, msm=py_msm):
    """PolyEvalProof::verify (dense_mlpoly.rs:536-560)."""
    L, Rv = factored_evals(r)
    C_LZ = msm(list(comm), L)
    return dotprod_verify(gens, tr, Rv, C_LZ, C_Zr, proof, msm)


def eval_verify_plain(gens, tr, r, Zr, comm, proof, msm=py_msm):
    """PolyEvalProof::verify_plain (dense_mlpoly.rs:562-574)."""
    return eval_verify(gens, tr, r, O.g1_mul(gens[2], Zr), comm, proof, msm)


# ----------------------------------------------------------------- fixture --
GOLDEN = os.path.join(_ROOT, "tests", "golden", "hyrax_eval.json")
LABEL = b"hyrax_eval"


def _hx(v):
    return "%x" % v


def _pt(p):
    return None if p is None else [_hx(p[0]), _hx(p[1])]


def pt_in(p):
    return None if p is None else (int(p[0], 16), int(p[1], 16))


def make_case(ell, seed):
    rng = random.Random(seed)
    fr = lambda: rng.randrange(1, R)  # noqa: E731
    gens = setup_gens(ell, LABEL)
    lv = ell // 2
    Rn = 1 << (ell - lv)
    Z = [fr() for _ in range(1 << ell)]
    r = [fr() for _ in range(ell)]
    blinds = [fr() for _ in range(1 << lv)]
    blind_Zr = fr()
    rnd = [fr() for _ in range(3 + 4 * (Rn.bit_length() - 1))]
    Zr = evaluate(Z, r)
    comm = commit_rows(Z, blinds, gens)
    tr = Transcript()
    proof, C_Zr = eval_prove(Z, blinds, r, Zr, blind_Zr, gens, tr, rnd)
    vt = Transcript()
    assert eval_verify(gens, vt, r, C_Zr, comm, proof)
    st, sq, idx = tr.state()
    assert vt.state() == tr.state()
    return {
        "ell": ell, "label": LABEL.decode(),
        "Z": [_hx(v) for v in Z], "r": [_hx(v) for v in r], "blinds": [_hx(v) for v in blinds],
        "blind_Zr": _hx(blind_Zr), "rnd": [_hx(v) for v in rnd], "Zr": _hx(Zr),
        "gens": {"G": [_pt(p) for p in gens[0]], "h": _pt(gens[1]), "Q": _pt(gens[2])},
        "comm": [_pt(p) for p in comm],
        "proof": {"L": [_pt(p) for p in proof["L"]], "R": [_pt(p) for p in proof["R"]],
                  "delta": _pt(proof["delta"]), "beta": _pt(proof["beta"]), "z1": _hx(proof["z1"]),
                  "z2": _hx(proof["z2"])},
        "C_Zr": _pt(C_Zr),
        "transcript_end": {"state": [_hx(v) for v in st], "squeezing": sq, "index": idx},
    }


def load_case(d):
    """fixture entry -> Python values"""
    g = d["gens"]
    pr = d["proof"]
    return {
        "ell": d["ell"], "label": d["label"].encode(),
        "Z": [int(v, 16) for v in d["Z"]], "r": [int(v, 16) for v in d["r"]],
        "blinds": [int(v, 16) for v in d["blinds"]], "blind_Zr": int(d["blind_Zr"], 16),
        "rnd": [int(v, 16) for v in d["rnd"]], "Zr": int(d["Zr"], 16),
        "gens": ([pt_in(p) for p in g["G"]], pt_in(g["h"]), pt_in(g["Q"])),
        "comm": [pt_in(p) for p in d["comm"]],
        "proof": {"L": [pt_in(p) for p in pr["L"]], "R": [pt_in(p) for p in pr["R"]], "delta": pt_in(pr["delta"]),
                  "beta": pt_in(pr["beta"]), "z1": int(pr["z1"], 16), "z2": int(pr["z2"], 16)},
        "C_Zr": pt_in(d["C_Zr"]),
        "transcript_end": ([int(v, 16) for v in d["transcript_end"]["state"]], d["transcript_end"]["squeezing"],
                           d["transcript_end"]["index"]),
    }


if __name__ == "__main__":
    out = {"cases": [make_case(3, 0x4859_0003), make_case(4, 0x4859_0004)]}
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
