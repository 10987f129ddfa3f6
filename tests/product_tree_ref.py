"""TEST INFRASTRUCTURE ONLY -- never imported by the product path.

First-principles restatement of the memory-checking grand-product argument of
product_tree.rs: ProductCircuit, DotProductCircuit and
ProductCircuitEvalProofBatched::{prove, verify}, driven by
SumcheckInstanceProof::{prove_cubic_batched, verify} (sumcheck.rs) over
PoseidonTranscript<Fr> -- the checker of csrc/product_tree.hip.  Scalars are
Python ints; the transcript and the eq table are hyrax_ref's.

A circuit is a list of layers [(left, right), ...], layer 0 first.  A proof is
{"layers": [{"polys": [[c0, c1, c2, c3], ...], "left": [...], "right": [...]}],
 "dotp": (left, right, weight)} in the reference's push order: layer proof i
has i rounds.

``python tests/product_tree_ref.py`` rewrites tests/golden/product_tree.json.
Parity with arkworks is unpinned (no Rust toolchain): the restatement and the
verifier's equations pin the device code.
"""
from __future__ import annotations

import json
import os
import random
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import hyrax_ref as H  # noqa: E402
from hyrax_ref import Transcript, eq_evals  # noqa: E402,F401

R = H.R


# --------------------------------------------------------------- circuits --
def compute_layer(left, right):
    """ProductCircuit::compute_layer (product_tree.rs:19-34)."""
    ln = len(left) + len(right)
    return ([left[i] * right[i] % R for i in range(ln // 4)],
            [left[i] * right[i] % R for i in range(ln // 4, ln // 2)])


def product_circuit(poly):
    """ProductCircuit::new (product_tree.rs:36-56): layer 0 = (first half,
    second half) of the input, log2(len) layers in all."""
    n = len(poly)
    assert n >= 2 and n & (n - 1) == 0
    layers = [([v % R for v in poly[:n // 2]], [v % R for v in poly[n // 2:]])]
    for i in range(n.bit_length() - 2):
        layers.append(compute_layer(*layers[i]))
    return layers


def circuit_evaluate(layers):
    """ProductCircuit::evaluate (product_tree.rs:58-63)."""
    left, right = layers[-1]
    assert len(left) == 1 and len(right) == 1
    return left[0] * right[0] % R


def dotp_evaluate(left, right, weight):
    """DotProductCircuit::evaluate (product_tree.rs:87-91)."""
    return sum(a * b * c for a, b, c in zip(left, right, weight)) % R


def dotp_split(left, right, weight):
    """DotProductCircuit::split (product_tree.rs:93-111)."""
    h = len(left) // 2
    assert 2 * h == len(left)
    return (left[:h], right[:h], weight[:h]), (left[h:], right[h:], weight[h:])


# ---------------------------------------------------------------- unipoly --
def from_evals(e):
    """UniPoly::from_evals (unipoly.rs:21-52), 4 evaluations -> [d, c, b, a]."""
    assert len(e) == 4
    two_inv, six_inv = pow(2, -1, R), pow(6, -1, R)
    d = e[0]
    a = six_inv * (e[3] - 3 * e[2] + 3 * e[1] - e[0]) % R
    b = two_inv * (2 * e[0] - 5 * e[1] + 4 * e[2] - e[3]) % R
    c = (e[1] - d - a - b) % R
    return [d % R, c, b, a]


def uni_eval(cs, r):
    """UniPoly::evaluate (unipoly.rs:66-74)."""
    out, pw = cs[0], r
    for c in cs[1:]:
        out = (out + pw * c) % R
        pw = pw * r % R
    return out


def bound_top(Z, r):
    """DensePolynomial::bound_poly_var_top (dense_mlpoly.rs:389-397)."""
    n = len(Z) // 2
    return [(Z[i] + r * (Z[i + n] - Z[i])) % R for i in range(n)]


# -------------------------------------------------------------- sum-check --
def _cubic_evals(A, B, C):
    """the three sums of one instance (sumcheck.rs:252-283): t = 0, 2, 3"""
    ln = len(A) // 2
    e0 = e2 = e3 = 0
    for i in range(ln):
        e0 += A[i] * B[i] * C[i]
        a2, b2, c2 = 2 * A[ln + i] - A[i], 2 * B[ln + i] - B[i], 2 * C[ln + i] - C[i]
        e2 += a2 * b2 * c2
        a3, b3, c3 = a2 + A[ln + i] - A[i], b2 + B[ln + i] - B[i], c2 + C[ln + i] - C[i]
        e3 += a3 * b3 * c3
    return e0 % R, e2 % R, e3 % R


def prove_cubic_batched(claim, num_rounds, par, seq, coeffs, tr):
    """SumcheckInstanceProof::prove_cubic_batched (sumcheck.rs:220-385).
    par = (A_vec, B_vec, C) sharing C; seq = (A_vec, B_vec, C_vec).  The tables
    are rebound, not modified.  -> (polys, r, (A finals, B finals, C final),
    (A, B, C finals of seq))."""
    A_par, B_par, C_par = [list(a) for a in par[0]], [list(b) for b in par[1]], list(par[2])
    A_seq, B_seq, C_seq = ([list(x) for x in v] for v in seq)
    e, r, polys = claim % R, [], []
    for _j in range(num_rounds):
        evals = [_cubic_evals(A, B, C_par) for A, B in zip(A_par, B_par)]
        evals += [_cubic_evals(A, B, C) for A, B, C in zip(A_seq, B_seq, C_seq)]
        comb = [sum(ev[k] * coeffs[i] for i, ev in enumerate(evals)) % R for k in range(3)]
        poly = from_evals([comb[0], (e - comb[0]) % R, comb[1], comb[2]])
        for c in poly:  # write_to_transcript (unipoly.rs:102-108)
            tr.append_scalar(c)
        r_j = tr.challenge()
        r.append(r_j)
        A_par = [bound_top(A, r_j) for A in A_par]
        B_par = [bound_top(B, r_j) for B in B_par]
        C_par = bound_top(C_par, r_j)
        A_seq = [bound_top(A, r_j) for A in A_seq]
        B_seq = [bound_top(B, r_j) for B in B_seq]
        C_seq = [bound_top(C, r_j) for C in C_seq]
        e = uni_eval(poly, r_j)
        polys.append(poly)
    return (polys, r, ([A[0] for A in A_par], [B[0] for B in B_par], C_par[0]),
            ([A[0] for A in A_seq], [B[0] for B in B_seq], [C[0] for C in C_seq]))


def sumcheck_verify(polys, claim, num_rounds, degree_bound, tr):
    """SumcheckInstanceProof::verify (sumcheck.rs:29-63) -> (e, r) or None."""
    e, r = claim % R, []
    if len(polys) != num_rounds:
        return None
    for poly in polys:
        if len(poly) - 1 != degree_bound:
            return None
        if (poly[0] + sum(poly)) % R != e:  # G(0) + G(1) = e
            return None
        for c in poly:
            tr.append_scalar(c)
        r_i = tr.challenge()
        r.append(r_i)
        e = uni_eval(poly, r_i)
    return e, r


# ----------------------------------------- ProductCircuitEvalProofBatched --
def challenge_vec(tr, n):
    """challenge_scalar_vec (transcript.rs:11-13): n single squeezes."""
    return [tr.challenge() for _ in range(n)]


def prove(circuits, dotps, tr):
    """ProductCircuitEvalProofBatched::prove (product_tree.rs:255-377).
    circuits: product circuits of one size; dotps: (left, right, weight)
    triples of half the input length -> (proof, rand)."""
    assert circuits
    num_layers = len(circuits[0])
    claims_to_verify = [circuit_evaluate(c) for c in circuits]
    claims_dotp_final = ([], [], [])
    layers, rand = [], []
    for layer_id in reversed(range(num_layers)):
        ln = len(circuits[0][layer_id][0]) + len(circuits[0][layer_id][1])
        poly_C = eq_evals(rand)
        assert len(poly_C) == ln // 2
        num_rounds = len(poly_C).bit_length() - 1
        par = ([c[layer_id][0] for c in circuits], [c[layer_id][1] for c in circuits], poly_C)
        seq = ([], [], [])
        if layer_id == 0 and dotps:
            for left, right, weight in dotps:
                claims_to_verify.append(dotp_evaluate(left, right, weight))
                assert len(left) == len(right) == len(weight) == ln // 2
            seq = ([d[0] for d in dotps], [d[1] for d in dotps], [d[2] for d in dotps])
        coeffs = challenge_vec(tr, len(claims_to_verify))
        claim = sum(c * k for c, k in zip(claims_to_verify, coeffs)) % R
        polys, rand_prod, (cl, cr, _ceq), cdotp = prove_cubic_batched(claim, num_rounds, par, seq, coeffs, tr)
        for a, b in zip(cl, cr):
            tr.append_scalar(a)
            tr.append_scalar(b)
        if layer_id == 0 and dotps:
            for a, b, c in zip(*cdotp):
                tr.append_scalar(a)
                tr.append_scalar(b)
                tr.append_scalar(c)
            claims_dotp_final = cdotp
        r_layer = tr.challenge()
        claims_to_verify = [(a + r_layer * (b - a)) % R for a, b in zip(cl, cr)]
        rand = [r_layer] + rand_prod
        layers.append({"polys": polys, "left": cl, "right": cr})
    return {"layers": layers, "dotp": tuple(list(v) for v in claims_dotp_final)}, rand


def verify(proof, claims_prod, claims_dotp, ln, tr):
    """ProductCircuitEvalProofBatched::verify (product_tree.rs:379-476); ln =
    the circuits' input length.  -> (claims, claims_dotp triples, rand), or
    False where the reference asserts."""
    num_layers = ln.bit_length() - 1
    layers = proof["layers"]
    if len(layers) != num_layers:
        return False
    P = len(claims_prod)
    rand = []
    claims_to_verify = [c % R for c in claims_prod]
    claims_to_verify_dotp = []
    for num_rounds, i in enumerate(range(num_layers)):
        last = i == num_layers - 1
        if last:
            claims_to_verify = claims_to_verify + [c % R for c in claims_dotp]
        coeffs = challenge_vec(tr, len(claims_to_verify))
        claim = sum(c * k for c, k in zip(claims_to_verify, coeffs)) % R
        res = sumcheck_verify(layers[i]["polys"], claim, num_rounds, 3, tr)
        if res is None:
            return False
        claim_last, rand_prod = res
        cl, cr = layers[i]["left"], layers[i]["right"]
        if len(cl) != P or len(cr) != P:
            return False
        for a, b in zip(cl, cr):
            tr.append_scalar(a)
            tr.append_scalar(b)
        if len(rand) != len(rand_prod):
            return False
        eq = 1
        for x, y in zip(rand, rand_prod):
            eq = eq * (x * y + (1 - x) * (1 - y)) % R
        expected = sum(coeffs[k] * (cl[k] * cr[k] % R * eq) for k in range(P)) % R
        dl, dr, dw = proof["dotp"]
        if last:
            for k in range(len(dl)):
                tr.append_scalar(dl[k])
                tr.append_scalar(dr[k])
                tr.append_scalar(dw[k])
                if k + P >= len(coeffs):  # the reference's index panics
                    return False
                expected = (expected + coeffs[k + P] * dl[k] * dr[k] * dw[k]) % R
        if expected != claim_last:
            return False
        r_layer = tr.challenge()
        claims_to_verify = [(a + r_layer * (b - a)) % R for a, b in zip(cl, cr)]
        if last:
            if len(claims_dotp) > len(dl):
                return False
            for k in range(len(claims_dotp) // 2):
                for v in (dl, dr, dw):
                    claims_to_verify_dotp.append((v[2 * k] + r_layer * (v[2 * k + 1] - v[2 * k])) % R)
        rand = [r_layer] + rand_prod
    return claims_to_verify, claims_to_verify_dotp, rand


# ----------------------------------------------------------------- fixture --
GOLDEN = os.path.join(os.path.dirname(_HERE), "tests", "golden", "product_tree.json")


def _hx(v):
    return "%x" % v


def _hxs(v):
    return [_hx(x) for x in v]


def _ints(v):
    return [int(x, 16) for x in v]


def random_inputs(ell, P, D, seed, special=False):
    """polys: P x 2^ell; dotp: D split circuits (left, right, weight) of
    2^(ell-1): circuits 2k, 2k + 1 are the halves of one unsplit triple.
    special: 0, 1 and r - 1 among the entries (never 0 in a product input)."""
    rng = random.Random(seed)
    fr = lambda: rng.randrange(1, R)  # noqa: E731
    n = 1 << ell
    polys = [[fr() for _ in range(n)] for _ in range(P)]
    assert D % 2 == 0
    whole = [tuple([fr() for _ in range(n)] for _ in range(3)) for _ in range(D // 2)]
    if special:
        polys[0][0], polys[0][n - 1] = 1, R - 1
        polys[-1][n // 2] = R - 1
        for w in whole:
            w[0][0], w[1][0], w[2][n - 1] = 0, 1, R - 1
            w[1][n // 2], w[2][0] = R - 1, 0
    dotps = [t for w in whole for t in dotp_split(*w)]
    return polys, dotps, whole


def run(polys, dotps):
    """prove, then verify on a fresh transcript -> the case's values"""
    circuits = [product_circuit(p) for p in polys]
    claims_prod = [circuit_evaluate(c) for c in circuits]
    claims_dotp = [dotp_evaluate(*d) for d in dotps]
    tr = Transcript()
    proof, rand = prove(circuits, dotps, tr)
    vt = Transcript()
    res = verify(proof, claims_prod, claims_dotp, len(polys[0]), vt)
    assert res is not False and res[2] == rand and vt.state() == tr.state()
    return {"claims_prod": claims_prod, "claims_dotp": claims_dotp, "proof": proof, "rand": rand,
            "claims_out": res[0], "claims_dotp_out": res[1], "transcript_end": tr.state()}


def make_case(ell, P, D, seed):
    polys, dotps, _whole = random_inputs(ell, P, D, seed)
    v = run(polys, dotps)
    st, sq, idx = v["transcript_end"]
    pr = v["proof"]
    return {
        "ell": ell, "P": P, "D": D,
        "polys": [_hxs(p) for p in polys],
        "dotp": [{"left": _hxs(d[0]), "right": _hxs(d[1]), "weight": _hxs(d[2])} for d in dotps],
        "claims_prod": _hxs(v["claims_prod"]), "claims_dotp": _hxs(v["claims_dotp"]),
        "proof": {"layers": [{"polys": [_hxs(p) for p in L["polys"]], "left": _hxs(L["left"]),
                              "right": _hxs(L["right"])} for L in pr["layers"]],
                  "dotp": {"left": _hxs(pr["dotp"][0]), "right": _hxs(pr["dotp"][1]),
                           "weight": _hxs(pr["dotp"][2])}},
        "rand": _hxs(v["rand"]), "claims_out": _hxs(v["claims_out"]), "claims_dotp_out": _hxs(v["claims_dotp_out"]),
        "transcript_end": {"state": _hxs(st), "squeezing": sq, "index": idx},
    }


def load_case(d):
    """fixture entry -> Python values"""
    pr = d["proof"]
    return {
        "ell": d["ell"], "P": d["P"], "D": d["D"],
        "polys": [_ints(p) for p in d["polys"]],
        "dotp": [(_ints(t["left"]), _ints(t["right"]), _ints(t["weight"])) for t in d["dotp"]],
        "claims_prod": _ints(d["claims_prod"]), "claims_dotp": _ints(d["claims_dotp"]),
        "proof": {"layers": [{"polys": [_ints(p) for p in L["polys"]], "left": _ints(L["left"]),
                              "right": _ints(L["right"])} for L in pr["layers"]],
                  "dotp": (_ints(pr["dotp"]["left"]), _ints(pr["dotp"]["right"]), _ints(pr["dotp"]["weight"]))},
        "rand": _ints(d["rand"]), "claims_out": _ints(d["claims_out"]), "claims_dotp_out": _ints(d["claims_dotp_out"]),
        "transcript_end": (_ints(d["transcript_end"]["state"]), d["transcript_end"]["squeezing"],
                           d["transcript_end"]["index"]),
    }


# --------------------------------------------- the C ABI's flat proof order --
def proof_len(ell, P, D):
    """Fr count of the flat proof (include/tpst.h tpst_prodcircuit_proof_len)."""
    return 4 * (ell * (ell - 1) // 2) + 2 * ell * P + 3 * D


def flatten(proof, ell, P, D):
    """round polynomials (layer proof i: i rounds x 4 coefficients, constant
    first), then ell x P left claims, ell x P right claims, then the 3 x D
    final dot-product claims (left, right, weight)."""
    out = [c for L in proof["layers"] for p in L["polys"] for c in p]
    out += [c for L in proof["layers"] for c in L["left"]]
    out += [c for L in proof["layers"] for c in L["right"]]
    for v in proof["dotp"]:
        out += list(v)
    assert len(out) == proof_len(ell, P, D)
    return out


def unflatten(flat, ell, P, D):
    flat = list(flat)
    assert len(flat) == proof_len(ell, P, D)
    npoly = ell * (ell - 1) // 2
    layers, o = [], 0
    for i in range(ell):
        layers.append({"polys": [flat[o + 4 * k:o + 4 * k + 4] for k in range(i)]})
        o += 4 * i
    for i in range(ell):
        layers[i]["left"] = flat[4 * npoly + i * P:4 * npoly + (i + 1) * P]
        layers[i]["right"] = flat[4 * npoly + ell * P + i * P:4 * npoly + ell * P + (i + 1) * P]
    o = 4 * npoly + 2 * ell * P
    return {"layers": layers, "dotp": (flat[o:o + D], flat[o + D:o + 2 * D], flat[o + 2 * D:o + 3 * D])}


if __name__ == "__main__":
    out = {"cases": [make_case(3, 2, 2, 0x5054_0003)]}
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
