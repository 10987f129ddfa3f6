"""CPU tests of the multi-point opening's definition (tests/pst_multi_ref.py)
and of the host-only verifier half tpst_pst_multi_reduce:

* the restatement against brute force at n = 4, B = 2, K = 3: every round's
  s(0) + s(1) is the full sum of the tables, u_j = f_j(rho) by the oracle's
  Polynomial.eval, the final identity holds; and once through the oracle's
  pairing, end to end;
* tpst_pst_multi_reduce through ctypes against the restatement's proofs: the
  same rho and the same transcript bytes at n = 4..7 x four (B, K) shapes;
  TPST_E_VERIFY with the transcript untouched for every tamper; TPST_E_ARG for
  misuse.

Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import bls377 as O
import golden_io as G
import pst as P
import pst_multi_ref as MR
from testudo_amd.encoding import fr_array, gt_array, limbs_to_int, ptr

R = O.R
OK, E_ARG, E_VERIFY = 0, -1, -5
SHAPES = [(1, 1), (1, 3), (2, 2), (3, 5)]


def _golden_gts():
    d = G.load("sqrt_pst_n4.json")
    towers = [G.gt(d["T"])] + [G.gt(t) for pair in d["comms_t"] for t in pair]
    return [O.fq12_from_tower(t) for t in towers]


_GTS = None


def gts(B):
    global _GTS
    if _GTS is None:
        _GTS = _golden_gts()
    return _GTS[:B]


def gt_limbs(f):
    return gt_array(O.fq12_to_tower(f)).reshape(72)


def make_case(n, B, K, seed=0x3A17):
    """B random tables, K claims with true values: claim k is on polynomial k mod B; with K > B the last
    claim repeats the point of claim 0 (a repeated point, and for B = 1 a repeated claim)"""
    k = 0
    Zs = []
    for _ in range(B):
        Z, k = P.fr_stream(seed + 64 * n + 8 * B + K, 1 << n, k)
        Zs.append(Z)
    claims = []
    for c in range(K):
        point, k = P.fr_stream(seed + 64 * n + 8 * B + K, n, k)
        if K > B and c == K - 1:
            point = list(claims[0][1])
        claims.append((c % B, point, P.dense_evaluate(Zs[c % B], point)))
    return Zs, claims


def ref_start():
    """a transcript mid-protocol: something absorbed, one challenge squeezed"""
    tr = P.PoseidonTranscript()
    tr.append_gt(gts(5)[4])
    tr.challenge_scalar()
    return tr


def lib_start():
    from testudo_amd.sqrt_pst import PoseidonTranscript
    tr = PoseidonTranscript()
    tr.append_gt(gt_limbs(gts(5)[4]))
    tr.challenge_scalar()
    return tr


def raw_reduce(tr, n, claims, Ts, rounds, u, B=None, K=None, null=None):
    """tpst_pst_multi_reduce on integers -> (rc, rho ints).  B / K override the counts handed over; null names
    one pointer argument to pass as NULL."""
    from testudo_amd import _lib
    from testudo_amd.sqrt_pst import _ptr_array
    lib = _lib.load()
    idx = np.ascontiguousarray([j for j, _, _ in claims], dtype=np.uint32)
    pts = fr_array([x for _, p, _ in claims for x in p])
    vals = fr_array([v for _, _, v in claims])
    tl = [gt_limbs(T) if not isinstance(T, np.ndarray) else T for T in Ts]
    rd = fr_array([c for cs in rounds for c in cs])
    ua = fr_array(u)
    rho = np.zeros((max(n, 1), 4), dtype=np.uint64)
    args = {"tr": C.byref(tr.t), "Ts": _ptr_array(tl), "idx": idx.ctypes.data_as(C.POINTER(C.c_uint32)),
            "pts": ptr(pts), "vals": ptr(vals), "rounds": ptr(rd), "u": ptr(ua), "rho": ptr(rho)}
    if null is not None:
        args[null] = None
    rc = lib.tpst_pst_multi_reduce(args["tr"], n, args["Ts"], len(tl) if B is None else B, args["idx"], args["pts"],
                                   args["vals"], len(claims) if K is None else K, args["rounds"], args["u"],
                                   args["rho"])
    return rc, [limbs_to_int(x) for x in rho]


# ------------------------------------------------------------ brute force ----
def test_restatement_against_brute_force_n4_b2_k3():
    n, B, K = 4, 2, 3
    Zs, claims = make_case(n, B, K)
    trace = []
    tr = ref_start()
    rounds, u, rho = MR.prove_reduction(tr, n, Zs, claims, gts(B), trace)
    assert len(rounds) == n and len(trace) == n
    for e, total, s0, s1, s2 in trace:
        assert (s0 + s1) % R == e == total          # e_i is the full sum of the bound tables
    for Z, uj in zip(Zs, u):
        assert P.Polynomial(Z).eval(rho) == uj      # the oracle's own evaluation
    # the final identity, with D_j(rho) from the definition of eq
    a = MR.absorb_statement(ref_start(), n, B, claims, gts(B))
    e_n = MR.uni_eval(rounds[-1], rho[-1])
    Drho = [sum(ak * MR.eq_at(p, rho) for ak, (j, p, _) in zip(a, claims) if j == jj) % R for jj in range(B)]
    assert sum(x * y for x, y in zip(u, Drho)) % R == e_n
    # and the restated verifier agrees, with the prover's transcript
    tv = ref_start()
    assert MR.verify_reduction(tv, n, B, claims, gts(B), rounds, u) == rho
    assert MR.transcript_bytes(tv) == MR.transcript_bytes(tr)
    # a wrong claimed value is not provable: the honest prover's rounds fail the final identity
    bad = [claims[0], (claims[1][0], claims[1][1], (claims[1][2] + 1) % R), claims[2]]
    rb, ub, _ = MR.prove_reduction(ref_start(), n, Zs, bad, gts(B))
    assert MR.verify_reduction(ref_start(), n, B, bad, gts(B), rb, ub) is None


def test_eval_order_is_the_msb_first_chi_sum():
    """Polynomial.eval of the oracle equals sum_x Z[x] eq(r, x) with r[0] the most significant bit (n = 4, 5)"""
    for n in (4, 5):
        Zs, claims = make_case(n, 1, 1, 0x3A18)
        assert P.Polynomial(Zs[0]).eval(claims[0][1]) == claims[0][2]


def test_whole_protocol_on_the_oracle_n4_b2_k3():
    """prover and verifier restated end to end over the oracle's commitments and pairing (one size: slow)"""
    n, B, K = 4, 2, 3
    srs = P.SRS(2)
    Zs, claims = make_case(n, B, K, 0x3A19)
    commitments = [P.Polynomial(Z).commit(srs) for Z in Zs]
    Ts = [T for _, T in commitments]
    tp = P.PoseidonTranscript()
    proof, rho, _ = MR.prove(srs, tp, Zs, commitments, claims)
    tv = P.PoseidonTranscript()
    assert MR.verify(srs, tv, n, claims, Ts, proof)
    assert MR.transcript_bytes(tv) == MR.transcript_bytes(tp)
    bad = list(claims)
    bad[2] = (bad[2][0], bad[2][1], (bad[2][2] + 1) % R)
    assert not MR.verify(srs, P.PoseidonTranscript(), n, bad, Ts, proof)


# ------------------------------------------------ tpst_pst_multi_reduce -------
@pytest.mark.parametrize("n", [4, 5, 6, 7])
@pytest.mark.parametrize("B,K", SHAPES)
def test_multi_reduce_matches_restatement(n, B, K):
    Zs, claims = make_case(n, B, K)
    ref = ref_start()
    rounds, u, rho = MR.prove_reduction(ref, n, Zs, claims, gts(B))
    lib = lib_start()
    assert bytes(lib.t) == MR.transcript_bytes(ref_start())
    rc, got = raw_reduce(lib, n, claims, gts(B), rounds, u)
    assert rc == OK
    assert got == rho
    assert bytes(lib.t) == MR.transcript_bytes(ref)
    assert limbs_to_int(lib.challenge_scalar()) == ref.challenge_scalar()


def test_multi_reduce_python_wrapper():
    from testudo_amd.sqrt_pst import multi_reduce
    n, B, K = 5, 2, 2
    Zs, claims = make_case(n, B, K)
    ref = ref_start()
    rounds, u, rho = MR.prove_reduction(ref, n, Zs, claims, gts(B))
    cl = [(j, fr_array(p), fr_array([v])[0]) for j, p, v in claims]
    tl = [gt_limbs(T) for T in gts(B)]
    rd = fr_array([c for cs in rounds for c in cs]).reshape(n, 3, 4)
    lib = lib_start()
    got = multi_reduce(lib, n, cl, tl, rd, fr_array(u))
    assert [limbs_to_int(x) for x in got] == rho and bytes(lib.t) == MR.transcript_bytes(ref)
    ub = fr_array(u)
    ub[1, 0] ^= np.uint64(1)
    lib = lib_start()
    assert multi_reduce(lib, n, cl, tl, rd, ub) is None and bytes(lib.t) == MR.transcript_bytes(ref_start())


def _tamper_case():
    n, B, K = 5, 3, 5
    Zs, claims = make_case(n, B, K)
    rounds, u, rho = MR.prove_reduction(ref_start(), n, Zs, claims, gts(B))
    return n, B, K, claims, rounds, u


def test_multi_reduce_rejects_every_tamper():
    n, B, K, claims, rounds, u = _tamper_case()
    Ts = gts(B)
    start = bytes(lib_start().t)

    def rejected(claims=claims, Ts=Ts, rounds=rounds, u=u):
        tr = lib_start()
        rc, _ = raw_reduce(tr, n, claims, Ts, rounds, u)
        return rc == E_VERIFY and bytes(tr.t) == start

    tr = lib_start()
    assert raw_reduce(tr, n, claims, Ts, rounds, u)[0] == OK and bytes(tr.t) != start
    for i in (0, n // 2, n - 1):                       # first, a middle, the last round
        for c in range(3):
            rd = [list(cs) for cs in rounds]
            rd[i][c] = (rd[i][c] + 1) % R
            assert rejected(rounds=rd), (i, c)
    for j in range(B):
        ub = list(u)
        ub[j] = (ub[j] + 1) % R
        assert rejected(u=ub), j
    for k in range(K):
        cb = list(claims)
        cb[k] = (cb[k][0], cb[k][1], (cb[k][2] + 1) % R)
        assert rejected(claims=cb), k
    cb = list(claims)
    pt = list(cb[2][1])
    pt[3] = (pt[3] + 1) % R
    cb[2] = (cb[2][0], pt, cb[2][2])
    assert rejected(claims=cb)                         # one coordinate
    assert claims[0] != claims[1]
    assert rejected(claims=[claims[1], claims[0]] + claims[2:])   # two claims swapped
    cb = list(claims)
    assert cb[3][0] == 0 and cb[0][0] == 0
    cb[3] = (1, cb[3][1], cb[3][2])
    assert rejected(claims=cb)                         # a changed polynomial index (every polynomial still claimed)
    assert rejected(Ts=[Ts[0], gts(5)[3], Ts[2]])      # a changed T_j
    # a value >= r in each scalar field, a T coefficient >= p
    cb = list(claims)
    cb[1] = (cb[1][0], cb[1][1], R)
    assert rejected(claims=cb)
    cb = list(claims)
    cb[4] = (cb[4][0], [R + 1] + list(cb[4][1][1:]), cb[4][2])
    assert rejected(claims=cb)
    rd = [list(cs) for cs in rounds]
    rd[1][2] = R
    assert rejected(rounds=rd)
    assert rejected(u=[u[0], 2**256 - 1, u[2]])
    big = gt_limbs(Ts[1]).copy()
    big[5] = np.uint64(2**64 - 1)
    assert rejected(Ts=[Ts[0], big, Ts[2]])


def test_multi_reduce_misuse():
    n, B, K, claims, rounds, u = _tamper_case()
    Ts = gts(B)
    start = bytes(lib_start().t)

    def misuse(**kw):
        tr = lib_start()
        args = dict(claims=claims, Ts=Ts, rounds=rounds, u=u)
        extra = {k: kw.pop(k) for k in ("B", "K", "null", "n") if k in kw}
        args.update(kw)
        rc, _ = raw_reduce(tr, extra.pop("n", n), args["claims"], args["Ts"], args["rounds"], args["u"], **extra)
        return rc == E_ARG and bytes(tr.t) == start

    for name in ("tr", "Ts", "idx", "pts", "vals", "rounds", "u", "rho"):
        assert misuse(null=name), name
    assert misuse(B=0) and misuse(K=0)
    assert misuse(Ts=[Ts[0]] * 257, u=[0] * 257)                                   # B > 256
    many = [claims[k % K] for k in range(4097)]
    assert misuse(claims=many)                                                     # K > 4096
    cb = list(claims)
    cb[0] = (B, cb[0][1], cb[0][2])
    assert misuse(claims=cb)                                                       # an index >= B
    assert misuse(claims=[c for c in claims if c[0] != 2])                         # polynomial 2 without a claim
    assert misuse(n=1) and misuse(n=-3) and misuse(n=41)                           # bad n
