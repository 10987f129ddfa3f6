"""GPU tests of the multi-point opening (include/tpst.h: tpst_poly_open_multi,
tpst_pst_verify_multi, tpst_poly_multi_sumcheck_stages), bit for bit:

* the device reduction alone against Python integers on brute-force tables
  (tests/pst_multi_ref.py): every round sum and every u_j, at sizes that take
  every path of the round kernels and on operands random data does not reach;
* open_multi against the restatement (round coefficients, u, rho) and against
  the library's own parent path for the inner opening: open_combined on a
  transcript advanced by multi_reduce;
* every tamper through verify_multi: rejected, transcript untouched."""
import ctypes as C
import random

import numpy as np
import pytest

import bls377 as O
import golden_io as G
import pst as P
import pst_multi_ref as MR
from testudo_amd import sqrt_pst as S
from testudo_amd.encoding import fr_array, gt_from_array, limbs_to_int, ptr

pytestmark = pytest.mark.gpu

OK, E_ARG, E_STATE, E_VERIFY = 0, -1, -4, -5
R = O.R
SHAPES = [(1, 1), (1, 3), (2, 2), (3, 5)]


def ints(a):
    return [limbs_to_int(x) for x in np.asarray(a).reshape(-1, 4)]


def fresh(label=None):
    tr = S.PoseidonTranscript()
    if label is not None:
        tr.append_bytes(label)
    return tr


def ref_fresh(label=None):
    tr = P.PoseidonTranscript()
    if label is not None:
        tr.sponge.absorb_bytes(label)
    return tr


def rc_of(fn):
    try:
        fn()
    except S.TpstError as e:
        return int(str(e).split("(")[1].split(")")[0])
    return 0


def lib_claims(claims):
    return [(j, fr_array(p), fr_array([v])[0]) for j, p, v in claims]


def gt_oracle(T):
    return O.fq12_from_tower(gt_from_array(T))


def same_proof(a, b):
    (Ua, pa, ma), (Ub, pb, mb) = a, b
    return (np.array_equal(Ua, Ub) and np.array_equal(pa, pb) and np.array_equal(ma.comms_t, mb.comms_t) and
            np.array_equal(ma.comms_u, mb.comms_u) and np.array_equal(ma.final_a, mb.final_a) and
            np.array_equal(ma.final_h, mb.final_h) and np.array_equal(ma.pst_proof_h, mb.pst_proof_h))


def tables(n, B, seed):
    return [ints(S.fr_stream(seed + 16 * n + j, 1 << n)[0]) for j in range(B)]


def random_claims(n, Zs, K, seed, values=True):
    """claim k on polynomial k mod B at a random point; with K > B the last claim repeats the point of claim 0"""
    B = len(Zs)
    rng = random.Random(seed)
    claims = []
    for c in range(K):
        point = [rng.randrange(R) for _ in range(n)]
        if K > B and c == K - 1:
            point = list(claims[0][1])
        claims.append((c % B, point, P.dense_evaluate(Zs[c % B], point) if values else 0))
    return claims


# ------------------------------------------------- the reduction alone -------
def check_stages(ctx, Zs, claims, a, rho, want=None):
    n = len(rho)
    polys = [S.Polynomial.from_evaluations(ctx, fr_array(Z)) for Z in Zs]
    sums, u = S.multi_sumcheck_stages(polys, lib_claims(claims), fr_array(a), fr_array(rho))
    want_sums, want_u = want if want is not None else MR.stages(n, Zs, claims, a, rho)
    assert [tuple(ints(s)) for s in sums] == want_sums
    assert ints(u) == want_u
    for p, Z in zip(polys, Zs):                     # the handles' tables are read, never written
        assert ints(p.evaluations()) == Z


_STAGE_CASES = {}


def stage_case(n, B, K):
    """random tables, claims, weights and challenges with the restatement's sums and u, computed once"""
    if (n, B, K) not in _STAGE_CASES:
        rng = random.Random(0x3A20 + n)
        Zs = tables(n, B, 0x3A20)
        claims = random_claims(n, Zs, K, 0x3A21 + n, values=False)
        a, rho = [rng.randrange(R) for _ in range(K)], [rng.randrange(R) for _ in range(n)]
        _STAGE_CASES[(n, B, K)] = (Zs, claims, a, rho, MR.stages(n, Zs, claims, a, rho))
    return _STAGE_CASES[(n, B, K)]


@pytest.mark.parametrize("n,B,K", [(4, 3, 5), (5, 3, 5), (6, 3, 5), (7, 3, 5),
                                   (12, 4, 6),      # round 0: 8 workgroups; rounds 0-3 more than one
                                   (13, 2, 3)])     # odd n: half tables of 2^7 and 2^6 entries
def test_stages_against_python_integers(ctx, n, B, K):
    check_stages(ctx, *stage_case(n, B, K))


@pytest.mark.parametrize("grid", [1, 3, 5])
def test_stages_do_not_depend_on_the_grid(ctx, monkeypatch, grid):
    """n = 12, B = 4, K = 6 with the grid capped (TPST_MULTI_GRID): 2048 index pairs of round 0 over 1, 3 or 5
    workgroups, so every lane walks the grid-stride loop, unevenly for 3 and 5, in every round that has more pairs
    than lanes -- the in-place rounds among them"""
    monkeypatch.setenv("TPST_MULTI_GRID", str(grid))
    check_stages(ctx, *stage_case(12, 4, 6))


def test_stages_default_grid_stride_n21(ctx):
    """n = 21, B = 1, K = 1: 2^20 index pairs in round 0 against the default grid's 2^19 lanes, so the stride
    loop runs at the shipped grid.  A constant polynomial c, where every round sum has a closed form:
    s_i(t) = a c prod_{l < i} eq(r_l, rho_l) (r_i t + (1 - r_i)(1 - t)), since the rest of eq sums to 1."""
    n = 21
    rng = random.Random(0x3A2F)
    c = rng.randrange(R)
    Z = np.tile(fr_array([c]), (1 << n, 1))
    p = S.Polynomial.from_evaluations(ctx, Z)
    point = [rng.randrange(R) for _ in range(n)]
    rho = [rng.randrange(R) for _ in range(n)]
    a = rng.randrange(R)
    sums, u = S.multi_sumcheck_stages([p], [(0, fr_array(point), fr_array([0])[0])], fr_array([a]), fr_array(rho))
    pre = a * c % R
    for i in range(n):
        s0 = pre * (1 - point[i]) % R
        s2 = pre * (2 * point[i] - (1 - point[i])) % R
        assert tuple(ints(sums[i])) == (s0, s2), i
        pre = pre * (point[i] * rho[i] + (1 - point[i]) * (1 - rho[i])) % R
    assert ints(u) == [c]


def test_stages_edge_operands(ctx):
    n, B = 5, 3
    rng = random.Random(0x3A22)
    Zs = tables(n, B, 0x3A22)
    rnd = lambda k: [rng.randrange(R) for _ in range(k)]  # noqa: E731
    base = random_claims(n, Zs, 5, 0x3A23, values=False)
    # challenges 0, 1 and r - 1
    check_stages(ctx, Zs, base, rnd(5), [0, 1, R - 1, rng.randrange(R), 0])
    check_stages(ctx, Zs, base, rnd(5), [R - 1, 1, 0, 1, R - 1])
    # Boolean points: D_j is an indicator
    bools = [(0, [1, 0, 1, 1, 0], 0), (1, [0, 0, 0, 0, 0], 0), (2, [1, 1, 1, 1, 1], 0)]
    check_stages(ctx, Zs, bools, [1, 1, 1], rnd(5))
    check_stages(ctx, Zs, bools, rnd(3), [1, 0, 1, 1, 0])   # and challenges that land on one of them
    # a coordinate equal to (r + 1) / 2
    halfp = (R + 1) // 2
    check_stages(ctx, Zs, [(0, [halfp] + rnd(4), 0), (1, rnd(4) + [halfp], 0), (2, [halfp] * 5, 0)], rnd(3), rnd(5))
    # the zero polynomial and a constant polynomial
    zc = [[0] * 32, [7] * 32, Zs[2]]
    check_stages(ctx, zc, base, rnd(5), rnd(5))
    # two claims on one polynomial at one point; the same point for different polynomials
    pt = rnd(5)
    check_stages(ctx, Zs, [(0, pt, 0), (0, pt, 0), (1, pt, 0), (2, pt, 0)], rnd(4), rnd(5))
    # K = 1
    check_stages(ctx, Zs[:1], [(0, rnd(5), 0)], rnd(1), rnd(5))
    # a_k = 0 for one claim (and for the only claim of a polynomial)
    check_stages(ctx, Zs, base, [rng.randrange(R), 0, rng.randrange(R), rng.randrange(R), 0], rnd(5))
    check_stages(ctx, Zs, base[:3], [rng.randrange(R), 0, 1], rnd(5))


# ------------------------------------------------------------- open_multi ----
class Setup:
    """B committed polynomials of one n on the loaded SRS"""

    def __init__(self, ctx, Zs):
        self.ctx, self.Zs = ctx, Zs
        self.n = len(Zs[0]).bit_length() - 1
        self.polys = [S.Polynomial.from_evaluations(ctx, fr_array(Z)) for Z in Zs]
        self.commitments = [p.commit() for p in self.polys]
        self.Ts = [T for _, T in self.commitments]

    def first(self, B):
        s = object.__new__(Setup)
        s.ctx, s.n = self.ctx, self.n
        s.Zs, s.polys, s.commitments, s.Ts = self.Zs[:B], self.polys[:B], self.commitments[:B], self.Ts[:B]
        return s

    def check(self, claims, label):
        """open_multi == the restatement on rounds, u and rho; its inner opening == open_combined on a transcript
        advanced by multi_reduce; verify_multi accepts; equal transcript end states"""
        n, B = self.n, len(self.polys)
        lc = lib_claims(claims)
        tr = fresh(label)
        proof, rho, comms, T, v = S.open_multi(self.polys, self.commitments, tr, lc)
        ref = ref_fresh(label)
        rounds, u, rrho = MR.prove_reduction(ref, n, self.Zs, claims, [gt_oracle(x) for x in self.Ts])
        assert [tuple(ints(r)) for r in proof.rounds] == rounds
        assert ints(proof.u) == u and ints(rho) == rrho
        # the parent path of the inner opening
        tp = fresh(label)
        rho2 = S.multi_reduce(tp, n, lc, self.Ts, proof.rounds, proof.u)
        assert rho2 is not None and np.array_equal(rho2, rho)
        assert bytes(tp.t) == MR.transcript_bytes(ref)
        # (the weights from u: Polynomial.eval would reuse the q a handle cached for its first point)
        w = S.combine_challenge(tp, rho, self.Ts, proof.u)
        _, pc, pT, pv, pproof = S.open_combined(self.polys, self.commitments, tp, rho, w)
        assert np.array_equal(comms, pc) and np.array_equal(T, pT) and np.array_equal(v, pv)
        assert same_proof((proof.U, proof.pst_proof, proof.mipp), pproof)
        assert bytes(tr.t) == bytes(tp.t)
        assert limbs_to_int(v) == sum(a * b for a, b in zip(ints(w), u)) % R
        tv = fresh(label)
        assert S.verify_multi(self.ctx, tv, lc, self.Ts, proof)
        assert bytes(tv.t) == bytes(tr.t) != bytes(fresh(label).t)
        return proof, rho, comms, T, v


_SETUPS = {}


def golden_setup(ctx, n):
    """the golden SRS of n loaded and 3 committed polynomials (polynomial 0 is the fixture's own), once per n"""
    d = G.load("sqrt_pst_n%d.json" % n)
    S.srs_load(ctx, d["srs_nv"], G.srs_flat(d))
    if n not in _SETUPS:
        Zs = [[G.i(x) for x in d["Z"]]] + tables(n, 2, 0x3A24)
        _SETUPS[n] = Setup(ctx, Zs)
    return _SETUPS[n]


@pytest.mark.parametrize("n", [4, 5, 6, 7])
@pytest.mark.parametrize("B,K", SHAPES)
def test_open_multi_equals_restatement_and_parent_path(ctx, n, B, K):
    s = golden_setup(ctx, n).first(B)
    claims = random_claims(n, s.Zs, K, 0x3A25 + 16 * n + K)
    s.check(claims, b"multi %d %d %d" % (n, B, K))


def test_k1_b1_inner_opening_is_a_plain_opening(ctx):
    n = 6
    s = golden_setup(ctx, n).first(1)
    claims = random_claims(n, s.Zs, 1, 0x3A26)
    proof, rho, comms, T, v = s.check(claims, b"plain")
    assert np.array_equal(T, s.Ts[0]) and np.array_equal(v, proof.u[0])   # w_0 = 1
    tr = fresh(b"plain")
    assert S.multi_reduce(tr, n, lib_claims(claims), s.Ts, proof.rounds, proof.u) is not None
    S.combine_challenge(tr, rho, s.Ts, proof.u)
    assert S.verify(s.ctx, tr, proof.U, rho, v, proof.pst_proof, proof.mipp, T)


def test_seeded_srs_n12_b4_k6(ctx):
    S.srs_setup(ctx, 6, 0x7E57D1)
    n, B, K = 12, 4, 6
    s = Setup(ctx, tables(n, B, 0x3A27))
    s.check(random_claims(n, s.Zs, K, 0x3A28), b"n12")


# -------------------------------------------------------------- rejections ---
def raw_verify(ctx, tr, n, claims, Ts, proof, rounds=None, u=None, inner=None, n_proof=None):
    """tpst_pst_verify_multi on integer claims -> rc (n_proof: the size the inner proof was made for)"""
    idx = np.ascontiguousarray([j for j, _, _ in claims], dtype=np.uint32)
    pts = fr_array([x for _, p, _ in claims for x in p])
    vals = fr_array([v for _, _, v in claims])
    tl = [np.ascontiguousarray(T, dtype=np.uint64).reshape(72) for T in Ts]
    rd = np.ascontiguousarray(proof.rounds if rounds is None else rounds, dtype=np.uint64)
    ua = np.ascontiguousarray(proof.u if u is None else u, dtype=np.uint64)
    pr = S.pack_proof(n if n_proof is None else n_proof, *((proof.U, proof.pst_proof, proof.mipp) if inner is None else inner))
    return ctx.lib.tpst_pst_verify_multi(ctx.h, C.byref(tr.t), n, S._ptr_array(tl), len(tl),
                                         idx.ctypes.data_as(C.POINTER(C.c_uint32)), ptr(pts), ptr(vals), len(claims),
                                         ptr(rd), ptr(ua), C.byref(pr))


def bump(a, *index):
    """a copy of a limb array with one Fr at `index` incremented mod r"""
    b = np.array(a, dtype=np.uint64, copy=True)
    b[index] = fr_array([(limbs_to_int(b[index]) + 1) % R])[0]
    return b


def test_rejections(ctx):
    """every tamper: TPST_E_VERIFY and the transcript untouched; the untampered call: TPST_OK, advanced"""
    n, B, K = 6, 3, 5
    s = golden_setup(ctx, n).first(B)
    claims = random_claims(n, s.Zs, K, 0x3A29)
    label = b"reject"
    proof, rho, _, _, _ = S.open_multi(s.polys, s.commitments, fresh(label), lib_claims(claims))
    start = bytes(fresh(label).t)
    inner = (proof.U, proof.pst_proof, proof.mipp)

    def rejected(claims=claims, Ts=s.Ts, **kw):
        tr = fresh(label)
        rc = raw_verify(ctx, tr, n, claims, Ts, proof, **kw)
        return rc == E_VERIFY and bytes(tr.t) == start

    tr = fresh(label)
    assert raw_verify(ctx, tr, n, claims, s.Ts, proof) == OK and bytes(tr.t) != start
    for i in (0, n // 2, n - 1):
        for c in range(3):
            assert rejected(rounds=bump(proof.rounds, i, c)), (i, c)
    for j in range(B):
        assert rejected(u=bump(proof.u, j)), j
    for k in range(K):
        cb = list(claims)
        cb[k] = (cb[k][0], cb[k][1], (cb[k][2] + 1) % R)
        assert rejected(claims=cb), k
    cb = list(claims)
    pt = list(cb[1][1])
    pt[n - 1] = (pt[n - 1] + 1) % R
    cb[1] = (cb[1][0], pt, cb[1][2])
    assert rejected(claims=cb)                                              # one coordinate
    assert rejected(claims=[claims[1], claims[0]] + claims[2:])             # two claims swapped
    cb = list(claims)
    cb[3] = (1, cb[3][1], cb[3][2])
    assert rejected(claims=cb)                                              # a changed polynomial index
    assert rejected(Ts=[s.Ts[1], s.Ts[0], s.Ts[2]])                         # a changed T_j
    cb = list(claims)
    cb[2] = (cb[2][0], cb[2][1], R)
    assert rejected(claims=cb)                                              # v_k >= r
    cb = list(claims)
    cb[2] = (cb[2][0], [R] + list(cb[2][1][1:]), cb[2][2])
    assert rejected(claims=cb)                                              # a coordinate >= r
    big = proof.rounds.copy()
    big[2, 1] = fr_array([R + 5])[0]
    assert rejected(rounds=big)
    bigu = proof.u.copy()
    bigu[0] = fr_array([R])[0]
    assert rejected(u=bigu)
    # the inner opening: one field each of U, pst_proof, comms_t and final_a replaced by another valid element
    other, _, _, _, _ = S.open_multi(s.polys, s.commitments, fresh(b"other"), lib_claims(claims))
    assert not np.array_equal(other.U, proof.U)
    assert rejected(inner=(other.U, proof.pst_proof, proof.mipp))
    pst = proof.pst_proof.copy()
    pst[1] = other.pst_proof[1]
    assert not np.array_equal(pst, proof.pst_proof) and rejected(inner=(proof.U, pst, proof.mipp))
    ct = proof.mipp.comms_t.copy()
    ct[0, 1] = other.mipp.comms_t[0, 1]
    m2 = S.MippProof(ct, proof.mipp.comms_u, proof.mipp.final_a, proof.mipp.final_h, proof.mipp.pst_proof_h)
    assert not np.array_equal(ct, proof.mipp.comms_t) and rejected(inner=(proof.U, proof.pst_proof, m2))
    m3 = S.MippProof(proof.mipp.comms_t, proof.mipp.comms_u, other.mipp.final_a, proof.mipp.final_h,
                     proof.mipp.pst_proof_h)
    assert not np.array_equal(other.mipp.final_a, proof.mipp.final_a)
    assert rejected(inner=(proof.U, proof.pst_proof, m3))
    del inner
    # a proof made with a claim whose value is wrong
    wrong = list(claims)
    wrong[4] = (wrong[4][0], wrong[4][1], (wrong[4][2] + 1) % R)
    bad, _, _, _, _ = S.open_multi(s.polys, s.commitments, fresh(label), lib_claims(wrong))
    tr = fresh(label)
    assert raw_verify(ctx, tr, n, wrong, s.Ts, bad) == E_VERIFY and bytes(tr.t) == start
    # a proof for other claims spliced in
    others = random_claims(n, s.Zs, K, 0x3A2A)
    po, _, _, _, _ = S.open_multi(s.polys, s.commitments, fresh(label), lib_claims(others))
    tr = fresh(label)
    assert raw_verify(ctx, tr, n, others, s.Ts, po) == OK
    tr = fresh(label)
    assert raw_verify(ctx, tr, n, claims, s.Ts, po) == E_VERIFY and bytes(tr.t) == start
    assert rejected(inner=(po.U, po.pst_proof, po.mipp))


# ------------------------------------------------------------------ misuse ---
def test_misuse(ctx):
    s5 = golden_setup(ctx, 5).first(2)
    claims = random_claims(5, s5.Zs, 2, 0x3A2B)
    lc = lib_claims(claims)
    tr = fresh()
    cols = S.Polynomial.from_evaluations_cols(ctx, fr_array(s5.Zs[1]), 0, 2)
    assert rc_of(lambda: S.open_multi([s5.polys[0], cols], s5.commitments, tr, lc)) == E_STATE
    assert rc_of(lambda: S.multi_sumcheck_stages([s5.polys[0], cols], lc, fr_array([1, 1]),
                                                 fr_array([1] * 5))) == E_STATE
    p4 = S.Polynomial.from_evaluations(ctx, fr_array(tables(4, 1, 0x3A2C)[0]))
    assert rc_of(lambda: S.open_multi([s5.polys[0], p4], s5.commitments, tr, lc)) == E_ARG         # differing n
    assert rc_of(lambda: S.open_multi(s5.polys, s5.commitments, tr, [lc[0], (2, lc[1][1], lc[1][2])])) == E_ARG
    assert rc_of(lambda: S.open_multi(s5.polys, s5.commitments, tr, [lc[0]])) == E_ARG             # no claim on 1
    assert rc_of(lambda: S.open_multi(s5.polys, s5.commitments, tr,
                                      [lc[0], (1, lc[1][1], fr_array([R])[0])])) == E_ARG          # a value >= r
    assert bytes(tr.t) == bytes(fresh().t)
    proof, _, _, _, _ = S.open_multi(s5.polys, s5.commitments, fresh(), lc)
    tv = fresh()
    # sizes that do not match n: the proof of n = 5 handed over with n = 6 claims
    pts6 = [(j, list(p) + [1], v) for j, p, v in claims]
    r6 = np.concatenate([proof.rounds, proof.rounds[:1]])
    assert raw_verify(ctx, tv, 6, pts6, s5.Ts, proof, rounds=r6, n_proof=5) == E_ARG
    # and against an SRS of another size
    golden_setup(ctx, 7)
    assert raw_verify(ctx, tv, 5, claims, s5.Ts, proof) == E_ARG
    assert bytes(tv.t) == bytes(fresh().t)
    golden_setup(ctx, 5)
    assert S.verify_multi(ctx, tv, lc, s5.Ts, proof) and bytes(tv.t) != bytes(fresh().t)
