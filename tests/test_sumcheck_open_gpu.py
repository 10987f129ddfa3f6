"""GPU tests of the product sum-check (include/tpst.h: tpst_poly_sumcheck_open,
tpst_pst_verify_sumcheck, tpst_poly_sumcheck_stages), bit for bit:

* the device rounds alone against Python integers on brute-force tables
  (tests/pst_sumcheck_ref.py): every round sum and every u_j, at sizes that take
  every path of the round kernels and on operands random data does not reach;
* sumcheck_open against the restatement (e_0, round coefficients, u, rho) and
  against the library's own parent path for the inner opening: open_combined
  on a transcript advanced by sumcheck_reduce;
* every tamper through verify_sumcheck: rejected, transcript untouched."""
import ctypes as C
import random

import numpy as np
import pytest

import bls377 as O
import golden_io as G
import pst_sumcheck_ref as SR
from testudo_amd import sqrt_pst as S
from testudo_amd.encoding import fr_array, gt_from_array, limbs_to_int, ptr

pytestmark = pytest.mark.gpu

OK, E_ARG, E_STATE, E_VERIFY = 0, -1, -4, -5
R = O.R
SHAPES = ["a", "b", "c", "c_bad", "d", "e"]


def ints(a):
    return [limbs_to_int(x) for x in np.asarray(a).reshape(-1, 4)]


def fresh(label=None):
    tr = S.PoseidonTranscript()
    if label is not None:
        tr.append_bytes(label)
    return tr


def ref_fresh(label=None):
    import pst as P
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


def lib_terms(terms):
    return [(fr_array([c])[0], idx) for c, idx in terms]


def lib_tau(tau):
    return None if tau is None else fr_array(tau)


def gt_oracle(T):
    return O.fq12_from_tower(gt_from_array(T))


def same_proof(a, b):
    (Ua, pa, ma), (Ub, pb, mb) = a, b
    return (np.array_equal(Ua, Ub) and np.array_equal(pa, pb) and np.array_equal(ma.comms_t, mb.comms_t) and
            np.array_equal(ma.comms_u, mb.comms_u) and np.array_equal(ma.final_a, mb.final_a) and
            np.array_equal(ma.final_h, mb.final_h) and np.array_equal(ma.pst_proof_h, mb.pst_proof_h))


def tables(n, B, seed):
    return [ints(S.fr_stream(seed + 16 * n + j, 1 << n)[0]) for j in range(B)]


# ---------------------------------------------------- the rounds alone -------
def check_stages(ctx, Zs, terms, tau, rho, want=None):
    n = len(rho)
    polys = [S.Polynomial.from_evaluations(ctx, fr_array(Z)) for Z in Zs]
    sums, u = S.sumcheck_stages(polys, lib_terms(terms), lib_tau(tau), fr_array(rho))
    want_sums, want_u = want if want is not None else SR.stages(n, Zs, terms, tau, rho)
    assert [tuple(ints(s)) for s in sums] == want_sums
    assert ints(u) == want_u
    for p, Z in zip(polys, Zs):                     # the handles' tables are read, never written
        assert ints(p.evaluations()) == Z
    return want_sums


_STAGE_CASES = {}


def stage_case(shape, n):
    """a term shape on random tables with random challenges and the restatement's sums and u, computed once"""
    if (shape, n) not in _STAGE_CASES:
        rng = random.Random(0x5C20 + n)
        Zs, terms, tau = SR.shape_case(shape, n, 0x5C21)
        rho = [rng.randrange(R) for _ in range(n)]
        _STAGE_CASES[(shape, n)] = (Zs, terms, tau, rho, SR.stages(n, Zs, terms, tau, rho))
    return _STAGE_CASES[(shape, n)]


@pytest.mark.parametrize("shape,n", [(s, n) for s in SHAPES for n in (4, 5, 6, 7)] +
                         [("e", 12),      # round 0: 8 workgroups; rounds 0-3 more than one
                          ("c", 13)])     # odd n: half tables of 2^7 and 2^6 entries
def test_stages_against_python_integers(ctx, shape, n):
    check_stages(ctx, *stage_case(shape, n))


@pytest.mark.parametrize("grid", [1, 3, 5])
def test_stages_do_not_depend_on_the_grid(ctx, monkeypatch, grid):
    """n = 12, shape e with the grid capped (TPST_SUMCHECK_GRID): 2048 index pairs of round 0 over 1, 3 or 5
    workgroups, so every lane walks the grid-stride loop, unevenly for 3 and 5, in every round that has more pairs
    than lanes -- the in-place rounds among them"""
    monkeypatch.setenv("TPST_SUMCHECK_GRID", str(grid))
    check_stages(ctx, *stage_case("e", 12))


def test_stages_default_grid_stride_n21(ctx):
    """n = 21: 2^20 index pairs in round 0 against the default grid's 2^19 lanes, so the stride loop runs at the
    shipped grid.  Constant polynomials c_0 and c_1, one term c f_0 f_1 under tau, where every round sum has a
    closed form: s_i(t) = c c_0 c_1 prod_{l < i} eq(tau_l, rho_l) (tau_i t + (1 - tau_i)(1 - t)), since the rest
    of eq sums to 1."""
    n = 21
    rng = random.Random(0x5C2F)
    c, c0, c1 = (rng.randrange(R) for _ in range(3))
    polys = [S.Polynomial.from_evaluations(ctx, np.tile(fr_array([x]), (1 << n, 1))) for x in (c0, c1)]
    tau = [rng.randrange(R) for _ in range(n)]
    rho = [rng.randrange(R) for _ in range(n)]
    sums, u = S.sumcheck_stages(polys, lib_terms([(c, [0, 1])]), fr_array(tau), fr_array(rho))
    pre = c * c0 * c1 % R
    for i in range(n):
        want = tuple(pre * (tau[i] * t + (1 - tau[i]) * (1 - t)) % R for t in range(4))
        assert tuple(ints(sums[i])) == want, i
        pre = pre * (tau[i] * rho[i] + (1 - tau[i]) * (1 - rho[i])) % R
    assert ints(u) == [c0, c1]


def test_stages_edge_operands(ctx):
    n = 5
    rng = random.Random(0x5C22)
    Zs = tables(n, 3, 0x5C22)
    rnd = lambda k: [rng.randrange(R) for _ in range(k)]  # noqa: E731
    quad = [(rng.randrange(R), [0, 1]), (rng.randrange(R), [2])]          # with tau: D = 3
    cubic = [(rng.randrange(R), [0, 1, 2])]
    halfp = (R + 1) // 2
    # challenges 0, 1, r - 1 and (r + 1) / 2
    check_stages(ctx, Zs, quad, rnd(5), [0, 1, R - 1, halfp, 0])
    check_stages(ctx, Zs, cubic, None, [R - 1, halfp, 0, 1, R - 1])
    # a Boolean tau: e_0 is g at that vertex
    vertex = [1, 0, 1, 1, 0]
    sums = check_stages(ctx, Zs, quad, vertex, rnd(5))
    x = int("".join(map(str, vertex)), 2)
    assert (sums[0][0] + sums[0][1]) % R == SR.g_at(quad, [Z[x] for Z in Zs])
    check_stages(ctx, Zs, quad, vertex, vertex)             # and challenges that land on it
    check_stages(ctx, Zs, quad, [halfp] * 5, rnd(5))        # a tau of (r + 1) / 2
    # the zero polynomial and a constant polynomial
    zc = [[0] * 32, [7] * 32, Zs[2]]
    check_stages(ctx, zc, quad, rnd(5), rnd(5))
    check_stages(ctx, zc, cubic, None, rnd(5))
    # a repeated index: f f f, and f f under tau
    check_stages(ctx, Zs[:1], [(rng.randrange(R), [0, 0, 0])], None, rnd(5))
    check_stages(ctx, Zs[:2], [(rng.randrange(R), [1, 1]), (1, [0])], rnd(5), rnd(5))
    # c_t = 0 (for the only term of a polynomial too) and c_t = r - 1
    check_stages(ctx, Zs, [(0, [0, 1]), (R - 1, [2, 0])], rnd(5), rnd(5))
    check_stages(ctx, Zs, [(R - 1, [0, 1, 2]), (0, [1])], None, rnd(5))
    # M = 1 and M = 64 (the same term repeated)
    check_stages(ctx, Zs[:2], [(rng.randrange(R), [0, 1])], None, rnd(5))
    check_stages(ctx, Zs[:2], [(rng.randrange(R), [1, 0])] * 64, rnd(5), rnd(5))
    # two terms that cancel: e_0 = 0 and every round sum 0
    c = rng.randrange(1, R)
    sums = check_stages(ctx, Zs, [(c, [0, 1, 2]), (R - c, [2, 0, 1])], None, rnd(5))
    assert all(s == (0, 0, 0, 0) for s in sums)


# ---------------------------------------------------------- sumcheck_open ----
class Setup:
    """B committed polynomials of one n on the loaded SRS, with the terms and tau of their relation"""

    def __init__(self, ctx, Zs, terms, tau):
        self.ctx, self.Zs, self.terms, self.tau = ctx, Zs, terms, tau
        self.n = len(Zs[0]).bit_length() - 1
        self.polys = [S.Polynomial.from_evaluations(ctx, fr_array(Z)) for Z in Zs]
        self.commitments = [p.commit() for p in self.polys]
        self.Ts = [T for _, T in self.commitments]

    def open(self, label, terms=None, tau=False):
        terms = self.terms if terms is None else terms
        tau = self.tau if tau is False else tau
        return S.sumcheck_open(self.polys, self.commitments, fresh(label), lib_terms(terms), lib_tau(tau))

    def check(self, label):
        """sumcheck_open == the restatement on e_0, rounds, u and rho; its inner opening == open_combined on a
        transcript advanced by sumcheck_reduce; verify_sumcheck accepts; equal transcript end states"""
        n = self.n
        lt, ta = lib_terms(self.terms), lib_tau(self.tau)
        tr = fresh(label)
        e0, proof, comms, T, v = S.sumcheck_open(self.polys, self.commitments, tr, lt, ta)
        ref = ref_fresh(label)
        re0, rounds, u, rrho = SR.prove(ref, n, self.Zs, self.terms, self.tau, [gt_oracle(x) for x in self.Ts])
        assert limbs_to_int(e0) == re0 == SR.plain_sum(self.Zs, self.terms, self.tau)
        assert [tuple(ints(r)) for r in proof.rounds] == rounds
        assert ints(proof.u) == u and ints(proof.rho) == rrho
        # the parent path of the inner opening
        tp = fresh(label)
        rho2 = S.sumcheck_reduce(tp, n, lt, ta, self.Ts, e0, proof.rounds, proof.u)
        assert rho2 is not None and np.array_equal(rho2, proof.rho)
        assert bytes(tp.t) == SR.transcript_bytes(ref)
        # (the weights from u: Polynomial.eval would reuse the q a handle cached for its first point)
        w = S.combine_challenge(tp, proof.rho, self.Ts, proof.u)
        _, pc, pT, pv, pproof = S.open_combined(self.polys, self.commitments, tp, proof.rho, w)
        assert np.array_equal(comms, pc) and np.array_equal(T, pT) and np.array_equal(v, pv)
        assert same_proof((proof.U, proof.pst_proof, proof.mipp), pproof)
        assert bytes(tr.t) == bytes(tp.t)
        assert limbs_to_int(v) == sum(a * b for a, b in zip(ints(w), u)) % R
        tv = fresh(label)
        assert S.verify_sumcheck(self.ctx, tv, lt, ta, self.Ts, e0, proof)
        assert bytes(tv.t) == bytes(tr.t) != bytes(fresh(label).t)
        return e0, proof


_SETUPS = {}


def golden_setup(ctx, shape, n):
    """the golden SRS of n loaded and the shape's polynomials committed, once per (shape, n)"""
    d = G.load("sqrt_pst_n%d.json" % n)
    S.srs_load(ctx, d["srs_nv"], G.srs_flat(d))
    if (shape, n) not in _SETUPS:
        _SETUPS[(shape, n)] = Setup(ctx, *SR.shape_case(shape, n, 0x5C24))
    return _SETUPS[(shape, n)]


@pytest.mark.parametrize("n", [4, 5, 6, 7])
@pytest.mark.parametrize("shape", SHAPES)
def test_sumcheck_open_equals_restatement_and_parent_path(ctx, shape, n):
    e0, _ = golden_setup(ctx, shape, n).check(b"sumcheck %s %d" % (shape.encode(), n))
    assert (limbs_to_int(e0) == 0) == (shape == "c")


def test_seeded_srs_n12_shape_e(ctx):
    S.srs_setup(ctx, 6, 0x7E57D1)
    Setup(ctx, *SR.shape_case("e", 12, 0x5C27)).check(b"n12")


# -------------------------------------------------------------- rejections ---
def raw_verify(ctx, tr, n, terms, tau, Ts, e0, proof, rounds=None, u=None, inner=None, n_proof=None):
    """tpst_pst_verify_sumcheck on integer terms -> rc (n_proof: the size the inner proof was made for)"""
    arr, _ = S._sc_terms(lib_terms(terms), tau is not None)
    ta = lib_tau(tau)
    tl = [np.ascontiguousarray(T, dtype=np.uint64).reshape(72) for T in Ts]
    rd = np.ascontiguousarray(proof.rounds if rounds is None else rounds, dtype=np.uint64)
    ua = np.ascontiguousarray(proof.u if u is None else u, dtype=np.uint64)
    ea = fr_array([e0])
    pr = S.pack_proof(n if n_proof is None else n_proof,
                      *((proof.U, proof.pst_proof, proof.mipp) if inner is None else inner))
    return ctx.lib.tpst_pst_verify_sumcheck(ctx.h, C.addressof(tr.t), n, S._ptr_array(tl), len(tl), C.addressof(arr),
                                            len(arr), None if ta is None else ptr(ta), ptr(ea), ptr(rd), ptr(ua),
                                            C.byref(pr))


def bump(a, *index):
    """a copy of a limb array with one Fr at `index` incremented mod r"""
    b = np.array(a, dtype=np.uint64, copy=True)
    b[index] = fr_array([(limbs_to_int(b[index]) + 1) % R])[0]
    return b


def test_rejections(ctx):
    """every tamper: TPST_E_VERIFY and the transcript untouched; the untampered call: TPST_OK, advanced"""
    n = 6
    s = golden_setup(ctx, "e", n)
    terms, tau, B = s.terms, s.tau, len(s.polys)
    label = b"reject"
    e0a, proof, _, _, _ = s.open(label)
    e0 = limbs_to_int(e0a)
    start = bytes(fresh(label).t)

    def rejected(terms=terms, tau=tau, Ts=s.Ts, e0=e0, **kw):
        tr = fresh(label)
        rc = raw_verify(ctx, tr, n, terms, tau, Ts, e0, proof, **kw)
        return rc == E_VERIFY and bytes(tr.t) == start

    tr = fresh(label)
    assert raw_verify(ctx, tr, n, terms, tau, s.Ts, e0, proof) == OK and bytes(tr.t) != start
    for i in (0, n // 2, n - 1):
        for c in range(4):
            assert rejected(rounds=bump(proof.rounds, i, c)), (i, c)
    for j in range(B):
        assert rejected(u=bump(proof.u, j)), j
    assert rejected(e0=(e0 + 1) % R)
    for t in range(len(terms)):
        tb = list(terms)
        tb[t] = ((tb[t][0] + 1) % R, tb[t][1])
        assert rejected(terms=tb), t                                            # a term's coefficient
    assert rejected(terms=[(terms[0][0], [1, 0])] + terms[1:])                  # two indices swapped
    assert rejected(terms=[terms[0], (terms[1][0], [2, 3]), terms[2]])          # a changed index
    tb = list(tau)
    tb[n - 1] = (tb[n - 1] + 1) % R
    assert rejected(tau=tb)                                                     # one coordinate
    assert rejected(Ts=[s.Ts[1], s.Ts[0], s.Ts[2], s.Ts[3]])                    # a changed T_j
    assert rejected(tau=None)                                                   # has_tau flipped
    assert rejected(terms=[terms[0], (R, terms[1][1]), terms[2]])               # c_t >= r
    assert rejected(tau=[R] + list(tau[1:]))                                    # a coordinate >= r
    assert rejected(e0=R + 2)
    big = proof.rounds.copy()
    big[2, 1] = fr_array([R + 5])[0]
    assert rejected(rounds=big)
    bigu = proof.u.copy()
    bigu[0] = fr_array([R])[0]
    assert rejected(u=bigu)
    # the inner opening: one field each of U, pst_proof, comms_t and final_a replaced by another valid element
    _, other, _, _, _ = s.open(b"other")
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
    # a proof spliced from two statements: the rounds of another statement on the same polynomials
    terms2 = [(5, [0, 1]), terms[1], terms[2]]
    e2a, p2, _, _, _ = s.open(label, terms=terms2)
    tr = fresh(label)
    assert raw_verify(ctx, tr, n, terms2, tau, s.Ts, limbs_to_int(e2a), p2) == OK
    tr = fresh(label)
    assert raw_verify(ctx, tr, n, terms, tau, s.Ts, e0, p2) == E_VERIFY and bytes(tr.t) == start
    assert rejected(rounds=p2.rounds)
    assert rejected(inner=(p2.U, p2.pst_proof, p2.mipp))


def test_wrong_hadamard_claim_is_rejected(ctx):
    """shape c with one entry of f_2 wrong: the prover's own e_0 is not 0 and verifies; presented as the
    zero-check (e_0 = 0) the same proof is rejected"""
    n = 6
    s = golden_setup(ctx, "c_bad", n)
    label = b"hadamard"
    e0a, proof, _, _, _ = s.open(label)
    assert limbs_to_int(e0a) != 0
    start = bytes(fresh(label).t)
    tr = fresh(label)
    assert raw_verify(ctx, tr, n, s.terms, s.tau, s.Ts, limbs_to_int(e0a), proof) == OK
    tr = fresh(label)
    assert raw_verify(ctx, tr, n, s.terms, s.tau, s.Ts, 0, proof) == E_VERIFY and bytes(tr.t) == start


# ------------------------------------------------------------------ misuse ---
def test_misuse(ctx):
    import torch
    from testudo_amd import Context
    n = 5
    s = golden_setup(ctx, "d", n)                                                  # B = 3, g = f_0 f_1 f_2, no tau
    lt = lib_terms(s.terms)
    tau = fr_array([3] * n)
    tr = fresh()
    opened = lambda polys, terms, tau=None: rc_of(  # noqa: E731
        lambda: S.sumcheck_open(polys, s.commitments, tr, terms, tau))
    staged = lambda polys, terms, tau=None: rc_of(  # noqa: E731
        lambda: S.sumcheck_stages(polys, terms, tau, fr_array([1] * n)))
    for call in (opened, staged):
        assert call(s.polys, lt, tau) == E_ARG                                     # D = 4: deg 3 with tau
        assert call(s.polys, [(lt[0][0], [0, 1, 3])]) == E_ARG                     # an index >= B
        assert call(s.polys, [(lt[0][0], [0, 1])]) == E_ARG                        # polynomial 2 in no term
        assert call(s.polys, [(fr_array([R])[0], [0, 1, 2])]) == E_ARG             # a coefficient >= r
        assert call(s.polys, [(lt[0][0], [0, 1]), (lt[0][0], [2])], fr_array([R] + [3] * (n - 1))) == E_ARG
        p4 = S.Polynomial.from_evaluations(ctx, fr_array(tables(4, 1, 0x5C2C)[0]))
        assert call([s.polys[0], s.polys[1], p4], lt) == E_ARG                     # differing n
        pq = S.Polynomial.from_q(ctx, n, fr_array([1] * n), torch.zeros(4 << (n - n // 2), dtype=torch.int64))
        assert call([s.polys[0], s.polys[1], pq], lt) == E_STATE                   # a from_q handle
        cols = S.Polynomial.from_evaluations_cols(ctx, fr_array(s.Zs[2]), 0, 2)
        assert call([s.polys[0], s.polys[1], cols], lt) == E_STATE                 # a column slice
    assert bytes(tr.t) == bytes(fresh().t)
    # no SRS loaded: a fresh context; the stages entry needs none
    other = Context(0)
    try:
        polys = [S.Polynomial.from_evaluations(other, fr_array(Z)) for Z in s.Zs]
        assert rc_of(lambda: S.sumcheck_open(polys, s.commitments, tr, lt)) == E_STATE
        assert rc_of(lambda: S.sumcheck_open([s.polys[0], polys[1], polys[2]], s.commitments, tr, lt)) == E_ARG
        rho = [7] * n
        sums, u = S.sumcheck_stages(polys, lt, None, fr_array(rho))
        assert ([tuple(ints(x)) for x in sums], ints(u)) == SR.stages(n, s.Zs, s.terms, None, rho)
        del polys
    finally:
        other.close()
    assert bytes(tr.t) == bytes(fresh().t)
    # the verifier: sizes that do not match the loaded SRS
    e0a, proof, _, _, _ = s.open(None)
    tv = fresh()
    golden_setup(ctx, "d", 7)
    assert raw_verify(ctx, tv, n, s.terms, None, s.Ts, limbs_to_int(e0a), proof) == E_ARG
    assert bytes(tv.t) == bytes(fresh().t)
    golden_setup(ctx, "d", n)
    assert S.verify_sumcheck(ctx, tv, lt, None, s.Ts, e0a, proof) and bytes(tv.t) != bytes(fresh().t)
