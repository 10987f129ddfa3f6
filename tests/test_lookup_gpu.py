"""GPU tests of the lookup argument (include/tpst.h: tpst_poly_lookup_open,
tpst_pst_verify_lookup, tpst_poly_lookup_stages), bit for bit:

* the device stages alone -- multiplicities, every h, the values at the 1/2
  point -- against Python integers and NumPy (tests/pst_lookup_ref.py), at
  sizes that take every path of the kernels and on tables random data does not
  reach; identical under every grid and at load factor 1;
* lookup_open against the restatement (every T, u, s, coefficient and rho) and
  against the library's own parent path for the closing: open_multi on a
  transcript advanced by the restated steps 1-5;
* every tamper through verify_lookup: rejected, transcript untouched."""
import ctypes as C
import random

import numpy as np
import pytest

import bls377 as O
import golden_io as G
import pst_lookup_ref as LR
from testudo_amd import sqrt_pst as S
from testudo_amd.encoding import fr_array, gt_array, gt_from_array, limbs_to_int, ptr

pytestmark = pytest.mark.gpu

OK, E_ARG, E_STATE, E_VERIFY = 0, -1, -4, -5
R = O.R


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


def err_of(fn):
    """(rc, message) of a call that raises TpstError, (0, "") otherwise"""
    try:
        fn()
    except S.TpstError as e:
        return int(str(e).split("(")[1].split(")")[0]), str(e)
    return 0, ""


def gt_oracle(T):
    return O.fq12_from_tower(gt_from_array(T))


def gt_limbs(f):
    return gt_array(O.fq12_to_tower(f)).reshape(72)


def same_proof(a, b):
    (Ua, pa, ma), (Ub, pb, mb) = a, b
    return (np.array_equal(Ua, Ub) and np.array_equal(pa, pb) and np.array_equal(ma.comms_t, mb.comms_t) and
            np.array_equal(ma.comms_u, mb.comms_u) and np.array_equal(ma.final_a, mb.final_a) and
            np.array_equal(ma.final_h, mb.final_h) and np.array_equal(ma.pst_proof_h, mb.pst_proof_h))


# ------------------------------------------------------------- the cases -----
KINDS = ["range", "repeat4", "all_equal", "perm", "edge"]


def make_case(kind, n, L, seed=0x10D0):
    """(As, t) as integers:
    range      t(y) = y, uniform witnesses
    repeat4    2^n / 4 random values, each 4 times in a shuffled table; witnesses drawn from them
    all_equal  a table of distinct random values, every witness entry equal to one of them
    perm       a table of distinct random values, every witness a permutation of it (m = L everywhere)
    edge       0, r - 1, and runs of values that differ from one another only in the top word or only in the
               bottom word, padded with random values; the witnesses draw mostly from the edge values"""
    rng = random.Random(seed + 64 * n + 8 * L + KINDS.index(kind))
    N = 1 << n
    if kind == "range":
        t = list(range(N))
        return [[rng.randrange(N) for _ in range(N)] for _ in range(L)], t
    if kind == "repeat4":
        t = [rng.randrange(R) for _ in range(N // 4)] * 4
        rng.shuffle(t)
        return [[t[rng.randrange(N)] for _ in range(N)] for _ in range(L)], t
    t = [rng.randrange(R) for _ in range(N)]
    if kind == "all_equal":
        return [[t[N // 3]] * N for _ in range(L)], t
    if kind == "perm":
        return [rng.sample(t, N) for _ in range(L)], t
    base = rng.randrange(1 << 200) << 32                        # bottom word 0, top word 0
    edge = [0, R - 1, 1, R - 2] + [base + (k << 224) for k in range(4)] + [base + k for k in range(1, 5)]
    assert all(v < R for v in edge) and len(set(edge)) == len(edge)
    t[:len(edge)] = edge
    rng.shuffle(t)
    pick = lambda: edge[rng.randrange(len(edge))] if rng.random() < 0.75 else t[rng.randrange(N)]  # noqa: E731
    return [[pick() for _ in range(N)] for _ in range(L)], t


def expected(As, t, beta):
    m, hs = LR.helpers(As, t, beta)
    return m, hs, [LR.half_value(h) for h in hs]


class Staged:
    """the handles of one case and the stages' outputs on a beta"""

    def __init__(self, ctx, As, t):
        self.As, self.t = As, t
        self.wits = [S.Polynomial.from_evaluations(ctx, fr_array(a)) for a in As]
        self.table = S.Polynomial.from_evaluations(ctx, fr_array(t))

    def run(self, beta):
        return S.lookup_stages(self.wits, self.table, fr_array([beta])[0])

    def check(self, beta):
        m, h, s = self.run(beta)
        wm, wh, ws = expected(self.As, self.t, beta)
        assert ints(m) == wm
        for k, want in enumerate(wh):
            assert ints(h[k]) == want, k
        assert ints(s) == ws
        assert sum(ws[:-1]) % R == ws[-1]
        for p, Z in zip(self.wits + [self.table], self.As + [self.t]):   # the handles' tables are read, never written
            assert ints(p.evaluations()) == Z
        return m, h, s


def beta_of(n, L):
    return random.Random(0x10D1 + 8 * n + L).randrange(R)


@pytest.mark.parametrize("n,L", [(n, L) for n in (4, 5, 6, 7) for L in (1, 2, 3)])
def test_stages_range_table(ctx, n, L):
    Staged(ctx, *make_case("range", n, L)).check(beta_of(n, L))


@pytest.mark.parametrize("kind", KINDS[1:])
@pytest.mark.parametrize("n,L", [(4, 1), (5, 2), (6, 3), (7, 2)])
def test_stages_other_tables(ctx, kind, n, L):
    As, t = make_case(kind, n, L)
    m, _, _ = Staged(ctx, As, t).check(beta_of(n, L))
    N = 1 << n
    mi = ints(m)
    if kind == "all_equal":
        assert sorted(mi) == [0] * (N - 1) + [L * N] and mi[t.index(As[0][0])] == L * N
    if kind == "perm":
        assert mi == [L] * N
    if kind == "repeat4":
        assert all(mi[y] == 0 for y, v in enumerate(t) if t.index(v) != y)


@pytest.mark.parametrize("kind,n,L", [(k, 12, 2) for k in KINDS] +          # 16 workgroups of table entries
                         [(k, 13, 1) for k in KINDS])                       # odd n
def test_stages_several_workgroups(ctx, kind, n, L):
    Staged(ctx, *make_case(kind, n, L)).check(beta_of(n, L))


def test_stages_beta_edge_values(ctx):
    """beta = 0 (no table value is 0 here), 1 and r - 1"""
    n, L = 5, 2
    As, t = make_case("repeat4", n, L)
    st = Staged(ctx, As, t)
    for beta in (0, 1, R - 1):
        assert all((beta + v) % R for v in t)
        st.check(beta)


# ------------------------------------------------------------------ hooks ----
_N12 = {}


def n12_default(ctx, kind):
    """the n = 12, L = 2 case of a kind and its outputs at the default grid and capacity, checked once"""
    if kind not in _N12:
        st = Staged(ctx, *make_case(kind, 12, 2))
        _N12[kind] = (st, st.check(beta_of(12, 2)))
    return _N12[kind]


@pytest.mark.parametrize("grid", [1, 3, 5])
@pytest.mark.parametrize("kind", ["range", "all_equal", "edge"])
def test_stages_do_not_depend_on_the_grid(ctx, monkeypatch, kind, grid):
    """TPST_LOOKUP_GRID caps the workgroups: every lane walks the stride loops, unevenly for 3 and 5; one lane
    of the inversion takes 16, 6 or 4 entries"""
    st, want = n12_default(ctx, kind)
    monkeypatch.setenv("TPST_LOOKUP_GRID", str(grid))
    got = st.run(beta_of(12, 2))
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("kind", ["perm", "range"])
def test_stages_full_index(ctx, monkeypatch, kind):
    """TPST_LOOKUP_SLOTS_LOG2 = n on distinct table values: load factor 1, long probe chains, no empty slot"""
    st, want = n12_default(ctx, kind)
    monkeypatch.setenv("TPST_LOOKUP_SLOTS_LOG2", "12")
    got = st.run(beta_of(12, 2))
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    monkeypatch.setenv("TPST_LOOKUP_SLOTS_LOG2", "14")
    got = st.run(beta_of(12, 2))
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    monkeypatch.setenv("TPST_LOOKUP_SLOTS_LOG2", "11")
    assert err_of(lambda: st.run(1))[0] == E_ARG                        # fewer slots than table entries
    monkeypatch.setenv("TPST_LOOKUP_SLOTS_LOG2", "32")
    assert err_of(lambda: st.run(1))[0] == E_ARG


def test_full_index_reports_a_non_member(ctx, monkeypatch):
    """load factor 1 and a value that is not in the table: the probe ends after one turn round the index"""
    st, _ = n12_default(ctx, "perm")
    bad = [list(a) for a in st.As]
    bad[1][77] = (st.t[0] + 1) % R
    assert bad[1][77] not in st.t
    monkeypatch.setenv("TPST_LOOKUP_SLOTS_LOG2", "12")
    rc, msg = err_of(lambda: Staged(ctx, bad, st.t).run(1))
    assert rc == E_ARG and "witness 1 entry 77 " in msg


def test_stages_default_grid_n21(ctx):
    """n = 21, L = 2 at the shipped grid: the range table, uniform witnesses.  m is np.bincount; h_l and h_t are
    multiplied back at 4096 seeded positions; sum_l s_l = s_t."""
    n, L = 21, 2
    N = 1 << n
    rng = np.random.default_rng(0x10D2)
    A = [rng.integers(0, N, N, dtype=np.uint64) for _ in range(L)]
    wits = []
    for a in A:
        Z = np.zeros((N, 4), dtype=np.uint64)
        Z[:, 0] = a
        wits.append(S.Polynomial.from_evaluations(ctx, Z))
    table = S.range_table(ctx, n)
    beta = beta_of(n, L)
    m, h, s = S.lookup_stages(wits, table, fr_array([beta])[0])
    want = sum(np.bincount(a.astype(np.int64), minlength=N) for a in A).astype(np.uint64)
    assert not m[:, 1:].any() and np.array_equal(m[:, 0], want)
    pos = random.Random(0x10D3).sample(range(N), 4096)
    for l in range(L):
        assert all(limbs_to_int(h[l][x]) * (beta + int(A[l][x])) % R == 1 for x in pos), l
    assert all(limbs_to_int(h[L][y]) * (beta + y) % R == int(want[y]) for y in pos)
    sv = ints(s)
    assert sum(sv[:L]) % R == sv[L] != 0


# ------------------------------------------------------------------ errors ---
@pytest.mark.parametrize("n,L", [(6, 2), (12, 1)])
def test_a_non_member_is_reported_with_the_least_index(ctx, n, L):
    As, t = make_case("range", n, L)
    N = 1 << n
    table = S.Polynomial.from_evaluations(ctx, fr_array(t))

    def run(bad):
        wits = [S.Polynomial.from_evaluations(ctx, fr_array(a)) for a in bad]
        return err_of(lambda: S.lookup_stages(wits, table, fr_array([5])[0]))

    for l, x in ((0, 0), (L - 1, N // 2 + 1), (L - 1, N - 1)):          # the first, a middle, the last entry
        bad = [list(a) for a in As]
        bad[l][x] = N                                                   # one past the range
        rc, msg = run(bad)
        assert rc == E_ARG and "witness %d entry %d " % (l, x) in msg, (l, x, msg)
    # several non-members: the least (l, x) is the one named; a value that differs from a member in the top word
    bad = [list(a) for a in As]
    bad[L - 1][N - 1] = N + 5
    bad[L - 1][3] = 7 + (1 << 224)
    bad[0][N - 2] = R - 1
    rc, msg = run(bad)
    want = (0, N - 2) if L > 1 else (0, 3)
    assert rc == E_ARG and "witness %d entry %d " % want in msg, msg
    assert run(As)[0] == OK


def test_a_zero_denominator_is_reported(ctx):
    n, L = 6, 2
    As, t = make_case("repeat4", n, L)
    st = Staged(ctx, As, t)
    x = 11
    rc, msg = err_of(lambda: st.run((R - As[0][x]) % R))                # beta = -a_0(x)
    assert rc == E_ARG and "= 0 at index %d of witness 0" % As[0].index(As[0][x]) in msg, msg
    # beta = -t(y) for a value that no witness holds: the table's report, at the least index holding it
    v = t[37]
    spare = next(w for w in t if w != v)
    As2 = [[w if w != v else spare for w in a] for a in As]
    rc, msg = err_of(lambda: Staged(ctx, As2, t).run((R - v) % R))
    assert rc == E_ARG and "= 0 at index %d of the table" % t.index(v) in msg, msg
    st.check(beta_of(n, L))                                             # and the handles still serve


# ------------------------------------------------------------ lookup_open ----
class Setup:
    """L committed witnesses and a committed table of one n on the loaded SRS"""

    def __init__(self, ctx, As, t):
        self.ctx, self.As, self.t = ctx, As, t
        self.L, self.n = len(As), len(t).bit_length() - 1
        self.wits = [S.Polynomial.from_evaluations(ctx, fr_array(a)) for a in As]
        self.table = S.Polynomial.from_evaluations(ctx, fr_array(t))
        self.commitments = [p.commit() for p in self.wits + [self.table]]
        self.Ts = [T for _, T in self.commitments]

    def open(self, label):
        return S.lookup_open(self.wits, self.table, self.commitments, fresh(label))

    def check(self, label):
        """lookup_open == the restatement on every T, u, s, coefficient and rho'; its closing == open_multi on a
        transcript advanced by the restated steps 1-5; lookup_reduce and verify_lookup accept; equal end states"""
        n, L = self.n, self.L
        B = 2 * L + 3
        tr = fresh(label)
        proof, comms, T, v = S.lookup_open(self.wits, self.table, self.commitments, tr)
        # the restatement, with the helper commitments taken from the library's own commit of the restated tables
        helper = []

        def commit_T(table):
            p = S.Polynomial.from_evaluations(self.ctx, fr_array(table))
            helper.append((p, p.commit()))
            return gt_oracle(helper[-1][1][1])

        ref = ref_fresh(label)
        rp, tables, rho2 = LR.prove_reduction(ref, self.As, self.t, [gt_oracle(x) for x in self.Ts], commit_T)
        assert np.array_equal(proof.T_m, helper[0][1][1])
        assert all(np.array_equal(proof.T_h[k], helper[k + 1][1][1]) for k in range(L + 1))
        assert [tuple(ints(r)) for r in proof.rounds] == [tuple(cs) for cs in rp["rounds"]]
        assert ints(proof.u) == rp["u"] and ints(proof.s) == rp["s"]
        assert [tuple(ints(r)) for r in proof.mp_rounds] == [tuple(cs) for cs in rp["mp_rounds"]]
        assert ints(proof.mp_u) == rp["mp_u"] and ints(proof.rho) == rho2
        # the parent path of the closing: the restated steps 1-5 on a library transcript, then open_multi
        tp = fresh(label)
        rho_sc = self.advance(tp, proof)
        polys = self.wits + [self.table] + [p for p, _ in helper]
        commitments = self.commitments + [c for _, c in helper]
        claims = [(j, fr_array(pt), fr_array([val])[0])
                  for j, pt, val in LR.lookup_claims(L, n, rho_sc, rp["u"], rp["s"])]
        mp, prho, pc, pT, pv = S.open_multi(polys, commitments, tp, claims)
        assert np.array_equal(mp.rounds, proof.mp_rounds) and np.array_equal(mp.u, proof.mp_u)
        assert np.array_equal(prho, proof.rho)
        assert np.array_equal(comms, pc) and np.array_equal(T, pT) and np.array_equal(v, pv)
        assert same_proof((proof.U, proof.pst_proof, proof.mipp), (mp.U, mp.pst_proof, mp.mipp))
        assert bytes(tr.t) == bytes(tp.t)
        # the verifier's halves
        tv = fresh(label)
        got = S.lookup_reduce(tv, n, self.Ts, proof)
        assert got is not None and np.array_equal(got, proof.rho)
        assert bytes(tv.t) == LR.transcript_bytes(ref)
        tv = fresh(label)
        assert S.verify_lookup(self.ctx, tv, self.Ts, proof)
        assert bytes(tv.t) == bytes(tr.t) != bytes(fresh(label).t)
        assert len(proof.u) == B
        return proof

    def advance(self, tp, proof):
        """steps 1-5 on a library transcript from the proof's parts, restated with the public calls: returns the
        sum-check's rho as integers"""
        n, L = self.n, self.L
        lib = tp.lib

        def append_int(x):
            lib.tpst_transcript_append_fr(C.byref(tp.t), ptr(fr_array([x])))

        append_int(L)
        append_int(n)
        for T in self.Ts:
            tp.append_gt(T)
        tp.append_gt(proof.T_m)
        beta = limbs_to_int(tp.challenge_scalar())
        for T in proof.T_h:
            tp.append_gt(T)
        tau = [limbs_to_int(tp.challenge_scalar()) for _ in range(n)]
        lam = limbs_to_int(tp.challenge_scalar())
        terms, claim = LR.lookup_terms(L, beta, lam)
        Tall = self.Ts + [proof.T_m] + list(proof.T_h)
        rho = S.sumcheck_reduce(tp, n, [(fr_array([c])[0], idx) for c, idx in terms], fr_array(tau), Tall,
                                fr_array([claim])[0], proof.rounds, proof.u)
        assert rho is not None
        return ints(rho)


_SETUPS = {}


def golden_setup(ctx, n, L, kind):
    """the golden SRS of n loaded and the case committed, once per (n, L, kind)"""
    d = G.load("sqrt_pst_n%d.json" % n)
    S.srs_load(ctx, d["srs_nv"], G.srs_flat(d))
    if (n, L, kind) not in _SETUPS:
        _SETUPS[(n, L, kind)] = Setup(ctx, *make_case(kind, n, L, 0x10D4))
    return _SETUPS[(n, L, kind)]


@pytest.mark.parametrize("n", [4, 5, 6, 7])
@pytest.mark.parametrize("L", [1, 2, 3])
def test_lookup_open_equals_restatement_and_parent_path(ctx, n, L):
    kind = ["range", "repeat4", "edge"][(n + L) % 3]
    golden_setup(ctx, n, L, kind).check(b"lookup %d %d" % (n, L))


def test_seeded_srs_n12_l2(ctx):
    S.srs_setup(ctx, 6, 0x7E57D1)
    Setup(ctx, *make_case("range", 12, 2, 0x10D5)).check(b"n12")


# -------------------------------------------------------------- rejections ---
def raw_verify(ctx, tr, n, Ts, proof, inner=None, n_proof=None, L=None, **kw):
    """tpst_pst_verify_lookup with proof parts replaced by keyword -> rc"""
    tl = [np.ascontiguousarray(T, dtype=np.uint64).reshape(72) for T in Ts]
    part = lambda k: np.ascontiguousarray(kw.get(k, getattr(proof, k)), dtype=np.uint64)  # noqa: E731
    th = np.ascontiguousarray(np.concatenate([part("T_m").reshape(1, 72), part("T_h").reshape(-1, 72)]))
    pr = S.pack_proof(n if n_proof is None else n_proof,
                      *((proof.U, proof.pst_proof, proof.mipp) if inner is None else inner))
    arrs = [th, part("rounds"), part("u"), part("s"), part("mp_rounds"), part("mp_u")]
    return ctx.lib.tpst_pst_verify_lookup(ctx.h, C.addressof(tr.t), n, len(tl) - 1 if L is None else L,
                                          S._ptr_array(tl), *[ptr(a) for a in arrs], C.byref(pr))


def bump(a, *index):
    """a copy of a limb array with one Fr at `index` incremented mod r"""
    b = np.array(a, dtype=np.uint64, copy=True)
    b[index] = fr_array([(limbs_to_int(b[index]) + 1) % R])[0]
    return b


def test_rejections(ctx):
    """every tamper: TPST_E_VERIFY and the transcript untouched; the untampered call: TPST_OK, advanced"""
    n, L = 6, 2
    B = 2 * L + 3
    s = golden_setup(ctx, n, L, "repeat4")
    label = b"reject"
    proof, _, _, _ = s.open(label)
    start = bytes(fresh(label).t)

    def rejected(Ts=s.Ts, **kw):
        tr = fresh(label)
        rc = raw_verify(ctx, tr, n, Ts, proof, **kw)
        return rc == E_VERIFY and bytes(tr.t) == start

    tr = fresh(label)
    assert raw_verify(ctx, tr, n, s.Ts, proof) == OK and bytes(tr.t) != start
    assert rejected(T_m=proof.T_h[0])                                             # T_m
    for k in range(L + 1):                                                        # a T_h
        th = proof.T_h.copy()
        th[k] = proof.T_m
        assert rejected(T_h=th), k
    assert rejected(T_h=proof.T_h[[1, 0, 2]])                                     # swapped h_0 / h_1
    assert rejected(Ts=[s.Ts[1], s.Ts[0], s.Ts[2]])
    for k in range(L + 1):                                                        # each s, s_t the last
        assert rejected(s=bump(proof.s, k)), k
    assert rejected(s=bump(bump(proof.s, 0), L))                                  # sum_l s_l = s_t kept, values wrong
    for i in (0, n // 2, n - 1):
        for c in range(4):
            assert rejected(rounds=bump(proof.rounds, i, c)), (i, c)
        for c in range(3):
            assert rejected(mp_rounds=bump(proof.mp_rounds, i, c)), (i, c)
    for j in range(B):
        assert rejected(u=bump(proof.u, j)), j
        assert rejected(mp_u=bump(proof.mp_u, j)), j
    # a value >= r in every scalar field, a T coefficient >= p
    for key, index in (("rounds", (1, 3)), ("mp_rounds", (2, 0)), ("u", (0,)), ("mp_u", (B - 1,)), ("s", (L,)),
                       ("s", (0,))):
        big = np.array(getattr(proof, key), copy=True)
        big[index] = fr_array([R + 3])[0]
        assert rejected(**{key: big}), key
    big = proof.T_h.copy()
    big[1, 5] = np.uint64(2**64 - 1)
    assert rejected(T_h=big)
    # the inner opening: one field each of U, pst_proof, comms_t and final_a replaced by another valid element
    other, _, _, _ = s.open(b"other")
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
    # a proof spliced from two statements: the same table, other witnesses
    s3 = Setup(ctx, [s.As[1], s.As[0]], s.t)                                      # the witnesses swapped
    p3, _, _, _ = s3.open(label)
    tr = fresh(label)
    assert raw_verify(ctx, tr, n, s3.Ts, p3) == OK
    tr = fresh(label)
    assert raw_verify(ctx, tr, n, s.Ts, p3) == E_VERIFY and bytes(tr.t) == start
    assert rejected(rounds=p3.rounds, u=p3.u)
    assert rejected(s=p3.s, mp_rounds=p3.mp_rounds, mp_u=p3.mp_u)
    assert rejected(inner=(p3.U, p3.pst_proof, p3.mipp))


def test_a_beta_drawn_before_t_m_is_rejected(ctx):
    """the unsound ordering: the restated prover with beta squeezed before T_m is absorbed, on the library's own
    commitments of its helper tables; the same prover under the stated ordering passes the reduction"""
    n, L = 5, 2
    s = golden_setup(ctx, n, L, "range")
    label = b"early"
    honest, _, _, _ = s.open(label)
    start = bytes(fresh(label).t)

    def commit_T(table):
        return gt_oracle(S.Polynomial.from_evaluations(ctx, fr_array(table)).commit()[1])

    def restated(**kw):
        rp, _, _ = LR.prove_reduction(ref_fresh(label), s.As, s.t, [gt_oracle(x) for x in s.Ts], commit_T, **kw)
        return S.LookupProof(gt_limbs(rp["T_m"]), np.stack([gt_limbs(T) for T in rp["T_h"]]),
                             fr_array([c for cs in rp["rounds"] for c in cs]).reshape(n, 4, 4), fr_array(rp["u"]),
                             fr_array(rp["s"]), fr_array([c for cs in rp["mp_rounds"] for c in cs]).reshape(n, 3, 4),
                             fr_array(rp["mp_u"]), honest.U, honest.pst_proof, honest.mipp)

    tr = fresh(label)
    assert S.lookup_reduce(tr, n, s.Ts, restated()) is not None and bytes(tr.t) != start
    forged = restated(beta_early=True)
    tr = fresh(label)
    assert S.lookup_reduce(tr, n, s.Ts, forged) is None and bytes(tr.t) == start
    assert not S.verify_lookup(ctx, tr, s.Ts, forged) and bytes(tr.t) == start


def test_a_non_member_cannot_be_proved(ctx):
    """the prover returns TPST_E_ARG with the least index and leaves the transcript alone"""
    n, L = 5, 2
    s = golden_setup(ctx, n, L, "range")
    bad = [list(a) for a in s.As]
    bad[1][9] = 1 << n
    sb = Setup(ctx, bad, s.t)
    tr = fresh(b"bad")
    rc, msg = err_of(lambda: S.lookup_open(sb.wits, sb.table, sb.commitments, tr))
    assert rc == E_ARG and "witness 1 entry 9 " in msg
    assert bytes(tr.t) == bytes(fresh(b"bad").t)


# ------------------------------------------------------------------ misuse ---
def test_misuse(ctx):
    import torch
    from testudo_amd import Context
    n, L = 5, 2
    s = golden_setup(ctx, n, L, "range")
    tr = fresh()
    beta = fr_array([9])[0]
    opened = lambda wits, table: err_of(  # noqa: E731
        lambda: S.lookup_open(wits, table, s.commitments[:len(wits)] + s.commitments[-1:], tr))[0]
    staged = lambda wits, table: err_of(lambda: S.lookup_stages(wits, table, beta))[0]              # noqa: E731
    for call in (opened, staged):
        p4 = S.Polynomial.from_evaluations(ctx, fr_array(list(range(16))))
        assert call([s.wits[0], p4], s.table) == E_ARG                             # differing n
        assert call(s.wits, p4) == E_ARG
        pq = S.Polynomial.from_q(ctx, n, fr_array([1] * n), torch.zeros(4 << (n - n // 2), dtype=torch.int64))
        assert call([s.wits[0], pq], s.table) == E_STATE                           # a from_q handle
        cols = S.Polynomial.from_evaluations_cols(ctx, fr_array(s.As[1]), 0, 2)
        assert call([s.wits[0], cols], s.table) == E_STATE                         # a column slice
        assert call([], s.table) == E_ARG                                          # L = 0
    assert err_of(lambda: S.lookup_stages(s.wits * 5, s.table, beta))[0] == E_ARG  # L = 10
    assert err_of(lambda: S.lookup_stages(s.wits, s.table, fr_array([R])[0]))[0] == E_ARG   # beta >= r
    hs = (C.c_void_p * 2)(s.wits[0].h, None)                                       # a null handle
    out = np.zeros((3 << n) * 4 + 64, dtype=np.uint64)
    assert ctx.lib.tpst_poly_lookup_stages(ctx.h, hs, 2, s.table.h, ptr(beta), ptr(out), ptr(out), ptr(out)) == E_ARG
    assert ctx.lib.tpst_poly_lookup_stages(ctx.h, hs, 1, s.table.h, None, ptr(out), ptr(out), ptr(out)) == E_ARG
    assert bytes(tr.t) == bytes(fresh().t)
    # no SRS loaded: a fresh context; the stages entry needs none
    other = Context(0)
    try:
        wits = [S.Polynomial.from_evaluations(other, fr_array(a)) for a in s.As]
        table = S.Polynomial.from_evaluations(other, fr_array(s.t))
        assert err_of(lambda: S.lookup_open(wits, table, s.commitments, tr))[0] == E_STATE
        assert err_of(lambda: S.lookup_stages([wits[0], s.wits[1]], table, beta))[0] == E_ARG   # another context
        m, h, sv = S.lookup_stages(wits, table, beta)
        wm, wh, ws = expected(s.As, s.t, 9)
        assert ints(m) == wm and [ints(x) for x in h] == wh and ints(sv) == ws
        del wits, table
    finally:
        other.close()
    assert bytes(tr.t) == bytes(fresh().t)
    # the verifier: sizes that do not match the loaded SRS
    proof, _, _, _ = s.open(None)
    tv = fresh()
    golden_setup(ctx, 7, L, "range")
    assert raw_verify(ctx, tv, n, s.Ts, proof) == E_ARG
    assert bytes(tv.t) == bytes(fresh().t)
    golden_setup(ctx, n, L, "range")
    assert raw_verify(ctx, tv, n, s.Ts, proof, L=0) == E_ARG and bytes(tv.t) == bytes(fresh().t)
    assert S.verify_lookup(ctx, tv, s.Ts, proof) and bytes(tv.t) != bytes(fresh().t)
