"""GPU tests of the combined opening (include/tpst.h: tpst_poly_open_combined,
tpst_commit_lincomb, tpst_pst_verify_combined), bit-exact against the parent's
own path: Z* = sum_j w_j Z_j formed with Python integers, then
Polynomial.from_evaluations(Z*), commit, eval and open.  Both routes give
canonical encodings of the same group elements, so comm_list, T, v, every
proof field and the transcript end state are compared for equality.

Shapes: the golden SRS of n = 4, 5, 6, 7 (5 and 7: the odd split) with B = 1,
2, 3, 8, and one size through the seeded SRS beyond the fixtures (n = 12, 64
rows, B = 4)."""
import ctypes as C
import random

import numpy as np
import pytest

import bls377 as O
import golden_io as G
from testudo_amd import sqrt_pst as S
from testudo_amd.encoding import fr_array, limbs_to_int, ptr

pytestmark = pytest.mark.gpu

OK, E_ARG, E_STATE, E_VERIFY = 0, -1, -4, -5
R = O.R


def tr_bytes(tr):
    return bytes(tr.t)


def fresh(label=None):
    tr = S.PoseidonTranscript()
    if label is not None:
        tr.append_bytes(label)
    return tr


def rc_of(fn):
    try:
        fn()
    except S.TpstError as e:
        return int(str(e).split("(")[1].split(")")[0])
    return 0


def ints(a):
    return [limbs_to_int(x) for x in np.asarray(a).reshape(-1, 4)]


def same_proof(a, b):
    (Ua, pa, ma), (Ub, pb, mb) = a, b
    return (np.array_equal(Ua, Ub) and np.array_equal(pa, pb) and np.array_equal(ma.comms_t, mb.comms_t) and
            np.array_equal(ma.comms_u, mb.comms_u) and np.array_equal(ma.final_a, mb.final_a) and
            np.array_equal(ma.final_h, mb.final_h) and np.array_equal(ma.pst_proof_h, mb.pst_proof_h))


def golden(n):
    return G.load("sqrt_pst_n%d.json" % n)


class Setup:
    """B polynomials of one n at one point with their commitments and values"""

    def __init__(self, ctx, Zs, point):
        self.ctx, self.Zs, self.point = ctx, Zs, fr_array(point)
        self.n = len(point)
        self.polys = [S.Polynomial.from_evaluations(ctx, fr_array(Z)) for Z in Zs]
        self.commitments = [p.commit() for p in self.polys]
        self.Ts = [T for _, T in self.commitments]
        self.vs = np.stack([p.eval(self.point) for p in self.polys])

    def first(self, B):
        s = object.__new__(Setup)
        s.ctx, s.n, s.point = self.ctx, self.n, self.point
        s.Zs, s.polys, s.commitments = self.Zs[:B], self.polys[:B], self.commitments[:B]
        s.Ts, s.vs = self.Ts[:B], self.vs[:B]
        return s

    def parent(self, w, tr):
        """the parent path on Z*: (comm_list, T, v, proof); tr is advanced by the opening"""
        w = ints(w)
        Zstar = [sum(wj * Z[i] for wj, Z in zip(w, self.Zs)) % R for i in range(1 << self.n)]
        pl = S.Polynomial.from_evaluations(self.ctx, fr_array(Zstar))
        comms, T = pl.commit()
        v = pl.eval(self.point)
        return comms, T, v, pl.open(tr, comms, self.point, T)

    def check(self, w=None, label=None):
        """open_combined == the parent path, value for value, and both verifiers accept both proofs with equal
        transcript end states.  w None: the weights come from combine_challenge on the opening's transcript."""
        derived = w is None
        tr_c, tr_p = fresh(label), fresh(label)
        wc, comms, T, v, proof = S.open_combined(self.polys, self.commitments, tr_c, self.point, w)
        if derived:
            w = S.combine_challenge(tr_p, self.point, self.Ts, self.vs)
            assert limbs_to_int(w[0]) == 1
        assert np.array_equal(wc, w)
        pc, pT, pv, pproof = self.parent(wc, tr_p)
        assert np.array_equal(comms, pc) and np.array_equal(T, pT) and np.array_equal(v, pv)
        assert same_proof(proof, pproof)
        assert tr_bytes(tr_c) == tr_bytes(tr_p) != tr_bytes(fresh(label))
        assert limbs_to_int(v) == sum(a * b for a, b in zip(ints(wc), ints(self.vs))) % R

        def start():  # the verifier's transcript where the opening started
            tr = fresh(label)
            if derived:
                assert np.array_equal(S.combine_challenge(tr, self.point, self.Ts, self.vs), wc)
            return tr

        # cross-acceptance: the parent's verifier on the combined proof with (T*, v*), the combined verifier
        # on the parent's proof, equal end states
        tv, tc = start(), start()
        assert S.verify(self.ctx, tv, proof[0], self.point, v, proof[1], proof[2], T)
        assert S.verify_combined(self.ctx, tc, pproof[0], self.point, self.vs, pproof[1], pproof[2], self.Ts, wc)
        assert tr_bytes(tv) == tr_bytes(tc) == tr_bytes(tr_c)
        return wc, comms, T, v, proof


_SETUPS = {}


def golden_setup(ctx, n):
    """the golden SRS of n loaded, and 8 polynomials at the golden point (polynomial 0 is the fixture's own),
    built once per n"""
    d = golden(n)
    S.srs_load(ctx, d["srs_nv"], G.srs_flat(d))
    if n not in _SETUPS:
        Zs = [[G.i(x) for x in d["Z"]]]
        for j in range(1, 8):
            Zs.append(ints(S.fr_stream(0xC0B0 + 16 * n + j, 1 << n)[0]))
        _SETUPS[n] = Setup(ctx, Zs, [G.i(x) for x in d["point"]])
    return d, _SETUPS[n]


# ------------------------------------------------------------ parent parity --
@pytest.mark.parametrize("n", [4, 5, 6, 7])
@pytest.mark.parametrize("B", [1, 2, 3, 8])
def test_open_combined_equals_parent_path(ctx, n, B):
    _, full = golden_setup(ctx, n)
    s = full.first(B)
    rng = random.Random(0xC0 + 16 * n + B)
    s.check(None, b"combined %d %d" % (n, B))                                  # combine_challenge
    s.check(fr_array([rng.getrandbits(128) | 1 for _ in range(B)]))            # 128-bit draws
    s.check(fr_array([rng.randrange(1, R) for _ in range(B)]))                 # full-size draws


@pytest.mark.parametrize("n", [4, 5, 6, 7])
def test_b1_w1_is_the_golden_proof(ctx, n):
    d, full = golden_setup(ctx, n)
    s = full.first(1)
    _, comms, T, v, (U, pst_proof, mipp) = s.check(fr_array([1]))
    assert np.array_equal(comms, G.g1_arr(d["comms"])) and np.array_equal(T, G.gt_array(d["T"]))
    assert np.array_equal(v, G.fr_arr([d["eval"]])[0])
    assert np.array_equal(U, G.g1_arr([d["U"]])[0]) and np.array_equal(pst_proof, G.g2_arr(d["pst_proof"]))
    assert np.array_equal(mipp.comms_t, np.stack([np.stack([G.gt_array(a), G.gt_array(b)]) for a, b in d["comms_t"]]))
    assert np.array_equal(mipp.comms_u, np.stack([G.g1_arr(pr) for pr in d["comms_u"]]))
    assert np.array_equal(mipp.final_a, G.g1_arr([d["final_a"]])[0])
    assert np.array_equal(mipp.final_h, G.g2_arr([d["final_h"]])[0])
    assert np.array_equal(mipp.pst_proof_h, G.g1_arr(d["pst_proof_h"]))


def test_commit_lincomb_parts(ctx):
    """the row list alone, T alone (what the verifier has) and both give the same values"""
    _, full = golden_setup(ctx, 5)
    s = full.first(3)
    w = fr_array([random.Random(0xC1).randrange(1, R) for _ in range(3)])
    comms, T = S.commit_lincomb(ctx, 5, [c for c, _ in s.commitments], s.Ts, w)
    only_c, none_T = S.commit_lincomb(ctx, 5, [c for c, _ in s.commitments], None, w)
    none_c, only_T = S.commit_lincomb(ctx, 5, None, s.Ts, w)
    assert none_T is None and none_c is None
    assert np.array_equal(only_c, comms) and np.array_equal(only_T, T)
    pc, pT, _, _ = s.parent(w, fresh())
    assert np.array_equal(comms, pc) and np.array_equal(T, pT)
    assert np.array_equal(S.g1_lincomb_rows(ctx, [c for c, _ in s.commitments], w), pc)
    assert np.array_equal(S.Polynomial.lincomb(s.polys, w).commit()[0], pc)


# -------------------------------------------------------------- degenerates --
def test_degenerates(ctx):
    d, full = golden_setup(ctx, 5)
    rng = random.Random(0xC2)
    Z0, point = full.Zs[0], ints(full.point)
    wv = rng.randrange(1, R)
    # the same polynomial twice
    Setup(ctx, [Z0, Z0], point).check(fr_array([wv, rng.randrange(1, R)]))
    Setup(ctx, [Z0, Z0], point).check(None)
    # Z_1 = -Z_0 under equal weights: the zero polynomial, an infinite row list, T* = 1
    neg = [(R - z) % R for z in Z0]
    _, comms, T, v, _ = Setup(ctx, [Z0, neg], point).check(fr_array([wv, wv]))
    one = np.zeros(72, dtype=np.uint64)
    one[0] = 1
    assert not comms.any() and np.array_equal(T, one) and not v.any()
    # a zero polynomial among the B: T_1 = 1
    s = Setup(ctx, [Z0, [0] * 32, full.Zs[1]], point)
    assert np.array_equal(s.Ts[1], one) and not s.commitments[1][0].any()
    s.check(None)
    s.check(fr_array([rng.getrandbits(128) | 1 for _ in range(3)]))
    # a constant polynomial
    Setup(ctx, [[7] * 32, Z0], point).check(None)
    Setup(ctx, [[R - 1] * 32], point).check(fr_array([R - 1]))


# --------------------------------------------------------------- rejections --
def raw_verify(ctx, tr, point, vs, Ts, w, proof, n=None):
    point = np.ascontiguousarray(point, dtype=np.uint64).reshape(-1, 4)
    Ts = [np.ascontiguousarray(T, dtype=np.uint64).reshape(72) for T in Ts]
    B = len(Ts)
    pr = S.pack_proof(len(point), *proof)
    vs = np.ascontiguousarray(vs, dtype=np.uint64).reshape(B, 4)
    w = np.ascontiguousarray(w, dtype=np.uint64).reshape(B, 4)
    return ctx.lib.tpst_pst_verify_combined(ctx.h, C.byref(tr.t), len(point) if n is None else n, ptr(point),
                                            ptr(vs), S._ptr_array(Ts), B, ptr(w), C.byref(pr))


def test_rejections(ctx):
    """every tamper: TPST_E_VERIFY and the transcript untouched; the untampered call: TPST_OK, advanced"""
    _, full = golden_setup(ctx, 6)
    s = full.first(3)
    rng = random.Random(0xC3)
    label = b"reject"
    w = fr_array([rng.randrange(1, R) for _ in range(3)])
    _, comms, T, v, proof = S.open_combined(s.polys, s.commitments, fresh(label), s.point, w)
    start = tr_bytes(fresh(label))

    def rejected(point=s.point, vs=s.vs, Ts=s.Ts, w=w, proof=proof):
        tr = fresh(label)
        rc = raw_verify(ctx, tr, point, vs, Ts, w, proof)
        return rc == E_VERIFY and tr_bytes(tr) == start

    tr = fresh(label)
    assert raw_verify(ctx, tr, s.point, s.vs, s.Ts, w, proof) == OK and tr_bytes(tr) != start
    vs = s.vs.copy()
    vs[1] = fr_array([(limbs_to_int(vs[1]) + 1) % R])[0]
    assert rejected(vs=vs)                                                     # one v_j changed
    assert limbs_to_int(w[0]) != limbs_to_int(w[1])
    assert rejected(Ts=[s.Ts[1], s.Ts[0], s.Ts[2]])                            # T_0, T_1 swapped
    assert rejected(w=fr_array([rng.randrange(1, R) for _ in range(3)]))       # another weight vector
    # every coordinate moved: the PST quotients do not depend on the coordinate folded last (point[0]), so a
    # point that differs only there has the very same proof
    other_point = fr_array([(x + 1) % R for x in ints(s.point)])
    other = S.open_combined(s.polys, s.commitments, fresh(label), other_point, w)
    assert rejected(proof=other[4])                                            # a proof for another point
    assert rejected(point=other_point)
    outside = s.Ts[2].copy()
    outside[0] += np.uint64(1)                                                 # < p, no longer in GT
    assert rejected(Ts=[s.Ts[0], s.Ts[1], outside])
    big = s.Ts[0].copy()
    big[5] = np.uint64(2**64 - 1)                                              # a coefficient >= p
    assert rejected(Ts=[big, s.Ts[1], s.Ts[2]])
    vs = s.vs.copy()
    vs[2] = fr_array([R])[0]
    assert rejected(vs=vs)                                                     # v_j >= r
    wz = w.copy()
    wz[1] = 0
    assert rejected(w=wz)                                                      # a zero weight
    wb = w.copy()
    wb[0] = fr_array([R + 2])[0]
    assert rejected(w=wb)                                                      # w_j >= r


# ------------------------------------------------------------------- misuse --
def test_misuse(ctx):
    from testudo_amd import Context
    _, s5 = golden_setup(ctx, 5)
    s = s5.first(2)
    w = fr_array([3, 5])
    Z4 = ints(S.fr_stream(0xC0B4, 16)[0])
    p4 = S.Polynomial.from_evaluations(ctx, fr_array(Z4))
    tr = fresh()
    assert rc_of(lambda: S.open_combined([s.polys[0], p4], s.commitments, tr, s.point, w)) == E_ARG   # differing n
    cols = S.Polynomial.from_evaluations_cols(ctx, fr_array(s.Zs[1]), 0, 2)
    assert rc_of(lambda: S.open_combined([s.polys[0], cols], s.commitments, tr, s.point, w)) == E_STATE
    other = Context(0)
    try:
        po = S.Polynomial.from_evaluations(other, fr_array(s.Zs[1]))
        assert rc_of(lambda: S.open_combined([s.polys[0], po], s.commitments, tr, s.point, w)) == E_ARG
        del po
    finally:
        other.close()
    assert rc_of(lambda: S.open_combined(s.polys, s.commitments, tr, s.point, fr_array([3, 0]))) == E_ARG  # zero weight
    assert rc_of(lambda: S.open_combined(s.polys, s.commitments, tr, s.point, fr_array([3, R]))) == E_ARG
    outside = s.Ts[1].copy()
    outside[0] += np.uint64(1)
    assert rc_of(lambda: S.commit_lincomb(ctx, 5, None, [s.Ts[0], outside], w)) == E_ARG              # T outside GT
    off = s.commitments[1][0].copy()
    off[1, 0] ^= np.uint64(1)
    assert rc_of(lambda: S.commit_lincomb(ctx, 5, [s.commitments[0][0], off], None, w)) == E_ARG       # off the curve
    assert rc_of(lambda: S.commit_lincomb(ctx, 1, None, s.Ts, w)) == E_ARG                             # bad n
    assert ctx.lib.tpst_commit_lincomb(ctx.h, 5, None, None, 2, ptr(w), None, None) == E_ARG
    assert tr_bytes(tr) == tr_bytes(fresh())
    # null arguments and B out of range of the verifier are TPST_E_ARG, not a verdict
    _, _, _, _, proof = S.open_combined(s.polys, s.commitments, fresh(), s.point, w)
    pr = S.pack_proof(5, *proof)
    pa = S._ptr_array(s.Ts)
    lib = ctx.lib
    assert lib.tpst_pst_verify_combined(ctx.h, C.byref(tr.t), 5, ptr(s.point), ptr(s.vs), pa, 0, ptr(w), C.byref(pr)) == E_ARG
    assert lib.tpst_pst_verify_combined(ctx.h, C.byref(tr.t), 5, ptr(s.point), None, pa, 2, ptr(w), C.byref(pr)) == E_ARG
    assert lib.tpst_pst_verify_combined(ctx.h, C.byref(tr.t), 5, ptr(s.point), ptr(s.vs), pa, 2, ptr(w), C.byref(pr)) == OK


# ------------------------------------------------------- beyond the fixtures --
def test_seeded_srs_n12_b4(ctx):
    """n = 12 through srs_setup: 64 rows, 4096 entries (16 workgroups of k_fr_lincomb), B = 4"""
    S.srs_setup(ctx, 6, 0x7E57D1)
    n, B = 12, 4
    Zs = [ints(S.fr_stream(0xC0BC + j, 1 << n)[0]) for j in range(B)]
    point = ints(S.fr_stream(0xC0BC, n, 1 << 13)[0])
    s = Setup(ctx, Zs, point)
    s.check(None, b"n12")
    s.check(fr_array([random.Random(0xC4).getrandbits(128) | 1 for _ in range(B)]))
