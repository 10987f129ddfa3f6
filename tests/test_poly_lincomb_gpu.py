"""GPU tests of the two kernels of csrc/poly_lincomb.hip alone, bit-exact.

k_fr_lincomb (tpst_poly_lincomb) against Python integers: n = 4 (16 entries,
less than a wave), 7 and 13 (32 workgroups); B = 1, 2, 5, 33; weights 0, 1,
r - 1, 2^128 - 1 and random; entries 0, r - 1 and random.

k_g1_lincomb_rows (tpst_g1_lincomb_rows) against oracle/py/bls377.py: the
points are k G for known k (0 = infinity), so the expected row is
(sum_j w_j k_j mod r) G -- one oracle scalar multiplication per row.  (C, B) =
(1, 1), (3, 2), (4, 5), (17, 3) (two workgroups), (4, 33) (the terms dealt to
16 chains, some with three terms)."""
import ctypes
import random

import numpy as np
import pytest

import bls377 as O
from testudo_amd import sqrt_pst as S
from testudo_amd.encoding import fr_array, g1_array, g1_from_array, limbs_to_int, ptr

pytestmark = pytest.mark.gpu

R, P = O.R, O.P
E_ARG, E_STATE = -1, -4
SPECIAL_W = [0, 1, R - 1, 2**128 - 1]


def rc_of(fn):
    """the return code in a TpstError's message, 0 if none was raised"""
    try:
        fn()
    except S.TpstError as e:
        return int(str(e).split("(")[1].split(")")[0])
    return 0


def table(rng, n):
    Z = [rng.randrange(R) for _ in range(1 << n)]
    Z[0], Z[1], Z[-1] = 0, R - 1, R - 1
    Z[rng.randrange(2, (1 << n) - 1)] = 0
    return Z


def weights(rng, B, shift):
    w = [SPECIAL_W[(j + shift) % 4] if j % 2 == 0 else rng.randrange(R) for j in range(B)]
    return w


# --------------------------------------------------------------- k_fr_lincomb
@pytest.mark.parametrize("n", [4, 7, 13])
@pytest.mark.parametrize("B", [1, 2, 5, 33])
def test_fr_lincomb(ctx, n, B):
    rng = random.Random(0xF1 + 64 * n + B)
    Zs = [table(rng, n) for _ in range(B)]
    polys = [S.Polynomial.from_evaluations(ctx, fr_array(Z)) for Z in Zs]
    for shift in range(4 if B < 33 else 1):
        w = weights(rng, B, shift)
        got = S.Polynomial.lincomb(polys, fr_array(w)).evaluations()
        want = [sum(wj * Z[i] for wj, Z in zip(w, Zs)) % R for i in range(1 << n)]
        assert np.array_equal(got, fr_array(want)), (n, B, shift)


def test_fr_lincomb_cancels(ctx):
    """Z_b = r - Z_a under equal weights: all zeros (also with a third, zero-weighted table)"""
    rng = random.Random(0xF2)
    for n in (4, 7):
        Za = table(rng, n)
        Zb = [(R - z) % R for z in Za]
        pa, pb = (S.Polynomial.from_evaluations(ctx, fr_array(Z)) for Z in (Za, Zb))
        for wv in (1, R - 1, 2**128 - 1, rng.randrange(R)):
            out = S.Polynomial.lincomb([pa, pb], fr_array([wv, wv])).evaluations()
            assert not out.any()
            out = S.Polynomial.lincomb([pa, pb, pa], fr_array([wv, wv, 0])).evaluations()
            assert not out.any()
        # the same handle twice is two terms
        out = S.Polynomial.lincomb([pa, pa], fr_array([3, R - 2])).evaluations()
        assert np.array_equal(out, fr_array(Za))


def test_fr_lincomb_misuse(ctx):
    from testudo_amd import Context
    rng = random.Random(0xF3)
    Z4, Z5 = table(rng, 4), table(rng, 5)
    p4 = S.Polynomial.from_evaluations(ctx, fr_array(Z4))
    p5 = S.Polynomial.from_evaluations(ctx, fr_array(Z5))
    one = fr_array([1, 1])
    assert rc_of(lambda: S.Polynomial.lincomb([p4, p5], one)) == E_ARG             # differing n
    assert rc_of(lambda: S.Polynomial.lincomb([p4, p4], fr_array([1, R]))) == E_ARG  # weight >= r
    assert rc_of(lambda: S.Polynomial.lincomb([p4] * 257, fr_array([1] * 257))) == E_ARG
    h = ctypes.c_void_p()
    assert ctx.lib.tpst_poly_lincomb(ctx.h, None, 0, ptr(one), ctypes.byref(h)) == E_ARG
    hs = (ctypes.c_void_p * 1)(p4.h)
    assert ctx.lib.tpst_poly_lincomb(ctx.h, hs, 0, ptr(one), ctypes.byref(h)) == E_ARG     # B = 0
    assert ctx.lib.tpst_poly_lincomb(ctx.h, hs, 1, None, ctypes.byref(h)) == E_ARG
    cols = S.Polynomial.from_evaluations_cols(ctx, fr_array(Z4), 1, 3)
    assert rc_of(lambda: S.Polynomial.lincomb([p4, cols], one)) == E_STATE
    assert rc_of(cols.evaluations) == E_STATE
    other = Context(0)
    try:
        po = S.Polynomial.from_evaluations(other, fr_array(Z4))
        assert rc_of(lambda: S.Polynomial.lincomb([p4, po], one)) == E_ARG          # another context's handle
        del po
    finally:
        other.close()
    assert np.array_equal(S.Polynomial.lincomb([p4, p4], one).evaluations(), fr_array([2 * z % R for z in Z4]))


# ---------------------------------------------------------- k_g1_lincomb_rows
_MUL = {}


def kG(k):
    """k G of the oracle (None for k = 0 mod r), memoised"""
    k %= R
    if k not in _MUL:
        _MUL[k] = O.g1_mul(O.G1_GEN, k) if k else None
    return _MUL[k]


def lists_of(ks):
    """ks[j][i] -> B arrays of (C, 12) canonical affine points"""
    return [g1_array([kG(k) for k in row]) for row in ks]


def check_rows(ctx, ks, w):
    got = S.g1_lincomb_rows(ctx, lists_of(ks), fr_array(w))
    want = [kG(sum(wj * row[i] for wj, row in zip(w, ks))) for i in range(len(ks[0]))]
    assert np.array_equal(got, g1_array(want))
    return got


def scalars(rng, C, B):
    """small multiples of G (cheap for the oracle), infinity at some rows of some lists"""
    ks = [[rng.randrange(1, 1 << 20) for _ in range(C)] for _ in range(B)]
    for j in range(0, B, 2):
        ks[j][rng.randrange(C)] = 0
    return ks


SHAPES = [(1, 1), (3, 2), (4, 5), (17, 3), (4, 33)]


@pytest.mark.parametrize("C,B", SHAPES)
def test_rows_weight_sets(ctx, C, B):
    rng = random.Random(0x6A + 64 * C + B)
    ks = scalars(rng, C, B)
    sets = {
        "short": [rng.getrandbits(128) for _ in range(B)],
        "bit 252": [(1 << 252) | rng.getrandbits(200) if j == B // 2 else rng.getrandbits(128) for j in range(B)],
        "full": [rng.randrange(R) for _ in range(B)],
        "single bits": [1 << ((37 * j + 5) % 252) for j in range(B)],
        "a zero weight": [0 if j == B - 1 else rng.randrange(R) for j in range(B)],
        "all zero": [0] * B,
    }
    for name, w in sets.items():
        got = check_rows(ctx, ks, w)
        if name == "all zero":
            assert not got.any()


@pytest.fixture(params=["default", "1", "2"])
def chains(request, monkeypatch):
    """TPST_ROW_CHAINS: the default deals the terms of these small shapes one per chain (the sum kernel adds
    them); 1 puts all B terms into ONE joint chain, 2 into two"""
    if request.param != "default":
        monkeypatch.setenv("TPST_ROW_CHAINS", request.param)
    return request.param


@pytest.mark.parametrize("C,B", [(3, 2), (4, 5), (4, 33)])
def test_rows_joint_chain(ctx, chains, C, B):
    rng = random.Random(0x6D + 64 * C + B)
    ks = scalars(rng, C, B)
    check_rows(ctx, ks, [rng.randrange(R) for _ in range(B)])
    check_rows(ctx, ks, [rng.getrandbits(128) if j else 0 for j in range(B)])


def test_rows_doubling_and_cancelling(ctx, chains):
    """the same list twice: (1, 1) adds P to P at the first step, (2, r - 1) meets acc = P_j in mid-chain
    and ends at P, (1, r - 1) ends at infinity; a list that is the negation of another; infinity at every row"""
    rng = random.Random(0x6B)
    C = 3
    row = [rng.randrange(1, R) for _ in range(C)]
    for w in ((1, 1), (2, R - 1), (1, R - 1), (R - 1, R - 1), (5, R - 5)):
        got = check_rows(ctx, [row, row], list(w))
        if (w[0] + w[1]) % R == 0:
            assert not got.any()
    neg = [R - k for k in row]
    lists = lists_of([row, neg])
    # the negated list really is (x, p - y)
    a, b = g1_from_array(lists[0]), g1_from_array(lists[1])
    assert all(q == (p[0], P - p[1]) for p, q in zip(a, b))
    for w in ((7, 7), (rng.randrange(R),) * 2, (2**128 - 1, 2**128 - 1)):
        assert not check_rows(ctx, [row, neg], list(w)).any()
    check_rows(ctx, [row, neg, row], [9, 4, R - 5])            # sums to zero over three lists
    check_rows(ctx, [row, [0] * C], [rng.randrange(R), rng.randrange(R)])   # one list all infinity
    assert not check_rows(ctx, [[0] * C, [0] * C], [rng.randrange(R), 3]).any()
    # three lists, running sum equal to the next term: acc = 2 P0 + P1 = P2
    check_rows(ctx, [[5, 7, 11], [1, 2, 3], [11, 16, 25]], [2, 1, 1])
    check_rows(ctx, [[5, 7, 11], [1, 2, 3], [R - 11, R - 16, R - 25]], [2, 1, 1])


def test_rows_misuse(ctx):
    rng = random.Random(0x6C)
    ks = scalars(rng, 4, 2)
    lists = lists_of(ks)
    w = fr_array([3, 5])
    assert rc_of(lambda: S.g1_lincomb_rows(ctx, lists, fr_array([3, R]))) == E_ARG   # weight >= r
    off = [x.copy() for x in lists]
    off[1][2, 0] ^= np.uint64(1)                                                      # off the curve
    assert rc_of(lambda: S.g1_lincomb_rows(ctx, off, w)) == E_ARG
    nc = [x.copy() for x in lists]
    v = limbs_to_int(nc[0][1, 6:12]) + P                                              # y + p: not canonical
    assert v < 2**384
    nc[0][1, 6:12] = [(v >> (64 * k)) & (2**64 - 1) for k in range(6)]
    assert rc_of(lambda: S.g1_lincomb_rows(ctx, nc, w)) == E_ARG
    assert rc_of(lambda: S.g1_lincomb_rows(ctx, [], np.zeros((0, 4), dtype=np.uint64))) == E_ARG   # B = 0
    assert rc_of(lambda: S.g1_lincomb_rows(ctx, [lists[0]] * 257, fr_array([1] * 257))) == E_ARG
    out = np.zeros((4, 12), dtype=np.uint64)
    pa = S._ptr_array(lists)
    assert ctx.lib.tpst_g1_lincomb_rows(ctx.h, pa, 2, 0, ptr(w), ptr(out)) == E_ARG                 # C = 0
    assert ctx.lib.tpst_g1_lincomb_rows(ctx.h, None, 2, 4, ptr(w), ptr(out)) == E_ARG
    assert ctx.lib.tpst_g1_lincomb_rows(ctx.h, pa, 2, 4, ptr(w), None) == E_ARG
    check_rows(ctx, ks, [3, 5])
