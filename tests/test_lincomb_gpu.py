"""GPU tests of the batched double-scalar multiplication (csrc/lincomb.hip,
tpst_g1_lincomb_batch / tpst_g2_lincomb_batch): out[i] = s_i P_i + t_i Q_i against
the integer arithmetic of oracle/py/bls377.py, both curves.

The kernel maps one quad of lanes to an output, 16 outputs to a block, and
tabulates P, Q, P + Q per quad; the cases are those in which the joint
double-and-add leaves the generic formulas: zero scalars, P = Q (the table
entry is a doubling), P = Q with s + t = 0 mod r (a result at infinity after
253 steps), P = -Q (the entry is infinity), inputs at infinity, s = r - 1
(every addition branch over a full-length scalar), 128-bit scalars without Q
(the short walk), n = 1 (one live quad in the block) and n = 257 (17 blocks,
a ragged last one).  The oracle's points are computed once per curve."""
import random

import numpy as np
import pytest

import bls377 as O
from testudo_amd.encoding import fr_array, g1_array, g1_from_array, g2_array, g2_from_array

pytestmark = pytest.mark.gpu

E_ARG = -1
R = O.R


class Curve:
    def __init__(self, g2: bool):
        self.g2 = g2
        self.gen, self.mul, self.add, self.neg = ((O.G2_GEN, O.g2_mul, O.g2_add, O.g2_neg) if g2 else
                                                  (O.G1_GEN, O.g1_mul, O.g1_add, O.g1_neg))
        self.arr, self.back = (g2_array, g2_from_array) if g2 else (g1_array, g1_from_array)
        rng = random.Random(0x11C0 + g2)
        self.rng = rng
        # a pool of subgroup points (the oracle's scalar multiplication is the slow part)
        self.pool = [self.mul(self.gen, rng.randrange(1, R)) for _ in range(6)]
        self._cases = None

    def call(self, ctx, P, s, Q=None, t=None):
        fn = ctx.g2_lincomb_batch if self.g2 else ctx.g1_lincomb_batch
        out = fn(self.arr(P), fr_array(s), None if Q is None else self.arr(Q), None if t is None else fr_array(t))
        return self.back(out)

    def lin(self, P, s, Q, t):
        return self.add(self.mul(P, s) if P is not None and s else None, self.mul(Q, t) if Q is not None and t else None)

    def cases(self):
        """(name, P, s, Q, t, expected) for about 40 elements, expected from the oracle"""
        if self._cases is None:
            rng, pool = self.rng, self.pool
            A, Bp, Cp = pool[0], pool[1], pool[2]
            rs = lambda: rng.randrange(1, R)  # noqa: E731
            rows = [("random %d" % k, pool[k % 6], rs(), pool[(k + 1) % 6], rs()) for k in range(12)]
            s0, t0 = rs(), rs()
            rows += [
                ("s = 0", A, 0, Bp, t0), ("t = 0", A, s0, Bp, 0), ("s = t = 0", A, 0, Bp, 0),
                ("P = Q", A, s0, A, t0), ("P = Q, s + t = 0", A, s0, A, R - s0), ("P = Q, s = t = 1", A, 1, A, 1),
                ("P = -Q", A, s0, self.neg(A), t0), ("P = -Q, s = t", A, s0, self.neg(A), s0),
                ("P at infinity", None, s0, Bp, t0), ("Q at infinity", A, s0, None, t0),
                ("both at infinity", None, s0, None, t0),
                ("s = r - 1", A, R - 1, Bp, t0), ("s = t = r - 1", A, R - 1, Bp, R - 1), ("s = 1, t = 0", Cp, 1, A, 0),
                ("s = 2^252", A, 1 << 252, Bp, 1), ("t = 2^127", A, 3, Bp, 1 << 127),
            ]
            rows += [("random tail %d" % k, pool[(k + 2) % 6], rs(), pool[(k + 5) % 6], rs()) for k in range(12)]
            self._cases = [(nm, P, s, Q, t, self.lin(P, s, Q, t)) for nm, P, s, Q, t in rows]
        return self._cases


_CURVES = {}


def curve(g2):
    if g2 not in _CURVES:
        _CURVES[g2] = Curve(g2)
    return _CURVES[g2]


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
def test_lincomb_cases(ctx, g2):
    """every case of the module docstring in one batch of 40 (three blocks, the last ragged)"""
    c = curve(g2)
    rows = c.cases()
    assert len(rows) == 40
    out = c.call(ctx, [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows], [r[4] for r in rows])
    for (name, *_, want), got in zip(rows, out):
        assert got == want, name
    assert any(r[5] is None for r in rows)  # results at infinity are among them


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
def test_lincomb_single(ctx, g2):
    """n = 1: one live quad, the other 15 of the block idle"""
    c = curve(g2)
    name, P, s, Q, t, want = c.cases()[0]
    assert c.call(ctx, [P], [s], [Q], [t]) == [want]
    name, P, s, Q, t, want = c.cases()[16]  # P = Q, s + t = 0: infinity
    assert want is None and c.call(ctx, [P], [s], [Q], [t]) == [None]


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
def test_lincomb_short_scalars_without_q(ctx, g2):
    """128-bit s with Q = t = NULL (the batch verifier's multipliers), zero and the largest 128-bit value
    included"""
    c = curve(g2)
    rng = random.Random(0x5107 + g2)
    s = [rng.getrandbits(128) for _ in range(6)] + [0, (1 << 128) - 1, 1]
    P = [c.pool[k % 6] for k in range(len(s) - 1)] + [None]
    want = [c.mul(p, k) if p is not None and k else None for p, k in zip(P, s)]
    assert c.call(ctx, P, s) == want


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
def test_lincomb_many_blocks(ctx, g2):
    """n = 257: 17 blocks of 16 quads, one live quad in the last.  The 40 cases repeated, so every output has
    an oracle value and a wrong index (an output written by another quad) shows."""
    c = curve(g2)
    rows = c.cases()
    idx = [(7 * k + 3) % len(rows) for k in range(257)]
    out = c.call(ctx, [rows[i][1] for i in idx], [rows[i][2] for i in idx], [rows[i][3] for i in idx],
                 [rows[i][4] for i in idx])
    assert out == [rows[i][5] for i in idx]


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
def test_lincomb_rejects_bad_input(ctx, g2):
    """TPST_E_ARG for a scalar >= r (s and t), an off-curve point (P and Q), a coordinate >= p, and for Q
    without t; n = 0 is TPST_OK"""
    from testudo_amd.encoding import ptr
    c = curve(g2)
    fn = ctx.lib.tpst_g2_lincomb_batch if g2 else ctx.lib.tpst_g1_lincomb_batch
    w = 24 if g2 else 12
    A, Bp = c.pool[0], c.pool[1]
    good_P, good_Q = c.arr([A, Bp]), c.arr([Bp, A])
    good_s, good_t = fr_array([5, 6]), fr_array([7, 8])
    out = np.zeros((2, w), dtype=np.uint64)

    def rc(P, s, Q, t, n=2):
        return fn(ctx.h, ptr(P), ptr(s), None if Q is None else ptr(Q), None if t is None else ptr(t), n, ptr(out))

    assert rc(good_P, good_s, good_Q, good_t) == 0
    assert rc(good_P, fr_array([5, R]), good_Q, good_t) == E_ARG
    assert rc(good_P, good_s, good_Q, fr_array([R + 1, 8])) == E_ARG
    off = good_P.copy()
    off[1, 0] ^= np.uint64(1)  # x changed: off the curve
    assert rc(off, good_s, good_Q, good_t) == E_ARG
    assert rc(good_P, good_s, off, good_t) == E_ARG
    big = good_P.copy()
    big[0, :6] = [(O.P >> (64 * k)) & (2**64 - 1) for k in range(6)]  # x = p
    assert rc(big, good_s, good_Q, good_t) == E_ARG
    assert rc(good_P, good_s, good_Q, None) == E_ARG
    assert rc(good_P, good_s, None, None) == 0
    assert rc(good_P, good_s, good_Q, good_t, n=0) == 0
