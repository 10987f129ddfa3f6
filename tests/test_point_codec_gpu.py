"""GPU tests of the batched point codec (csrc/point_codec.hip): k_point_decompress
and k_point_check against the per-point host routines tpst_de_g1 / tpst_de_g2 /
tpst_g1_check / tpst_g2_check, which define the result -- same limbs where they
accept, a rejection where they reject, first_bad = the lowest rejected index.

G1 at n = 1, 63, 64, 65, 257 and G2 at n = 1, 65: one lane per point in blocks
of 64, so these sizes are one ragged block, a full block, a block and one lane,
and several blocks with a ragged tail.  Inputs are built with oracle/py/bls377.py."""
import ctypes as C
import random

import numpy as np
import pytest

import bls377 as O
import serialize as OS  # oracle/py/serialize.py
from testudo_amd.encoding import g1_array, g2_array

pytestmark = pytest.mark.gpu

P = O.P
E_ARG, E_VERIFY = -1, -5
G1_SIZES = (1, 63, 64, 65, 257)
G2_SIZES = (1, 65)


def _le(v, n=48):
    return v.to_bytes(n, "little")


def _flag(b, fl):
    b = bytearray(b)
    b[-1] = (b[-1] & 0x3F) | fl
    return bytes(b)


class Group:
    """one group's inputs, its library calls and the per-point host verdicts (cached)"""

    def __init__(self, g2: bool):
        from testudo_amd import _lib
        lib = _lib.load()
        rng = random.Random(0xC0DEC + g2)
        self.g2, self.size, self.words = g2, 96 if g2 else 48, 24 if g2 else 12
        self.de_one = lib.tpst_de_g2 if g2 else lib.tpst_de_g1
        self.de_batch = lib.tpst_de_g2_batch if g2 else lib.tpst_de_g1_batch
        self.check_one = lib.tpst_g2_check if g2 else lib.tpst_g1_check
        self.check_batch = lib.tpst_g2_check_batch if g2 else lib.tpst_g1_check_batch
        self.arr = g2_array if g2 else g1_array
        gen, mul, neg = (O.G2_GEN, O.g2_mul, O.g2_neg) if g2 else (O.G1_GEN, O.g1_mul, O.g1_neg)
        ser = OS.ser_g2 if g2 else OS.ser_g1
        pts = [mul(gen, rng.randrange(1, O.R)) for _ in range(5)]
        self.points = pts + [neg(p) for p in pts]                    # both y signs
        self.valid = [ser(p) for p in self.points] + [ser(None)]     # and infinity
        assert {b[-1] & 0x80 for b in self.valid[:-1]} == {0, 0x80}
        self.off_subgroup = self._off_subgroup(rng)
        x_of = (lambda x: _le(x[0]) + _le(x[1])) if g2 else _le
        lift = (lambda v: (v, 0)) if g2 else (lambda v: v)
        self.bad = {
            "both flags": _flag(self.valid[0], 0xC0),
            "x = p": x_of(lift(P)),
            "x = p + 1": x_of(lift(P + 1)),
            "non-residue": x_of(self._non_residue_x(rng)),
            "off subgroup": ser(self.off_subgroup),
            "x = 0 unflagged": bytes(self.size),
        }
        if g2:
            self.bad["x.c1 = p"] = _le(1) + _le(P)
        else:
            self.bad["y = 0, positive"] = _le(P - 1)               # x = p - 1: x^3 + 1 = 0, a point of order 2
            self.bad["y = 0, negative"] = _flag(_le(P - 1), 0x80)
        # the corner the host settles the other way: the infinity flag over a canonical x != 0
        self.flagged_inf = _flag(self.valid[0], 0x40)
        self._host = {}

    def _rhs(self, x):
        if self.g2:
            r = O.f2_mul(O.f2_sqr(x), x)
            return ((r[0] + O.G2_B[0]) % P, (r[1] + O.G2_B[1]) % P)
        return (x * x * x + 1) % P

    def _rand_x(self, rng):
        return (rng.randrange(P), rng.randrange(P)) if self.g2 else rng.randrange(P)

    def _non_residue_x(self, rng):
        sqrt = OS._fq2_sqrt if self.g2 else OS._fq_sqrt
        while True:
            x = self._rand_x(rng)
            if sqrt(self._rhs(x)) is None:
                return x

    def _off_subgroup(self, rng):
        sqrt, on, sub = ((OS._fq2_sqrt, O.g2_on_curve, O.g2_in_subgroup) if self.g2
                         else (OS._fq_sqrt, O.g1_on_curve, O.g1_in_subgroup))
        while True:
            x = self._rand_x(rng)
            y = sqrt(self._rhs(x))
            if y is not None and on((x, y)) and not sub((x, y)):    # the oracle confirms [r]P != O
                return (x, y)

    def host(self, b: bytes):
        """tpst_de_g1 / tpst_de_g2 on one point -> its limbs, or None if rejected"""
        if b not in self._host:
            out = np.zeros(self.words, dtype=np.uint64)
            rc = self.de_one(b, out.ctypes.data_as(C.POINTER(C.c_uint64)))
            assert rc in (0, E_ARG)
            self._host[b] = out if rc == 0 else None
        return self._host[b]

    def batch(self, ctx, items):
        """the device reader on a list of encodings -> (rc, first_bad, limbs)"""
        n = len(items)
        out = np.full((n, self.words), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        bad = C.c_size_t(n + 7)
        rc = self.de_batch(ctx.h, b"".join(items), n, out.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(bad))
        return rc, bad.value, out

    def expect(self, ctx, items):
        """the batch result must be what the per-point reader gives on every element"""
        host = [self.host(b) for b in items]
        rejected = [i for i, h in enumerate(host) if h is None]
        rc, bad, out = self.batch(ctx, items)
        if rejected:
            assert (rc, bad) == (E_ARG, rejected[0]), (rc, bad, rejected)
        else:
            assert rc == 0 and bad == len(items)
            assert np.array_equal(out, np.stack(host))

    def fill(self, n):
        return [self.valid[i % len(self.valid)] for i in range(n)]


_GROUPS = {}


def _group(g2):
    if g2 not in _GROUPS:
        _GROUPS[g2] = Group(g2)
    return _GROUPS[g2]


CASES = [(False, n) for n in G1_SIZES] + [(True, n) for n in G2_SIZES]
IDS = ["%s-%d" % ("g2" if g else "g1", n) for g, n in CASES]


@pytest.mark.parametrize("g2,n", CASES, ids=IDS)
def test_valid_batch_equals_per_point_reader(ctx, g2, n):
    g = _group(g2)
    items = g.fill(n)
    assert all(g.host(b) is not None for b in items)
    g.expect(ctx, items)
    # the points themselves, not only the host's word for them
    rc, _bad, out = g.batch(ctx, items[:min(n, len(g.points))])
    assert rc == 0 and np.array_equal(out, g.arr(g.points[:len(out)]))


@pytest.mark.parametrize("g2,n", CASES, ids=IDS)
def test_first_bad_is_the_lowest_rejected_index(ctx, g2, n):
    g = _group(g2)
    names = sorted(g.bad)
    places = [(0,), (n - 1,)] + ([(n // 3, n - 1), (1, n // 2)] if n > 2 else [])
    for k, where in enumerate(places):
        items = g.fill(n)
        for j, i in enumerate(where):
            items[i] = g.bad[names[(k + j) % len(names)]]
        assert g.host(items[where[0]]) is None
        g.expect(ctx, items)
        assert g.batch(ctx, items)[1] == min(where)


@pytest.mark.parametrize("g2,n", CASES, ids=IDS)
def test_mixed_batch_every_class(ctx, g2, n):
    """every class somewhere in one batch (as many as fit), the accepted corner first"""
    g = _group(g2)
    items = g.fill(n)
    rng = random.Random(n)
    classes = [g.flagged_inf] + [g.bad[k] for k in sorted(g.bad)]
    slots = sorted(rng.sample(range(n), min(n, len(classes))))
    for i, b in zip(slots, classes):
        items[i] = b
    g.expect(ctx, items)


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
def test_every_class_alone(ctx, g2):
    """n = 1: the verdict of every class is the per-point reader's, and the classes are what their names say"""
    g = _group(g2)
    for name, b in sorted(g.bad.items()):
        assert g.host(b) is None, name
        assert g.batch(ctx, [b])[:2] == (E_ARG, 0), name
    # the infinity flag over x != 0: the host reads it as infinity, so does the device
    assert g.host(g.flagged_inf) is not None and not g.host(g.flagged_inf).any()
    rc, bad, out = g.batch(ctx, [g.flagged_inf])
    assert (rc, bad) == (0, 1) and not out.any()
    for b in g.valid:
        g.expect(ctx, [b])


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
def test_empty_batch_and_arguments(ctx, g2):
    g = _group(g2)
    bad = C.c_size_t(99)
    assert g.de_batch(ctx.h, None, 0, None, C.byref(bad)) == 0
    assert g.check_batch(ctx.h, None, 0, None) == 0
    assert g.de_batch(ctx.h, None, 1, None, None) == E_ARG
    out = np.zeros((1, g.words), dtype=np.uint64)
    assert g.de_batch(ctx.h, g.valid[0], 1, out.ctypes.data_as(C.POINTER(C.c_uint64)), None) == 0  # first_bad may be NULL
    assert np.array_equal(out[0], g.host(g.valid[0]))


@pytest.mark.parametrize("g2,n", CASES, ids=IDS)
def test_check_kernel_equals_host_check(ctx, g2, n):
    """canonical affine input: a valid point, one bit of y flipped, x and y swapped, a coordinate
    equal to p, all-zero, the point outside the subgroup -- alone and placed in a batch"""
    g = _group(g2)
    w, h = g.words, g.words // 2
    good = g.arr(g.points)
    p_limbs = np.array([(P >> (64 * k)) & (2 ** 64 - 1) for k in range(6)], dtype=np.uint64)
    flipped, swapped, coord_p = good[0].copy(), good[1].copy(), good[2].copy()
    flipped[h] ^= np.uint64(1)
    swapped[:h], swapped[h:] = good[1][h:], good[1][:h]
    coord_p[w - 6:] = p_limbs
    cases = {"valid": good[3], "y bit": flipped, "swapped": swapped, "coordinate p": coord_p,
             "zero": np.zeros(w, dtype=np.uint64), "off subgroup": g.arr([g.off_subgroup])[0]}
    verdict = {}
    for name, pt in cases.items():
        pt = np.ascontiguousarray(pt)
        verdict[name] = g.check_one(pt.ctypes.data_as(C.POINTER(C.c_uint64)))
        assert verdict[name] in (0, E_VERIFY)
    assert [k for k, v in verdict.items() if v == 0] == ["valid", "zero"]
    names = sorted(cases)
    rng = random.Random(1000 + n)
    for trial in range(3):
        batch = np.stack([good[i % len(good)] for i in range(n)])
        want = n
        for i in sorted(rng.sample(range(n), min(n, 1 + trial))):
            name = names[(i + trial) % len(names)]
            batch[i] = cases[name]
            if verdict[name] != 0:
                want = min(want, i)
        bad = C.c_size_t(n + 7)
        rc = g.check_batch(ctx.h, batch.ctypes.data_as(C.POINTER(C.c_uint64)), n, C.byref(bad))
        assert (rc, bad.value) == ((0, n) if want == n else (E_VERIFY, want)), (trial, rc, bad.value, want)
    if n == 1:
        for name, pt in cases.items():
            pt = np.ascontiguousarray(pt).reshape(1, w)
            bad = C.c_size_t(9)
            rc = g.check_batch(ctx.h, pt.ctypes.data_as(C.POINTER(C.c_uint64)), 1, C.byref(bad))
            assert rc == verdict[name] and bad.value == (1 if rc == 0 else 0), name


def test_python_wrappers(ctx):
    from testudo_amd import serialize as ser
    g = _group(False)
    out = ser.de_g1_batch(ctx, b"".join(g.valid))
    assert np.array_equal(out, np.stack([g.host(b) for b in g.valid]))
    with pytest.raises(ser.SerializationError, match="index 2"):
        ser.de_g1_batch(ctx, b"".join(g.valid[:2] + [g.bad["non-residue"]] + g.valid[:1]))
    assert ser.check_g1_batch(ctx, out) is None
    pts = out.copy()
    pts[3, 6] ^= np.uint64(1)
    assert ser.check_g1_batch(ctx, pts) == 3
    g2 = _group(True)
    out2 = ser.de_g2_batch(ctx, b"".join(g2.valid[:3]))
    assert ser.check_g2_batch(ctx, out2) is None
    with pytest.raises(ser.SerializationError):
        ser.de_g2_batch(ctx, g2.bad["off subgroup"])
