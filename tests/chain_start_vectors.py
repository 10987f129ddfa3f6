"""Operands of the chain-start mixed add (curve.h add_affine_unit: p is
infinity or has ZZ = ZZZ = 1), shared by tests/test_add_affine_unit.py (host)
and tests/test_selftest_unit.py (device).  They are arith_vectors.py's curve
pairs with every finite p brought to ZZ = ZZZ = 1: p infinity (plain and with
junk in X, Y), q infinity, both, p = q (doubling), p = -q (same x, other y:
the result is infinity), same y with another x, the points with a coordinate
0, 1 or p - 1 ((p - 1, 0), (0, 1), (0, p - 1); x = 1 and y = p - 1 with x != 0
are not on y^2 = x^3 + 1) against each other and against random points, and
500 random pairs per group."""
import subprocess

import numpy as np

import arith_vectors as V
from testudo_amd import engine as E


class UnitSet:
    def __init__(self, grp):
        cs = V.curve_set(grp)
        G, F = cs.G, cs.G.F
        self.cs, self.G = cs, G
        self.p = [cs.p[i] if pa is None else (pa[0], pa[1], F.one, F.one) for i, pa in enumerate(cs.pa)]
        self.q = cs.q_aff
        for (X, Y, ZZ, ZZZ), pa in zip(self.p, cs.pa):
            assert (ZZ, ZZZ) == ((F.zero, F.zero) if pa is None else (F.one, F.one))
        for tag in ("p inf", "q inf", "both inf", "p == q", "p == -q", "same y, other x", "random"):
            assert tag in cs.tags
        if grp == "g1":
            for tag in ("order 2 doubled", "x = 0 doubled", "x = 0 cancels", "q y = 0", "p y = 0", "q x = 0", "p x = 0"):
                assert tag in cs.tags

    def operands(self, mont):
        G = self.G
        conv = lambda c: mont(c) if G.cw == 12 else (mont(c[0]), mont(c[1]))
        enc = lambda rows: V.words([sum(G.flat(conv(c)) << (32 * G.cw * j) for j, c in enumerate(r)) for r in rows],
                                   4 * G.cw)
        return enc(self.p), enc(self.q)

    def check(self, out, unmont, what):
        """XYZZ words against the affine sums p + q from Python integers"""
        self.cs.check("add_affine", out, unmont, what)


_SETS = {}


def unit_set(grp):
    if grp not in _SETS:
        _SETS[grp] = UnitSet(grp)
    return _SETS[grp]


def form_operands(form):
    """(UnitSet, p words, q words, unmont) of a lane form of csrc/selftest_ops.h"""
    grp, (mont, unmont) = V.CURVE_FORMS[form]
    us = unit_set(grp)
    p, q = us.operands(mont)
    return us, p, q, unmont


def build_host_dispatch(out):
    """tests/cpp/test_selftest_ops.cpp: the host run of csrc/selftest_ops.h"""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(root, "testudo_amd", "csrc"),
                    os.path.join(root, "tests", "cpp", "test_selftest_ops.cpp"), "-o", out], check=True)
    return out


def host_curve(exe, op, p, q):
    import struct
    inp = struct.pack("<iii", 1, op, len(p)) + p.tobytes() + q.tobytes()
    r = subprocess.run([exe], input=inp, capture_output=True, check=True)
    return np.frombuffer(r.stdout, dtype=np.uint32).reshape(p.shape)


def unit_op(form):
    return E.selftest_curve_unit_op(form)
