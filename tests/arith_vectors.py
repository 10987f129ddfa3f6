"""Operands and expected values of the arithmetic self-tests, shared by the
host run of csrc/selftest_ops.h (test_selftest_ops.py) and the device run
(test_device_arith.py).  Everything is Python integers: the Montgomery
products are restated as a b R^-1 mod p, the curve operations go through
oracle/py/bls377.py's affine formulas.

Constructed classes carry their defining property as an assertion made here,
from integers alone: e.g. a pair built so that the Montgomery reduction word
m_k of its product is zero is checked by computing m = -a b p^-1 mod 2^(wN)
and asserting that limb k of m is 0.  COUNTS records how many operands each
class produced.
"""
import functools
import random

import numpy as np

import bls377 as O
from testudo_amd import engine as E

P = O.P
R_SCALAR = O.R
COUNTS = {}


class Fld:
    """a Montgomery field as the kernels lay it out: N limbs of w bits, R = 2^(w N)"""

    def __init__(self, name, p, w, n):
        self.name, self.p, self.w, self.n = name, p, w, n
        self.bits = w * n
        self.R = 1 << self.bits
        self.Ri = pow(self.R, -1, p)
        self.pinv = pow(p, -1, self.R)

    def limbs(self, v):
        return [(v >> (self.w * i)) & ((1 << self.w) - 1) for i in range(self.n)]

    def m_of(self, t):
        """the reduction words of Montgomery-reducing t: t + m p = 0 mod R"""
        return self.limbs((-t * self.pinv) % self.R)

    def redc(self, t):
        return t * self.Ri % self.p


FQ = Fld("fq", P, 32, 12)
FR = Fld("fr", R_SCALAR, 32, 8)
F29 = Fld("fq29", P, 29, 13)
R384 = 1 << 384
R384I = pow(R384, -1, P)


def _count(key, n):
    COUNTS[key] = COUNTS.get(key, 0) + n


def words(vals, nwords):
    """ints -> (len, nwords) u32 little-endian"""
    buf = b"".join(int(v).to_bytes(4 * nwords, "little") for v in vals)
    return np.frombuffer(buf, dtype=np.uint32).reshape(len(vals), nwords).copy()


def ints(arr, nwords):
    """(n, k * nwords) u32 -> n lists of k ints"""
    arr = np.ascontiguousarray(arr, dtype=np.uint32)
    n, tot = arr.shape
    raw = arr.tobytes()
    k = tot // nwords
    step = 4 * nwords
    return [[int.from_bytes(raw[(i * k + j) * step:(i * k + j + 1) * step], "little") for j in range(k)]
            for i in range(n)]


# ------------------------------------------------------ constructed pairs --
def _m_cleared(F, rng, cols, low=None):
    m = rng.randrange(F.R)
    for k in cols:
        m &= ~(((1 << F.w) - 1) << (F.w * k))
    if low is not None:  # force the low 3 bits
        m = (m & ~7) | low
    return m


def mul_mk0(F, rng, cols, per=2):
    """(a, b) with reduction word m_k == 0 for k in cols in a b"""
    out = []
    tries = 0
    while len(out) < per:
        a = rng.randrange(1, F.p) | 1
        ai = pow(a, -1, F.R)
        for _ in range(400):
            tries += 1
            m = _m_cleared(F, rng, cols)
            b = (-m * F.p * ai) % F.R
            if b < F.p:
                mm = F.m_of(a * b)
                assert all(mm[k] == 0 for k in cols), (F.name, cols)
                out.append((a, b))
                break
    _count("%s.mul.m_k=0 cols=%s" % (F.name, list(cols)), len(out))
    COUNTS["%s.mul.tries" % F.name] = COUNTS.get("%s.mul.tries" % F.name, 0) + tries
    return out


def _sqrt_2adic(s, bits):
    """x with x^2 = s mod 2^bits for s = 1 mod 8 (Hensel, one bit per step)"""
    assert s % 8 == 1
    x = 1
    for k in range(3, bits):
        if (x * x - s) >> k & 1:
            x += 1 << (k - 1)
    assert (x * x - s) % (1 << bits) == 0
    return x


def sqr_mk0(F, rng, k, per=1):
    """a with reduction word m_k == 0 in a^2, k >= 1 (p = 1 mod 8: m = 7 mod 8 makes -m p a 2-adic square)"""
    assert k >= 1 and F.p % 8 == 1
    out = []
    tries = 0
    while len(out) < per:
        tries += 1
        m = _m_cleared(F, rng, [k], low=7)
        s = (-m * F.p) % F.R
        x = _sqrt_2adic(s, F.bits)
        half = F.R >> 1
        for a in (x, F.R - x, (x + half) % F.R, (F.R - x + half) % F.R):
            if a < F.p and len(out) < per:
                assert F.m_of(a * a)[k] == 0, (F.name, k)
                out.append(a)
    _count("%s.sqr.m_k=0 col=%d" % (F.name, k), len(out))
    COUNTS["%s.sqr.tries" % F.name] = COUNTS.get("%s.sqr.tries" % F.name, 0) + tries
    return out


def sqr_m0(F, rng):
    """a with a_0^2 = 0 mod 2^w: m_0 == 0"""
    lows = (0, 1 << 16, 1 << 31) if F.w == 32 else (0, 1 << 15)
    out = []
    for lo in lows:
        a = (rng.randrange(F.p >> F.w) << F.w) | lo
        assert a < F.p and F.m_of(a * a)[0] == 0
        out.append(a)
    _count("%s.sqr.m_0=0" % F.name, len(out))
    return out


def solve_mk0(F, rng, cols, fixed, mult, name, per=2):
    """x < p with m_k == 0 (k in cols) in x * mult + fixed, for an odd mult"""
    assert mult & 1
    mi = pow(mult, -1, F.R)
    out = []
    for _ in range(20000):
        m = _m_cleared(F, rng, cols)
        x = ((-m * F.p - fixed) * mi) % F.R
        if x < F.p:
            mm = F.m_of(x * mult + fixed)
            assert all(mm[k] == 0 for k in cols)
            out.append(x)
            if len(out) == per:
                break
    assert len(out) == per, name
    _count("%s.%s.m_k=0 cols=%s" % (F.name, name, list(cols)), len(out))
    return out


def edges(F):
    p, w = F.p, F.w
    top = p.bit_length() - 1
    e = [0, 1, 2, F.R % p, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, (1 << top) - 1, (1 << top), p - (F.R % p)]
    for i in range(F.n + 1):
        for v in ((1 << (w * i)), (1 << (w * i)) - 1, ((1 << (w * i)) - 1) ^ 1):
            if 0 <= v < p:
                e.append(v)
    seen, out = set(), []
    for v in e:
        if v not in seen:
            seen.add(v)
            out.append(v)
    assert all(0 <= v < p for v in out)
    return out


def mk0_columns(F):
    return [[k] for k in range(F.n)] + [[1, F.n - 2], [0, F.n - 1]]


# ------------------------------------------------------------ field cases --
class FieldCase:
    """one device call: op, operands and expected result as u32 word arrays"""

    def __init__(self, name, a, b, exp, wi, wo):
        self.name = name
        self.op = E.SELFTEST_FIELD[name]
        self.a, self.b, self.exp = words(a, wi), words(b, wi), words(exp, wo)
        assert E.selftest_field_words(self.op) == (wi, wo)
        self.inputs = list(zip(a, b))


def _fp_cases(F, seed):
    """Fq / Fr lane ops of field.h"""
    rng = random.Random(seed)
    p = F.p
    ed = edges(F)
    rnd = [(rng.randrange(p), rng.randrange(p)) for _ in range(2000)]
    cross = [(a, b) for a in ed for b in ed]
    mulp = list(cross)
    for cols in mk0_columns(F):
        mulp += mul_mk0(F, rng, cols)
    sq = list(ed) + sqr_m0(F, rng)
    for k in range(1, F.n):
        sq += sqr_mk0(F, rng, k)
    addp, subp = list(cross), list(cross)
    for _ in range(40):
        a = rng.randrange(2, p - 1)
        addp += [(a, p - a), (a, p - a + 1), (a, p - a - 1)]
        subp += [(a, a), (a, a + 1), (a, a - 1), (a - 1, a)]
    _count("%s.add a+b in {p-1,p,p+1}" % F.name, 120)
    _count("%s.sub a-b in {-1,0,1}" % F.name, 160)
    for a, b in addp[-120:]:
        assert a + b in (p - 1, p, p + 1)
    for a, b in subp[-160:]:
        assert a - b in (-1, 0, 1)
    mulp += rnd
    sqp = [(a, a) for a in sq] + rnd
    addp += rnd
    subp += rnd
    un = [(a, a) for a in ed] + rnd
    n32 = F.n
    mk = lambda nm, prs, f: FieldCase("%s.%s" % (F.name, nm), [a for a, _ in prs], [b for _, b in prs],
                                      [f(a, b) for a, b in prs], n32, n32)
    return [
        mk("mul", mulp, lambda a, b: F.redc(a * b)),
        mk("sqr", sqp, lambda a, b: F.redc(a * a)),
        mk("add", addp, lambda a, b: (a + b) % p),
        mk("sub", subp, lambda a, b: (a - b) % p),
        mk("neg", un, lambda a, b: (-a) % p),
        mk("to_mont", un, lambda a, b: a * F.R % p),
        mk("from_mont", un, lambda a, b: F.redc(a)),
    ]


def _f29_cases(seed):
    """field29.h: operands are the radix-2^29 values themselves, packed (pack377)"""
    F = F29
    rng = random.Random(seed)
    p = P
    ed = edges(F)
    rnd = [(rng.randrange(p), rng.randrange(p)) for _ in range(2000)]
    cross = [(a, b) for a in ed for b in ed]
    mulp = list(cross)
    for cols in mk0_columns(F):
        mulp += mul_mk0(F, rng, cols)
    sq = list(ed) + sqr_m0(F, rng)
    for k in range(1, F.n):
        sq += sqr_mk0(F, rng, k)
    # mul_sum(a, b, a, a) = a b + a^2: solve b;  mul_sub(a, b, b, b) = a b + b (p - b): solve a
    msum, msub = list(cross), list(cross)
    for cols in mk0_columns(F):
        a = rng.randrange(1, p) | 1
        msum += [(a, b) for b in solve_mk0(F, rng, cols, a * a, a, "mul_sum")]
        b = rng.randrange(1, p) | 1
        msub += [(a2, b) for a2 in solve_mk0(F, rng, cols, b * (p - b), b, "mul_sub")]
    msum.append((p - 1, p - 1))
    msub.append((p - 1, 0))
    # four-operand forms: (a, c) and (b, d)
    sum4, sub4 = [], []
    for cols in mk0_columns(F):
        a, c, d = rng.randrange(1, p) | 1, rng.randrange(p), rng.randrange(p)
        sum4 += [(a, b, c, d) for b in solve_mk0(F, rng, cols, c * d, a, "mul_sum4")]
        sub4 += [(a, b, c, d) for b in solve_mk0(F, rng, cols, c * (p - d), a, "mul_sub4")]
        sub4 += [(a, b, c, 0) for b in solve_mk0(F, rng, cols, c * p, a, "mul_sub4 d=0")]  # p_minus(0) = p
    sum4 += [(p - 1, p - 1, p - 1, p - 1), (0, 0, 0, 0), (p - 1, p - 1, 0, 0)]
    sub4 += [(p - 1, p - 1, p - 1, 0), (p - 1, p - 1, p - 1, p - 1), (p - 1, p - 1, p - 1, 1), (0, 0, p - 1, p - 1),
             (1, 1, p - 1, 0)]
    _count("fq29.mul_sum/mul_sub bound cases", 3 + 5 + 2)
    for _ in range(2000):
        q4 = tuple(rng.randrange(p) for _ in range(4))
        sum4.append(q4)
        sub4.append(q4)
    addp, subp = list(cross), list(cross)
    for _ in range(40):
        a = rng.randrange(2, p - 1)
        addp += [(a, p - a), (a, p - a + 1), (a, p - a - 1)]
        subp += [(a, a), (a, a + 1), (a, a - 1), (a - 1, a)]
    for a, b in addp[-120:]:
        assert a + b in (p - 1, p, p + 1)
    for a, b in subp[-160:]:
        assert a - b in (-1, 0, 1)
    _count("fq29.add a+b in {p-1,p,p+1}", 120)
    _count("fq29.sub a-b in {-1,0,1}", 160)
    # to_std: W = 128 Y within 128 of a multiple of p (the q - 1 arm of the quotient estimate)
    ts = [0, p - 1]
    for q in range(1, 128):
        y = -(-q * p // 128)
        for v in (y, y - 1):
            assert 0 <= v < p and min(128 * v % p, p - 128 * v % p) <= 128
            ts.append(v)
    _count("fq29.to_std 128 Y within 128 of q p", len(ts) - 2)
    ts += list(ed) + [a for a, _ in rnd]
    # from_std: field.h words in; low 7 bits 0 (k = 0) and 0x7f; wide operands below 64 p
    fs = []
    for _ in range(100):
        v = rng.randrange(p >> 7) << 7
        fs += [v, v | 0x7F]
    for v in fs:
        assert v < p and v & 0x7F in (0, 0x7F)
    _count("fq29.from_std low bits 0 / 0x7f", len(fs))
    wide = []
    for wx in (1, 2, 4, 8, 16, 32, 64):
        wide += [wx * p - 1, wx * p - 128, wx * p - 127] + [rng.randrange(wx * p) for _ in range(100)]
    assert all(0 <= v < 64 * p for v in wide)
    _count("fq29.from_std wide operands < 64 p", len(wide))
    fs += wide + list(ed) + [a for a, _ in rnd]

    Ri = F.Ri
    mk = lambda nm, prs, f: FieldCase("fq29." + nm, [a for a, _ in prs], [b for _, b in prs], [f(a, b) for a, b in prs],
                                      12, 12)
    un = lambda vals: [(a, a) for a in vals]
    mk4 = lambda nm, qs, f: FieldCase("fq29." + nm, [a | (c << 384) for a, b, c, d in qs],
                                      [b | (d << 384) for a, b, c, d in qs], [f(*q4) for q4 in qs], 24, 12)
    every = un(ed) + rnd
    return [
        mk("mul", mulp + rnd, lambda a, b: a * b * Ri % p),
        mk("sqr", un(sq) + rnd, lambda a, b: a * a * Ri % p),
        mk("mul_sum", msum + rnd, lambda a, b: (a * b + a * a) * Ri % p),
        mk("mul_sub", msub + rnd, lambda a, b: (a * b - b * b) * Ri % p),
        mk("add", addp + rnd, lambda a, b: (a + b) % p),
        mk("sub", subp + rnd, lambda a, b: (a - b) % p),
        mk("cneg", every, lambda a, b: (-a) % p),
        mk("p_minus", every, lambda a, b: p - a),
        mk("to_std", un(ts), lambda a, b: a * 128 % p),
        mk("to_std_mul", un(ts), lambda a, b: a * 128 % p),
        mk("from_std", un(fs), lambda a, b: (a + ((-a) % 128) * p) >> 7),
        mk("roundtrip", every + un([(1 << 377) - 1, 1 << 376]), lambda a, b: a),
        mk4("mul_sum4", sum4, lambda a, b, c, d: (a * b + c * d) * Ri % p),
        mk4("mul_sub4", sub4, lambda a, b, c, d: (a * b - c * d) * Ri % p),
    ]


def _fq2_cases(seed):
    rng = random.Random(seed)
    p = P
    comp = [0, 1, R384 % p, p - 1, (p - 1) // 2, (1 << 376) - 1]
    el = [(x, y) for x in comp for y in comp]
    prs = [(a, b) for a in el for b in el[::5]]
    prs += [((rng.randrange(p), rng.randrange(p)), (rng.randrange(p), rng.randrange(p))) for _ in range(2000)]
    red = lambda v: (v[0] * R384I % p, v[1] * R384I % p)
    enc = lambda v: v[0] | (v[1] << 384)
    A, B = [enc(a) for a, _ in prs], [enc(b) for _, b in prs]
    mulx = [enc(red(O.f2_mul(a, b))) for a, b in prs]
    sqrx = [enc(red(O.f2_mul(a, a))) for a, _ in prs]
    # pair flags: zero / equal in one coordinate only must not count
    x, y = rng.randrange(1, p), rng.randrange(1, p)
    fl = [((0, 0), (0, 0)), ((x, 0), (x, 0)), ((0, y), (0, y)), ((x, y), (x, y)), ((x, y), (x, 0)), ((x, y), (0, y)),
          ((x, y), (x, y ^ 1)), ((x, y), (x ^ 1, y)), ((0, 0), (x, y)), ((x, 0), (0, 0)), ((0, y), (0, 0)),
          ((x, y), (y, x)), ((1, 0), (0, 1))]
    fl = fl * 11 + prs[:200]  # more than one wave, flags differing between neighbouring pairs
    _count("fq2p.is_zero / eq one-coordinate cases", 13 * 11)
    FA, FB = [enc(a) for a, _ in fl], [enc(b) for _, b in fl]
    iz = [(1 | 1 << 32) if a == (0, 0) else 0 for a, _ in fl]
    eqx = [(1 | 1 << 32) if a == b else 0 for a, b in fl]
    assert sum(1 for v in iz if v) >= 11 and sum(1 for v in eqx if v) >= 44
    return [
        FieldCase("fq2.mul", A, B, mulx, 24, 24),
        FieldCase("fq2.sqr", A, B, sqrx, 24, 24),
        FieldCase("fq2p.mul", A, B, mulx, 24, 24),
        FieldCase("fq2p.is_zero", FA, FB, iz, 24, 2),
        FieldCase("fq2p.eq", FA, FB, eqx, 24, 2),
    ]


@functools.lru_cache(maxsize=None)
def field_cases():
    """{family: [FieldCase]}"""
    f2 = _fq2_cases(4)
    return {
        "fq": _fp_cases(FQ, 1),
        "fr": _fp_cases(FR, 2),
        "fq29": _f29_cases(3),
        "fq2": [c for c in f2 if c.name.startswith("fq2.")],
        "fq2p": [c for c in f2 if c.name.startswith("fq2p.")],
    }


# ------------------------------------------------------------ curve cases --
class Grp:
    def __init__(self, name, F, gen, cw):
        self.name, self.F, self.gen, self.cw = name, F, gen, cw  # cw: u32 words per coordinate

    def rand_el(self, rng):
        return rng.randrange(1, P) if self.cw == 12 else (rng.randrange(1, P), rng.randrange(P))

    def scale(self, pt, lam):
        """affine -> XYZZ (l^2 x, l^3 y, l^2, l^3); None -> (1, 1, 0, 0)"""
        F = self.F
        if pt is None:
            return (F.one, F.one, F.zero, F.zero)
        l2 = F.mul(lam, lam)
        l3 = F.mul(l2, lam)
        return (F.mul(l2, pt[0]), F.mul(l3, pt[1]), l2, l3)

    def smul(self, c, s):
        return c * s % P if self.cw == 12 else (c[0] * s % P, c[1] * s % P)

    def flat(self, c):
        return c if self.cw == 12 else c[0] | (c[1] << 384)

    def unflat(self, v):
        return v if self.cw == 12 else (v & ((1 << 384) - 1), v >> 384)


G1 = Grp("g1", O._FqOps, O.G1_GEN, 12)
G2 = Grp("g2", O._Fq2Ops, O.G2_GEN, 24)


def _beta():
    for g in range(2, 50):
        b = pow(g, (P - 1) // 3, P)
        if b != 1:
            assert b * b * b % P == 1
            return b
    raise AssertionError


class CurveSet:
    """operand pairs of one group, in plain (non-Montgomery) field values:
    mixed[i] = (p XYZZ, q affine-as-XYZZ), full[i] = (p XYZZ, q XYZZ), with the
    affine points pa[i], qa[i] (None: infinity) they represent"""

    def __init__(self, G, seed, nrand=500):
        rng = random.Random(seed)
        F = G.F
        mul = O.g1_mul if G is G1 else O.g2_mul
        add = lambda a, b: O._add_affine(F, a, b)
        q0, st = mul(G.gen, rng.randrange(1, R_SCALAR)), mul(G.gen, rng.randrange(1, R_SCALAR))
        pts = [q0]
        for _ in range(2 * nrand + 40):
            pts.append(add(pts[-1], st))
        assert all(O._on_curve(F, t) for t in pts[:5] + pts[-5:])
        it = iter(pts)
        beta = _beta()
        one = F.one
        inf_junk = (G.rand_el(rng), G.rand_el(rng), F.zero, F.zero)  # infinity is ZZ == 0 whatever X, Y hold
        cases = []  # (pa, lam, qa, mu, tag)

        def both(pa, qa, tag):
            for lam, mu in ((G.rand_el(rng), G.rand_el(rng)), (one, one), (G.rand_el(rng), one)):
                cases.append((pa, lam, qa, mu, tag))

        A, B = next(it), next(it)
        both(None, B, "p inf")
        both(A, None, "q inf")
        both(None, None, "both inf")
        both(A, A, "p == q")
        both(A, O._neg(F, A), "p == -q")
        Ab = (G.smul(A[0], beta), A[1])
        assert O._on_curve(F, Ab) and Ab[0] != A[0]
        both(A, Ab, "same y, other x")
        both(Ab, O._neg(F, A), "other x, negated y")
        if G is G1:
            t2, t3, t3n = (P - 1, 0), (0, 1), (0, P - 1)
            assert all(O._on_curve(F, t) for t in (t2, t3, t3n))
            for a, b, tag in ((t2, t2, "order 2 doubled"), (t3, t3, "x = 0 doubled"), (t3, t3n, "x = 0 cancels"),
                              (t3n, t3n, "x = 0 doubled"), (t2, t3, "low order"), (t3, t2, "low order"),
                              (A, t2, "q y = 0"), (t2, A, "p y = 0"), (A, t3, "q x = 0"), (t3, A, "p x = 0"),
                              (A, t3n, "q x = 0"), (t3n, B, "p x = 0"), (None, t3, "inf + x = 0"),
                              (t3n, None, "x = 0 + inf"), (None, t2, "inf + y = 0")):
                both(a, b, tag)
        self.n_edge = len(cases)
        for _ in range(nrand):
            cases.append((next(it), G.rand_el(rng), next(it), G.rand_el(rng), "random"))
        self.G = G
        self.pa = [c[0] for c in cases]
        self.qa = [c[2] for c in cases]
        self.tags = [c[4] for c in cases]
        self.p = [G.scale(pa, lam) for pa, lam, _, _, _ in cases]
        self.q_full = [G.scale(qa, mu) for _, _, qa, mu, _ in cases]
        self.q_aff = [(F.zero,) * 4 if qa is None else (qa[0], qa[1], one, one) for qa in self.qa]
        # every third infinity carries junk in X, Y
        k = 0
        for i, pa in enumerate(self.pa):
            if pa is None:
                k += 1
                if k % 3 == 0:
                    self.p[i] = inf_junk
        for i, qa in enumerate(self.qa):
            if qa is None and i % 2:
                self.q_full[i] = inf_junk
        # the properties the classes are named for, from integers alone
        for i, (pa, lam, qa, mu, tag) in enumerate(cases):
            X, Y, ZZ, ZZZ = self.p[i]
            if pa is None:
                assert ZZ == F.zero
            else:
                assert ZZ != F.zero and F.mul(pa[0], ZZ) == X and F.mul(pa[1], ZZZ) == Y
                assert F.mul(F.mul(ZZ, ZZ), ZZ) == F.mul(ZZZ, ZZZ)
            if tag == "p == q":
                assert pa == qa and ((ZZ != one) == (lam != one))
            if tag == "p == -q":
                assert pa[0] == qa[0] and pa[1] == F.neg(qa[1]) and pa[1] != qa[1]
            if tag == "same y, other x":
                assert pa[1] == qa[1] and pa[0] != qa[0]
        _count("%s curve edge pairs" % G.name, self.n_edge)
        _count("%s curve edge pairs with ZZ != 1" % G.name, sum(1 for c in cases[:self.n_edge] if c[1] != one))
        _count("%s curve random pairs" % G.name, nrand)
        neg = lambda t: O._neg(F, t)
        dbl = lambda t: add(t, t)
        self.expected = {
            "add_affine": [add(a, b) for a, b in zip(self.pa, self.qa)],
            "sub_affine": [add(a, neg(b)) for a, b in zip(self.pa, self.qa)],
            "dbl": [dbl(a) for a in self.pa],
            "dbl_affine": [dbl(b) for b in self.qa],
            "to_affine": list(self.pa),
        }
        self.expected["add"] = self.expected["add_affine"]
        if G is G1:
            i = self.tags.index("order 2 doubled")
            assert self.expected["dbl"][i] is None and self.expected["add"][i] is None
            i = self.tags.index("x = 0 doubled")
            assert self.expected["dbl"][i] == (0, P - 1)
        assert self.expected["add"][self.tags.index("p == -q")] is None
        assert self.expected["add"][self.tags.index("same y, other x")] is not None

    def operands(self, cop, mont):
        """(p words, q words) of an op; mont: plain value -> int as the form holds it"""
        G = self.G
        q = self.q_full if cop == "add" else self.q_aff
        conv = lambda c: mont(c) if G.cw == 12 else (mont(c[0]), mont(c[1]))
        enc = lambda rows: words([sum(G.flat(conv(c)) << (32 * G.cw * j) for j, c in enumerate(r)) for r in rows],
                                 4 * G.cw)
        return enc(self.p), enc(q)

    def check(self, cop, out, unmont, what):
        """device / host XYZZ words against the affine expectation"""
        G, F = self.G, self.G.F
        exp = self.expected[cop]
        rows = ints(out, G.cw)
        assert len(rows) == len(exp)
        conv = lambda v: unmont(v) if G.cw == 12 else (unmont(v & ((1 << 384) - 1)), unmont(v >> 384))
        for i, (r, e) in enumerate(zip(rows, exp)):
            X, Y, ZZ, ZZZ = (conv(v) for v in r)
            ctx = (what, cop, i, self.tags[i])
            if e is None:
                assert ZZ == F.zero, ctx
                continue
            assert ZZ != F.zero, ctx
            assert F.mul(F.mul(ZZ, ZZ), ZZ) == F.mul(ZZZ, ZZZ), ctx
            assert F.mul(e[0], ZZ) == X and F.mul(e[1], ZZZ) == Y, ctx
            if cop == "to_affine":
                assert (X, Y, ZZ, ZZZ) == (e[0], e[1], F.one, F.one), ctx


@functools.lru_cache(maxsize=None)
def curve_set(name):
    return CurveSet(G1, 11) if name == "g1" else CurveSet(G2, 12)


# form -> (group, value -> stored int, stored int -> value)
_M384 = (lambda v: v * R384 % P, lambda v: v * R384I % P)
_M377 = (lambda v: v * F29.R % P, lambda v: v * F29.Ri % P)
CURVE_FORMS = {
    "fq": ("g1", _M384), "fq29_acc": ("g1", _M384), "fq29_pk": ("g1", _M377), "fq2": ("g2", _M384),
    "coop_fq29_acc": ("g1", _M384), "coop_fq29_pk": ("g1", _M377), "coop_fq2_acc": ("g2", _M384),
    "fq2_acc": ("g2", _M384), "pair": ("g2", _M384),
}
CURVE_FORM_OPS = {
    "fq": ("add_affine", "add", "dbl", "dbl_affine", "sub_affine", "to_affine"),
    "pair": ("add_affine", "add", "dbl", "dbl_affine", "sub_affine"),
    "fq2_acc": ("add_affine", "add", "dbl", "dbl_affine", "sub_affine"),
}
for _f in ("coop_fq29_acc", "coop_fq29_pk", "coop_fq2_acc"):  # coop.h: add_affine_quad, add_quad, dbl_quad
    CURVE_FORM_OPS[_f] = ("add_affine", "add", "dbl")
for _f in ("fq29_acc", "fq29_pk", "fq2"):
    CURVE_FORM_OPS[_f] = CURVE_FORM_OPS["fq"]
LANE_FORMS = ("fq", "fq29_acc", "fq29_pk", "fq2")


def curve_op(form, cop):
    return E.SELFTEST_CURVE_FORMS[form] * 16 + E.SELFTEST_CURVE_OPS[cop]


# -------------------------------------------------------------- glv_split --
LAMBDA = O.X * O.X - 1


@functools.lru_cache(maxsize=None)
def glv_scalars():
    r = R_SCALAR
    assert (LAMBDA * LAMBDA + LAMBDA + 1) % r == 0 and LAMBDA.bit_length() == 127
    ks = [0, 1, r - 1]
    n0 = len(ks)
    for m in (1, 2, 1 << 63, (r - 1) // LAMBDA):
        for d in (-1, 0, 1):
            k = m * LAMBDA + d
            if 0 <= k < r:
                assert k % LAMBDA in (0, 1, LAMBDA - 1)
                ks.append(k)
    _count("glv scalars m lambda + {-1,0,1}", len(ks) - n0)
    rng = random.Random(77)
    ks += [rng.randrange(r) for _ in range(2000)]
    return ks
