"""Operands of the fixed-base table self-test (tpst_selftest_fbt, csrc/fbt.h)
and a pure-Python model of the table's digit recoding.

The model is written from the definition, not from the kernel: a scalar v is
read four bits at a time from the bottom; a nibble plus the incoming carry that
exceeds 8 becomes that value minus 16 and carries 1 into the next window.  The
plain table recodes k over 64 windows; the GLV table recodes k1 = k mod lambda
and k2 = k div lambda over 32 windows each (k = k1 + lambda k2, lambda = x^2 - 1,
r = lambda^2 + lambda + 1, so k < r gives k1 < lambda and k2 <= lambda + 1).

By that definition a digit lies in [-7, 8]: nibble + carry <= 16 maps 9..16 to
-7..0, so -8 never occurs (reachable_digits() proves it by exhaustion) and the
table's m = 8 entries are read through digit +8 only.

tests/test_fbt_vectors.py proves, from integers alone, the property each class
below is named after; tests/test_fbt_gpu.py runs them through the device.
"""
import functools

import numpy as np

import bls377 as O

R = O.R
LAMBDA = O.X * O.X - 1
FORMS = ("plain", "glv")
NW = {"plain": 64, "glv": 32}
DIGITS = tuple(range(1, 9)) + tuple(range(-7, 0))  # every nonzero digit the recoding can produce
LPQS = (1, 2, 4, 8)


# ------------------------------------------------------------- the model --
def recode(v, nw):
    """(digits, carry_in) of v over nw windows: digits[w] in [-7, 8], carry_in[w]
    the carry entering window w (carry_in[nw] = the carry out of the top)."""
    digits, carry_in, c = [], [0], 0
    for w in range(nw):
        d = ((v >> (4 * w)) & 15) + c
        c = 1 if d > 8 else 0
        digits.append(d - 16 if c else d)
        carry_in.append(c)
    assert v >> (4 * nw) == 0
    return digits, carry_in


def resum(digits):
    return sum(d << (4 * w) for w, d in enumerate(digits))


def halves(k, form):
    """the integers whose digits the table form looks up: (k,) or (k1, k2)"""
    assert 0 <= k < R
    return (k,) if form == "plain" else (k % LAMBDA, k // LAMBDA)


def half_bounds(form):
    """largest value of each half over all k < r"""
    return (R - 1,) if form == "plain" else (LAMBDA - 1, LAMBDA + 1)


def compose(form, half, v):
    """the scalar whose half `half` is v and whose other half is 0"""
    return v if form == "plain" or half == 0 else LAMBDA * v


def min_carry_source(w):
    """smallest integer below 16^w whose recoding carries into window w:
    0x88...89 (w nibbles); none for w = 0"""
    return int("8" * (w - 1) + "9", 16) if w else None


@functools.lru_cache(maxsize=None)
def reachable_digits(form, half):
    """{(w, d)}: the nonzero digits a value <= the half's bound can show at
    window w.  Digit d at w needs nibble x and carry c with x + c = d or d + 16;
    the smallest value doing so is x 16^w (+ min_carry_source(w) when c = 1),
    every other nibble zero, so (w, d) is reachable iff that value is within
    the bound."""
    bound = half_bounds(form)[half]
    out = {}
    for w in range(NW[form]):
        for x in range(16):
            for c in (0, 1):
                if c and not w:
                    continue
                t = x + c
                d = t - 16 if t > 8 else t
                v = (x << (4 * w)) + (min_carry_source(w) if c else 0)
                if d and v <= bound and ((w, d) not in out or v < out[(w, d)]):
                    out[(w, d)] = v
    return out


def clear_top(v, bound):
    """v with its top nonzero nibbles cleared until it is <= bound (the nibble
    pattern below survives, unlike v mod bound)"""
    while v > bound:
        v &= (1 << (4 * ((v.bit_length() - 1) // 4))) - 1
    return v


# ---------------------------------------------------------- scalar classes --
EDGE = {
    "0": 0, "1": 1, "2": 2, "r-1": R - 1, "r-2": R - 2,
    "lambda-1": LAMBDA - 1, "lambda": LAMBDA, "lambda+1": LAMBDA + 1,
    "k2max": LAMBDA * (LAMBDA + 1),               # k1 = 0, k2 = lambda + 1: the largest k2 (this is r - 1)
    "halves_max": LAMBDA * LAMBDA + LAMBDA - 1,   # k1 = lambda - 1, k2 = lambda
}
PATTERNS = {"8": "8" * 64, "9": "9" * 64, "F": "F" * 64, "7..78": "7" * 63 + "8", "8..89": "8" * 63 + "9"}


@functools.lru_cache(maxsize=None)
def pattern_scalars(form):
    """{name: k}: every nibble of k (plain) or of k1 / k2 / both (glv) follows
    the pattern, up to the cleared top nibbles"""
    out = {}
    for name, hexs in PATTERNS.items():
        if form == "plain":
            out[name] = clear_top(int(hexs, 16), R - 1)
        else:
            v = int(hexs[-32:], 16)
            k1, k2 = clear_top(v, LAMBDA - 1), clear_top(v, LAMBDA)
            out[name + ".k1"] = k1
            out[name + ".k2"] = LAMBDA * k2
            out[name + ".k1k2"] = k1 + LAMBDA * k2
    return out


@functools.lru_cache(maxsize=None)
def carry_into(form):
    """{(half, b): k}: the recoding of that half carries into window b and into
    no other window (nibble 9 at b - 1: digit -7 there, digit 1 at b).  Every
    window b >= 1 is the start of a chunk (b = 8 ch), of a sub-chunk (b = 8 ch +
    sub lpq) or both: boundaries(b) names them."""
    out = {}
    for half, bound in enumerate(half_bounds(form)):
        for b in range(1, NW[form]):
            v = 9 << (4 * (b - 1))
            assert v <= bound
            out[(half, b)] = compose(form, half, v)
    return out


def boundaries(form, half, b):
    """the (chunk, lpq, sub) starts that window b of a half is, chunk counted over
    the 8 chunks of 8 windows that fbt_msm splits a scalar's 64 lookups into
    (glv: chunks 0-3 are k1's windows, 4-7 k2's)"""
    ch = b // 8 + (4 * half if form == "glv" else 0)
    return [(ch, lpq, (b % 8) // lpq) for lpq in LPQS if (b % 8) % lpq == 0]


@functools.lru_cache(maxsize=None)
def single_digit(form):
    """{(half, w, d): k} for d in (1, 8): that half's only nonzero digit is d at
    window w (8 is the largest digit: nibble 8, no carry), wherever the half's
    bound admits it"""
    out = {}
    for half, bound in enumerate(half_bounds(form)):
        for w in range(NW[form]):
            for d in (1, 8):
                if d << (4 * w) <= bound:
                    out[(half, w, d)] = compose(form, half, d << (4 * w))
    return out


@functools.lru_cache(maxsize=None)
def coverage(form):
    """scalars whose digits take every reachable nonzero value in every window
    of every half: the nibble-d scalars (digit d everywhere), nibble 16 - d on
    alternate windows (digit -d there, +1 after it), then one smallest scalar
    for each reachable (window, digit) the packed ones miss near the top"""
    nw = NW[form]
    packed = [int("%x" % d * nw, 16) for d in range(1, 9)]
    for d in range(1, 8):
        for par in (0, 1):
            packed.append(sum((16 - d) << (4 * w) for w in range(par, nw - 1, 2)))
    ks = []
    for v in packed:
        if form == "plain":
            ks.append(clear_top(v, R - 1))
        else:
            ks.append(clear_top(v, LAMBDA - 1) + LAMBDA * clear_top(v, LAMBDA))
    have = covered(form, ks)
    for half in range(len(half_bounds(form))):
        for (w, d), v in sorted(reachable_digits(form, half).items()):
            if (half, w, d) not in have:
                ks.append(compose(form, half, v))
    return ks


def covered(form, ks):
    """{(half, w, d)}: the nonzero digits the scalars show"""
    out = set()
    for k in ks:
        for half, v in enumerate(halves(k, form)):
            out.update((half, w, d) for w, d in enumerate(recode(v, NW[form])[0]) if d)
    return out


@functools.lru_cache(maxsize=None)
def scalar_list(form):
    """every constructed scalar of a table form, without repeats, as integers"""
    ks = list(EDGE.values()) + list(pattern_scalars(form).values()) + list(carry_into(form).values())
    ks += list(single_digit(form).values()) + coverage(form)
    return list(dict.fromkeys(ks))


def fr_words(ks):
    """canonical Fr rows (n, 4) u64"""
    return np.array([[(k >> (64 * i)) & (2**64 - 1) for i in range(4)] for k in ks], dtype=np.uint64).reshape(-1, 4)


# -------------------------------------------------------------- groups ------
def members_strided(g, members, L, D):
    """base indices of group g, from the definition in csrc/fbt.h"""
    return [(m // D) * L + g * D + m % D for m in range(members)]


def members_seg(seg, g):
    return [int(seg[g]) + m for m in range(int(seg[g + 1]) - int(seg[g]))]


def small_quad_shape(members):
    """(lpq, units) of the one-launch kernel for a member count: the smallest
    power of two lookups per quad at which members * 8 * (8 / lpq) units fit the
    64 quads of a block"""
    assert 1 <= members <= 8
    lpq = 1
    while members * 8 * (8 // lpq) > 64:
        lpq *= 2
    return lpq, members * 8 * (8 // lpq)


def tree_levels(members, Q=64):
    """segment lengths through fbt_msm's two-launch path: len = 8 * members
    partial sums per group, each launch reducing to ceil(len / per) with per = Q
    when len <= Q and 4 Q otherwise"""
    n, out = 8 * members, [8 * members]
    while n > 1:
        per = Q if n <= Q else 4 * Q
        n = (n + per - 1) // per
        out.append(n)
    return out


# ---------------------------------------------------------------- bases ----
BASE_KINDS = ("distinct", "equal", "cancel", "inf", "allinf")


def negate(points, g2):
    """-P of canonical affine rows (infinity stays infinity)"""
    w = 12 if g2 else 6  # words of x; y follows with as many (G2: c0, c1)
    out = points.copy()
    for row in out:
        if row.any():
            for j in range(w, 2 * w, 6):
                v = (O.P - sum(int(x) << (64 * i) for i, x in enumerate(row[j:j + 6]))) % O.P
                row[j:j + 6] = [(v >> (64 * i)) & (2**64 - 1) for i in range(6)]
    return out


def base_set(pool, kind, n, g2):
    """n bases of a kind from a pool of distinct points b_i G (canonical rows)"""
    assert len(pool) >= n
    b = pool[:n].copy()
    if kind == "equal":
        b[:] = pool[3]
    elif kind == "cancel":
        b[0::2] = pool[5]
        b[1::2] = negate(pool[5:6], g2)[0]
    elif kind == "inf":
        b[0] = 0
        b[n // 2] = 0
        b[n - 1] = 0
    elif kind == "allinf":
        b[:] = 0
    else:
        assert kind == "distinct"
    return b
