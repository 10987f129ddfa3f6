"""tests/fbt_vectors.py proved from integers alone: the recoding model resums
to the scalar, and every constructed scalar has the property its class is
named after (digit 8 without a carry, a carry into exactly one chunk or
sub-chunk start, one nonzero digit, the coverage of every reachable digit in
every window).  The GPU test (test_fbt_gpu.py) then has the device code as its
only unknown."""
import random

import numpy as np
import pytest

import bls377 as O
import fbt_vectors as V


def _streams(k, form):
    return [V.recode(v, V.NW[form]) for v in V.halves(k, form)]


def test_constants():
    assert V.R == V.LAMBDA * V.LAMBDA + V.LAMBDA + 1 and V.LAMBDA.bit_length() == 127 and V.R.bit_length() == 253
    assert V.halves(V.R - 1, "glv") == (0, V.LAMBDA + 1)
    assert V.half_bounds("glv") == (V.LAMBDA - 1, V.LAMBDA + 1)
    # the split is k1 = k mod lambda, k2 = k div lambda and phi acts as lambda
    rng = random.Random(5)
    for k in [rng.randrange(V.R) for _ in range(200)] + list(V.EDGE.values()):
        k1, k2 = V.halves(k, "glv")
        assert k1 + V.LAMBDA * k2 == k and 0 <= k1 < V.LAMBDA and 0 <= k2 <= V.LAMBDA + 1


@pytest.mark.parametrize("form", V.FORMS)
def test_recoding_resums_and_stays_in_range(form):
    rng = random.Random(6)
    ks = V.scalar_list(form) + [rng.randrange(V.R) for _ in range(500)]
    for k in ks:
        for (digits, carry_in), v in zip(_streams(k, form), V.halves(k, form)):
            assert V.resum(digits) == v, hex(k)
            assert carry_in[0] == 0 and carry_in[-1] == 0, hex(k)  # nothing is carried out of the top window
            assert all(-7 <= d <= 8 for d in digits), hex(k)
            for w, d in enumerate(digits):  # the definition, window by window
                t = ((v >> (4 * w)) & 15) + carry_in[w]
                assert (d, carry_in[w + 1]) == ((t - 16, 1) if t > 8 else (t, 0))


def test_digit_minus_eight_cannot_occur():
    got = {(t - 16 if t > 8 else t) for x in range(16) for c in (0, 1) for t in (x + c,)}
    assert got == set(range(-7, 9))
    assert set(V.DIGITS) == got - {0}
    # 8 without a carry against 9 with one
    assert V.recode(8, 2) == ([8, 0], [0, 0, 0]) and V.recode(9, 2) == ([-7, 1], [0, 1, 0])


def test_edge_scalars():
    E = V.EDGE
    assert [E[n] for n in ("0", "1", "2", "r-1", "r-2")] == [0, 1, 2, O.R - 1, O.R - 2]
    assert V.halves(E["lambda-1"], "glv") == (V.LAMBDA - 1, 0)
    assert V.halves(E["lambda"], "glv") == (0, 1)
    assert V.halves(E["lambda+1"], "glv") == (1, 1)
    assert E["k2max"] == V.R - 1 and V.halves(E["k2max"], "glv") == (0, V.LAMBDA + 1)
    assert max(k // V.LAMBDA for k in (V.R - 1, V.R - 2)) == V.LAMBDA + 1  # no k < r has a larger k2
    assert V.halves(E["halves_max"], "glv") == (V.LAMBDA - 1, V.LAMBDA)
    assert all(0 <= k < V.R for k in E.values())


@pytest.mark.parametrize("form", V.FORMS)
def test_pattern_scalars_keep_their_nibbles(form):
    nw = V.NW[form]
    for name, k in V.pattern_scalars(form).items():
        assert 0 <= k < V.R
        base = name.split(".k")[0]
        pat = V.PATTERNS[base][-nw:]
        which = {"plain": (0,), "k1": (0,), "k2": (1,), "k1k2": (0, 1)}[name.split(".")[-1] if form == "glv" else "plain"]
        hv = V.halves(k, form)
        for half in range(len(hv)):
            if half not in which:
                assert hv[half] == 0, name
                continue
            v = hv[half]
            top = (v.bit_length() + 3) // 4
            assert top >= nw - 2, name  # at most two top nibbles were cleared
            assert "%x" % v == pat[nw - top:].lower(), name
            digits, carry_in = V.recode(v, nw)
            if base in ("8..89", "9", "F"):  # a carry chain through every window
                assert carry_in[1:top + 1] == [1] * top, name
            if base == "8":                       # digit 8 and no carry anywhere
                assert digits[:top] == [8] * top and not any(carry_in), name
            if base == "7..78":
                assert digits[:top] == [8] + [7] * (top - 1) and not any(carry_in), name
            if base == "8..89":                 # 8 + carry = 9: the carry test's other side
                assert digits[:top] == [-7] * top and digits[top] == 1, name
            if base == "F":                          # digit 0 that still carries
                assert digits[:top] == [-1] + [0] * (top - 1) and digits[top] == 1, name


@pytest.mark.parametrize("form", V.FORMS)
def test_carry_crosses_exactly_one_boundary(form):
    nw = V.NW[form]
    seen = set()
    for (half, b), k in V.carry_into(form).items():
        hv = V.halves(k, form)
        assert all(hv[h] == 0 for h in range(len(hv)) if h != half)
        digits, carry_in = V.recode(hv[half], nw)
        assert [w for w in range(nw + 1) if carry_in[w]] == [b]
        assert digits[b - 1] == -7 and digits[b] == 1 and sum(1 for d in digits if d) == 2
        seen.update(V.boundaries(form, half, b))
    # every chunk start but the first of a half and every sub-chunk start but a chunk's first, for every lpq
    n_half = 1 if form == "plain" else 2
    want = set()
    for half in range(n_half):
        for c in range(nw // 8):
            ch = c + (4 * half if form == "glv" else 0)
            for lpq in V.LPQS:
                for sub in range(8 // lpq):
                    if c or sub:
                        want.add((ch, lpq, sub))
    assert seen == want
    assert {ch for ch, _, _ in want} == set(range(8))


@pytest.mark.parametrize("form", V.FORMS)
def test_single_digit_scalars(form):
    nw = V.NW[form]
    S = V.single_digit(form)
    for (half, w, d), k in S.items():
        hv = V.halves(k, form)
        digits, carry_in = V.recode(hv[half], nw)
        assert [(i, x) for i, x in enumerate(digits) if x] == [(w, d)] and not any(carry_in)
        assert all(hv[h] == 0 for h in range(len(hv)) if h != half)
    # left out: only what no value within the half's bound can hold
    for half, bound in enumerate(V.half_bounds(form)):
        missing = {(w, d) for w in range(nw) for d in (1, 8) if (half, w, d) not in S}
        assert missing == {(w, d) for w in range(nw) for d in (1, 8) if d << (4 * w) > bound}
        assert missing == ({(63, 8)} if form == "plain" else {(31, 8)})
        assert (half, nw - 1, 1) in S  # the top window


@pytest.mark.parametrize("form", V.FORMS)
def test_coverage_is_every_reachable_digit_in_every_window(form):
    nw = V.NW[form]
    ks = V.coverage(form)
    assert all(0 <= k < V.R for k in ks) and len(ks) <= 64
    have = V.covered(form, ks)
    for half, bound in enumerate(V.half_bounds(form)):
        reach = V.reachable_digits(form, half)
        # the condition: nothing reachable is left out, nothing unreachable appears
        assert {(w, d) for h, w, d in have if h == half} == set(reach)
        # every digit in every window below the top ones
        for w in range(nw - 2 if form == "plain" else nw - 1):
            assert {d for ww, d in reach if ww == w} == set(V.DIGITS), (half, w)
        # the top windows: what the bound leaves, by brute force over the top nibbles with and without a carry in
        # (both are fixed by the top two nibbles and the carry into them, whose smallest source is 0x88..89)
        for w in (nw - 2, nw - 1):
            brute = set()
            for hi in range(0, (bound >> (4 * (nw - 2))) + 1):  # the top two nibbles
                for low in (0, V.min_carry_source(nw - 2)):
                    v = (hi << (4 * (nw - 2))) + low
                    if v <= bound:
                        d = V.recode(v, nw)[0][w]
                        if d:
                            brute.add(d)
            assert brute == {d for ww, d in reach if ww == w}, (half, w)
    print(form, len(ks), "coverage scalars;", {h: sorted((w, d) for (w, d) in V.reachable_digits(form, h)
                                                          if w >= nw - 2) for h in range(len(V.half_bounds(form)))})


@pytest.mark.parametrize("form", V.FORMS)
def test_scalar_list(form):
    ks = V.scalar_list(form)
    assert len(set(ks)) == len(ks) and all(0 <= k < V.R for k in ks)
    assert set(V.EDGE.values()) <= set(ks) and set(V.coverage(form)) <= set(ks)
    w = V.fr_words(ks)
    assert w.shape == (len(ks), 4) and w.dtype == np.uint64
    assert [sum(int(x) << (64 * i) for i, x in enumerate(r)) for r in w] == ks
    print(form, len(ks), "scalars")


def test_group_members_and_shapes():
    # the MIPP fold (D = 1): group g takes every L-th base from g
    assert V.members_strided(2, 3, 4, 1) == [2, 6, 10]
    # a cross product (D = L / 2): two groups, halves of each block of L
    assert V.members_strided(1, 4, 4, 2) == [2, 3, 6, 7]
    assert V.members_seg([0, 1, 1, 6, 14], 2) == [1, 2, 3, 4, 5] and V.members_seg([0, 1, 1, 6, 14], 1) == []
    assert [V.small_quad_shape(m) for m in (1, 2, 3, 4, 5, 7, 8)] == [
        (1, 64), (2, 64), (4, 48), (4, 64), (8, 40), (8, 56), (8, 64)]
    assert V.tree_levels(1) == [8, 1] and V.tree_levels(8) == [64, 1]
    assert V.tree_levels(9) == [72, 1] and V.tree_levels(32) == [256, 1]
    assert V.tree_levels(33) == [264, 2, 1] and V.tree_levels(64) == [512, 2, 1]
    assert V.tree_levels(8193) == [65544, 257, 2, 1]


def test_base_kinds():
    rng = np.random.default_rng(3)
    for g2 in (False, True):
        w = 24 if g2 else 12
        pool = rng.integers(1, 1 << 40, (9, w), dtype=np.uint64)  # stand-ins: only the layout matters here
        neg = V.negate(pool, g2)
        assert np.array_equal(neg[:, :w // 2], pool[:, :w // 2])
        for j in range(w // 2, w, 6):
            for a, b in zip(pool, neg):
                assert sum((int(x) + int(y)) << (64 * i) for i, (x, y) in enumerate(zip(a[j:j + 6], b[j:j + 6]))) == O.P
        assert not V.negate(np.zeros((1, w), dtype=np.uint64), g2).any()
        assert np.array_equal(V.negate(neg, g2), pool)
        b = V.base_set(pool, "inf", 9, g2)
        assert [i for i in range(9) if not b[i].any()] == [0, 4, 8]
        assert not V.base_set(pool, "allinf", 5, g2).any()
        c = V.base_set(pool, "cancel", 6, g2)
        assert np.array_equal(c[0], c[2]) and np.array_equal(c[1], neg[5]) and np.array_equal(c[0], pool[5])
        assert len({r.tobytes() for r in V.base_set(pool, "equal", 7, g2)}) == 1
        assert len({r.tobytes() for r in V.base_set(pool, "distinct", 7, g2)}) == 7
