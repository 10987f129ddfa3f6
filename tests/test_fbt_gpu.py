"""The fixed-base table engine (csrc/fbt.h: fbt_build, fbt_msm) through its
self-test entry point (tpst_selftest_fbt), bit-exact against the CPU oracle.

The reference of a group's sum is the oracle MSM (orc.g1_msm / orc.g2_msm) over
that group's members, listed from the definition in csrc/fbt.h
(fbt_vectors.members_strided / members_seg); of a table entry (k, w, m) it is
((m + 1) 16^w b_k mod r) G.  No tolerance anywhere: np.array_equal on canonical
words.  Scalars are the constructed classes of tests/fbt_vectors.py (proved on
the host by test_fbt_vectors.py), bases b_i G.

Paths of fbt_msm, with Q = 64 quads per block, len = 8 * members, G = groups *
sets:
  small       strided, members <= 8, G <= 256: k_fbt_small_quad in one launch;
  one level   k_fbt_partial_quad, then k_seg_sum_quad once (len <= 256);
  two levels  ... twice (len <= 65536);
  three       ... three times, the third writing back into the first buffer.
Segment groups always take the two-launch path.
"""
import numpy as np
import pytest

import bls377 as O
import fbt_vectors as V
import orc
from testudo_amd import TpstError
from testudo_amd.encoding import fr_array, limbs_to_int

pytestmark = pytest.mark.gpu

F3 = (("g1", "plain"), ("g1", "glv"), ("g2", "plain"))
F3_IDS = ["-".join(f) for f in F3]
POOL = 600


@pytest.fixture(scope="module")
def pools():
    """distinct bases b_i G of both groups and the b_i"""
    b, _ = orc.fr_stream(0xFB70, POOL)
    out = {"b": [limbs_to_int(x) for x in b], "g1": orc.g1_mul_gen(b), "g2": orc.g2_mul_gen(b)}
    for k in ("g1", "g2"):
        out[k].setflags(write=False)
    return out


@pytest.fixture(scope="module")
def scalars():
    """the constructed scalars of each table form, then uniform ones"""
    rnd, _ = orc.fr_stream(0xFB71, 9000)
    out = {f: np.concatenate([V.fr_words(V.scalar_list(f)), rnd]) for f in V.FORMS}
    for v in out.values():
        v.setflags(write=False)
    return out


def _msm(grp, bases, s):
    if not len(bases):
        return np.zeros(24 if grp == "g2" else 12, dtype=np.uint64)
    return (orc.g2_msm if grp == "g2" else orc.g1_msm)(bases, s, parallel=len(bases) > 64)


def _run(ctx, f3, bases, s, **shape):
    return ctx.selftest_fbt(bases, s, g2=f3[0] == "g2", glv=f3[1] == "glv", **shape)


def _check(ctx, f3, path, bases, s, groups, members, L=1, D=1, seg=None, sets=1, set_stride=0, got=None):
    """run one grouped MSM and compare every output with the oracle"""
    if got is None:
        got = _run(ctx, f3, bases, s, groups=groups, members=members, L=L, D=D, seg=seg, sets=sets,
                   set_stride=set_stride)
    assert got.shape[0] == sets * groups
    for q in range(sets):
        for g in range(groups):
            idx = np.array(V.members_seg(seg, g) if seg is not None else V.members_strided(g, members, L, D), dtype=int)
            ref = _msm(f3[0], bases[idx], s[idx + q * set_stride])
            assert np.array_equal(got[q * groups + g], ref), \
                "form=%s-%s path=%s members=%d L=%d D=%d sets=%d set=%d group=%d" % (f3 + (path, members, L, D, sets, q, g))
    return got


# ------------------------------------------------------------------ table --
@pytest.mark.parametrize("f3", F3, ids=F3_IDS)
def test_table_entries(ctx, pools, f3):
    """every entry (k, w, m) of the table of a generic base, G itself and
    infinity: k_fbt_pow_quad + k_fbt_mult8 (G1, plain and GLV; the infinity base
    takes k_fbt_mult8's ZZ == 0 arm in every window) and k_fbt_pow + k_fbt_mult
    (G2)"""
    grp, form = f3
    nw = V.NW[form]
    bs = [pools["b"][7], 1, None]
    bases = np.concatenate([pools[grp][7:8], (orc.g2_mul_gen if grp == "g2" else orc.g1_mul_gen)(fr_array([1])),
                            np.zeros((1, pools[grp].shape[1]), dtype=np.uint64)])
    got = _run(ctx, f3, bases, None, table=True).reshape(3, nw, 8, -1)
    for k, b in enumerate(bs):
        if b is None:
            assert not got[k].any(), "form=%s-%s base=%d (infinity)" % (grp, form, k)
            continue
        mult = fr_array([(m + 1) * 16**w * b % O.R for w in range(nw) for m in range(8)])
        ref = (orc.g2_mul_gen if grp == "g2" else orc.g1_mul_gen)(mult).reshape(nw, 8, -1)
        bad = np.argwhere((got[k] != ref).any(axis=2))
        assert not len(bad), "form=%s-%s base=%d first wrong (w, m)=%s of %d" % (grp, form, k, bad[0], len(bad))


# ------------------------------------------------------- small-quad path --
@pytest.mark.parametrize("members", [1, 2, 3, 4, 5, 7, 8])
@pytest.mark.parametrize("f3", F3, ids=F3_IDS)
def test_small_quad_fold_groups(ctx, pools, scalars, f3, members):
    """D = 1 (the MIPP fold's groups) over every constructed scalar: lpq 1, 2,
    4, 4, 8, 8, 8 and 64, 64, 48, 64, 40, 56, 64 units in quad_tree"""
    n_list = len(V.scalar_list(f3[1]))
    groups = -(-n_list // members)
    assert groups <= 256 and V.small_quad_shape(members)[1] <= 64
    n = groups * members
    _check(ctx, f3, "small", pools[f3[0]][:n], scalars[f3[1]][:n], groups, members, L=groups, D=1)


@pytest.mark.parametrize("members", [2, 4, 8])
@pytest.mark.parametrize("f3", F3, ids=F3_IDS)
def test_small_quad_cross_groups(ctx, pools, scalars, f3, members):
    """D = L / 2 (the cross products' two groups): 2 * members scalars per call,
    over every constructed scalar"""
    n_list = len(V.scalar_list(f3[1]))
    n = 2 * members
    for c in range(-(-n_list // n)):
        _check(ctx, f3, "small call %d" % c, pools[f3[0]][c * n:(c + 1) * n], scalars[f3[1]][c * n:(c + 1) * n], 2,
               members, L=members, D=members // 2)


# ---------------------------------------------------------------- the cap --
@pytest.mark.parametrize("members", [1, 8])
@pytest.mark.parametrize("f3", F3, ids=F3_IDS)
def test_cap_by_groups(ctx, pools, scalars, f3, members):
    """G = 256 is the last size of the one-launch kernel, G = 257 the first of
    the two-launch path (len 8 and 64: one block per segment).  Same L, so the
    first 256 groups are the same sums."""
    L = 257
    n = L * members
    bases = np.concatenate([pools[f3[0]]] * -(-n // POOL))[:n]
    s = scalars[f3[1]][:n]
    two = _check(ctx, f3, "two-launch G=257", bases, s, 257, members, L=L, D=1)
    one = _run(ctx, f3, bases, s, groups=256, members=members, L=L, D=1)
    assert np.array_equal(one, two[:256]), "form=%s-%s members=%d: G=256 and G=257 differ in groups %s" % (
        f3 + (members, np.nonzero((one != two[:256]).any(axis=1))[0][:8]))


@pytest.mark.parametrize("members", [1, 8])
@pytest.mark.parametrize("f3", F3, ids=F3_IDS)
def test_cap_by_sets(ctx, pools, scalars, f3, members):
    """G = 129 groups * 2 sets = 258 takes the two-launch path; each set alone
    (G = 129) the one-launch kernel"""
    L = 129
    n = L * members
    bases = np.concatenate([pools[f3[0]]] * -(-n // POOL))[:n]
    s = scalars[f3[1]][:2 * n]
    two = _check(ctx, f3, "two-launch G=258", bases, s, L, members, L=L, D=1, sets=2, set_stride=n)
    for q in range(2):
        one = _run(ctx, f3, bases, s[q * n:(q + 1) * n], groups=L, members=members, L=L, D=1)
        assert np.array_equal(one, two[q * L:(q + 1) * L]), (f3, members, q)


# ------------------------------------------------------ two-launch path ----
@pytest.mark.parametrize("members,shape", [(9, "one"), (32, "one"), (32, "four"), (33, "one"), (64, "one"),
                                           (33, "four"), (64, "four")])
@pytest.mark.parametrize("f3", F3, ids=F3_IDS)
def test_tree_levels(ctx, pools, scalars, f3, members, shape):
    """members 9 and 32: len 72 and 256, one k_seg_sum_quad launch (per = 256,
    parts = 1); 33 and 64: len 264 and 512, parts = 2, a second launch.  'one':
    a plain MSM (L = D = n); 'four': four groups, L = 4 D"""
    assert len(V.tree_levels(members)) == (2 if members <= 32 else 3)
    if shape == "one":
        groups, L, D = 1, members, members
    else:
        D = 2 if members % 2 == 0 else 1
        groups, L = 4, 4 * D
    n = groups * members
    _check(ctx, f3, "%d levels" % (len(V.tree_levels(members)) - 1), pools[f3[0]][:n], scalars[f3[1]][:n], groups,
           members, L=L, D=D)


def test_three_tree_levels(ctx):
    """n = members = 8193, one group, G1 GLV: len 65544 -> 257 -> 2 -> 1.  The
    only case whose third k_seg_sum_quad launch runs -- the first to write back
    into buffer a after the a / b swap.  The opening does not reach it at its
    tested sizes (its largest group there has far fewer than 8193 members).
    Bases b_i G from the device, so the expected sum is (sum s_i b_i mod r) G."""
    n = 8193
    assert V.tree_levels(n) == [65544, 257, 2, 1]
    b, _ = orc.fr_stream(0xFB72, n)
    s, _ = orc.fr_stream(0xFB73, n)
    edge = V.fr_words(V.scalar_list("glv"))
    s[::37][:len(edge)] = edge[:len(s[::37])]
    bases = ctx.g1_mul_generator(b)
    got = ctx.selftest_fbt(bases, s, glv=True, groups=1, members=n, L=n, D=n)
    tot = sum(limbs_to_int(x) * limbs_to_int(y) for x, y in zip(s, b)) % O.R
    assert np.array_equal(got[0], orc.g1_mul_gen(fr_array([tot]))[0]), "form=g1-glv path=3 levels members=8193"


# --------------------------------------------------------------- segments --
SEGS = {"1,0,5,8": (1, 0, 5, 8), "33,2,0,64": (33, 2, 0, 64), "pst k=4": (8, 4, 2, 1)}


@pytest.mark.parametrize("lens", list(SEGS), ids=list(SEGS))
@pytest.mark.parametrize("f3", [F3[1], F3[2]], ids=[F3_IDS[1], F3_IDS[2]])
def test_segment_groups(ctx, pools, scalars, f3, lens):
    """d_seg groups: unequal lengths (the m >= hi - lo arm), an empty segment
    (infinity), a whole segment in one block with len <= 64 (lengths 1..8), and
    the PST level proofs' shape (groups = k, members = 2^(k-1), segments of
    2^(k-1) .. 1 bases)"""
    lens = SEGS[lens]
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    n = int(seg[-1])
    got = _check(ctx, f3, "segments " + str(lens), pools[f3[0]][:n], scalars[f3[1]][:n], len(lens), max(lens), seg=seg)
    for g, ln in enumerate(lens):
        if not ln:
            assert not got[g].any()
    # members above the longest segment: every group takes the m >= hi - lo arm
    more = _run(ctx, f3, pools[f3[0]][:n], scalars[f3[1]][:n], groups=len(lens), members=max(lens) + 3, seg=seg)
    assert np.array_equal(more, got)
    # segments that start past base 0 and leave bases unused at the end
    seg2 = (seg + 2).astype(np.uint32)
    _check(ctx, f3, "segments+2 " + str(lens), pools[f3[0]][:n + 5], scalars[f3[1]][:n + 5], len(lens), max(lens), seg=seg2)


# ------------------------------------------------------------------- sets --
@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("sets", [2, 3])
@pytest.mark.parametrize("path,groups,members", [("small", 3, 4), ("two-launch", 2, 12), ("segments", 3, 5)])
@pytest.mark.parametrize("f3", F3, ids=F3_IDS)
def test_scalar_sets(ctx, pools, scalars, f3, path, groups, members, sets, pad):
    """sets > 1: set q reads the scalars at k + q set_stride and writes slot q
    groups + g.  pad > 0: scalars between the sets that no group may read, set
    to r - 1, then to 0: the result must not move."""
    seg = None
    if path == "segments":
        seg = np.array([0, 5, 7, 11], dtype=np.uint32)
    n = int(seg[-1]) if seg is not None else groups * members
    stride = n + pad
    s = scalars[f3[1]][40:40 + sets * stride].copy()
    rm1 = fr_array([O.R - 1])[0]
    for q in range(sets):
        s[q * stride + n:(q + 1) * stride] = rm1
    kw = dict(L=groups, D=1, seg=seg, sets=sets, set_stride=stride)
    got = _check(ctx, f3, path, pools[f3[0]][:n], s, groups, members, **kw)
    assert len({r.tobytes() for r in got}) == sets * groups  # the sets differ
    if pad:
        for q in range(sets):
            s[q * stride + n:(q + 1) * stride] = 0
        again = _run(ctx, f3, pools[f3[0]][:n], s, groups=groups, members=members, **kw)
        assert np.array_equal(again, got), "form=%s-%s path=%s sets=%d: the padding scalars were read" % (f3 + (path, sets))


# ------------------------------------------------------------- collisions --
PATHS = {"small": (3, 8), "one level": (2, 20), "two levels": (2, 40)}
COLLISIONS = ("equal", "cancel", "zero", "last", "inf", "allinf")


@pytest.mark.parametrize("kind", COLLISIONS)
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("f3", F3, ids=F3_IDS)
def test_collisions(ctx, pools, scalars, f3, path, kind):
    """equal and opposite operands in quad_tree and in k_seg_sum_quad's serial
    sums, which distinct random bases never produce:
      equal   every member of a group the same base and scalar: add_quad(P, P)
              at every tree level;
      cancel  P, -P alternating with equal scalars: add_quad(P, -P), each
              group's sum is infinity (all-zero words);
      zero    every scalar 0;  last: only the last member's scalar nonzero;
      inf     infinity bases at the first, a middle and the last index;
      allinf  every base infinity."""
    groups, members = PATHS[path]
    grp = f3[0]
    n = groups * members
    pool = pools[grp]
    bases = pool[:n].copy()
    s = scalars[f3[1]][100:100 + n].copy()
    idx = [V.members_strided(g, members, groups, 1) for g in range(groups)]
    if kind in ("equal", "cancel"):
        neg = V.negate(pool[:groups], grp == "g2")
        for g in range(groups):
            for j, k in enumerate(idx[g]):
                bases[k] = neg[g] if kind == "cancel" and j % 2 else pool[g]
                s[k] = scalars[f3[1]][3 + g]  # r - 1, r - 2, lambda - 1: a nonzero scalar per group
    elif kind == "zero":
        s[:] = 0
    elif kind == "last":
        s[:] = 0
        for g in range(groups):
            s[idx[g][-1]] = scalars[f3[1]][3 + g]
    else:
        bases = V.base_set(pool, kind, n, grp == "g2")
    got = _check(ctx, f3, path + " " + kind, bases, s, groups, members, L=groups, D=1)
    if kind in ("cancel", "zero", "allinf"):
        assert not got.any(), (f3, path, kind)
    else:
        assert got.any(axis=1).all(), (f3, path, kind)


@pytest.mark.parametrize("f3", F3, ids=F3_IDS)
def test_no_members_is_infinity(ctx, pools, scalars, f3):
    got = _run(ctx, f3, pools[f3[0]][:4], scalars[f3[1]][:4], groups=3, members=0, L=3, D=1)
    assert got.shape[0] == 3 and not got.any()


# ------------------------------------------------- agreement of the forms --
@pytest.mark.parametrize("groups,members", [(58, 8), (16, 29), (8, 64)])
def test_glv_and_plain_tables_agree(ctx, pools, scalars, groups, members):
    """the same bases and scalars (both forms' constructed classes) through the
    G1 GLV table and the G1 plain table"""
    n = groups * members
    s = np.concatenate([V.fr_words(V.scalar_list("glv")), scalars["plain"]])[:n]
    assert n >= len(V.scalar_list("glv")) + len(V.scalar_list("plain"))
    kw = dict(groups=groups, members=members, L=groups, D=1)
    a = ctx.selftest_fbt(pools["g1"][:n], s, glv=True, **kw)
    b = ctx.selftest_fbt(pools["g1"][:n], s, glv=False, **kw)
    assert np.array_equal(a, b), (groups, members, np.nonzero((a != b).any(axis=1))[0])
    _check(ctx, ("g1", "plain"), "forms", pools["g1"][:n], s, got=b, **kw)


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
def test_product_entry_points_agree(ctx, pools, scalars, g2):
    """tpst_g1_msm_fixed / tpst_g2_msm_fixed against the self-test entry on the
    shapes both can express"""
    n = 64
    bases = pools["g2" if g2 else "g1"][:n].copy()
    bases[5] = 0
    s = scalars["plain"][:n]
    for L, D in ((n, n), (16, 1), (16, 8), (8, 2)):
        a = ctx.msm_fixed(bases, s, L, D, g2=g2)
        b = ctx.selftest_fbt(bases, s, g2=g2, groups=L // D, members=n // L * D, L=L, D=D)
        assert np.array_equal(a, b), (g2, L, D)


# ---------------------------------------------------------- bad arguments --
def test_bad_arguments_are_errors(ctx, pools, scalars):
    """every validation rule of tpst_selftest_fbt as an error return: nothing
    here is launched"""
    b1, b2, s = pools["g1"][:16], pools["g2"][:16], scalars["plain"][:32]
    ok = dict(groups=4, members=4, L=4, D=1)

    def bad(bases=b1, sc=s, **kw):
        a = dict(ok)
        a.update(kw)
        with pytest.raises(TpstError):
            ctx.selftest_fbt(bases, sc, **a)

    bad(bases=b2, g2=True, glv=True)                    # GLV with G2
    bad(bases=b2, g2=True, glv=True, table=True)
    bad(groups=0)
    bad(sets=0)
    bad(L=0)
    bad(D=0)
    bad(groups=5)                                       # group 4's last member is base 16 = n
    bad(members=5)                                      # member 4 of group 0 is base 16
    bad(L=5)                                            # (m / D) L walks past n
    bad(L=8, D=3, groups=1, members=8)                  # m / D = 2 starts a third block of 8 at base 16
    bad(sc=s[:15])                                      # base 15's scalar is missing
    bad(sets=2, set_stride=16, sc=s[:31])               # set 1's last scalar is missing
    bad(sets=3, set_stride=16)                          # set 2 is past the 32 scalars
    bad(sets=2, set_stride=17)
    bad(sets=2, set_stride=1 << 40)
    bad(groups=1 << 17, members=0)                      # above the documented bounds
    bad(members=1 << 17, groups=1)
    bad(L=1 << 40)
    seg = np.array([0, 3, 3, 8, 16], dtype=np.uint32)
    ctx.selftest_fbt(b1, s, groups=4, members=8, seg=seg)  # valid
    bad(members=7, seg=seg)                             # the longest segment has 8
    bad(members=8, seg=np.array([0, 3, 2, 8, 16], dtype=np.uint32))   # decreasing
    bad(members=16, seg=np.array([0, 3, 3, 8, 17], dtype=np.uint32))  # ends past n
    bad(members=8, seg=np.array([9, 3, 3, 8, 16], dtype=np.uint32))
    bad(members=8, seg=seg, sc=s[:15])                  # a segment's scalar is missing
    bad(members=8, seg=seg, sets=2, set_stride=17)
    lib, h = ctx.lib, ctx.h
    from testudo_amd.encoding import ptr
    out = np.zeros((16, 12), dtype=np.uint64)
    big = np.zeros(((1 << 14) + 1, 12), dtype=np.uint64)
    args = (ptr(s), 32, 4, 4, 4, 1, None, 1, 0, ptr(out))
    assert lib.tpst_selftest_fbt(h, 1, 0, 0, ptr(b1), 16, *args) == 0
    assert lib.tpst_selftest_fbt(h, 1, 0, 0, ptr(b1), 0, *args) != 0          # n == 0
    assert lib.tpst_selftest_fbt(h, 1, 0, 0, ptr(big), len(big), *args) != 0  # n above the cap
    assert lib.tpst_selftest_fbt(h, 0, 0, 0, ptr(b1), 16, *args) != 0         # no such group
    assert lib.tpst_selftest_fbt(h, 3, 0, 0, ptr(b1), 16, *args) != 0
    assert lib.tpst_selftest_fbt(h, 1, 2, 0, ptr(b1), 16, *args) != 0         # no such table form
    assert lib.tpst_selftest_fbt(h, 1, 0, 2, ptr(b1), 16, *args) != 0         # no such mode
    assert lib.tpst_selftest_fbt(h, 1, 0, 0, None, 16, *args) != 0
    assert lib.tpst_selftest_fbt(h, 1, 0, 0, ptr(b1), 16, None, *args[1:]) != 0
    assert lib.tpst_selftest_fbt(h, 1, 0, 0, ptr(b1), 16, ptr(s), 0, *args[2:]) != 0
    assert lib.tpst_selftest_fbt(h, 1, 0, 0, ptr(b1), 16, *args[:-1], None) != 0
    assert lib.tpst_selftest_fbt(None, 1, 0, 0, ptr(b1), 16, *args) != 0
    for groups, members, sets in ((1 << 40, 1 << 40, 1), (1 << 62, 4, 4), (1 << 16, 1, 2), (1 << 63, 0, 2)):
        assert lib.tpst_selftest_fbt(h, 1, 0, 0, ptr(b1), 16, ptr(s), 32, groups, members, 4, 1, None, sets, 0,
                                     ptr(out)) != 0, (groups, members, sets)  # products that overflow or pass 2^16
    # and the context still works
    _check(ctx, ("g1", "plain"), "after errors", b1, s, **ok)
