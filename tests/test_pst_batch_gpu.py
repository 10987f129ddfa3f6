"""GPU tests of tpst_pst_verify_batch (csrc/pst_verify_batch.hip): B openings
decided by one combined pairing check.

Shapes: n = 4 (m_col = m_row = 2), n = 5 (odd split 2 / 3), n = 6, n = 7;
B = 1, 2, 3, 5 (multiplier and item indexing) and B = 96 (several blocks of
k_lincomb2, 96 x 11 G1 points >= POINT_CHECK_DEVICE_MIN: the device-side
validation).  tpst_pst_verify on the same item is the definition of every
verdict and of every transcript end state.

An item is the tuple sqrt_pst.verify_batch takes: (transcript, U, point, v,
pst_proof, mipp, T).  Items proved on the device start from distinct transcript
states (a label appended before the opening), so that an untouched or a
swapped transcript shows."""
import ctypes as C
import random
from dataclasses import replace

import numpy as np
import pytest

import bls377 as O
import golden_io as G
from testudo_amd import sqrt_pst as S
from testudo_amd.encoding import fr_array, g1_array, gt_array, gt_from_array, limbs_to_int, ptr

pytestmark = pytest.mark.gpu

OK, E_ARG, E_STATE, E_VERIFY = 0, -1, -4, -5
R, P = O.R, O.P


def make_rho(B, seed):
    rng = random.Random(seed)
    rho = np.zeros((B, 4, 2), dtype=np.uint64)
    for j in range(B):
        for k in range(4):
            x = rng.getrandbits(128) | 1
            rho[j, k] = (x & (2**64 - 1), x >> 64)
    return rho


def tr_bytes(tr):
    return bytes(tr.t)


def fresh(label=None):
    tr = S.PoseidonTranscript()
    if label is not None:
        tr.append_bytes(label)
    return tr


def raw(ctx, items, rho, with_ok=True, n=None):
    """the C call on (transcript, ...) tuples -> (rc, ok or None)"""
    nn, arr, keep = S.pack_items(items)
    ok = np.full(len(items), 7, dtype=np.uint8)
    rc = ctx.lib.tpst_pst_verify_batch(ctx.h, nn if n is None else n, C.cast(arr, C.c_void_p), len(items), ptr(rho),
                                       ok.ctypes.data_as(C.POINTER(C.c_uint8)) if with_ok else None)
    del keep
    return rc, (ok if with_ok else None)


def single(ctx, item, label=None):
    """tpst_pst_verify on the item from its starting state -> (verdict, end state bytes)"""
    tr = fresh(label)
    good = S.verify(ctx, tr, *item[1:])
    return good, tr_bytes(tr)


def golden_item(n):
    d = G.load("sqrt_pst_n%d.json" % n)
    mipp = S.MippProof(comms_t=np.stack([np.stack([G.gt_array(a), G.gt_array(b)]) for a, b in d["comms_t"]]),
                       comms_u=np.stack([G.g1_arr(pr) for pr in d["comms_u"]]),
                       final_a=G.g1_arr([d["final_a"]])[0], final_h=G.g2_arr([d["final_h"]])[0],
                       pst_proof_h=G.g1_arr(d["pst_proof_h"]))
    body = (G.g1_arr([d["U"]])[0], G.fr_arr(d["point"]), G.fr_arr([d["eval"]])[0], G.g2_arr(d["pst_proof"]), mipp,
            G.gt_array(d["T"]))
    return d, body


def load_golden_srs(ctx, d):
    S.srs_load(ctx, d["srs_nv"], G.srs_flat(d))


_PROVED = {}


def proved(ctx, n, B):
    """B openings of distinct polynomials at distinct points, proved on the device from labelled transcripts:
    (labels, bodies); the SRS of n is left loaded.  Proved once per n (the first B of 5)."""
    S.srs_setup(ctx, (n + 1) // 2, 0x7E57D1)
    if n not in _PROVED:
        labels, bodies = [], []
        for j in range(5):
            Z, k = S.fr_stream(0xB47C0 + 16 * n + j, 1 << n)
            pt, _ = S.fr_stream(0xB47C0 + 16 * n + j, n, k)
            pl = S.Polynomial.from_evaluations(ctx, Z)
            v = pl.eval(pt)
            comms, T = pl.commit()
            label = b"item %d" % j
            U, pst_proof, mipp = pl.open(fresh(label), comms, pt, T)
            labels.append(label)
            bodies.append((U, pt, v, pst_proof, mipp, T))
        _PROVED[n] = (labels, bodies)
    labels, bodies = _PROVED[n]
    return labels[:B], bodies[:B]


def items_of(labels, bodies):
    return [(fresh(lb),) + tuple(b) for lb, b in zip(labels, bodies)]


# ------------------------------------------------------------- 1. goldens ---
@pytest.mark.parametrize("n", [4, 5, 6, 7])
def test_golden_b1(ctx, n):
    """the golden proof as a batch of one, built from the JSON fields with no proving: TPST_OK and the
    transcript ends exactly where tpst_pst_verify leaves a copy"""
    d, body = golden_item(n)
    load_golden_srs(ctx, d)
    good, end = single(ctx, (None,) + body)
    assert good
    tr = fresh()
    rc, ok = raw(ctx, [(tr,) + body], make_rho(1, 100 + n))
    assert rc == OK and list(ok) == [1]
    assert tr_bytes(tr) == end and end != tr_bytes(fresh())


# ------------------------------------------------------ 2. valid batches ---
@pytest.mark.parametrize("n", [5, 6])
@pytest.mark.parametrize("B", [2, 3, 5])
def test_valid_batch(ctx, n, B):
    """B distinct openings: TPST_OK, every verdict 1, every transcript at the single verifier's end state"""
    labels, bodies = proved(ctx, n, B)
    ends = []
    for lb, b in zip(labels, bodies):
        good, end = single(ctx, (None,) + b, lb)
        assert good
        ends.append(end)
    assert len(set(ends)) == B
    items = items_of(labels, bodies)
    all_ok, ok = S.verify_batch(ctx, items, make_rho(B, 200 + 10 * n + B))
    assert all_ok and list(ok) == [1] * B
    assert [tr_bytes(it[0]) for it in items] == ends
    # the Python wrapper draws its own multipliers when none are given
    all_ok, ok = S.verify_batch(ctx, items_of(labels, bodies))
    assert all_ok and ok.all()


def test_agrees_with_reference_n4_b2(ctx):
    """n = 4, B = 2 (the golden proof and a second one proved on the device), same multipliers as
    tests/pst_batch_ref.py's restatement over the oracle: both accept the valid batch, both reject it with
    v + 1 in the second item"""
    import pst as OP
    import pst_batch_ref as BR
    from testudo_amd.encoding import g1_from_array, g2_from_array
    d, gbody = golden_item(4)
    load_golden_srs(ctx, d)
    Z, k = S.fr_stream(0xBA7C4, 16)
    pt, _ = S.fr_stream(0xBA7C4, 4, k)
    pl = S.Polynomial.from_evaluations(ctx, Z)
    v = pl.eval(pt)
    comms, T = pl.commit()
    U, pst_proof, mipp = pl.open(fresh(), comms, pt, T)
    bodies = [gbody, (U, pt, v, pst_proof, mipp, T)]
    rho = make_rho(2, 0x2B0)

    def to_ref(b):
        U, pt, v, pst_proof, mp, T = b
        gt = lambda t: O.fq12_from_tower(gt_from_array(t))  # noqa: E731  (limbs hold arkworks' tower order)
        return {"U": g1_from_array(U)[0], "point": [limbs_to_int(x) for x in pt], "v": limbs_to_int(v),
                "pst_proof": g2_from_array(pst_proof),
                "mipp": {"comms_t": [(gt(a), gt(b_)) for a, b_ in mp.comms_t],
                         "comms_u": [tuple(g1_from_array(pr)) for pr in mp.comms_u],
                         "final_a": g1_from_array(mp.final_a)[0], "final_h": g2_from_array(mp.final_h)[0],
                         "pst_proof_h": g1_from_array(mp.pst_proof_h)},
                "T": gt(T), "tr": OP.PoseidonTranscript}

    srs = OP.SRS(d["srs_nv"], d["srs_seed"])
    ref_rho = [tuple(int(r[k, 0]) | (int(r[k, 1]) << 64) for k in range(4)) for r in rho]
    bad_v = fr_array([(limbs_to_int(v) + 1) % R])[0]
    bad = [gbody, (U, pt, bad_v, pst_proof, mipp, T)]
    for bs, want in ((bodies, True), (bad, False)):
        rc, ok = raw(ctx, [(fresh(),) + tuple(b) for b in bs], rho)
        assert (rc == OK) == want
        assert BR.batch_accepts(srs, [to_ref(b) for b in bs], ref_rho) == want


# ------------------------------------------------------ 3. single tampers ---
def _swap01(a):
    a = a.copy()
    a[0, 0], a[0, 1] = a[0, 1].copy(), a[0, 0].copy()
    return a


def _first_from(a, other):
    a = a.copy()
    a[0] = other[0]
    return a


def _point_plus_one(pt, i):
    pt = pt.copy()
    pt[i] = fr_array([(limbs_to_int(pt[i]) + 1) % R])[0]
    return pt


# (U, point, v, pst_proof, mipp, T) of the item and of another item -> the tampered body
TAMPERS = {
    "v + 1": lambda a, o: (a[0], a[1], fr_array([(limbs_to_int(a[2]) + 1) % R])[0], a[3], a[4], a[5]),
    "other T": lambda a, o: a[:5] + (o[5],),
    "other U": lambda a, o: (o[0],) + a[1:],
    "comms_t[0] swapped": lambda a, o: a[:4] + (replace(a[4], comms_t=_swap01(a[4].comms_t)), a[5]),
    "comms_u[0] swapped": lambda a, o: a[:4] + (replace(a[4], comms_u=_swap01(a[4].comms_u)), a[5]),
    "other final_a": lambda a, o: a[:4] + (replace(a[4], final_a=o[4].final_a), a[5]),
    "other final_h": lambda a, o: a[:4] + (replace(a[4], final_h=o[4].final_h), a[5]),
    "other pst_proof[0]": lambda a, o: a[:3] + (_first_from(a[3], o[3]), a[4], a[5]),
    "other pst_proof_h[0]": lambda a, o: a[:4] + (replace(a[4], pst_proof_h=_first_from(a[4].pst_proof_h, o[4].pst_proof_h)),
                                                 a[5]),
    "point[0] + 1": lambda a, o: (a[0], _point_plus_one(a[1], 0)) + a[2:],
    "point[last] + 1": lambda a, o: (a[0], _point_plus_one(a[1], len(a[1]) - 1)) + a[2:],
}


@pytest.mark.parametrize("name", sorted(TAMPERS))
def test_single_tamper(ctx, name):
    """B = 5 at n = 5, one field of one item changed, at the first, a middle and the last item: TPST_E_VERIFY,
    ok[] has exactly that item 0 and equals the five single verdicts, the tampered item's transcript is
    unchanged and the others are at their end states; with ok = NULL the same return code"""
    labels, bodies = proved(ctx, 5, 5)
    for pos in (0, 2, 4):
        bs = list(bodies)
        bs[pos] = TAMPERS[name](tuple(bodies[pos]), tuple(bodies[(pos + 1) % 5]))
        verdicts, ends = zip(*[single(ctx, (None,) + tuple(b), lb) for lb, b in zip(labels, bs)])
        assert list(verdicts) == [j != pos for j in range(5)], (name, pos)
        items = items_of(labels, bs)
        rc, ok = raw(ctx, items, make_rho(5, 300 + pos))
        assert rc == E_VERIFY
        assert list(ok) == [int(x) for x in verdicts], (name, pos)
        for j, it in enumerate(items):
            assert tr_bytes(it[0]) == (tr_bytes(fresh(labels[j])) if j == pos else ends[j]), (name, pos, j)
        rc, _ = raw(ctx, items_of(labels, bs), make_rho(5, 300 + pos), with_ok=False)
        assert rc == E_VERIFY


# ------------------------------------------------------ 4. cancelling pair ---
def test_cancelling_pair(ctx):
    """Items a and b carry T_a delta and T_b / delta with delta = e(g, h) (from multi_pairing): each is
    invalid on its own, but their errors cancel in an unweighted product of the T checks.  With distinct
    multipliers the batch is rejected and ok marks both; with rho_T EQUAL for a and b (ok = NULL) it is
    accepted.  That acceptance is the black-box evidence that one combined equation decided -- no per-item
    check could pass -- and it is why include/tpst.h demands multipliers drawn uniformly at random after the
    proofs are fixed: a prover who knows that two items share a multiplier can forge this pair."""
    labels, bodies = proved(ctx, 5, 3)
    flat = S.srs_export(ctx, 3)
    delta = O.fq12_from_tower(gt_from_array(ctx.multi_pairing(flat[:12], flat[12:36])))
    mul = lambda T, f: gt_array(O.fq12_to_tower(O.f12_mul(O.fq12_from_tower(gt_from_array(T)), f))).reshape(72)  # noqa: E731
    bs = [tuple(b) for b in bodies]
    bs[0] = bs[0][:5] + (mul(bs[0][5], delta),)
    bs[2] = bs[2][:5] + (mul(bs[2][5], O.f12_inv(delta)),)
    assert [single(ctx, (None,) + b, lb)[0] for lb, b in zip(labels, bs)] == [False, True, False]
    rho = make_rho(3, 400)
    assert tuple(rho[0, 0]) != tuple(rho[2, 0])
    rc, ok = raw(ctx, items_of(labels, bs), rho)
    assert rc == E_VERIFY and list(ok) == [0, 1, 0]
    rho[2, 0] = rho[0, 0]
    rc, _ = raw(ctx, items_of(labels, bs), rho, with_ok=False)
    assert rc == OK


# --------------------------------------------------- 5. malformed elements ---
def _g1_off_subgroup():
    """a curve point outside the r-torsion, as tests/test_point_codec_gpu.py builds it"""
    import serialize as OS
    rng = random.Random(0x0FF5)
    while True:
        x = rng.randrange(P)
        y = OS._fq_sqrt((x * x * x + 1) % P)
        if y is not None and O.g1_on_curve((x, y)) and not O.g1_in_subgroup((x, y)):
            return g1_array([(x, y)])[0]


def _limbs_plus_p(a, off):
    """the canonical Fq at a[off : off + 6] plus p: the same residue, not canonical"""
    a = a.copy()
    v = limbs_to_int(a[off:off + 6]) + P
    assert v < 2**384
    a[off:off + 6] = [(v >> (64 * k)) & (2**64 - 1) for k in range(6)]
    return a


def _gt_outside(T):
    T = T.copy()
    T[0] += np.uint64(1)  # one coefficient + 1: still < p, no longer of order dividing r
    return T


def _comms_t_outside(mp):
    ct = mp.comms_t.copy()
    ct[1, 0] = _gt_outside(ct[1, 0])
    return replace(mp, comms_t=ct)


def _off_curve(pt):
    pt = pt.copy()
    pt[0] ^= np.uint64(1)
    return pt


MALFORMED = {
    "Fq limb + p": lambda a: (_limbs_plus_p(a[0], 6),) + a[1:],
    "off-curve final_a": lambda a: a[:4] + (replace(a[4], final_a=_off_curve(a[4].final_a)), a[5]),
    "final_a outside the subgroup": lambda a: a[:4] + (replace(a[4], final_a=_g1_off_subgroup()), a[5]),
    "comms_u outside the subgroup": lambda a: a[:4] + (replace(a[4], comms_u=_first_from(
        a[4].comms_u, np.stack([np.stack([_g1_off_subgroup(), a[4].comms_u[0, 1]])]))), a[5]),
    "comms_t outside GT": lambda a: a[:4] + (_comms_t_outside(a[4]), a[5]),
    "T outside GT": lambda a: a[:5] + (_gt_outside(a[5]),),
    "v >= r": lambda a: a[:2] + (fr_array([R])[0],) + a[3:],
    "point coordinate >= r": lambda a: (a[0], np.concatenate([a[1][:1], fr_array([R + 5]), a[1][2:]])) + a[2:],
}


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_malformed_element(ctx, name):
    """B = 3 at n = 6, one malformed element in the middle item: that item is rejected with its transcript
    untouched (nothing of it was absorbed), the other two are accepted and advanced; tpst_pst_verify rejects
    the item too"""
    labels, bodies = proved(ctx, 6, 3)
    bs = [tuple(b) for b in bodies]
    bs[1] = MALFORMED[name](bs[1])
    assert not single(ctx, (None,) + bs[1], labels[1])[0]
    ends = [single(ctx, (None,) + bs[j], labels[j])[1] for j in (0, 2)]
    items = items_of(labels, bs)
    rc, ok = raw(ctx, items, make_rho(3, 500))
    assert rc == E_VERIFY and list(ok) == [1, 0, 1]
    assert tr_bytes(items[1][0]) == tr_bytes(fresh(labels[1]))
    assert [tr_bytes(items[0][0]), tr_bytes(items[2][0])] == ends


# ------------------------------------------------------------- 6. B = 96 ---
def test_b96_device_validation(ctx):
    """96 copies of the n = 7 golden proof, each with its own transcript; item 57 carries a final_a outside
    the subgroup.  96 x 11 G1 points >= POINT_CHECK_DEVICE_MIN, so they are validated on the device (the
    point_codec stage shows the launch).  ok has its single zero at 57; without the tamper TPST_OK."""
    d, body = golden_item(7)
    load_golden_srs(ctx, d)
    B = 96
    assert B * (2 + 3 * 3) >= 1024
    _, end = single(ctx, (None,) + body)
    bad = body[:4] + (replace(body[4], final_a=_g1_off_subgroup()), body[5])
    items = [(fresh(),) + (bad if j == 57 else body) for j in range(B)]
    rho = make_rho(B, 600)
    ctx.profile(True)
    try:
        ctx.profile_reset()
        rc, ok = raw(ctx, items, rho)
        launches = ctx.profile_read()["point_codec"][1]
    finally:
        ctx.profile(False)
    assert rc == E_VERIFY
    assert [j for j in range(B) if not ok[j]] == [57]
    assert launches >= 1
    start = tr_bytes(fresh())
    assert all(tr_bytes(it[0]) == (start if j == 57 else end) for j, it in enumerate(items))
    items = [(fresh(),) + body for j in range(B)]
    rc, ok = raw(ctx, items, rho)
    assert rc == OK and ok.all()
    assert all(tr_bytes(it[0]) == end for it in items)


# -------------------------------------------------------------- 7. misuse ---
def test_misuse(ctx):
    """B = 0 -> TPST_OK; null items, null rho, a zero multiplier, an item whose proof->m_col does not match
    n -> TPST_E_ARG; a context without an SRS -> TPST_E_STATE"""
    from testudo_amd import Context
    d, body = golden_item(4)
    load_golden_srs(ctx, d)
    lib = ctx.lib
    rho = make_rho(1, 700)
    _, arr, keep = S.pack_items([(fresh(),) + body])
    items_p = C.cast(arr, C.c_void_p)
    okp = np.zeros(1, dtype=np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))
    assert lib.tpst_pst_verify_batch(ctx.h, 4, items_p, 1, ptr(rho), okp) == OK
    assert lib.tpst_pst_verify_batch(ctx.h, 4, None, 0, None, None) == OK
    assert lib.tpst_pst_verify_batch(ctx.h, 4, None, 1, ptr(rho), okp) == E_ARG
    assert lib.tpst_pst_verify_batch(ctx.h, 4, items_p, 1, None, okp) == E_ARG
    for k in range(4):
        zero = rho.copy()
        zero[0, k] = 0
        assert lib.tpst_pst_verify_batch(ctx.h, 4, items_p, 1, ptr(zero), okp) == E_ARG
    assert lib.tpst_pst_verify_batch(ctx.h, 1, items_p, 1, ptr(rho), okp) == E_ARG   # bad n
    keep[0][3].m_col = 3                                                               # proof->m_col != n / 2
    assert lib.tpst_pst_verify_batch(ctx.h, 4, items_p, 1, ptr(rho), okp) == E_ARG
    keep[0][3].m_col = 2
    other = Context(0)
    try:
        assert lib.tpst_pst_verify_batch(other.h, 4, items_p, 1, ptr(rho), okp) == E_STATE
    finally:
        other.close()
