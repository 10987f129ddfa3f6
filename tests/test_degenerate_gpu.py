"""Degenerate polynomials and points through the device's sqrt-PST commit /
open / verify (tests/degenerate_vectors.py): zero and constant polynomials,
zero rows (padding), boolean and extreme points.  Their proofs are full of the
point at infinity and of GT's one, which the random-input tests never produce:
infinity entries of comm_list under the fold and rebase tables, look-ahead
partials equal to one, infinity through xyzz_to_affine, the transcript and the
verifier's point checks.  Every comparison is bit-exact against the C++ oracle
(oracle/cpu), whose agreement with the Python oracle on these inputs and whose
class properties tests/test_degenerate_ref.py checks without a device.

Sizes by the device paths they reach: n = 6, 7 (even / odd, C = 8), n = 10, 11
(the look-ahead rounds), n = 16, 17 (the a-side rebase in round 4, over folded
points many of which are infinity).
"""
import numpy as np
import pytest

import bls377 as O
import degenerate_vectors as V
import orc
import pst as P
import r1cs as Q
from testudo_amd.encoding import fr_array, g1_array, g1_from_array, g2_array, g2_from_array, limbs_to_int

pytestmark = pytest.mark.gpu

FIELDS = ("U", "pst_proof", "comms_u", "comms_t", "final_a", "final_h", "pst_proof_h")


def _setup(ctx, n):
    from testudo_amd import sqrt_pst as S
    S.srs_setup(ctx, (n + 1) // 2, V.SEED_SRS)
    return S


def _mipp(S, pr, **repl):
    f = {k: pr[k] for k in ("comms_t", "comms_u", "final_a", "final_h", "pst_proof_h")}
    f.update(repl)
    return S.MippProof(**f)


def _commit_open(ctx, S, Z, pt, comm_list=None):
    """device eval, commit and opening of Z at pt -> (v, comms, T, proof dict)"""
    pl = S.Polynomial.from_evaluations(ctx, Z)
    v = pl.eval(pt)
    comms, T = pl.commit()
    U, pst_proof, mipp = pl.open(S.PoseidonTranscript(), comms if comm_list is None else comm_list, pt, T)
    return v, comms, T, V.proof_fields(U, pst_proof, mipp)


def _differs(got, want):
    """the elements (rows of the flattened array) at which got != want"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype
    w = got.shape[-1]
    return [int(i) for i in np.nonzero((got.reshape(-1, w) != want.reshape(-1, w)).any(axis=1))[0]]


def _proof_diff(pr, want):
    return {f: _differs(pr[f], want[f]) for f in FIELDS if not np.array_equal(pr[f], want[f])}


def _assert_matches(got, ref, tag):
    v, comms, T, pr = got
    assert np.array_equal(v, ref["v"]), tag + ("eval",)
    assert np.array_equal(comms, ref["comms"]), tag + ("comms", _differs(comms, ref["comms"]))
    assert np.array_equal(T, ref["T"]), tag + ("T",)
    bad = _proof_diff(pr, ref["pr"])  # every field at once: the first wrong element names the stage
    assert not bad, tag + (bad,)


# ------------------------------------------ a. commit / eval / open / verify --
@pytest.mark.parametrize("case,n", V.GRID)
def test_degenerate_commit_open_verify(ctx, case, n):
    ref = V.reference(case, n)
    V.check_class(case, n, ref["Z"], ref["v"], ref["comms"], ref["T"], ref["pr"])  # the reference first
    S = _setup(ctx, n)
    got = _commit_open(ctx, S, ref["Z"], ref["pt"])
    v, comms, T, pr = got
    try:
        _assert_matches(got, ref, (case, n))
    except AssertionError as e:
        # say which side moved: the oracle recomputed, and its verdict on the device's proof
        srs = V.oracle_srs((n + 1) // 2)
        again = orc.pst_open(srs, ref["Z"], n, ref["pt"], ref["comms"])
        raise AssertionError("%s; the oracle recomputed differs from itself at %s; the oracle %s the device's proof"
                             % (e, _proof_diff(again, ref["pr"]) or "nothing",
                                "accepts" if orc.pst_verify(srs, n, ref["pt"], v, pr, T) else "rejects")) from None
    V.check_class(case, n, ref["Z"], v, comms, T, pr)
    assert S.verify(ctx, S.PoseidonTranscript(), pr["U"], ref["pt"], v, pr["pst_proof"], _mipp(S, pr), T)


# ------------------------- b. verifier completeness and soundness at n = 6 --
def _verify(ctx, S, ref, v=None, T=None, pst_proof=None, U=None, **repl):
    pr = ref["pr"]
    return S.verify(ctx, S.PoseidonTranscript(), pr["U"] if U is None else U, ref["pt"],
                    ref["v"] if v is None else v, pr["pst_proof"] if pst_proof is None else pst_proof,
                    _mipp(S, pr, **repl), ref["T"] if T is None else T)


@pytest.mark.parametrize("case", V.CASES)
def test_device_verifier_accepts_oracle_proof(ctx, case):
    S = _setup(ctx, 6)
    ref = V.reference(case, 6)
    assert _verify(ctx, S, ref), ctx.lib.tpst_last_error(ctx.h)
    assert not _verify(ctx, S, ref, v=V.fr(V.fr_int(ref["v"]) + 1))


def test_device_verifier_rejects_tampered_degenerate_proofs(ctx):
    S = _setup(ctx, 6)
    zero, const, two = (V.reference(c, 6) for c in ("zero", "const", "two_rows"))
    g1 = orc.g1_mul_gen(fr_array([1]))[0]
    g2 = orc.g2_mul_gen(fr_array([1]))[0]
    assert g1_from_array(g1)[0] == O.G1_GEN and g2_from_array(g2)[0] == O.G2_GEN
    assert _verify(ctx, S, zero) and _verify(ctx, S, const)
    # the zero polynomial: every element is infinity / one, each is still bound
    assert not _verify(ctx, S, zero, v=V.fr(1))
    assert not V.is_one(two["T"])[0]
    assert not _verify(ctx, S, zero, T=two["T"])  # a non-trivial GT element
    assert not _verify(ctx, S, zero, final_a=g1)
    cu = zero["pr"]["comms_u"].copy()
    assert not cu[1, 0].any()
    cu[1, 0] = g1
    assert not _verify(ctx, S, zero, comms_u=cu)
    assert not _verify(ctx, S, zero, U=g1)
    # the constant polynomial: pst_proof is all infinity
    pst = const["pr"]["pst_proof"].copy()
    assert not pst.any()
    pst[1] = g2
    assert not _verify(ctx, S, const, pst_proof=pst)
    # x = 0 is not infinity: (0, 2) is off the curve, (0, 1) on it but of order 3
    for y in (2, 1):
        cu = zero["pr"]["comms_u"].copy()
        cu[0, 1] = g1_array([(0, y)])[0]
        assert not _verify(ctx, S, zero, comms_u=cu), y
        pst = const["pr"]["pst_proof"].copy()
        pst[0] = g2_array([((0, 0), (y, 0))])[0]
        assert not _verify(ctx, S, const, pst_proof=pst), y


# ------------------------------------------ c. the content-keyed table cache --
def test_fold_table_cache_across_degenerate_openings(ctx):
    """The commit prebuilds the fold table over its comm_list and keys it by
    content (t_A_key); the next opening uses it when the caller's comm_list has
    the same bytes and rebuilds it otherwise (pst_open.hip, table_and_U).  One
    context, one SRS: two_rows, zero, two_rows again -- tables over mostly
    infinity, all infinity, then the first again -- each equal to the oracle.
    Then a comm_list the cache has not seen: commit `const`, open with the
    comm_list of `const_max`.  The key does not match, so the table is rebuilt
    from the caller's list: the opening is the oracle's for that list (U from
    the given commitments, q from the handle).  The key is consumed by that
    opening, so opening `const` with its own list afterwards rebuilds again."""
    n = 10
    S = _setup(ctx, n)
    outs = []
    for case in ("two_rows", "zero", "two_rows"):
        ref = V.reference(case, n)
        got = _commit_open(ctx, S, ref["Z"], ref["pt"])
        _assert_matches(got, ref, (case, n, len(outs)))
        outs.append(got)
    for f in FIELDS:
        assert np.array_equal(outs[0][3][f], outs[2][3][f]), f
    const, cmax = V.reference("const", n), V.reference("const_max", n)
    assert np.array_equal(const["pt"], cmax["pt"]) and not np.array_equal(const["comms"], cmax["comms"])
    want = orc.pst_open(V.oracle_srs((n + 1) // 2), const["Z"], n, const["pt"], cmax["comms"])
    pl = S.Polynomial.from_evaluations(ctx, const["Z"])
    comms, T = pl.commit()
    assert np.array_equal(comms, const["comms"])
    for comm_list, exp in ((cmax["comms"], want), (const["comms"], const["pr"]), (cmax["comms"], want)):
        U, pst_proof, mipp = pl.open(S.PoseidonTranscript(), comm_list, const["pt"], T)
        pr = V.proof_fields(U, pst_proof, mipp)
        for f in FIELDS:
            assert np.array_equal(pr[f], exp[f]), f
    assert np.array_equal(want["U"], cmax["pr"]["U"])  # U follows the list, pst_proof the handle's q
    assert np.array_equal(want["pst_proof"], const["pr"]["pst_proof"])


# ---------------------------------------------------------- d. sharded pieces --
def test_sharded_pieces_of_zero_shards(ctx):
    """(n, world) = (11, 4) with two_rows: ranks 1-3 hold only zeros"""
    import torch
    n, world = 11, 4
    S = _setup(ctx, n)
    ref = V.reference("two_rows", n)
    Z, pt = ref["Z"], ref["pt"]
    m_col, m_row, C = V.dims(n)
    N, R = 1 << m_row, C // world
    flat = S.srs_export(ctx, (n + 1) // 2)
    off = 36 + N * 12 + N * 24 + (N // 2) * 12  # powers_of_h[1] (n odd)
    hvec = flat[off:off + C * 24].reshape(C, 24)
    full = S.Polynomial.from_evaluations(ctx, Z)
    comms, T = full.commit()
    v = full.eval(pt)
    assert np.array_equal(comms, ref["comms"]) and np.array_equal(T, ref["T"]) and np.array_equal(v, ref["v"])
    U, pst_proof, mipp = full.open(S.PoseidonTranscript(), comms, pt, T)
    dev = torch.device("cuda", 0)
    zq_parts = torch.empty((world, N * 4), dtype=torch.int64, device=dev)
    cm_parts = torch.empty((world, R * 12 + 72), dtype=torch.int64, device=dev)
    cu = []
    for g in range(world):
        sl = S.Polynomial.from_evaluations_cols(ctx, Z, g * R, (g + 1) * R)
        c, ml = sl.commit_rows_partial(g * R, (g + 1) * R)
        zq = sl.get_q_partial(pt, g * R, (g + 1) * R)
        sl.get_q_partial_into(pt, g * R, (g + 1) * R, zq_parts[g])
        sl.commit_rows_partial_into(g * R, (g + 1) * R, cm_parts[g])
        got = cm_parts[g].cpu().numpy().view(np.uint64)
        assert np.array_equal(got[:12 * R].reshape(R, 12), c) and np.array_equal(got[12 * R:], ml)
        assert np.array_equal(zq_parts[g].cpu().numpy().view(np.uint64).reshape(-1, 4), zq)
        assert np.array_equal(c, comms[g * R:(g + 1) * R])
        assert np.array_equal(ml, orc.miller_product(c, hvec[g * R:(g + 1) * R])), g
        cu.append(S.cu_partial(ctx, n, pt, g * R, (g + 1) * R, c))
        if g:  # a shard of zeros
            assert not c.any() and not zq.any() and not cu[g].any(), g
        else:
            assert c[:2].any(axis=1).all() and not c[2:].any() and zq.any() and cu[g].any()
    ml = cm_parts.cpu().numpy().view(np.uint64)[:, 12 * R:]
    assert np.array_equal(S.gt_final_exp_product(ctx, ml), T)
    assert np.array_equal(S.gt_final_exp_product_gathered(ctx, cm_parts, R), T)
    Uc = S.g1_sum(ctx, np.stack(cu))
    assert np.array_equal(Uc, ref["pr"]["U"])
    zq = S.fr_sum(ctx, zq_parts)
    for Ugiven in (Uc, None):
        pq = S.Polynomial.from_q(ctx, n, pt, zq, Ugiven)
        assert np.array_equal(pq.eval(pt), v)
        U2, pst2, mipp2 = pq.open(S.PoseidonTranscript(), comms, pt, T)
        pr2 = V.proof_fields(U2, pst2, mipp2)
        for f in FIELDS:
            assert np.array_equal(pr2[f], ref["pr"][f]), f
    for f, a in V.proof_fields(U, pst_proof, mipp).items():
        assert np.array_equal(a, ref["pr"][f]), f
    assert S.verify(ctx, S.PoseidonTranscript(), U, pt, v, pst_proof, mipp, T)


# ------------------------------------------- e. MultilinearPC single calls --
@pytest.mark.parametrize("value", [7, 0, O.R - 1], ids=["7", "0", "r-1"])
def test_multilinear_pc_constant_polynomial(ctx, value):
    """open / open_g1 of a constant polynomial: every quotient is zero, every
    level proof infinity; check / check_2 then compare e(C - g^v, h) = 1 with an
    empty product, and still bind the value"""
    from testudo_amd import sqrt_pst as S
    ck = 4
    S.srs_setup(ctx, ck, V.SEED_SRS)
    srs = _py_srs(ck)
    for nv in (4, 3):
        ev = np.tile(V.fr(value), (1 << nv, 1))
        pt, _ = orc.fr_stream(940 + nv, nv)
        pti = [limbs_to_int(x) for x in pt]
        c = S.MultilinearPC.commit(ctx, ev)
        ch = S.MultilinearPC.commit_g2(ctx, ev)
        assert g1_from_array(c)[0] == P.pst_commit(srs, [value] * (1 << nv))
        assert g2_from_array(ch)[0] == P.pst_commit_g2(srs, [value] * (1 << nv))
        assert (not c.any()) == (value == 0)
        pr = S.MultilinearPC.open(ctx, ev, pt)
        pr1 = S.MultilinearPC.open_g1(ctx, ev, pt)
        assert P.pst_open(srs, [value] * (1 << nv), pti) == [None] * nv == g2_from_array(pr)
        assert P.pst_open_g1(srs, [value] * (1 << nv), pti) == [None] * nv == g1_from_array(pr1)
        assert pr.shape == (nv, 24) and pr1.shape == (nv, 12) and not pr.any() and not pr1.any()
        v = V.fr(value)
        assert S.MultilinearPC.check(ctx, c, pt, v, pr), ctx.lib.tpst_last_error(ctx.h)
        assert S.MultilinearPC.check_2(ctx, ch, pt, v, pr1), ctx.lib.tpst_last_error(ctx.h)
        bad = V.fr(value + 1)
        assert not S.MultilinearPC.check(ctx, c, pt, bad, pr)
        assert not S.MultilinearPC.check_2(ctx, ch, pt, bad, pr1)


_PY_SRS = {}


def _py_srs(nv):
    if nv not in _PY_SRS:
        _PY_SRS[nv] = P.SRS(nv, V.SEED_SRS)
    return _PY_SRS[nv]


# ---------------------------------- f. R1CS prove over a degenerate witness --
@pytest.mark.parametrize("witness", ["zero", "upper_half_zero"])
def test_r1cs_prove_degenerate_witness(ctx, witness):
    """R1CSProof::prove takes the caller's vars and does not require
    satisfaction: the all-zero witness (T = 1, U and the whole opening at
    infinity) and the synthetic witness with its upper half zeroed, against
    oracle/py/r1cs.py element by element"""
    from test_r1cs import _compare
    from testudo_amd import r1cs as D
    from testudo_amd import sqrt_pst as S
    num_cons, num_vars, num_inputs, seed = 16, 16, 3, 1016
    S.srs_setup(ctx, 2, V.SEED_SRS)
    inst, vars_, inputs = D.R1CSInstance.produce_synthetic_r1cs(ctx, num_cons, num_vars, num_inputs, seed)
    mats, v, x = Q.synthetic_r1cs(num_cons, num_vars, num_inputs, seed)
    assert [limbs_to_int(a) for a in vars_] == v and [limbs_to_int(a) for a in inputs] == x
    assert inst.is_sat(vars_, inputs)
    if witness == "zero":
        w = [0] * num_vars
    else:
        w = v[:num_vars // 2] + [0] * (num_vars // 2)
    Az, Bz, Cz = (Q.multiply_vec(M, num_cons, w + [1] + x) for M in mats)
    assert any((a * b - c) % O.R for a, b, c in zip(Az, Bz, Cz))  # the oracle's is_sat is False
    assert not inst.is_sat(fr_array(w), inputs)
    proof, _, _ = D.R1CSProof.prove(inst, fr_array(w), inputs, S.PoseidonTranscript())
    out = Q.r1cs_prove(mats, num_cons, num_vars, w, x, _py_srs(2), P.PoseidonTranscript())
    if witness == "zero":
        assert out["U"] is None and out["mipp"]["final_a"] is None and out["T"] == O.f12_one()
        assert not proof.comm.any() and np.array_equal(np.asarray(proof.T).reshape(72), V.GT_ONE)
    else:
        assert out["U"] is not None
    _compare(proof, out)
