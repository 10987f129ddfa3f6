"""GPU tests of the SPARK evaluation proofs (csrc/sparse_eval.hip):
R1CSEvalProof prove on the device, bit-exact against the first-principles
restatement tests/sparse_eval_ref.py and the fixture tests/golden/r1cs_eval.json;
the library's verifier on the device's proofs, the fixture's and tampered ones;
the prover's stages alone.

Shapes (num_cons x num_vars, inputs): a 2 x 2, b 8 x 4, c 32 x 4 (general
matrices, sparse_eval_ref.shape), d 2^10 x 2^10 and e 2^16 x 2^16 (synthetic)."""
import ctypes as C
import random

import numpy as np
import pytest

import hyrax_ref as H
import product_tree_ref as T
import sparse_eval_ref as S
from testudo_amd.encoding import fr_array, g1_array, g1_from_array, limbs_to_int, ptr

pytestmark = pytest.mark.gpu

R = S.R
SEG_BS = 256  # csrc/sparse_eval.hip SE_BS: lanes per block of k_seg_eval / k_hash_*
D_DIMS = (1 << 10, 1 << 10, 10, 0xD0D0)
E_DIMS = (1 << 16, 1 << 16, 10, 0xE0E0)
assert D_DIMS[0] // 4 == SEG_BS and E_DIMS[0] > SEG_BS  # d: round 0 of the ops proof is one block


def _ints(a):
    return [limbs_to_int(x) for x in np.asarray(a).reshape(-1, 4)]


def _state(tr):
    st, sq, idx = tr.state()
    return [limbs_to_int(x) for x in st], sq, idx


def _pts(a):
    a = np.asarray(a).reshape(-1, 12)
    return g1_from_array(a) if len(a) else []


# ---------------------------------------------------------- conversions ----
def _hyrax_dict(pr):
    return {"L": _pts(pr.L), "R": _pts(pr.R), "delta": _pts(pr.delta)[0], "beta": _pts(pr.beta)[0],
            "z1": limbs_to_int(pr.z1), "z2": limbs_to_int(pr.z2)}


def _hyrax_arrays(p):
    from testudo_amd.hyrax import DotProductProof
    k = len(p["L"])
    return DotProductProof(L=g1_array(p["L"]).reshape(k, 12), R=g1_array(p["R"]).reshape(k, 12),
                           delta=g1_array([p["delta"]])[0], beta=g1_array([p["beta"]])[0],
                           z1=fr_array([p["z1"]])[0], z2=fr_array([p["z2"]])[0])


def _proof_values(pr):
    """a device proof as the restatement's values (product proofs flat)"""
    e4 = lambda a: [_ints(a[0])[0], _ints(a[1:4]), _ints(a[4:7]), _ints(a[7])[0]]  # noqa: E731
    e3 = lambda a: [_ints(a[0:3]), _ints(a[3:6]), _ints(a[6])[0]]  # noqa: E731
    return {"comm_derefs": _pts(pr.comm_derefs),
            "prod": {"eval_row": e4(pr.prod_row), "eval_col": e4(pr.prod_col),
                     "eval_val": [_ints(pr.prod_val[0]), _ints(pr.prod_val[1])],
                     "proof_ops": _ints(pr.proof_ops.pack()), "proof_mem": _ints(pr.proof_mem.pack())},
            "hash": {"eval_row": e3(pr.hash_row), "eval_col": e3(pr.hash_col), "eval_val": _ints(pr.hash_val),
                     "eval_derefs": [_ints(pr.hash_derefs[0]), _ints(pr.hash_derefs[1])],
                     "proof_derefs": _hyrax_dict(pr.open_derefs), "proof_ops": _hyrax_dict(pr.open_ops),
                     "proof_mem": _hyrax_dict(pr.open_mem)}}


def _ref_values(p, log_ops, log_cells):
    """a restatement proof in the same form"""
    pd, hs = p["prod"], p["hash"]
    l = lambda e: [list(x) if isinstance(x, (list, tuple)) else x for x in e]  # noqa: E731
    return {"comm_derefs": list(p["comm_derefs"]),
            "prod": {"eval_row": l(pd["eval_row"]), "eval_col": l(pd["eval_col"]), "eval_val": l(pd["eval_val"]),
                     "proof_ops": T.flatten(pd["proof_ops"], log_ops, 12, 6),
                     "proof_mem": T.flatten(pd["proof_mem"], log_cells, 4, 0)},
            "hash": {"eval_row": l(hs["eval_row"]), "eval_col": l(hs["eval_col"]), "eval_val": list(hs["eval_val"]),
                     "eval_derefs": l(hs["eval_derefs"]), "proof_derefs": hs["proof_derefs"],
                     "proof_ops": hs["proof_ops"], "proof_mem": hs["proof_mem"]}}


def _proof_arrays(p, log_ops, log_cells):
    """a restatement proof as the library's R1CSEvalProof"""
    from testudo_amd.product_tree import ProductCircuitProof
    from testudo_amd.r1cs_eval import R1CSEvalProof
    pd, hs = p["prod"], p["hash"]
    f4 = lambda e: fr_array([e[0]] + list(e[1]) + list(e[2]) + [e[3]])  # noqa: E731
    f3 = lambda e: fr_array(list(e[0]) + list(e[1]) + [e[2]])  # noqa: E731
    return R1CSEvalProof(
        comm_derefs=g1_array(p["comm_derefs"]).reshape(-1, 12), prod_row=f4(pd["eval_row"]), prod_col=f4(pd["eval_col"]),
        prod_val=fr_array(list(pd["eval_val"][0]) + list(pd["eval_val"][1])).reshape(2, 3, 4),
        proof_ops=ProductCircuitProof.unpack(fr_array(T.flatten(pd["proof_ops"], log_ops, 12, 6)), log_ops, 12, 6),
        proof_mem=ProductCircuitProof.unpack(fr_array(T.flatten(pd["proof_mem"], log_cells, 4, 0)), log_cells, 4, 0),
        hash_row=f3(hs["eval_row"]), hash_col=f3(hs["eval_col"]), hash_val=fr_array(hs["eval_val"]),
        hash_derefs=fr_array(list(hs["eval_derefs"][0]) + list(hs["eval_derefs"][1])).reshape(2, 3, 4),
        open_derefs=_hyrax_arrays(hs["proof_derefs"]), open_ops=_hyrax_arrays(hs["proof_ops"]),
        open_mem=_hyrax_arrays(hs["proof_mem"]))


# -------------------------------------------------------------- instances --
def _mats(name):
    if name in "abc":
        mats, nc, nv, ni = S.shape(name)
        return mats, nc, nv, ni
    nc, nv, ni, seed = D_DIMS if name == "d" else E_DIMS
    return S.synthetic(nc, nv, ni, seed), nc, nv, ni


_DEV = {}


def _device(ctx, name):
    """(instance, gens, commitment, decommitment) of a shape, built once"""
    from testudo_amd.r1cs import R1CSInstance
    from testudo_amd.r1cs_eval import R1CSCommitmentGens, commit_decomm
    if name not in _DEV:
        if name in "abc":
            mats, nc, nv, ni = _mats(name)
            A, B, C_ = ([(r, c, fr_array([v])[0]) for r, c, v in M] for M in mats)
            inst = R1CSInstance.new(ctx, nc, nv, ni, A, B, C_)
            nz = max(len(M) for M in mats)
        else:
            nc, nv, ni, seed = D_DIMS if name == "d" else E_DIMS
            inst, _v, _x = R1CSInstance.produce_synthetic_r1cs(ctx, nc, nv, ni, seed)
            nz = nc
        gens = R1CSCommitmentGens.setup(ctx, S.LABEL, nc, nv, ni, nz)
        comm, decomm = commit_decomm(inst, gens)
        _DEV[name] = (inst, gens, comm, decomm)
    return _DEV[name]


def _ref_gens(ctx, name):
    """the restatement's generators: pure Python at a-c, read back from the
    device's own MultiCommitGens::new at d (pinned against Python at a-c)"""
    mats, nc, nv, _ni = _mats(name)
    nz = max(len(M) for M in mats)
    if name in "abc":
        return S.gens_setup(S.LABEL, nc, nv, nz)
    from testudo_amd.hyrax import HyraxGens
    sz = _device(ctx, name)[1].sizes
    ell = {"ops": sz.ell_ops, "mem": sz.ell_mem, "derefs": sz.ell_derefs}
    out = {"ell": ell}
    for k, v in ell.items():
        hg = HyraxGens.setup(ctx, v, S.LABEL)
        out[k] = (g1_from_array(hg.gens.G), g1_from_array(hg.gens.h)[0], g1_from_array(hg.Q)[0])
        hg.close()
    return out


_REF = {}


def _reference(ctx, name):
    """the restatement's commitment and proof of a shape, computed once"""
    if name not in _REF:
        mats, nc, nv, _ni = _mats(name)
        gens = _ref_gens(ctx, name)
        msm = H.py_msm if name in "abc" else H.orc_msm
        rng = random.Random(0x5345_1000 + ord(name))
        comm, dense = S.multi_commit(mats, nc, nv, gens, msm)
        rx, ry = S.point(nc, nv, rng)
        evals = S.multi_evaluate(mats, rx, ry)
        rnd = S.draws(gens, rng)
        tr = S.Transcript()
        proof, aux = S.prove(dense, rx, ry, evals, gens, tr, rnd, msm)
        _REF[name] = {"gens": gens, "comm": comm, "dense": dense, "rx": rx, "ry": ry, "evals": evals, "rnd": rnd,
                      "proof": proof, "aux": aux, "transcript_end": tr.state()}
    return _REF[name]


def _prove(ctx, name, v, tr=None, evals=None):
    from testudo_amd.hyrax import FrTranscript
    from testudo_amd.r1cs_eval import R1CSEvalProof
    _inst, gens, _comm, decomm = _device(ctx, name)
    tr = tr or FrTranscript()
    pr = R1CSEvalProof.prove(decomm, fr_array(v["rx"]), fr_array(v["ry"]), fr_array(v["evals"] if evals is None else evals),
                             gens, tr, [fr_array(r) for r in v["rnd"]])
    return pr, tr


# -------------------------------------------------------------- bit-exact --
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_prove_bit_exact_vs_restatement(ctx, name):
    """every proof element, comm_derefs, the commitment and the transcript's
    end state; the library's verifier accepts and ends in the same state"""
    from testudo_amd.hyrax import FrTranscript
    v = _reference(ctx, name)
    inst, gens, comm, _decomm = _device(ctx, name)
    sz = gens.sizes
    assert _pts(comm.comm_ops) == v["comm"]["comm_ops"] and _pts(comm.comm_mem) == v["comm"]["comm_mem"]
    assert (comm.num_ops, comm.num_mem_cells) == (v["comm"]["num_ops"], v["comm"]["num_mem_cells"])
    assert _ints(inst.evaluate(fr_array(v["rx"]), fr_array(v["ry"]))) == v["evals"]
    pr, tr = _prove(ctx, name, v)
    got, want = _proof_values(pr), _ref_values(v["proof"], sz.log_ops, sz.log_cells)
    for part in ("comm_derefs", "prod", "hash"):
        if part == "comm_derefs":
            assert got[part] == want[part]
            continue
        for k in want[part]:
            assert got[part][k] == want[part][k], (part, k)
    assert _state(tr) == v["transcript_end"]
    vt = FrTranscript()
    assert pr.verify(comm, fr_array(v["rx"]), fr_array(v["ry"]), fr_array(v["evals"]), gens, vt)
    assert _state(vt) == v["transcript_end"]


def test_fixture(ctx):
    """the committed fixture itself: the device's proof at (b) equals it, and the
    library verifies the fixture's proof"""
    from testudo_amd.hyrax import FrTranscript
    fx = S.load_fixture()
    assert fx["mats"] == S.shape("b")[0] and fx["label"] == S.LABEL
    _inst, gens, comm, _decomm = _device(ctx, "b")
    sz = gens.sizes
    assert _pts(comm.comm_ops) == fx["comm"]["comm_ops"] and _pts(comm.comm_mem) == fx["comm"]["comm_mem"]
    pr, tr = _prove(ctx, "b", fx)
    assert _proof_values(pr) == _ref_values(fx["proof"], sz.log_ops, sz.log_cells)
    assert _state(tr) == fx["transcript_end"]
    fp = _proof_arrays(fx["proof"], sz.log_ops, sz.log_cells)
    vt = FrTranscript()
    assert fp.verify(comm, fr_array(fx["rx"]), fr_array(fx["ry"]), fr_array(fx["evals"]), gens, vt)
    assert _state(vt) == fx["transcript_end"]


def test_two_proofs_chained_on_one_transcript(ctx):
    from testudo_amd.hyrax import FrTranscript
    v = _reference(ctx, "a")
    rt = S.Transcript()
    refs = [S.prove(v["dense"], v["rx"], v["ry"], v["evals"], v["gens"], rt, v["rnd"])[0] for _ in range(2)]
    _inst, gens, comm, _decomm = _device(ctx, "a")
    sz = gens.sizes
    tr, vt = FrTranscript(), FrTranscript()
    for ref in refs:
        pr, _ = _prove(ctx, "a", v, tr)
        assert _proof_values(pr) == _ref_values(ref, sz.log_ops, sz.log_cells)
        assert pr.verify(comm, fr_array(v["rx"]), fr_array(v["ry"]), fr_array(v["evals"]), gens, vt)
    assert _state(tr) == rt.state() == _state(vt)


# ------------------------------------------------------------ stages alone --
@pytest.mark.parametrize("name", ["b", "c"])
def test_deref_and_hash_layer(ctx, name):
    """k_deref against a NumPy gather of the device's eq tables, k_hash_ops /
    k_hash_mem against Python integers"""
    from testudo_amd.r1cs import EqPolynomial
    v = _reference(ctx, name)
    _inst, gens, _comm, decomm = _device(ctx, name)
    N, cells = gens.sizes.num_ops, gens.sizes.num_mem_cells
    rmc = v["aux"]["r_mem_check"]
    out = decomm.stages(fr_array(v["rx"]), fr_array(v["ry"]), r_mem_check=fr_array(rmc))
    rxe, rye = S.equalize(v["rx"], v["ry"])
    d = v["dense"]
    for side, pt, off in (("row", rxe, 0), ("col", rye, 3 * N)):
        eq = EqPolynomial(fr_array(pt)).evals(ctx)
        addr = np.array(sum(d[side]["addr"], []))
        assert np.array_equal(out["derefs"][off:off + 3 * N], eq[addr])
    assert not out["derefs"][6 * N:].any()
    assert _ints(out["derefs"]) == v["aux"]["comb_derefs"]
    (ri, rr, rw, ra), (ci, cr, cw, ca) = v["aux"]["layers"]
    assert _ints(out["hash_ops"]) == sum(rr + rw + cr + cw, [])
    assert _ints(out["hash_mem"]) == ri + ra + ci + ca
    assert len(ri) == cells


def _seg_check(ctx, decomm, sz, rx, ry, comb_ops, comb_mem, rng):
    from testudo_amd.hyrax import dense_evaluate
    N, cells = sz.num_ops, sz.num_mem_cells
    ro = fr_array([rng.randrange(1, R) for _ in range(sz.log_ops)])
    rm = fr_array([rng.randrange(1, R) for _ in range(sz.log_cells)])
    out = decomm.stages(rx, ry, rand_ops=ro, rand_mem=rm)
    derefs = out["derefs"]
    want = [dense_evaluate(ctx, comb_ops[k * N:(k + 1) * N], ro) for k in range(15)]
    want += [dense_evaluate(ctx, derefs[k * N:(k + 1) * N], ro) for k in range(6)]
    want += [dense_evaluate(ctx, comb_mem[k * cells:(k + 1) * cells], rm) for k in range(2)]
    assert np.array_equal(out["seg"], np.stack(want))
    return out


def test_seg_eval_small(ctx):
    """k_seg_eval against tpst_dense_evaluate per segment at (b)"""
    v = _reference(ctx, "b")
    _inst, gens, _comm, decomm = _device(ctx, "b")
    d = v["dense"]
    _seg_check(ctx, decomm, gens.sizes, fr_array(v["rx"]), fr_array(v["ry"]), fr_array(d["comb_ops"]),
               fr_array(d["comb_mem"]), random.Random(41))


def _dense_arrays_e():
    """comb_ops / comb_mem of (e) by NumPy (the synthetic instance has one entry
    per row: row addresses 0..N-1, timestamps by counting)"""
    nc, nv, ni, seed = E_DIMS
    mats = S.synthetic(nc, nv, ni, seed)
    N, cells = nc, 2 * nv
    segs, audits = [], []
    for k in (0, 1):
        addr = np.array([[e[k] for e in M] for M in mats], dtype=np.int64)
        flat = addr.reshape(-1)
        order = np.argsort(flat, kind="stable")
        sk = flat[order]
        first = np.searchsorted(sk, sk, side="left")
        rts = np.empty(3 * N, dtype=np.int64)
        rts[order] = np.arange(3 * N) - first
        audits.append(np.bincount(flat, minlength=cells))
        segs += [flat, rts]
    small = lambda a: np.concatenate([np.asarray(a, dtype=np.uint64).reshape(-1, 1),  # noqa: E731
                                      np.zeros((len(a), 3), dtype=np.uint64)], axis=1)
    vals = fr_array([e[2] for M in mats for e in M])
    comb_ops = np.concatenate([small(s) for s in segs] + [vals, np.zeros((N, 4), dtype=np.uint64)])
    return comb_ops, np.concatenate([small(a) for a in audits])


def test_seg_eval_beyond_one_block(ctx):
    """(e): more than one block per segment in k_seg_eval, k_deref and k_hash_*;
    the segments are the NumPy dense representation, so this pins the resident
    decommitment too"""
    _inst, gens, _comm, decomm = _device(ctx, "e")
    sz = gens.sizes
    assert sz.num_ops == 1 << 16 and sz.num_mem_cells == 1 << 17
    rng = random.Random(43)
    rx = fr_array([rng.randrange(1, R) for _ in range(16)])
    ry = fr_array([rng.randrange(1, R) for _ in range(17)])
    comb_ops, comb_mem = _dense_arrays_e()
    _seg_check(ctx, decomm, sz, rx, ry, comb_ops, comb_mem, rng)


@pytest.mark.parametrize("name", ["b", "d"])
def test_commit_decomm_equals_commit(ctx, name):
    inst, _gens, comm, _decomm = _device(ctx, name)
    ops, mem = inst.commit(S.LABEL)
    assert np.array_equal(ops, comm.comm_ops) and np.array_equal(mem, comm.comm_mem)


def test_self_consistency_at_e(ctx):
    """prove, then verify accepts; evals = tpst_r1cs_evaluate(rx, ry)"""
    from testudo_amd.hyrax import FrTranscript
    from testudo_amd.r1cs_eval import R1CSEvalProof
    inst, gens, comm, decomm = _device(ctx, "e")
    sz = gens.sizes
    assert (sz.ell_ops, sz.ell_derefs, sz.ell_mem) == (20, 19, 18)
    rng = random.Random(47)
    rx = fr_array([rng.randrange(1, R) for _ in range(16)])
    ry = fr_array([rng.randrange(1, R) for _ in range(17)])
    rnd = [fr_array([rng.randrange(1, R) for _ in range(sz.rnd_len[k])]) for k in range(3)]
    evals = inst.evaluate(rx, ry)
    tr, vt = FrTranscript(), FrTranscript()
    pr = R1CSEvalProof.prove(decomm, rx, ry, evals, gens, tr, rnd)
    assert pr.verify(comm, rx, ry, evals, gens, vt)
    assert _state(tr) == _state(vt)
    bad = evals.copy()
    bad[1, 0] ^= 1
    assert not pr.verify(comm, rx, ry, bad, gens, FrTranscript())


# -------------------------------------------------------------- rejections --
def _verify_b(ctx, v, proof_values, evals=None, rx=None, ry=None):
    from testudo_amd.hyrax import FrTranscript
    _inst, gens, comm, _decomm = _device(ctx, "b")
    sz = gens.sizes
    fp = proof_values if not isinstance(proof_values, dict) else _proof_arrays(proof_values, sz.log_ops, sz.log_cells)
    tr = FrTranscript()
    before = _state(tr)
    ok = fp.verify(comm, fr_array(v["rx"] if rx is None else rx), fr_array(v["ry"] if ry is None else ry),
                   fr_array(v["evals"] if evals is None else evals), gens, tr)
    if not ok:
        assert _state(tr) == before  # a rejected proof leaves the transcript untouched
    return ok


def _tampers():
    return S.tamper_list(3, 3)  # shape (b): N = cells = 8


@pytest.mark.parametrize("tname,path", _tampers(), ids=[t[0] for t in _tampers()])
def test_verifier_rejects_every_single_field_tamper(ctx, tname, path):
    v = _reference(ctx, "b")
    assert not _verify_b(ctx, v, S.tampered(v["proof"], path))


def test_verifier_rejects_wrong_inputs(ctx):
    v = _reference(ctx, "b")
    assert _verify_b(ctx, v, v["proof"])
    evals = list(v["evals"])
    evals[0] = (evals[0] + 1) % R
    assert not _verify_b(ctx, v, v["proof"], evals=evals)
    assert not _verify_b(ctx, v, v["proof"], rx=v["ry"], ry=v["rx"])  # vx = vy at (b)


def test_verifier_rejects_malformed_elements(ctx):
    """a non-canonical Fr (v + r < 2^256) and an off-curve point: TPST_E_VERIFY"""
    v = _reference(ctx, "b")
    _inst, gens, _comm, _decomm = _device(ctx, "b")
    sz = gens.sizes
    r_limbs = fr_array([0])[0].copy()
    big = v["proof"]["hash"]["eval_val"][0] + R
    assert big < 1 << 256
    for k in range(4):
        r_limbs[k] = (big >> (64 * k)) & (2 ** 64 - 1)
    fp = _proof_arrays(v["proof"], sz.log_ops, sz.log_cells)
    fp.hash_val[0] = r_limbs
    assert not _verify_b(ctx, v, fp)
    fp = _proof_arrays(v["proof"], sz.log_ops, sz.log_cells)
    fp.proof_ops.claims_left[0, 0] = r_limbs
    assert not _verify_b(ctx, v, fp)
    fp = _proof_arrays(v["proof"], sz.log_ops, sz.log_cells)
    fp.comm_derefs[0, 6] ^= np.uint64(1)  # y + 1 or y - 1: off the curve
    assert not _verify_b(ctx, v, fp)
    fp = _proof_arrays(v["proof"], sz.log_ops, sz.log_cells)
    fp.open_mem.delta[0] ^= np.uint64(1)
    assert not _verify_b(ctx, v, fp)


def test_prover_rejects_wrong_evals(ctx):
    """the prover's assertion: TPST_E_ARG with a message, the transcript untouched"""
    from testudo_amd.engine import TpstError
    from testudo_amd.hyrax import FrTranscript
    v = _reference(ctx, "b")
    for m in range(3):
        evals = list(v["evals"])
        evals[m] = (evals[m] + 1) % R
        tr = FrTranscript()
        before = _state(tr)
        with pytest.raises(TpstError, match=r"\(-1\).*evals"):
            _prove(ctx, "b", v, tr, evals=evals)
        assert _state(tr) == before


def test_misuse(ctx):
    """handles of another context or another shape: TPST_E_ARG"""
    from testudo_amd import Context
    from testudo_amd.engine import TpstError
    from testudo_amd.r1cs_eval import R1CSCommitmentGens, commit_decomm
    v = _reference(ctx, "b")
    inst, gens, comm, decomm = _device(ctx, "b")
    _i, gens_c, _c, _d = _device(ctx, "c")
    with pytest.raises(TpstError, match=r"\(-1\).*shape"):
        _prove_with(ctx, decomm, gens_c, v)
    with pytest.raises(TpstError, match=r"\(-1\).*shape"):
        commit_decomm(inst, gens_c)
    other = Context(0)
    try:
        gens_o = R1CSCommitmentGens.setup(other, S.LABEL, 8, 4, 1, 7)
        with pytest.raises(TpstError, match=r"\(-1\)"):
            _prove_with(ctx, decomm, gens_o, v)      # gens of another context
        with pytest.raises(TpstError, match=r"\(-1\)"):
            _prove_with(other, decomm, gens_o, v)    # decommitment of another context
        gens_o.close()
    finally:
        other.close()
    # commitment dimensions that do not match the generators
    pr = _proof_arrays(v["proof"], gens.sizes.log_ops, gens.sizes.log_cells)
    from testudo_amd.hyrax import FrTranscript
    from testudo_amd.r1cs_eval import R1CSCommitment
    wrong = R1CSCommitment(comm.num_ops * 2, comm.num_mem_cells, comm.comm_ops, comm.comm_mem)
    with pytest.raises(TpstError, match=r"\(-1\)"):
        pr.verify(wrong, fr_array(v["rx"]), fr_array(v["ry"]), fr_array(v["evals"]), gens, FrTranscript())


def _prove_with(ctx, decomm, gens, v):
    """the C call with a chosen context, decommitment and generators"""
    from testudo_amd import _lib
    from testudo_amd.hyrax import FrTranscript
    sz = gens.sizes
    pr = _lib.R1CSEvalProof()
    big = np.zeros((1 << 12, 4), dtype=np.uint64)
    rx, ry, ev = fr_array(v["rx"]), fr_array(v["ry"]), fr_array(v["evals"])
    rnd = [np.ones((max(sz.rnd_len[k], 64), 4), dtype=np.uint64) for k in range(3)]
    tr = FrTranscript()
    ctx.check(ctx.lib.tpst_r1cs_eval_prove(ctx.h, decomm.h, gens.h, ptr(rx), ptr(ry), ptr(ev), ptr(rnd[0]), ptr(rnd[1]),
                                           ptr(rnd[2]), C.byref(tr.t), C.byref(pr), ptr(big), ptr(big), ptr(big)),
              "tpst_r1cs_eval_prove")
