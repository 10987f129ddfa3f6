"""CPU tests of the restatement tests/sparse_eval_ref.py (R1CSEvalProof prove
and verify over Python integers), of its fixture tests/golden/r1cs_eval.json,
and of the host-only part of the C entry points (the size query and the
argument checks, which need no context): no GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import hyrax_ref as H
import sparse_eval_ref as S

R = S.R
E_ARG = -1


@functools.lru_cache(maxsize=None)
def _run(name):
    mats, nc, nv, _ni = S.shape(name)
    return mats, nc, nv, S.run(mats, nc, nv, 0x5345_0000 + ord(name))


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_prove_then_verify_accepts(name):
    """S.run asserts that the verifier accepts on a fresh transcript and ends
    in the prover's transcript state"""
    mats, nc, nv, v = _run(name)
    N, vx, vy, cells = S.dims(mats, nc, nv)
    ell = v["gens"]["ell"]
    want = {"a": (2, 4, (5, 4, 3)), "b": (8, 8, (7, 6, 4)), "c": (16, 32, (8, 7, 6))}[name]
    assert (N, cells, (ell["ops"], ell["derefs"], ell["mem"])) == want
    assert (vx < vy, vx == vy, vx > vy) == {"a": (1, 0, 0), "b": (0, 1, 0), "c": (0, 0, 1)}[name]
    pd = v["proof"]["prod"]
    assert len(pd["proof_ops"]["layers"]) == N.bit_length() - 1
    assert len(pd["proof_mem"]["layers"]) == cells.bit_length() - 1


def test_shape_b_reaches_padding_reads_of_cell_zero():
    """unequal nnz, repeated rows and columns, an entry at (0, 0): the padding
    ops read cell 0, whose timestamps count them"""
    mats, nc, nv, v = _run("b")
    assert [len(M) for M in mats] == [5, 3, 7] and mats[0][0][:2] == (0, 0)
    d = v["dense"]
    for side, k in (("row", 0), ("col", 1)):
        keys = [e[k] for M in mats for e in M]
        assert len(set(keys)) < len(keys)
        pads = sum(d["N"] - len(M) for M in mats)
        assert d[side]["audit_ts"][0] == pads + keys.count(0)
        assert sum(d[side]["audit_ts"]) == 3 * d["N"]
        assert max(max(r) for r in d[side]["read_ts"]) >= pads


@pytest.mark.parametrize("which", [0, 1, 2])
def test_prover_asserts_on_wrong_evals(which):
    mats, nc, nv, v = _run("b")
    evals = list(v["evals"])
    evals[which] = (evals[which] + 1) % R
    with pytest.raises(S.ProverAssert, match=r"evals\[%d\]" % which):
        S.prove(v["dense"], v["rx"], v["ry"], evals, v["gens"], S.Transcript(), v["rnd"])


@pytest.mark.parametrize("side", ["row", "col"])
def test_prover_asserts_on_broken_memory(side):
    """a wrong read timestamp breaks init * writes = reads * audit on that side"""
    import copy
    mats, nc, nv, v = _run("b")
    dense = copy.deepcopy(v["dense"])
    dense[side]["read_ts"][1][0] += 1
    with pytest.raises(S.ProverAssert, match="subset"):
        S.prove(dense, v["rx"], v["ry"], v["evals"], v["gens"], S.Transcript(), v["rnd"])


def test_fixture_regenerates_byte_equal():
    with open(S.GOLDEN) as f:
        assert f.read() == S.dump_fixture(S.make_fixture())


def test_fixture_verifies():
    fx = S.load_fixture()
    gens = S.gens_setup(fx["label"], fx["num_cons"], fx["num_vars"], max(len(M) for M in fx["mats"]))
    tr = S.Transcript()
    assert S.verify(fx["comm"], gens, fx["rx"], fx["ry"], fx["evals"], tr, fx["proof"])
    assert tr.state() == fx["transcript_end"]
    assert fx["evals"] == S.multi_evaluate(fx["mats"], fx["rx"], fx["ry"])


def _tampers():
    return S.tamper_list(3, 3)  # shape (b): N = cells = 8


@pytest.mark.parametrize("name,path", _tampers(), ids=[t[0] for t in _tampers()])
def test_every_single_field_tamper_is_rejected(name, path):
    mats, nc, nv, v = _run("b")
    bad = S.tampered(v["proof"], path)
    assert not S.verify(v["comm"], v["gens"], v["rx"], v["ry"], v["evals"], S.Transcript(), bad)


def test_tamper_list_covers_every_field():
    pd = _run("b")[3]["proof"]["prod"]
    assert (len(pd["proof_ops"]["layers"]), len(pd["proof_mem"]["layers"])) == (3, 3)
    names = [t[0] for t in _tampers()]
    assert len(names) == len(set(names)) == 2 * (2 + 6 + 1 + 6) + 15 + 2 + 1 + 3 * 6


def test_verifier_rejects_wrong_evals_and_swapped_point():
    mats, nc, nv, v = _run("b")
    evals = list(v["evals"])
    evals[2] = (evals[2] + 1) % R
    assert not S.verify(v["comm"], v["gens"], v["rx"], v["ry"], evals, S.Transcript(), v["proof"])
    assert not S.verify(v["comm"], v["gens"], v["ry"], v["rx"], v["evals"], S.Transcript(), v["proof"])


def test_two_proofs_chain_on_one_transcript():
    mats, nc, nv, v = _run("a")
    tr = S.Transcript()
    p1, _ = S.prove(v["dense"], v["rx"], v["ry"], v["evals"], v["gens"], tr, v["rnd"])
    mid = tr.state()
    p2, _ = S.prove(v["dense"], v["rx"], v["ry"], v["evals"], v["gens"], tr, v["rnd"])
    assert mid == v["transcript_end"] and tr.state() != mid
    assert p1["hash"]["proof_mem"] != p2["hash"]["proof_mem"]
    vt = S.Transcript()
    assert S.verify(v["comm"], v["gens"], v["rx"], v["ry"], v["evals"], vt, p1)
    assert S.verify(v["comm"], v["gens"], v["rx"], v["ry"], v["evals"], vt, p2)
    assert vt.state() == tr.state()


def test_restated_pieces():
    assert S.merge([[1, 2], [3, 4], [5, 6]]) == [1, 2, 3, 4, 5, 6, 0, 0]
    assert S.bound_bot([1, 3, 10, 20], 2) == [5, 30]
    r = [5, 7, 11]
    assert S.identity_eval(r) == 4 * 5 + 2 * 7 + 11
    # the identity polynomial is the multilinear extension of i -> i
    assert S.identity_eval(r) == H.evaluate(list(range(8)), r)
    assert S.eq_eval(r, [2, 3, 4]) == H.evaluate(H.eq_evals(r), [2, 3, 4])
    assert S.equalize([1], [2, 3, 4]) == ([0, 0, 1], [2, 3, 4])
    assert S.equalize([2, 3, 4], [1]) == ([2, 3, 4], [0, 0, 1])


# ------------------------------------------------ the C entries, host side --
def _lib():
    from testudo_amd import _lib as L
    return L, L.load()


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_size_query(name):
    L, lib = _lib()
    mats, nc, nv, _ni = S.shape(name)
    sz = L.R1CSEvalSizes()
    assert lib.tpst_r1cs_eval_proof_sizes(nc, nv, max(len(M) for M in mats), C.byref(sz)) == 0
    N, _vx, _vy, cells = S.dims(mats, nc, nv)
    g = S.gens_setup(S.LABEL, nc, nv, max(len(M) for M in mats))["ell"]
    assert (sz.num_ops, sz.num_mem_cells) == (N, cells)
    assert (sz.ell_ops, sz.ell_mem, sz.ell_derefs) == (g["ops"], g["mem"], g["derefs"])
    assert (sz.log_ops, sz.log_cells) == (N.bit_length() - 1, cells.bit_length() - 1)
    assert (sz.ops_rows, sz.mem_rows, sz.derefs_rows) == tuple(1 << (g[k] // 2) for k in ("ops", "mem", "derefs"))
    import product_tree_ref as PT
    assert sz.prod_ops_len == PT.proof_len(sz.log_ops, 12, 6) and sz.prod_mem_len == PT.proof_len(sz.log_cells, 4, 0)
    assert list(sz.rnd_len) == [3 + 4 * (g[k] - g[k] // 2) for k in ("derefs", "ops", "mem")]


@pytest.mark.parametrize("dims", [(0, 4, 4), (6, 4, 4), (8, 3, 4), (8, 4, 0), (8, 4, 1)])
def test_size_query_rejects_bad_dimensions(dims):
    L, lib = _lib()
    sz = L.R1CSEvalSizes()
    assert lib.tpst_r1cs_eval_proof_sizes(*dims, C.byref(sz)) == E_ARG
    assert lib.tpst_r1cs_eval_proof_sizes(8, 4, 4, None) == E_ARG


def test_entries_reject_null_arguments_without_a_context():
    """no context, no handles: every entry answers TPST_E_ARG and touches nothing"""
    L, lib = _lib()
    z = np.zeros((64, 4), dtype=np.uint64)
    p = z.ctypes.data_as(C.POINTER(C.c_uint64))
    t, pr = L.TranscriptFr(), L.R1CSEvalProof()
    lib.tpst_transcript_fr_init(C.byref(t))
    before = bytes(t)
    h = C.c_void_p()
    n = C.c_size_t(0)
    assert lib.tpst_r1cs_gens_setup(None, b"x", 1, 8, 4, 1, 4, C.byref(h)) == E_ARG and not h.value
    assert lib.tpst_r1cs_commit_decomm(None, None, None, p, C.byref(n), p, C.byref(n), C.byref(h)) == E_ARG
    assert lib.tpst_r1cs_eval_prove(None, None, None, p, p, p, p, p, p, C.byref(t), C.byref(pr), p, p, p) == E_ARG
    assert lib.tpst_r1cs_eval_verify(None, p, p, 8, 8, None, p, p, p, C.byref(t), C.byref(pr), p, p, p) == E_ARG
    assert lib.tpst_r1cs_eval_stages(None, None, p, p, p, p, p, p, p, p, p) == E_ARG
    assert bytes(t) == before
    lib.tpst_r1cs_gens_free(None)
    lib.tpst_r1cs_decomm_free(None)
