"""CPU tests of the wire-format writers of the SPARK objects
(tpst_ser_r1cs_commitment / tpst_ser_r1cs_eval_proof, host only): byte-equal to
the first-principles restatement tests/spark_wire_ref.py and to the fixture
tests/golden/r1cs_eval_wire.json on the golden proof and commitment of
tests/golden/r1cs_eval.json; the length query, a short capacity, and elements a
writer must refuse."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import sparse_eval_ref as S
import spark_wire_ref as W
from testudo_amd.encoding import g1_array

E_ARG = -1
R = S.R


@pytest.fixture(scope="module")
def golden():
    """the fixture's proof and commitment as the library's objects, with their sizes"""
    import test_r1cs_eval_gpu as E
    from testudo_amd import r1cs_eval
    fx = S.load_fixture()
    sz = r1cs_eval.sizes(fx["num_cons"], fx["num_vars"], max(len(M) for M in fx["mats"]))
    proof = E._proof_arrays(fx["proof"], sz.log_ops, sz.log_cells)
    comm = r1cs_eval.R1CSCommitment(fx["comm"]["num_ops"], fx["comm"]["num_mem_cells"],
                                    g1_array(fx["comm"]["comm_ops"]).reshape(-1, 12),
                                    g1_array(fx["comm"]["comm_mem"]).reshape(-1, 12))
    return fx, sz, proof, comm


def _u64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def _proof_call(sz, proof, out, cap):
    """tpst_ser_r1cs_eval_proof on the proof's packed buffers -> (rc, len)"""
    from testudo_amd import _lib
    pr = proof.pack()
    cd = np.ascontiguousarray(proof.comm_derefs, dtype=np.uint64)
    po, pm = proof.proof_ops.pack(), proof.proof_mem.pack()
    n = C.c_size_t(0)
    rc = _lib.load().tpst_ser_r1cs_eval_proof(C.byref(sz), C.byref(pr), _u64p(cd), _u64p(po), _u64p(pm), out, cap,
                                              C.byref(n))
    return rc, n.value


def _comm_call(fx, comm, out, cap):
    from testudo_amd import _lib
    ops = np.ascontiguousarray(comm.comm_ops, dtype=np.uint64)
    mem = np.ascontiguousarray(comm.comm_mem, dtype=np.uint64)
    n = C.c_size_t(0)
    rc = _lib.load().tpst_ser_r1cs_commitment(fx["num_cons"], fx["num_vars"], fx["num_inputs"], comm.num_ops,
                                              comm.num_mem_cells, _u64p(ops), len(ops), _u64p(mem), len(mem), out, cap,
                                              C.byref(n))
    return rc, n.value


def test_fixture_is_the_restatement():
    got, raw = W.load_fixture()
    want = dict(zip(("proof", "commitment"), W.fixture_bytes()))
    assert got == want
    for k, b in want.items():
        assert raw[k]["len"] == len(b) and raw[k]["sha256"] == hashlib.sha256(b).hexdigest()


def test_writers_byte_equal(golden):
    from testudo_amd import serialize as ser
    fx, sz, proof, comm = golden
    want, _raw = W.load_fixture()
    assert ser.ser_r1cs_eval_proof(proof, sz) == want["proof"] == W.ser_r1cs_eval_proof(fx["proof"])
    got = ser.ser_r1cs_commitment(comm, fx["num_cons"], fx["num_vars"], fx["num_inputs"])
    assert got == want["commitment"] == W.ser_r1cs_commitment(fx["num_cons"], fx["num_vars"], fx["num_inputs"],
                                                              fx["comm"])


def test_length_query_and_short_capacity(golden):
    fx, sz, proof, comm = golden
    want, _raw = W.load_fixture()
    for call, args, name in ((_proof_call, (sz, proof), "proof"), (_comm_call, (fx, comm), "commitment")):
        n = len(want[name])
        assert call(*args, None, 0) == (0, n)          # out == NULL reports the length
        buf = C.create_string_buffer(n)
        assert call(*args, buf, n) == (0, n) and buf.raw == want[name]
        short = C.create_string_buffer(n)
        rc, need = call(*args, short, n - 1)           # one byte short
        assert rc == E_ARG and need == n


def test_writers_refuse_bad_elements(golden):
    import copy
    fx, sz, proof, comm = golden
    r_limbs = np.array([(R >> (64 * k)) & (2 ** 64 - 1) for k in range(4)], dtype=np.uint64)
    # a non-canonical Fr: in the fixed part, in a product proof, in an opening
    for edit in (lambda p: p.hash_val.__setitem__(0, r_limbs),
                 lambda p: p.proof_mem.claims_right.__setitem__((0, 0), r_limbs),
                 lambda p: setattr(p.open_ops, "z2", r_limbs)):
        bad = copy.deepcopy(proof)
        edit(bad)
        assert _proof_call(sz, bad, None, 0)[0] == E_ARG
    # an off-curve point (y + 1 or y - 1), and a coordinate >= p
    bad = copy.deepcopy(proof)
    bad.comm_derefs[1, 6] ^= np.uint64(1)
    assert _proof_call(sz, bad, None, 0)[0] == E_ARG
    bad = copy.deepcopy(proof)
    bad.open_mem.L[0, 6] ^= np.uint64(1)
    assert _proof_call(sz, bad, None, 0)[0] == E_ARG
    bad = copy.deepcopy(proof)
    bad.open_derefs.beta[5] = np.uint64(2 ** 64 - 1)
    assert _proof_call(sz, bad, None, 0)[0] == E_ARG
    badc = copy.deepcopy(comm)
    badc.comm_mem[0, 6] ^= np.uint64(1)
    assert _comm_call(fx, badc, None, 0)[0] == E_ARG
    # rows that do not follow from the dimensions
    badc = copy.deepcopy(comm)
    badc.comm_ops = badc.comm_ops[:-1]
    assert _comm_call(fx, badc, None, 0)[0] == E_ARG
    assert _proof_call(sz, proof, None, 0)[0] == 0 and _comm_call(fx, comm, None, 0)[0] == 0
