"""GPU tests of the wire-format readers of the SPARK objects and of the
CommitterKey (csrc/serialize.hip over csrc/wire_spark.h and the batched point
codec), and of the verifiers' row-commitment checks on the device.

Round trips at the smallest shapes of tests/test_r1cs_eval_gpu.py (a 2 x 2,
b 8 x 4, c 32 x 4 general matrices; its cached instances and restatement
proofs are shared): prove, write proof and commitment, read both back, every
field equal, and the re-read proof verifies against the re-read commitment."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import bls377 as O
import serialize as OS  # oracle/py/serialize.py
import spark_wire_ref as W
import test_r1cs_eval_gpu as E
from testudo_amd.encoding import fr_array, g1_array

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, P = O.R, O.P


def _off_subgroup_g1(rng):
    while True:
        x = rng.randrange(P)
        y = OS._fq_sqrt((x * x * x + 1) % P)
        if y is not None and not O.g1_in_subgroup((x, y)):
            return (x, y)


def _non_residue_x(rng):
    while True:
        x = rng.randrange(P)
        if OS._fq_sqrt((x * x * x + 1) % P) is None:
            return x


def _written(ctx, name):
    """(reference values, device proof, its end transcript, proof bytes, commitment bytes)"""
    from testudo_amd import serialize as ser
    v = E._reference(ctx, name)
    _inst, gens, comm, _decomm = E._device(ctx, name)
    pr, tr = E._prove(ctx, name, v)
    pb = ser.ser_r1cs_eval_proof(pr, gens.sizes)
    cb = ser.ser_r1cs_commitment(comm, gens.num_cons, gens.num_vars, gens.num_inputs)
    return v, pr, tr, pb, cb


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_round_trip_and_verify(ctx, name):
    from testudo_amd import serialize as ser
    from testudo_amd.hyrax import FrTranscript
    v, pr, tr, pb, cb = _written(ctx, name)
    _inst, gens, comm, _decomm = E._device(ctx, name)
    sz = gens.sizes
    # the writers against the restatement of the layout
    assert pb == W.ser_r1cs_eval_proof(v["proof"])
    assert cb == W.ser_r1cs_commitment(gens.num_cons, gens.num_vars, gens.num_inputs, v["comm"])
    pr2 = ser.de_r1cs_eval_proof(ctx, pb, sz)
    comm2, dims = ser.de_r1cs_commitment(ctx, cb)
    assert E._proof_values(pr2) == E._proof_values(pr)
    assert [len(x.L) for x in (pr2.open_derefs, pr2.open_ops, pr2.open_mem)] == \
        [len(x.L) for x in (pr.open_derefs, pr.open_ops, pr.open_mem)]
    assert dims == (gens.num_cons, gens.num_vars, gens.num_inputs)
    assert (comm2.num_ops, comm2.num_mem_cells) == (comm.num_ops, comm.num_mem_cells)
    assert np.array_equal(comm2.comm_ops, comm.comm_ops) and np.array_equal(comm2.comm_mem, comm.comm_mem)
    assert ser.ser_r1cs_eval_proof(pr2, sz) == pb
    vt = FrTranscript()
    assert pr2.verify(comm2, fr_array(v["rx"]), fr_array(v["ry"]), fr_array(v["evals"]), gens, vt)
    assert E._state(vt) == E._state(tr) == v["transcript_end"]


def test_dimensions_only(ctx):
    from testudo_amd import _lib
    _v, _pr, _tr, _pb, cb = _written(ctx, "b")
    _inst, gens, comm, _decomm = E._device(ctx, "b")
    dims, n_ops, n_mem = (C.c_size_t * 5)(), C.c_size_t(0), C.c_size_t(0)
    lib = _lib.load()
    assert lib.tpst_de_r1cs_commitment(ctx.h, cb, len(cb), dims, None, 0, C.byref(n_ops), None, 0, C.byref(n_mem)) == 0
    assert list(dims) == [gens.num_cons, gens.num_vars, gens.num_inputs, comm.num_ops, comm.num_mem_cells]
    assert (n_ops.value, n_mem.value) == (len(comm.comm_ops), len(comm.comm_mem))
    ops = np.zeros((n_ops.value, 12), dtype=np.uint64)
    mem = np.zeros((n_mem.value, 12), dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))  # noqa: E731
    # a capacity one row short
    assert lib.tpst_de_r1cs_commitment(ctx.h, cb, len(cb), dims, p(ops), len(ops) - 1, C.byref(n_ops), p(mem), len(mem),
                                       C.byref(n_mem)) == -1


def test_negated_point_reads_but_does_not_verify(ctx):
    """the sign flag of one comm_derefs point flipped: -P is a valid point, the proof is another proof"""
    from testudo_amd import serialize as ser
    from testudo_amd.hyrax import FrTranscript
    v, pr, _tr, pb, _cb = _written(ctx, "b")
    _inst, gens, comm, _decomm = E._device(ctx, "b")
    b = bytearray(pb)
    b[8 + 48 * 2 + 47] ^= 0x80
    pr2 = ser.de_r1cs_eval_proof(ctx, bytes(b), gens.sizes)
    assert np.array_equal(pr2.comm_derefs[2, :6], pr.comm_derefs[2, :6])
    assert not np.array_equal(pr2.comm_derefs[2, 6:], pr.comm_derefs[2, 6:])
    assert np.array_equal(np.delete(pr2.comm_derefs, 2, 0), np.delete(pr.comm_derefs, 2, 0))
    assert not pr2.verify(comm, fr_array(v["rx"]), fr_array(v["ry"]), fr_array(v["evals"]), gens, FrTranscript())


def test_reader_rejections(ctx):
    from testudo_amd import serialize as ser
    _v, _pr, _tr, pb, cb = _written(ctx, "b")
    _inst, gens, _comm, _decomm = E._device(ctx, "b")
    sz = gens.sizes
    rng = random.Random(0x57A7)
    first_fr = 8 + 48 * sz.derefs_rows                       # prod eval_row's init claim

    def edit(b, off, new):
        b = bytearray(b)
        b[off:off + len(new)] = new
        return bytes(b)

    bad_proofs = {
        "non-residue x": edit(pb, 8 + 48, _non_residue_x(rng).to_bytes(48, "little")),
        "off-subgroup point": edit(pb, 8, OS.ser_g1(_off_subgroup_g1(rng))),
        "point in an opening": edit(pb, len(pb) - 64 - 48, _non_residue_x(rng).to_bytes(48, "little")),
        "Vec length + 1": edit(pb, 0, (sz.derefs_rows + 1).to_bytes(8, "little")),
        "Vec length - 1": edit(pb, first_fr + 32, (2).to_bytes(8, "little")),
        "Vec length 2^63 + 1": edit(pb, first_fr + 32, ((1 << 63) + 1).to_bytes(8, "little")),
        "trailing byte": pb + b"\0",
        "truncation": pb[:-1],
        "half": pb[:len(pb) // 2],
        "empty": b"",
        "Fr = r": edit(pb, first_fr, R.to_bytes(32, "little")),
        "last Fr = r": edit(pb, len(pb) - 32, R.to_bytes(32, "little")),
    }
    for name, b in bad_proofs.items():
        with pytest.raises(ser.SerializationError):
            ser.de_r1cs_eval_proof(ctx, b, sz)
            pytest.fail("accepted: " + name)
    ops_at = 6 * 8 + 8
    bad_comms = {
        "non-residue x": edit(cb, ops_at, _non_residue_x(rng).to_bytes(48, "little")),
        "off-subgroup point": edit(cb, len(cb) - 48, OS.ser_g1(_off_subgroup_g1(rng))),
        "batch_size 4": edit(cb, 24, (4).to_bytes(8, "little")),
        "Vec length + 1": edit(cb, 48, (sz.ops_rows + 1).to_bytes(8, "little")),
        "num_ops doubled": edit(cb, 32, (2 * sz.num_ops).to_bytes(8, "little")),
        "trailing byte": cb + b"\0",
        "truncation": cb[:-1],
    }
    for name, b in bad_comms.items():
        with pytest.raises(ser.SerializationError):
            ser.de_r1cs_commitment(ctx, b)
            pytest.fail("accepted: " + name)
    ser.de_r1cs_eval_proof(ctx, pb, sz)
    ser.de_r1cs_commitment(ctx, cb)


@pytest.mark.parametrize("nv", [4, 5])
def test_committer_key_round_trip(nv):
    """tpst_srs_setup -> export -> tpst_ser_committer_key -> tpst_de_committer_key gives the flat array
    back limb for limb (the masks rebuilt from the powers), and tpst_srs_load takes it"""
    from testudo_amd import Context
    from testudo_amd import serialize as ser
    own = Context(0)  # the session's context keeps its SRS
    try:
        lib = own.lib
        own.check(lib.tpst_srs_setup(own.h, nv, 0xC0FFEE + nv), "tpst_srs_setup")
        flat = np.zeros(lib.tpst_srs_flat_len(nv), dtype=np.uint64)
        p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))  # noqa: E731
        own.check(lib.tpst_srs_export(own.h, p(flat)), "tpst_srs_export")
        kb = ser.ser_committer_key(nv, flat)
        nv2, flat2 = ser.de_committer_key(own, kb)
        assert nv2 == nv and np.array_equal(flat2, flat)
        own.check(lib.tpst_srs_load(own.h, nv2, p(flat2)), "tpst_srs_load")
        again = np.zeros_like(flat)
        own.check(lib.tpst_srs_export(own.h, p(again)), "tpst_srs_export")
        assert np.array_equal(again, flat)
        # one G2 point replaced by a twist point outside the subgroup
        g2_at = 8 + 8 + sum(8 + 48 * (1 << (nv - i)) for i in range(nv)) + 8 + 8
        rng = random.Random(nv)
        while True:
            x = (rng.randrange(P), rng.randrange(P))
            r = O.f2_mul(O.f2_sqr(x), x)
            y = OS._fq2_sqrt(((r[0] + O.G2_B[0]) % P, (r[1] + O.G2_B[1]) % P))
            if y is not None and O.g2_on_curve((x, y)) and not O.g2_in_subgroup((x, y)):
                break
        assert kb[g2_at - 8:g2_at] == (1 << nv).to_bytes(8, "little")
        bad = kb[:g2_at + 96] + OS.ser_g2((x, y)) + kb[g2_at + 192:]
        with pytest.raises(ser.SerializationError):
            ser.de_committer_key(own, bad)
        for b in (kb + b"\0", kb[:-1], (nv + 1).to_bytes(8, "little") + kb[8:]):
            with pytest.raises(ser.SerializationError):
                ser.de_committer_key(own, b)
    finally:
        own.close()


# ---------------------------------------------- the verifiers' device check --
def _threshold():
    src = open(os.path.join(ROOT, "testudo_amd", "csrc", "point_codec.h")).read()
    return int(re.search(r"POINT_CHECK_DEVICE_MIN = (\d+);", src).group(1))


def test_verifier_checks_rows_on_the_device(ctx):
    """The shape follows from T = POINT_CHECK_DEVICE_MIN (csrc/point_codec.h): comm_ops has
    2^((log2 N + 4) / 2) rows, so the smallest synthetic instance (N = num_cons entries per matrix)
    with ops_rows >= T is taken.  One verify of a valid proof and one with a row of comm_ops
    replaced by a point outside the subgroup; the point_codec stage shows that the device check ran."""
    from testudo_amd.hyrax import FrTranscript
    from testudo_amd.r1cs import R1CSInstance
    from testudo_amd.r1cs_eval import R1CSCommitment, R1CSCommitmentGens, R1CSEvalProof, commit_decomm
    T = _threshold()
    log_n = 1
    while 1 << ((log_n + 4) // 2) < T:
        log_n += 1
    n = 1 << log_n
    own = (n, n) != E.E_DIMS[:2]  # shape (e) of tests/test_r1cs_eval_gpu.py is this shape at T = 1024: built once
    if own:
        inst, _vars, _inputs = R1CSInstance.produce_synthetic_r1cs(ctx, n, n, 1, 0x7E57)
        gens = R1CSCommitmentGens.setup(ctx, b"point_codec", n, n, 1, n)
        comm, decomm = commit_decomm(inst, gens)
    else:
        inst, gens, comm, decomm = E._device(ctx, "e")
    sz = gens.sizes
    assert sz.ops_rows >= T and (log_n == 1 or 1 << ((log_n + 3) // 2) < T)
    rng = random.Random(0xD15C)
    rx = fr_array([rng.randrange(1, R) for _ in range(log_n)])
    ry = fr_array([rng.randrange(1, R) for _ in range(log_n + 1)])
    rnd = [fr_array([rng.randrange(1, R) for _ in range(sz.rnd_len[k])]) for k in range(3)]
    evals = inst.evaluate(rx, ry)
    pr = R1CSEvalProof.prove(decomm, rx, ry, evals, gens, FrTranscript(), rnd)
    ctx.profile(True)
    try:
        ctx.profile_reset()
        assert pr.verify(comm, rx, ry, evals, gens, FrTranscript())
        _ms, launches = ctx.profile_read()["point_codec"]
        assert launches >= 1                      # comm_ops at least went through k_point_check
        ops = comm.comm_ops.copy()
        ops[sz.ops_rows - 1] = g1_array([_off_subgroup_g1(rng)])[0]
        ctx.profile_reset()
        tr = FrTranscript()
        before = E._state(tr)
        assert not pr.verify(R1CSCommitment(comm.num_ops, comm.num_mem_cells, ops, comm.comm_mem), rx, ry, evals, gens, tr)
        assert E._state(tr) == before
        assert ctx.profile_read()["point_codec"][1] >= 1
    finally:
        ctx.profile(False)
        if own:
            decomm.close()
            gens.close()
