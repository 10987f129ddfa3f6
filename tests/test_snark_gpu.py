"""GPU tests of TestudoSnark / TestudoNizk (csrc/snark.hip): the end-to-end
proofs on the device, bit-exact against the first-principles restatement
tests/snark_ref.py and the fixture tests/golden/snark.json; the padded instance
of the reference's own SNARK test through Instance.new; the wire format round
trip at 2^10 x 2^10; every tamper of the restatement's list rejected with the
caller's transcript unchanged; misuse; two proofs chained on one transcript.

Shapes (num_cons x num_vars / inputs): 16 x 16 / 3 (the fixture), 64 x 16 / 5
(rx longer than ry: equalize pads ry), 32 x 32 / 0 (the other way round, no
inputs), 2 x 4 / 3 (the padded instance: one round of the first sum-check, no
witness values), 2^10 x 2^10 / 10 (self-consistency only)."""
import copy
import ctypes as C
import hashlib
import random

import numpy as np
import pytest

import hyrax_ref as H
import snark_conv as V
import snark_ref as N
from testudo_amd.encoding import fr_array, ptr

pytestmark = pytest.mark.gpu

R = N.R
SRS_SEED = N.FIXTURE_SRS_SEED
SHAPES = {"fx": (*N.FIXTURE_DIMS, N.FIXTURE_SEED), "wide": (64, 16, 5, 0x534E_0040), "tall": (32, 32, 0, 0x534E_0020)}
BIG = (1 << 10, 1 << 10, 10, 0x534E_0400)


def _srs(ctx, gens):
    from testudo_amd import sqrt_pst
    sqrt_pst.srs_setup(ctx, gens.srs_nv, SRS_SEED)


_REF, _DEV = {}, {}


def _reference(name):
    """the restatement's case of a shape, computed once"""
    if name not in _REF:
        if name == "fx":
            _REF[name] = N.fixture_case()
        elif name == "other":  # the fixture's shape, another instance, a transcript with another prefix
            _REF[name] = N.make_case(*N.FIXTURE_DIMS, N.FIXTURE_SEED + 1, SRS_SEED, prefix=[7],
                                     gens=_reference("fx")["gens"], nizk=False)
        else:
            nc, nv, ni, seed = SHAPES[name]
            _REF[name] = N.make_case(nc, nv, ni, seed, SRS_SEED, msm=H.orc_msm)
    return _REF[name]


def _device(ctx, dims_seed):
    """(instance, vars, inputs, gens, commitment, decommitment) of a synthetic shape, built once"""
    from testudo_amd.r1cs import R1CSInstance
    from testudo_amd.snark import TestudoSnarkGens, encode
    if dims_seed not in _DEV:
        nc, nv, ni, seed = dims_seed
        inst, vars_, inputs = R1CSInstance.produce_synthetic_r1cs(ctx, nc, nv, ni, seed)
        gens = TestudoSnarkGens.setup(ctx, nc, nv, ni, nc)
        comm, decomm = encode(inst, gens)
        _DEV[dims_seed] = (inst, vars_, inputs, gens, comm, decomm)
    return _DEV[dims_seed]


def _transcript(prefix=()):
    from testudo_amd.hyrax import FrTranscript
    tr = FrTranscript()
    if len(prefix):
        tr.append_scalars(fr_array(list(prefix)))
    return tr


def _rnd(case):
    return [fr_array(r) for r in case["rnd"]]


# -------------------------------------------------------------- bit-exact --
@pytest.mark.parametrize("name", ["fx", "wide", "tall"])
def test_bit_exact_vs_restatement(ctx, name):
    """every element of both proofs, inst_evals, c, and F's end state after prove and after verify"""
    from testudo_amd.snark import TestudoNizk, TestudoSnark
    ref = _reference(name)
    inst, vars_, inputs, gens, comm, decomm = _device(ctx, SHAPES[name])
    _srs(ctx, gens)
    assert V.ints(vars_) == ref["vars"] and V.ints(inputs) == ref["inputs"]
    assert V.E._pts(comm.comm.comm_ops) == ref["comm"]["comm_ops"]
    assert V.E._pts(comm.comm.comm_mem) == ref["comm"]["comm_mem"]
    tr = _transcript()
    comm.write_to_transcript(tr)
    assert V.ints(tr.challenge_scalar())[0] == ref["c"]
    # SNARK
    tr = _transcript()
    proof = TestudoSnark.prove(comm, decomm, vars_, inputs, gens, tr, _rnd(ref))
    V.assert_snark_equal(proof, ref["proof"], gens.sizes)
    assert V.ints(proof.inst_evals) == V.ints(inst.evaluate(proof.r1cs_sat_proof.rx, proof.r1cs_sat_proof.ry))
    assert V.state(tr) == ref["f_end"]
    vt = _transcript()
    assert proof.verify(gens, comm, inputs, vt) is True
    assert V.state(vt) == ref["f_end"]
    # NIZK
    nz = ref["nizk"]
    tr = _transcript()
    nproof = TestudoNizk.prove(inst, ref["digest"], vars_, inputs, tr)
    a, b = V.sat_values(nproof.r1cs_sat_proof), V.ref_sat_values(nz["proof"])
    for k in b:
        assert a[k] == b[k], ("nizk", k)
    assert V.state(tr) == nz["f_end"]
    vt = _transcript()
    assert nproof.verify(inst, ref["digest"], inputs, vt) is True
    assert V.state(vt) == nz["f_end"]


def test_fixture(ctx):
    """the committed fixture itself: the device's proofs equal it, and the library verifies the
    fixture's proofs"""
    from testudo_amd.snark import TestudoNizk, TestudoSnark
    fx = N.load_fixture()
    assert fx["dims"] == N.FIXTURE_DIMS and fx["label"] == N.LABEL == b"gens_r1cs_eval"
    inst, vars_, inputs, gens, comm, decomm = _device(ctx, SHAPES["fx"])
    _srs(ctx, gens)
    assert V.ints(vars_) == fx["vars"] and V.ints(inputs) == fx["inputs"]
    tr = _transcript()
    proof = TestudoSnark.prove(comm, decomm, vars_, inputs, gens, tr, [fr_array(r) for r in fx["rnd"]])
    V.assert_snark_equal(proof, fx["proof"], gens.sizes)
    assert V.state(tr) == fx["f_end"]
    blobs, _raw = N.load_wire_fixture()
    assert proof.to_bytes(gens) == blobs["snark_proof"]
    fcomm = V.commitment(fx["dims"], fx["comm"])
    vt = _transcript()
    assert V.snark_arrays(fx["proof"], gens.sizes).verify(gens, fcomm, fr_array(fx["inputs"]), vt) is True
    assert V.state(vt) == fx["f_end"]
    vt = _transcript()
    assert TestudoSnark.from_bytes(ctx, blobs["snark_proof"], gens).verify(gens, fcomm, inputs, vt) is True
    assert V.state(vt) == fx["f_end"]
    nz = fx["nizk"]
    tr = _transcript()
    nproof = TestudoNizk.prove(inst, nz["digest"], vars_, inputs, tr)
    assert nproof.to_bytes() == blobs["r1cs_proof"] and V.state(tr) == nz["f_end"]
    vt = _transcript()
    assert TestudoNizk(V.sat_arrays(nz["proof"])).verify(inst, nz["digest"], inputs, vt) is True
    assert V.state(vt) == nz["f_end"]
    vt = _transcript()
    assert TestudoNizk.from_bytes(ctx, blobs["r1cs_proof"], 16, 16).verify(inst, nz["digest"], inputs, vt) is True


def test_two_proofs_chained_on_one_transcript(ctx):
    from testudo_amd.snark import TestudoSnark
    ref = _reference("fx")
    _inst, vars_, inputs, gens, comm, decomm = _device(ctx, SHAPES["fx"])
    _srs(ctx, gens)
    rt = H.Transcript()
    refs = [N.snark_prove(ref["mats"], ref["dims"], ref["vars"], ref["inputs"], ref["srs"], ref["comm"], ref["dense"],
                          ref["gens"], rt, ref["rnd"])[0] for _ in range(2)]
    assert refs[0]["sat"]["rx"] != refs[1]["sat"]["rx"]
    tr, vt = _transcript(), _transcript()
    for r in refs:
        proof = TestudoSnark.prove(comm, decomm, vars_, inputs, gens, tr, _rnd(ref))
        V.assert_snark_equal(proof, r, gens.sizes)
        assert proof.verify(gens, comm, inputs, vt) is True
    assert V.state(tr) == rt.state() == V.state(vt)


# ------------------------------------------------- the padded instance ----
def test_padded_instance(ctx):
    """testudo_snark.rs:298-376 through Instance.new -> encode -> prove -> verify: 2 x 4 after padding,
    one round of the first sum-check, an n_vars = 0 witness; bit-exact against the restatement too"""
    from testudo_amd.instance import Assignment, Instance
    from testudo_amd.snark import TestudoNizk, TestudoSnark, TestudoSnarkGens, encode
    pc = N.padded_case()
    inst = Instance.new(pc["num_cons"], pc["num_vars"], pc["num_inputs"], pc["A"], pc["B"], pc["C"])
    vars_, inputs = Assignment.new(pc["vars"]), Assignment.new(pc["inputs"])
    assert (inst.num_cons, inst.num_vars) == (2, 4) and len(vars_) == 0
    assert inst.is_sat(ctx, vars_, inputs) is True
    assert inst.is_sat(ctx, vars_, Assignment([16, 1, 3])) is False
    gens = TestudoSnarkGens.setup(ctx, pc["num_cons"], pc["num_vars"], pc["num_inputs"], pc["num_nz_entries"])
    assert (gens.num_cons, gens.num_vars, gens.srs_nv) == (2, 4, 1)
    _srs(ctx, gens)
    comm, decomm = encode(inst, gens)
    # the restatement of the same instance
    dims, mats = (2, 4, 3), [inst.A, inst.B, inst.C]
    rgens = N.S.gens_setup(N.LABEL, 2, 4, pc["num_nz_entries"])
    rcomm, dense = N.S.multi_commit(mats, 2, 4, rgens)
    rnd = N.draw_rnd(rgens, random.Random(0x2A4))
    srs = N.P.SRS(1, SRS_SEED)
    rt = H.Transcript()
    rproof, _aux = N.snark_prove(mats, dims, [], inputs.assignment, srs, rcomm, dense, rgens, rt, rnd)
    assert V.E._pts(comm.comm.comm_ops) == rcomm["comm_ops"] and V.E._pts(comm.comm.comm_mem) == rcomm["comm_mem"]
    tr = _transcript()
    proof = TestudoSnark.prove(comm, decomm, vars_, inputs, gens, tr, [fr_array(r) for r in rnd])
    assert len(proof.r1cs_sat_proof.rx) == 1 and len(proof.r1cs_sat_proof.ry) == 3
    V.assert_snark_equal(proof, rproof, gens.sizes)
    assert V.state(tr) == rt.state()
    vt = _transcript()
    assert proof.verify(gens, comm, inputs, vt) is True
    assert V.state(vt) == rt.state()
    assert proof.verify(gens, comm, Assignment([16, 1, 3]), _transcript()) is False
    blob = proof.to_bytes(gens)
    assert blob == N.ser_snark_proof(rproof)
    assert TestudoSnark.from_bytes(ctx, blob, gens).verify(gens, comm, inputs, _transcript()) is True
    # NIZK over the instance's digest
    tr, vt = _transcript(), _transcript()
    nproof = TestudoNizk.prove(decomm.inst, inst.digest, vars_, inputs, tr)
    assert nproof.verify(decomm.inst, inst.digest, inputs, vt) is True
    assert V.state(tr) == V.state(vt)
    gens.close()


# ------------------------------------------------------ self-consistency ----
def test_self_consistency_and_wire_round_trip_at_2_10(ctx):
    """prove -> bytes -> from_bytes -> verify, both modes, without the Python restatement"""
    from testudo_amd.snark import TestudoNizk, TestudoSnark
    inst, vars_, inputs, gens, comm, decomm = _device(ctx, BIG)
    _srs(ctx, gens)
    sz = gens.sizes
    rng = random.Random(0x400)
    rnd = [fr_array([rng.randrange(1, R) for _ in range(sz.rnd_len[k])]) for k in range(3)]
    tr, vt = _transcript(), _transcript()
    proof = TestudoSnark.prove(comm, decomm, vars_, inputs, gens, tr, rnd)
    blob = proof.to_bytes(gens)
    back = TestudoSnark.from_bytes(ctx, blob, gens)
    assert back.to_bytes(gens) == blob
    assert V.sat_values(back.r1cs_sat_proof, wire_only=True) == V.sat_values(proof.r1cs_sat_proof, wire_only=True)
    assert not back.r1cs_sat_proof.r_abc.any() and not back.r1cs_sat_proof.claims_z_abc.any()
    assert back.verify(gens, comm, inputs, vt) is True
    assert V.state(tr) == V.state(vt)
    bad = inputs.copy()
    bad[9, 0] ^= np.uint64(1)
    assert back.verify(gens, comm, bad, _transcript()) is False
    for cut in (blob[:-1], blob + b"\0", bytes([blob[0] ^ 1]) + blob[1:]):  # the last: the first length prefix
        with pytest.raises(ValueError):
            TestudoSnark.from_bytes(ctx, cut, gens)
    digest = hashlib.shake_256(b"2^10 x 2^10").digest(256)
    tr, vt = _transcript(), _transcript()
    nproof = TestudoNizk.prove(inst, digest, vars_, inputs, tr)
    nblob = nproof.to_bytes()
    nback = TestudoNizk.from_bytes(ctx, nblob, BIG[0], BIG[1])
    assert nback.to_bytes() == nblob and nback.verify(inst, digest, inputs, vt) is True
    assert V.state(tr) == V.state(vt)
    with pytest.raises(ValueError):
        TestudoNizk.from_bytes(ctx, nblob, BIG[0], 2 * BIG[1])


# ------------------------------------------------------------- rejections --
def _tamper_ids():
    return N.SAT_TAMPERS + N.EVALS_TAMPERS + [n for n, _ in N._eval_tamper_paths(4, 5)] + N.OTHER_TAMPERS


@pytest.mark.parametrize("name", _tamper_ids())
def test_verifier_rejects_tamper(ctx, name):
    """each is TPST_E_VERIFY (False, not an exception) with the caller's transcript unchanged"""
    ref, other = _reference("fx"), _reference("other")
    assert N.tamper_names(ref) == _tamper_ids()
    _inst, _vars, _inputs, gens, _comm, _decomm = _device(ctx, SHAPES["fx"])
    _srs(ctx, gens)
    t = N.apply_tamper(name, ref, other)
    proof = V.snark_arrays(t["proof"], gens.sizes)
    comm = V.commitment(ref["dims"], t["comm"])
    tr = _transcript(t["prefix"])
    before = V.state(tr)
    assert proof.verify(gens, comm, fr_array(t["inputs"]), tr) is False
    assert V.state(tr) == before


def test_untampered_reference_proofs_verify(ctx):
    """the two proofs the tampers start from are valid, each on its own prefix"""
    _inst, _vars, _inputs, gens, _comm, _decomm = _device(ctx, SHAPES["fx"])
    _srs(ctx, gens)
    for name in ("fx", "other"):
        ref = _reference(name)
        tr = _transcript(ref["prefix"])
        assert V.snark_arrays(ref["proof"], gens.sizes).verify(gens, V.commitment(ref["dims"], ref["comm"]),
                                                               fr_array(ref["inputs"]), tr) is True
        assert V.state(tr) == ref["f_end"]


def test_nizk_rejections(ctx):
    from testudo_amd.snark import TestudoNizk
    ref = _reference("fx")
    inst, _vars, inputs, gens, _comm, _decomm = _device(ctx, SHAPES["fx"])
    _srs(ctx, gens)
    good = V.sat_arrays(ref["nizk"]["proof"])

    def rejected(proof, digest=ref["digest"], x=inputs, prefix=()):
        tr = _transcript(prefix)
        before = V.state(tr)
        ok = TestudoNizk(proof).verify(inst, digest, x, tr)
        assert ok or V.state(tr) == before
        return not ok

    assert not rejected(good)
    flipped = bytearray(ref["digest"])
    flipped[200] ^= 0x10
    assert rejected(good, digest=bytes(flipped))
    assert rejected(good, digest=ref["digest"][:-1])
    assert rejected(good, prefix=[1])
    bad_x = inputs.copy()
    bad_x[1, 0] ^= np.uint64(1)
    assert rejected(good, x=bad_x)
    assert rejected(good, x=inputs[:2])
    for edit in (lambda p: p.rx.__setitem__(0, fr_array([(V.ints(p.rx[0])[0] + 1) % R])[0]),
                 lambda p: p.ry.__setitem__(0, fr_array([V.ints(p.ry[0])[0] + R])[0]),
                 lambda p: p.comm.__setitem__(6, p.comm[6] ^ np.uint64(1)),
                 lambda p: setattr(p, "transcript_sat_state", fr_array([1])[0])):
        bad = copy.deepcopy(good)
        edit(bad)
        assert rejected(bad)
    # the SNARK's satisfiability part is no NIZK proof: its sponge forked from another absorb
    assert rejected(V.sat_arrays(ref["proof"]["sat"]))


# ------------------------------------------------------------------ misuse --
def _raises(code):
    from testudo_amd.engine import TpstError
    return pytest.raises(TpstError, match=r"\(%d\)" % code)


def test_misuse(ctx):
    """TPST_E_ARG for n_vars > num_vars, num_vars < 4, handles of another context or shape; the
    transcript is left as it was"""
    from testudo_amd import Context
    from testudo_amd.r1cs import R1CSInstance
    from testudo_amd.snark import TestudoNizk, TestudoSnark, TestudoSnarkGens, encode
    ref = _reference("fx")
    inst, vars_, inputs, gens, comm, decomm = _device(ctx, SHAPES["fx"])
    _i, _v, _x, gens_w, comm_w, decomm_w = _device(ctx, SHAPES["wide"])
    _srs(ctx, gens)
    rnd = _rnd(ref)
    tr = _transcript()
    before = V.state(tr)
    too_many = np.concatenate([vars_, vars_[:1]])
    with _raises(-1):
        TestudoSnark.prove(comm, decomm, too_many, inputs, gens, tr, rnd)
    with _raises(-1):
        TestudoNizk.prove(inst, ref["digest"], too_many, inputs, tr)
    with _raises(-1):   # a witness value >= r
        TestudoSnark.prove(comm, decomm, fr_array([R]), inputs, gens, tr, rnd)
    big = [np.ones((64, 4), dtype=np.uint64)] * 3
    with _raises(-1):   # generators of another shape
        _prove_with(ctx, inst, comm, decomm, gens_w, vars_, inputs, big, tr)
    with _raises(-1):   # a commitment of another shape
        _prove_with(ctx, inst, comm_w, decomm, gens, vars_, inputs, big, tr)
    with _raises(-1):   # a decommitment of another shape
        _prove_with(ctx, inst, comm, decomm_w, gens, vars_, inputs, big, tr)
    good = V.snark_arrays(ref["proof"], gens.sizes)
    with _raises(-1):   # verify: commitment dimensions that do not match the generators
        good.verify(gens, comm_w, inputs, tr)
    # num_vars < 4: the witness commitment needs two variables at least
    m2, nc, nv, ni = N.S.shape("a")
    small = R1CSInstance.new(ctx, nc, nv, ni, *[[(r, c, fr_array([v])[0]) for r, c, v in M] for M in m2])
    gens_s = TestudoSnarkGens.setup(ctx, nc, nv, ni, 2)
    comm_s, decomm_s = encode(small, gens_s)
    with _raises(-1):
        _prove_with(ctx, small, comm_s, decomm_s, gens_s, fr_array([1, 2]), fr_array([3]), big, tr)
    with _raises(-1):
        TestudoNizk.prove(small, b"", fr_array([1, 2]), fr_array([3]), tr)
    gens_s.close()
    other = Context(0)
    try:
        gens_o = TestudoSnarkGens.setup(other, *N.FIXTURE_DIMS, 16)
        with _raises(-1):   # generators of another context
            _prove_with(ctx, inst, comm, decomm, gens_o, vars_, inputs, big, tr)
        with _raises(-1):   # instance and decommitment of another context
            _prove_with(other, inst, comm, decomm, gens_o, vars_, inputs, big, tr)
        gens_o.close()
    finally:
        other.close()
    assert V.state(tr) == before


def _prove_with(ctx, inst, comm, decomm, gens, vars_, inputs, rnd, tr):
    """the C call with a chosen context and handles, output buffers large enough for any of them"""
    from testudo_amd import _lib
    c, _keep = comm.struct()
    pr = _lib.SnarkProof()
    out = [np.zeros((1 << 12, 12), dtype=np.uint64) for _ in range(3)]
    v, x = np.ascontiguousarray(vars_), np.ascontiguousarray(inputs)
    ctx.check(ctx.lib.tpst_snark_prove(ctx.h, inst.h, C.byref(c), decomm.decomm.h, gens.gens_r1cs_eval.h, ptr(v), len(v),
                                       ptr(x), ptr(rnd[0]), ptr(rnd[1]), ptr(rnd[2]), C.byref(tr.t), C.byref(pr),
                                       ptr(out[0]), ptr(out[1]), ptr(out[2])), "tpst_snark_prove")


def test_without_srs_is_a_state_error(ctx):
    """a fresh context has no SRS: TPST_E_STATE from both provers and both verifiers"""
    from testudo_amd import Context
    from testudo_amd.r1cs import R1CSInstance
    from testudo_amd.snark import TestudoNizk, TestudoSnark, TestudoSnarkGens, encode
    ref = _reference("fx")
    nc, nv, ni, seed = SHAPES["fx"]
    other = Context(0)
    try:
        inst, vars_, inputs = R1CSInstance.produce_synthetic_r1cs(other, nc, nv, ni, seed)
        gens = TestudoSnarkGens.setup(other, nc, nv, ni, nc)
        comm, decomm = encode(inst, gens)
        tr = _transcript()
        before = V.state(tr)
        with _raises(-4):
            TestudoSnark.prove(comm, decomm, vars_, inputs, gens, tr, _rnd(ref))
        with _raises(-4):
            TestudoNizk.prove(inst, ref["digest"], vars_, inputs, tr)
        with _raises(-4):
            V.snark_arrays(ref["proof"], gens.sizes).verify(gens, comm, inputs, tr)
        with _raises(-4):
            TestudoNizk(V.sat_arrays(ref["nizk"]["proof"])).verify(inst, ref["digest"], inputs, tr)
        assert V.state(tr) == before
        gens.close()
        del decomm, inst
    finally:
        other.close()
