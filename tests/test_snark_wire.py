"""CPU tests of the wire-format writers of R1CSProof and the SNARK proof
(tpst_ser_r1cs_proof / tpst_ser_snark_proof, host only): byte-equal to the
restatement tests/snark_ref.py and to tests/golden/snark_wire.json on the proofs
of tests/golden/snark.json; the length query, a short capacity, elements and
dimensions a writer must refuse; the host-only transcript calls
(tpst_transcript_fr_append_u64 / _new_from_state, tpst_r1cs_commitment_absorb)
against the restatement."""
import copy
import ctypes as C

import numpy as np
import pytest

import snark_conv as V
import snark_ref as N
from testudo_amd.encoding import fr_array

E_ARG = -1
R = N.R


@pytest.fixture(scope="module")
def golden():
    from testudo_amd import r1cs_eval
    fx = N.load_fixture()
    nc, nv, _ni = fx["dims"]
    sz = r1cs_eval.sizes(nc, nv, nc)
    return fx, sz, V.snark_arrays(fx["proof"], sz), V.sat_arrays(fx["nizk"]["proof"])


def _snark_call(sz, proof, out, cap):
    from testudo_amd import _lib
    from testudo_amd.encoding import ptr
    pr, cd, po, pm = proof.pack()
    n = C.c_size_t(0)
    rc = _lib.load().tpst_ser_snark_proof(C.byref(sz), C.byref(pr), ptr(cd), ptr(po), ptr(pm), out, cap, C.byref(n))
    return rc, n.value


def _sat_call(sat, out, cap, edit=None):
    from testudo_amd import _lib
    pr = sat.pack()
    if edit:
        edit(pr)
    n = C.c_size_t(0)
    rc = _lib.load().tpst_ser_r1cs_proof(C.byref(pr), out, cap, C.byref(n))
    return rc, n.value


def test_writers_byte_equal(golden):
    from testudo_amd import snark
    fx, sz, proof, sat = golden
    want, _raw = N.load_wire_fixture()

    class G:  # what to_bytes reads of the generators
        sizes = sz

    assert proof.to_bytes(G) == want["snark_proof"] == N.ser_snark_proof(fx["proof"])
    assert snark.ser_r1cs_proof(sat) == want["r1cs_proof"] == N.ser_r1cs_proof(fx["nizk"]["proof"])
    # the SNARK layout starts with the R1CSProof of its own satisfiability part
    own = snark.ser_r1cs_proof(proof.r1cs_sat_proof)
    assert want["snark_proof"].startswith(own) and own == N.ser_r1cs_proof(fx["proof"]["sat"])


def test_r_abc_and_phase_two_finals_are_not_written(golden):
    from testudo_amd import snark
    _fx, _sz, _proof, sat = golden
    blind = copy.deepcopy(sat)
    blind.r_abc[:] = 0
    blind.claims_z_abc[:] = 0
    assert snark.ser_r1cs_proof(blind) == snark.ser_r1cs_proof(sat)


def test_length_query_and_short_capacity(golden):
    _fx, sz, proof, sat = golden
    want, _raw = N.load_wire_fixture()
    for call, args, name in ((_snark_call, (sz, proof), "snark_proof"), (_sat_call, (sat,), "r1cs_proof")):
        n = len(want[name])
        assert call(*args, None, 0) == (0, n)          # out == NULL reports the length
        buf = C.create_string_buffer(n)
        assert call(*args, buf, n) == (0, n) and buf.raw == want[name]
        short = C.create_string_buffer(n)
        rc, need = call(*args, short, n - 1)           # one byte short
        assert rc == E_ARG and need == n


def test_writers_refuse_bad_elements_and_dimensions(golden):
    _fx, sz, proof, sat = golden
    r_limbs = fr_array([R])[0]
    for edit in (lambda p: p.rx.__setitem__(1, r_limbs), lambda p: p.sc_proof_phase2.__setitem__((2, 1), r_limbs),
                 lambda p: setattr(p, "initial_state", r_limbs)):
        bad = copy.deepcopy(sat)
        edit(bad)
        assert _sat_call(bad, None, 0)[0] == E_ARG
    bad = copy.deepcopy(sat)
    bad.comm[6] ^= np.uint64(1)                          # U off the curve
    assert _sat_call(bad, None, 0)[0] == E_ARG
    bad = copy.deepcopy(sat)
    bad.T[5] = np.uint64(2 ** 64 - 1)                    # an Fq12 coefficient >= p
    assert _sat_call(bad, None, 0)[0] == E_ARG
    bad = copy.deepcopy(sat)
    bad.mipp_proof.final_h[5] = np.uint64(2 ** 64 - 1)   # a G2 coordinate >= p
    assert _sat_call(bad, None, 0)[0] == E_ARG
    for field, v in (("rounds_x", 0), ("rounds_x", 49), ("rounds_y", 49), ("num_vars_log", 3)):
        assert _sat_call(sat, None, 0, edit=lambda pr: setattr(pr, field, v))[0] == E_ARG  # noqa: B023
    assert _sat_call(sat, None, 0, edit=lambda pr: setattr(pr.open, "m_col", 21))[0] == E_ARG
    bad = copy.deepcopy(proof)
    bad.inst_evals[2] = r_limbs
    assert _snark_call(sz, bad, None, 0)[0] == E_ARG
    bad = copy.deepcopy(proof)
    bad.r1cs_eval_proof.hash_val[0] = r_limbs
    assert _snark_call(sz, bad, None, 0)[0] == E_ARG
    assert _sat_call(sat, None, 0)[0] == 0 and _snark_call(sz, proof, None, 0)[0] == 0


# ------------------------------------------------- host transcript calls ----
def test_append_u64_and_new_from_state():
    from testudo_amd.hyrax import FrTranscript
    from testudo_amd.snark import transcript_append_u64, transcript_new_from_state
    tr, ref = FrTranscript(), N.H.Transcript()
    for x in (0, 3, 16, 2 ** 64 - 1):
        transcript_append_u64(tr, x)
        N.append_u64(ref, x)
    assert V.state(tr) == ref.state()
    c = V.ints(tr.challenge_scalar())[0]
    assert c == ref.challenge()
    transcript_new_from_state(tr, fr_array([c]))
    N.new_from_state(ref, c)
    assert V.state(tr) == ref.state()
    fresh = FrTranscript()
    fresh.append_scalar(fr_array([c]))
    assert V.state(fresh) == V.state(tr)
    with pytest.raises(ValueError):
        transcript_new_from_state(tr, fr_array([R]))


def test_commitment_absorb(golden):
    from testudo_amd.hyrax import FrTranscript
    fx = golden[0]
    comm = V.commitment(fx["dims"], fx["comm"])
    tr, ref = FrTranscript(), N.H.Transcript()
    comm.write_to_transcript(tr)
    N.absorb_commitment(ref, fx["dims"], fx["comm"])
    assert V.state(tr) == ref.state()
    assert V.ints(tr.challenge_scalar())[0] == ref.challenge() == fx["c"]
    # a row missing, a point that is not canonical: refused, the transcript untouched
    tr = FrTranscript()
    before = V.state(tr)
    bad = copy.deepcopy(comm)
    bad.comm.comm_ops = bad.comm.comm_ops[:-1]
    with pytest.raises(ValueError):
        bad.write_to_transcript(tr)
    bad = copy.deepcopy(comm)
    bad.comm.comm_mem[1, 5] = np.uint64(2 ** 64 - 1)
    with pytest.raises(ValueError):
        bad.write_to_transcript(tr)
    assert V.state(tr) == before
