"""TEST INFRASTRUCTURE ONLY: conversions between the restatement's values
(tests/snark_ref.py: Python integers, affine tuples) and the library's objects
(testudo_amd.snark), shared by the CPU wire-format tests and the GPU tests."""
import numpy as np

import bls377 as O
import test_r1cs_eval_gpu as E
from testudo_amd.encoding import (fr_array, g1_array, g1_from_array, g2_array, g2_from_array, gt_array, gt_from_array,
                                  limbs_to_int)


def ints(a):
    return [limbs_to_int(x) for x in np.asarray(a).reshape(-1, 4)]


def state(tr):
    st, sq, idx = tr.state()
    return [limbs_to_int(x) for x in st], sq, idx


def sat_arrays(s):
    """a restatement satisfiability proof as the library's r1cs.R1CSProof"""
    from testudo_amd.r1cs import R1CSProof
    from testudo_amd.sqrt_pst import MippProof
    m = s["mipp"]
    tw = lambda t: np.asarray(gt_array(O.fq12_to_tower(t)), dtype=np.uint64).reshape(72)  # noqa: E731
    mc = len(m["comms_t"])
    mipp = MippProof(comms_t=np.stack([np.stack([tw(a), tw(b)]) for a, b in m["comms_t"]]).reshape(mc, 2, 72),
                     comms_u=np.stack([g1_array([a, b]).reshape(2, 12) for a, b in m["comms_u"]]).reshape(mc, 2, 12),
                     final_a=g1_array([m["final_a"]]).reshape(12), final_h=g2_array([m["final_h"]]).reshape(24),
                     pst_proof_h=g1_array(list(m["pst_proof_h"])).reshape(mc, 12))
    rxn, ryn = len(s["rx"]), len(s["ry"])
    return R1CSProof(T=tw(s["T"]), initial_state=fr_array([s["initial_state"]])[0],
                     sc_proof_phase1=fr_array([c for cs in s["sc1"] for c in cs]).reshape(rxn, 4, 4),
                     claims_phase2=fr_array(list(s["claims_phase2"])),
                     sc_proof_phase2=fr_array([c for cs in s["sc2"] for c in cs]).reshape(ryn, 3, 4),
                     claims_z_abc=fr_array(list(s.get("claims2", [0, 0]))), r_abc=fr_array(list(s.get("r_abc", [0, 0, 0]))),
                     rx=fr_array(s["rx"]), ry=fr_array(s["ry"]),
                     transcript_sat_state=fr_array([s["transcript_sat_state"]])[0],
                     eval_vars_at_ry=fr_array([s["eval_vars_at_ry"]])[0], comm=g1_array([s["U"]]).reshape(12),
                     proof_eval_vars_at_ry=g2_array(list(s["pst_proof"])).reshape(-1, 24), mipp_proof=mipp)


def sat_values(p, wire_only=False):
    """a library R1CSProof as comparable values; wire_only drops the two fields the wire format does not carry"""
    m = p.mipp_proof
    out = {"T": gt_from_array(p.T), "initial_state": limbs_to_int(p.initial_state),
           "sc1": [ints(x) for x in p.sc_proof_phase1], "claims_phase2": ints(p.claims_phase2),
           "sc2": [ints(x) for x in p.sc_proof_phase2], "rx": ints(p.rx), "ry": ints(p.ry),
           "transcript_sat_state": limbs_to_int(p.transcript_sat_state),
           "eval_vars_at_ry": limbs_to_int(p.eval_vars_at_ry), "U": g1_from_array(p.comm)[0],
           "pst_proof": g2_from_array(p.proof_eval_vars_at_ry),
           "comms_t": [[gt_from_array(t) for t in pr] for pr in m.comms_t],
           "comms_u": [list(g1_from_array(pr)) for pr in m.comms_u], "final_a": g1_from_array(m.final_a)[0],
           "final_h": g2_from_array(m.final_h)[0], "pst_proof_h": g1_from_array(m.pst_proof_h)}
    if not wire_only:
        out["r_abc"], out["claims2"] = ints(p.r_abc), ints(p.claims_z_abc)
    return out


def ref_sat_values(s, wire_only=False):
    m = s["mipp"]
    out = {"T": O.fq12_to_tower(s["T"]), "initial_state": s["initial_state"], "sc1": [list(c) for c in s["sc1"]],
           "claims_phase2": list(s["claims_phase2"]), "sc2": [list(c) for c in s["sc2"]], "rx": list(s["rx"]),
           "ry": list(s["ry"]), "transcript_sat_state": s["transcript_sat_state"],
           "eval_vars_at_ry": s["eval_vars_at_ry"], "U": s["U"], "pst_proof": list(s["pst_proof"]),
           "comms_t": [[O.fq12_to_tower(t) for t in pr] for pr in m["comms_t"]],
           "comms_u": [list(pr) for pr in m["comms_u"]], "final_a": m["final_a"], "final_h": m["final_h"],
           "pst_proof_h": list(m["pst_proof_h"])}
    if not wire_only:
        out["r_abc"], out["claims2"] = list(s["r_abc"]), list(s["claims2"])
    return out


def snark_arrays(proof, sz):
    """a restatement SNARK proof as the library's snark.TestudoSnark"""
    from testudo_amd.snark import TestudoSnark
    return TestudoSnark(sat_arrays(proof["sat"]), E._proof_arrays(proof["eval"], sz.log_ops, sz.log_cells),
                        fr_array(list(proof["inst_evals"])))


def commitment(dims, comm):
    """a restatement commitment as the library's snark.ComputationCommitment"""
    from testudo_amd.r1cs_eval import R1CSCommitment
    from testudo_amd.snark import ComputationCommitment
    return ComputationCommitment(*dims, R1CSCommitment(comm["num_ops"], comm["num_mem_cells"],
                                                       g1_array(comm["comm_ops"]).reshape(-1, 12),
                                                       g1_array(comm["comm_mem"]).reshape(-1, 12)))


def assert_snark_equal(got, ref, sz):
    """a library TestudoSnark against a restatement proof, element by element"""
    a, b = sat_values(got.r1cs_sat_proof), ref_sat_values(ref["sat"])
    for k in b:
        assert a[k] == b[k], ("sat", k)
    assert ints(got.inst_evals) == list(ref["inst_evals"])
    gv, rv = E._proof_values(got.r1cs_eval_proof), E._ref_values(ref["eval"], sz.log_ops, sz.log_cells)
    assert gv["comm_derefs"] == rv["comm_derefs"]
    for part in ("prod", "hash"):
        for k in rv[part]:
            assert gv[part][k] == rv[part][k], (part, k)

