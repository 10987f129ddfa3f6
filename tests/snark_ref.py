"""TEST INFRASTRUCTURE ONLY -- never imported by the product path.

First-principles restatement of TestudoSnark / TestudoNizk (testudo_snark.rs:
120-235, testudo_nizk.rs:80-157) over Python integers: the checker of
csrc/snark.hip.  It shares no code with the library.  Composed from

  oracle/py/r1cs.py         synthetic_r1cs, r1cs_prove, the Fq transcript helpers
  tests/sparse_eval_ref.py  gens_setup, multi_commit, multi_evaluate, prove, verify
  tests/hyrax_ref.py        the Fr Transcript
  oracle/py/serialize.py    the element encoders of the wire format

and restated here: the two-sponge protocol (include/tpst.h has it step by
step), the verifier of the satisfiability proof (the checks of
constraints.rs:263-397 with Polynomial::verify, r1csproof.rs:443-486),
Instance::new with its digest (lib.rs:129-235, r1csinstance.rs:155-164), the
byte layouts of R1CSProof (r1csproof.rs:32-53) and of the SNARK proof
(R1CSProof || R1CSEvalProof || Ar || Br || Cr, this project's layout), and a
tamper list.

A satisfiability proof is the dict oracle/py/r1cs.py returns; a SNARK proof is
{"sat", "eval", "inst_evals"} with "eval" a sparse_eval_ref proof.

``python tests/snark_ref.py`` rewrites tests/golden/snark.json and
tests/golden/snark_wire.json (recorded results only).  Parity with arkworks is
unpinned (no Rust toolchain; the reference's SNARK layer is commented out).
"""
from __future__ import annotations

import copy
import hashlib
import json
import os
import random
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import hyrax_ref as H  # noqa: E402  (puts oracle/py on the path)
import sparse_eval_ref as S  # noqa: E402
import spark_wire_ref as W  # noqa: E402
import bls377 as O  # noqa: E402
import pst as P  # noqa: E402
import r1cs as OR  # noqa: E402
from gens import FrSponge  # noqa: E402
from serialize import _le, _u64, ser_g1, ser_g2, ser_gt  # noqa: E402

R = O.R
LABEL = b"gens_r1cs_eval"
BATCH = 3


def log2(n):
    return n.bit_length() - 1


def next_pow2(n):
    p = 1
    while p < n:
        p *= 2
    return p


# ------------------------------------------------------------ transcripts --
def append_u64(F, x):
    """append_u64 (poseidon_transcript.rs:65-67): one native absorb of the element x"""
    F.sp.absorb_elems([x])


def new_from_state(F, c):
    """new_from_state (poseidon_transcript.rs:50-53): a fresh sponge that absorbs c"""
    F.sp = FrSponge()
    F.append_scalar(c)


def absorb_commitment(F, dims, comm):
    """R1CSCommitment::write_to_transcript (r1csinstance.rs:63-70, sparse_mlpoly.rs:335-341,
    dense_mlpoly.rs:464-470); dims = (num_cons, num_vars, num_inputs)"""
    for x in (*dims, BATCH, comm["num_ops"], comm["num_mem_cells"]):
        append_u64(F, x)
    for p in comm["comm_ops"]:
        F.append_point(p)
    for p in comm["comm_mem"]:
        F.append_point(p)


def fork(F):
    """steps 2-4: c = F.challenge; F.new_from_state(&c); Q = fresh Fq sponge + new_from_state2(&c)"""
    c = F.challenge()
    new_from_state(F, c)
    Q = P.PoseidonTranscript()
    OR.new_from_state2(Q, c)
    return c, Q


def bind(F, sat, evals=None):
    """step 8: sat.transcript_sat_state, rx, ry and (SNARK) Ar, Br, Cr into F"""
    F.append_scalar(sat["transcript_sat_state"])
    F.append_scalars(sat["rx"])
    F.append_scalars(sat["ry"])
    if evals is not None:
        for e in evals:
            F.append_scalar(e)


def q_state(Q):
    """the Fq sponge as the library's tpst_transcript holds it"""
    mode, idx = Q.sponge.mode
    return list(Q.sponge.state), 1 if mode == "squeeze" else 0, idx


# ---------------------------------------------- satisfiability verifier ----
def _points_ok(g1s=(), g2s=()):
    return all(p is None or (O.g1_on_curve(p) and O.g1_in_subgroup(p)) for p in g1s) and \
        all(p is None or (O.g2_on_curve(p) and O.g2_in_subgroup(p)) for p in g2s)


def sat_verify(sat, evals, inputs, num_cons, num_vars, srs, Q):
    """R1CSVerifierProof::verify as intended (r1csproof.rs:443-486) with the checks
    of the verifier circuit (constraints.rs:263-397) done natively, in the order
    the prover's transcript saw them.  False where the reference rejects."""
    nlog = log2(num_vars)
    rounds_x, rounds_y = log2(num_cons), nlog + 1
    if [len(sat["sc1"]), len(sat["rx"])] != [rounds_x] * 2 or [len(sat["sc2"]), len(sat["ry"])] != [rounds_y] * 2:
        return False
    if any(len(cs) != 4 for cs in sat["sc1"]) or any(len(cs) != 3 for cs in sat["sc2"]):
        return False
    m = sat["mipp"]
    if len(sat["pst_proof"]) != nlog - nlog // 2 or [len(m["comms_t"]), len(m["comms_u"]), len(m["pst_proof_h"])] != \
            [nlog // 2] * 3:
        return False
    scalars = [sat["initial_state"], sat["transcript_sat_state"], sat["eval_vars_at_ry"], *sat["claims_phase2"],
               *sat["rx"], *sat["ry"], *[c for cs in sat["sc1"] for c in cs], *[c for cs in sat["sc2"] for c in cs],
               *evals, *inputs]
    if any(not 0 <= x < R for x in scalars):
        return False
    if not _points_ok([sat["U"], m["final_a"], *m["pst_proof_h"], *[u for pr in m["comms_u"] for u in pr]],
                      [m["final_h"], *sat["pst_proof"]]):
        return False
    # the commitment's transcript state, then the inputs (r1csproof.rs:251-262)
    Q.append_gt(sat["T"])
    if Q.challenge_scalar() != sat["initial_state"]:
        return False
    OR.new_from_state2(Q, sat["initial_state"])
    for x in inputs:
        OR.append_scalar(Q, x)
    tau = [Q.challenge_scalar() for _ in range(rounds_x)]

    def rounds(polys, e):  # SumcheckInstanceProof::verify (sumcheck.rs:29-66)
        rs = []
        for cs in polys:
            if (2 * cs[0] + sum(cs[1:])) % R != e:  # p(0) + p(1)
                return None, None
            for c in cs:
                OR.append_scalar(Q, c)
            r = Q.challenge_scalar()
            rs.append(r)
            e = OR.unipoly_eval(cs, r)
        return e, rs

    e1, rx = rounds(sat["sc1"], 0)
    if e1 is None or rx != list(sat["rx"]):
        return False
    az, bz, cz, azbz = sat["claims_phase2"]
    eq_tau_rx = 1
    for t, r in zip(tau, rx):
        eq_tau_rx = eq_tau_rx * (t * r + (1 - t) * (1 - r)) % R
    if azbz != az * bz % R or e1 != (azbz - cz) * eq_tau_rx % R:
        return False
    ra, rb, rc = Q.challenge_scalar(), Q.challenge_scalar(), Q.challenge_scalar()
    e2, ry = rounds(sat["sc2"], (ra * az + rb * bz + rc * cz) % R)
    if e2 is None or ry != list(sat["ry"]):
        return False
    # z(ry) = (1 - ry[0]) vars(ry[1..]) + ry[0] (1, inputs)(ry[1..])   (r1csproof.rs:390-398)
    chi = OR.eq_evals(ry[1:])
    io = sum(v * chi[i] for i, v in enumerate([1] + list(inputs))) % R
    z_ry = ((1 - ry[0]) * sat["eval_vars_at_ry"] + ry[0] * io) % R
    if e2 != z_ry * (ra * evals[0] + rb * evals[1] + rc * evals[2]) % R:
        return False
    if Q.challenge_scalar() != sat["transcript_sat_state"]:
        return False
    OR.new_from_state2(Q, sat["transcript_sat_state"])
    return bool(P.Polynomial.verify(Q, srs, sat["U"], ry[1:], sat["eval_vars_at_ry"], sat["pst_proof"], m, sat["T"]))


# ------------------------------------------------------------ the flows ----
def pad_vars(vars_, num_vars):
    """lib.rs:99-113"""
    assert len(vars_) <= num_vars
    return list(vars_) + [0] * (num_vars - len(vars_))


def snark_prove(mats, dims, vars_, inputs, srs, comm, dense, gens, F, rnd, msm=H.py_msm):
    """TestudoSnark::prove (testudo_snark.rs:120-196) -> (proof, aux)"""
    num_cons, num_vars, _ni = dims
    absorb_commitment(F, dims, comm)
    c, Q = fork(F)
    sat = OR.r1cs_prove(mats, num_cons, num_vars, pad_vars(vars_, num_vars), list(inputs), srs, Q)
    evals = S.multi_evaluate(mats, sat["rx"], sat["ry"])
    bind(F, sat, evals)
    ev, _aux = S.prove(dense, sat["rx"], sat["ry"], evals, gens, F, rnd, msm)
    return {"sat": sat, "eval": ev, "inst_evals": evals}, {"c": c, "q_end": q_state(Q)}


def snark_verify(proof, dims, inputs, srs, comm, gens, F, msm=H.py_msm):
    """TestudoSnark::verify (testudo_snark.rs:198-235); F is stored back only on success"""
    num_cons, num_vars, num_inputs = dims
    if len(inputs) != num_inputs:
        return False
    if not _points_ok(list(comm["comm_ops"]) + list(comm["comm_mem"]) + list(proof["eval"]["comm_derefs"])):
        return False
    W_ = copy.deepcopy(F)
    absorb_commitment(W_, dims, comm)
    _c, Q = fork(W_)
    sat, evals = proof["sat"], list(proof["inst_evals"])
    if not sat_verify(sat, evals, list(inputs), num_cons, num_vars, srs, Q):
        return False
    bind(W_, sat, evals)
    if not eval_elements_ok(proof["eval"]):
        return False
    if not S.verify(comm, gens, sat["rx"], sat["ry"], evals, W_, proof["eval"], msm):
        return False
    F.sp = W_.sp
    return True


def _flat_ints(x):
    if isinstance(x, int):
        return [x]
    return [v for y in (x.values() if isinstance(x, dict) else x) for v in _flat_ints(y)]


def eval_elements_ok(ev):
    """what Validate::Yes would reject in an evaluation proof: scalars >= r, points off the curve"""
    pts, frs = list(ev["comm_derefs"]), []
    for k in ("proof_derefs", "proof_ops", "proof_mem"):
        pr = ev["hash"][k]
        pts += list(pr["L"]) + list(pr["R"]) + [pr["delta"], pr["beta"]]
        frs += [pr["z1"], pr["z2"]]
    for k in ("eval_row", "eval_col", "eval_val", "proof_ops", "proof_mem"):  # the product layer holds no point
        frs += _flat_ints(ev["prod"][k])
    for k in ("eval_row", "eval_col", "eval_val", "eval_derefs"):
        frs += _flat_ints(ev["hash"][k])
    return all(0 <= x < R for x in frs) and _points_ok(pts)


def nizk_prove(mats, dims, digest, vars_, inputs, srs, F):
    """TestudoNizk::prove (testudo_nizk.rs:80-130) and the first three absorbs of step 8"""
    num_cons, num_vars, _ni = dims
    F.append_bytes(digest)
    c, Q = fork(F)
    sat = OR.r1cs_prove(mats, num_cons, num_vars, pad_vars(vars_, num_vars), list(inputs), srs, Q)
    bind(F, sat)
    return sat, {"c": c, "q_end": q_state(Q)}


def nizk_verify(sat, mats, dims, digest, inputs, srs, F):
    """TestudoNizk::verify (testudo_nizk.rs:136-157), mirroring the prover's squeeze of c"""
    num_cons, num_vars, num_inputs = dims
    if len(inputs) != num_inputs or any(not 0 <= x < R for x in list(sat["rx"]) + list(sat["ry"])):
        return False
    W_ = copy.deepcopy(F)
    W_.append_bytes(digest)
    _c, Q = fork(W_)
    evals = S.multi_evaluate(mats, sat["rx"], sat["ry"])
    if not sat_verify(sat, evals, list(inputs), num_cons, num_vars, srs, Q):
        return False
    bind(W_, sat)
    F.sp = W_.sp
    return True


# --------------------------------------------------------- Instance::new ----
class InvalidIndex(Exception):
    pass


class InvalidScalar(Exception):
    pass


def from_random_bytes(b):
    """ark-ff 0.4 Fp::from_random_bytes, restated: at most 32 LE bytes, zero-extended, the top 3
    bits of byte 31 cleared, None if >= r (parity unpinned)"""
    if len(b) > 32:
        return None
    v = int.from_bytes(bytes(b) + bytes(32 - len(b)), "little") & ((1 << 253) - 1)
    return v if v < R else None


def instance_new(num_cons, num_vars, num_inputs, A, B, C):
    """Instance::new (lib.rs:129-235) -> (num_cons_padded, num_vars_padded, num_inputs, mats)"""
    nvp = next_pow2(max(num_vars, num_inputs + 1))
    ncp = 2 if num_cons in (0, 1) else num_cons
    if next_pow2(num_cons) != num_cons:  # also num_cons = 0: 0usize.next_power_of_two() is 1 (lib.rs:160-162)
        ncp = next_pow2(num_cons)
    mats = []
    for tups in (A, B, C):
        M = []
        for row, col, vb in tups:
            if row >= num_cons or col >= num_vars + 1 + num_inputs:
                raise InvalidIndex()
            v = from_random_bytes(vb)
            if v is None:
                raise InvalidScalar()
            M.append((row, col + nvp - num_vars if col >= num_vars else col, v))
        if num_cons in (0, 1):
            M += [(i, num_vars, 0) for i in range(len(tups), ncp)]
        mats.append(M)
    return ncp, nvp, num_inputs, mats


def instance_digest(num_cons, num_vars, num_inputs, mats):
    """get_digest (r1csinstance.rs:155-164): SHAKE-256 over the Compress::Yes bytes of R1CSInstance
    (r1csinstance.rs:20-27; SparseMatPolynomial and SparseMatEntry, sparse_mlpoly.rs:25-44)"""
    b = _u64(num_cons) + _u64(num_vars) + _u64(num_inputs)
    for M in mats:
        b += _u64(log2(num_cons)) + _u64(log2(2 * num_vars)) + _u64(len(M))
        b += b"".join(_u64(r) + _u64(c) + _le(v, 32) for r, c, v in M)
    return hashlib.shake_256(b).digest(256)


def padded_case():
    """the instance of testudo_snark.rs:298-335: 1 constraint, 0 variables, 3 inputs"""
    le = lambda v: _le(v % R, 32)  # noqa: E731
    nv = 0
    A = [(0, nv + 2, le(1))]
    B = [(0, nv + 2, le(1))]
    C = [(0, nv + 1, le(1)), (0, nv, le(-13)), (0, nv + 3, le(-1))]
    return {"num_cons": 1, "num_vars": 0, "num_inputs": 3, "num_nz_entries": 3, "A": A, "B": B, "C": C,
            "vars": [], "inputs": [le(16), le(1), le(2)]}


# ------------------------------------------------------------ wire format --
def _fr(v):
    return _le(v, 32)


def _vec_fr(v):
    return _u64(len(v)) + b"".join(_fr(x) for x in v)


def ser_r1cs_proof(sat):
    """R1CSProof, Compress::Yes, fields in declaration order (r1csproof.rs:32-53)"""
    m = sat["mipp"]
    out = _u64(len(sat["pst_proof"])) + ser_g1(sat["U"])                 # comm: nv = q.num_vars = m_row
    out += _u64(len(sat["sc1"])) + b"".join(_vec_fr(cs) for cs in sat["sc1"])
    out += b"".join(_fr(x) for x in sat["claims_phase2"])
    out += _u64(len(sat["sc2"])) + b"".join(_vec_fr(cs) for cs in sat["sc2"])
    out += _fr(sat["eval_vars_at_ry"])
    out += _u64(len(sat["pst_proof"])) + b"".join(ser_g2(q) for q in sat["pst_proof"])
    out += _vec_fr(sat["rx"]) + _vec_fr(sat["ry"])
    out += _fr(sat["transcript_sat_state"]) + _fr(sat["initial_state"])
    out += ser_gt(O.fq12_to_tower(sat["T"]))
    out += _u64(len(m["comms_t"])) + b"".join(ser_gt(O.fq12_to_tower(a)) + ser_gt(O.fq12_to_tower(b))
                                              for a, b in m["comms_t"])
    out += _u64(len(m["comms_u"])) + b"".join(ser_g1(a) + ser_g1(b) for a, b in m["comms_u"])
    out += ser_g1(m["final_a"]) + ser_g2(m["final_h"])
    out += _u64(len(m["pst_proof_h"])) + b"".join(ser_g1(q) for q in m["pst_proof_h"])
    return out


def ser_snark_proof(proof):
    """R1CSProof || R1CSEvalProof || Ar || Br || Cr"""
    return ser_r1cs_proof(proof["sat"]) + W.ser_r1cs_eval_proof(proof["eval"]) + \
        b"".join(_fr(e) for e in proof["inst_evals"])


# ------------------------------------------------------------------ cases --
def draw_rnd(gens, rng):
    return S.draws(gens, rng)


def make_case(num_cons, num_vars, num_inputs, seed, srs_seed, prefix=(), msm=H.py_msm, gens=None, nizk=True):
    """a synthetic instance through both modes on transcripts that first absorbed `prefix`"""
    mats, v, x = OR.synthetic_r1cs(num_cons, num_vars, num_inputs, seed)
    mats = [list(M) for M in mats]
    dims = (num_cons, num_vars, num_inputs)
    srs = P.SRS((log2(num_vars) + 1) // 2, srs_seed)
    gens = gens or S.gens_setup(LABEL, num_cons, num_vars, num_cons)
    comm, dense = S.multi_commit(mats, num_cons, num_vars, gens, msm)
    rnd = draw_rnd(gens, random.Random(seed ^ 0x5A5A))
    F = H.Transcript()
    F.append_scalars(prefix)
    proof, aux = snark_prove(mats, dims, v, x, srs, comm, dense, gens, F, rnd, msm)
    case = {"mats": mats, "dims": dims, "vars": v, "inputs": x, "srs": srs, "srs_seed": srs_seed, "gens": gens,
            "comm": comm, "dense": dense, "rnd": rnd, "prefix": list(prefix), "proof": proof, "c": aux["c"],
            "q_end": aux["q_end"], "f_end": F.state()}
    if nizk:
        case["digest"] = instance_digest(*dims, mats)
        G = H.Transcript()
        G.append_scalars(prefix)
        sat, naux = nizk_prove(mats, dims, case["digest"], v, x, srs, G)
        case["nizk"] = {"proof": sat, "c": naux["c"], "q_end": naux["q_end"], "f_end": G.state()}
    return case


def verify_case(case, proof=None, inputs=None, comm=None, prefix=None, msm=H.py_msm):
    """the restated SNARK verifier on a case, with replacements -> (ok, F)"""
    F = H.Transcript()
    F.append_scalars(case["prefix"] if prefix is None else prefix)
    ok = snark_verify(case["proof"] if proof is None else proof, case["dims"],
                      case["inputs"] if inputs is None else inputs, case["srs"],
                      case["comm"] if comm is None else comm, case["gens"], F, msm)
    return ok, F


# ---------------------------------------------------------------- tampers --
def _bump(v):
    return (v + 1) % R


def _sat_tampers():
    """one per field of R1CSProof that the verifier reads"""
    def f(name, fn):
        return (name, fn)

    def cl(i):
        def g(s):
            c = list(s["claims_phase2"])
            c[i] = _bump(c[i])
            s["claims_phase2"] = tuple(c)
        return g

    return [
        f("sat.comm", lambda s: s.__setitem__("U", O.g1_add(s["U"], s["U"]))),
        f("sat.sc_proof_phase1", lambda s: s["sc1"][1].__setitem__(2, _bump(s["sc1"][1][2]))),
        f("sat.claims_phase2", cl(0)),
        f("sat.sc_proof_phase2", lambda s: s["sc2"][2].__setitem__(1, _bump(s["sc2"][2][1]))),
        f("sat.eval_vars_at_ry", lambda s: s.__setitem__("eval_vars_at_ry", _bump(s["eval_vars_at_ry"]))),
        f("sat.proof_eval_vars_at_ry",
          lambda s: s.__setitem__("pst_proof", [O.g2_add(s["pst_proof"][0], s["pst_proof"][0])] + list(s["pst_proof"][1:]))),
        f("sat.rx", lambda s: s["rx"].__setitem__(1, _bump(s["rx"][1]))),
        f("sat.ry", lambda s: s["ry"].__setitem__(2, _bump(s["ry"][2]))),
        f("sat.transcript_sat_state", lambda s: s.__setitem__("transcript_sat_state", _bump(s["transcript_sat_state"]))),
        f("sat.initial_state", lambda s: s.__setitem__("initial_state", _bump(s["initial_state"]))),
        f("sat.t", lambda s: s.__setitem__("T", O.f12_mul(s["T"], s["T"]))),
        f("sat.mipp_proof", lambda s: s.__setitem__("mipp", dict(s["mipp"], final_a=O.g1_mul(O.G1_GEN, 5)))),
    ]


def _eval_tamper_paths(log_ops, log_cells):
    """at least one element of each part of the evaluation proof"""
    want = {"comm_derefs[0]", "prod.proof_ops coefficient", "prod.proof_ops left claim", "prod.proof_mem coefficient",
            "prod.proof_mem left claim", "hash.eval_val[0]", "hash.proof_derefs.z1", "hash.proof_ops.z1",
            "hash.proof_mem.z1", "prod.eval_row.init", "hash.eval_derefs.row[0]"}
    return [(n, p) for n, p in S.tamper_list(log_ops, log_cells) if n in want]


SAT_TAMPERS = [n for n, _ in _sat_tampers()]
EVALS_TAMPERS = ["inst_evals.Ar", "inst_evals.Br", "inst_evals.Cr"]
OTHER_TAMPERS = ["wrong_input", "extra_input", "other_commitment", "splice", "prefix", "non_canonical", "off_curve"]


def eval_tamper_names(case):
    sz_ops, sz_cells = log2(case["comm"]["num_ops"]), log2(case["comm"]["num_mem_cells"])
    return [n for n, _ in _eval_tamper_paths(sz_ops, sz_cells)]


def tamper_names(case):
    return SAT_TAMPERS + EVALS_TAMPERS + eval_tamper_names(case) + OTHER_TAMPERS


def copy_proof(proof):
    return {"sat": copy.deepcopy(proof["sat"]), "eval": copy.deepcopy(proof["eval"]),
            "inst_evals": list(proof["inst_evals"])}


def apply_tamper(name, case, other):
    """-> dict(proof, inputs, comm, prefix): `case` with one thing changed.  `other` = a case of the
    same shape over another instance, proved on a transcript with another prefix."""
    out = {"proof": copy_proof(case["proof"]), "inputs": list(case["inputs"]), "comm": case["comm"],
           "prefix": list(case["prefix"])}
    p = out["proof"]
    sat = dict(_sat_tampers())
    if name in sat:
        sat[name](p["sat"])
    elif name in EVALS_TAMPERS:
        k = EVALS_TAMPERS.index(name)
        p["inst_evals"][k] = _bump(p["inst_evals"][k])
    elif name == "wrong_input":
        out["inputs"][0] = _bump(out["inputs"][0])
    elif name == "extra_input":
        out["inputs"].append(1)
    elif name == "other_commitment":
        out["comm"] = other["comm"]
    elif name == "splice":  # this proof's sat part with the other proof's evaluation part
        p["eval"] = copy.deepcopy(other["proof"]["eval"])
    elif name == "prefix":
        out["prefix"] = list(case["prefix"]) + [1]
    elif name == "non_canonical":
        c = list(p["sat"]["claims_phase2"])
        c[1] += R
        assert c[1] < 1 << 256
        p["sat"]["claims_phase2"] = tuple(c)
    elif name == "off_curve":
        x, y = p["eval"]["comm_derefs"][0]
        p["eval"]["comm_derefs"][0] = (x, y ^ 1)
    else:
        paths = dict(_eval_tamper_paths(log2(case["comm"]["num_ops"]), log2(case["comm"]["num_mem_cells"])))
        p["eval"] = S.tampered(p["eval"], paths[name])
    return out


# ---------------------------------------------------------------- fixture --
GOLDEN = os.path.join(_HERE, "golden", "snark.json")
GOLDEN_WIRE = os.path.join(_HERE, "golden", "snark_wire.json")
FIXTURE_DIMS = (16, 16, 3)
FIXTURE_SEED, FIXTURE_SRS_SEED = 0x534E_0010, 0x7E57D1

_hx, _hxs, _ints = S._hx, S._hxs, S._ints


def _pt(p):
    return H._pt(p)


def _pt2(p):
    return None if p is None else [[_hx(p[0][0]), _hx(p[0][1])], [_hx(p[1][0]), _hx(p[1][1])]]


def _pt2_in(p):
    return None if p is None else ((int(p[0][0], 16), int(p[0][1], 16)), (int(p[1][0], 16), int(p[1][1], 16)))


def _gt(t):
    return _hxs(O.fq12_to_tower(t))


def _gt_in(t):
    return O.fq12_from_tower(_ints(t))


def enc_sat(s):
    m = s["mipp"]
    return {"comm": _pt(s["U"]), "sc_proof_phase1": [_hxs(cs) for cs in s["sc1"]],
            "claims_phase2": _hxs(s["claims_phase2"]), "sc_proof_phase2": [_hxs(cs) for cs in s["sc2"]],
            "eval_vars_at_ry": _hx(s["eval_vars_at_ry"]), "proof_eval_vars_at_ry": [_pt2(q) for q in s["pst_proof"]],
            "rx": _hxs(s["rx"]), "ry": _hxs(s["ry"]), "transcript_sat_state": _hx(s["transcript_sat_state"]),
            "initial_state": _hx(s["initial_state"]), "t": _gt(s["T"]),
            "mipp_proof": {"comms_t": [[_gt(a), _gt(b)] for a, b in m["comms_t"]],
                           "comms_u": [[_pt(a), _pt(b)] for a, b in m["comms_u"]], "final_a": _pt(m["final_a"]),
                           "final_h": _pt2(m["final_h"]), "pst_proof_h": [_pt(q) for q in m["pst_proof_h"]]},
            "r_abc": _hxs(s["r_abc"]), "claims_phase2_z_abc": _hxs(s["claims2"])}


def dec_sat(d):
    m = d["mipp_proof"]
    return {"U": H.pt_in(d["comm"]), "sc1": [_ints(cs) for cs in d["sc_proof_phase1"]],
            "claims_phase2": tuple(_ints(d["claims_phase2"])), "sc2": [_ints(cs) for cs in d["sc_proof_phase2"]],
            "eval_vars_at_ry": int(d["eval_vars_at_ry"], 16),
            "pst_proof": [_pt2_in(q) for q in d["proof_eval_vars_at_ry"]], "rx": _ints(d["rx"]), "ry": _ints(d["ry"]),
            "transcript_sat_state": int(d["transcript_sat_state"], 16), "initial_state": int(d["initial_state"], 16),
            "T": _gt_in(d["t"]),
            "mipp": {"comms_t": [(_gt_in(a), _gt_in(b)) for a, b in m["comms_t"]],
                     "comms_u": [(H.pt_in(a), H.pt_in(b)) for a, b in m["comms_u"]], "final_a": H.pt_in(m["final_a"]),
                     "final_h": _pt2_in(m["final_h"]), "pst_proof_h": [H.pt_in(q) for q in m["pst_proof_h"]]},
            "r_abc": tuple(_ints(d["r_abc"])), "claims2": _ints(d["claims_phase2_z_abc"]),
            "n_vars": len(d["ry"]) - 1}


def _enc_state(st):
    s, sq, idx = st
    return {"state": _hxs(s), "squeezing": sq, "index": idx}


def _dec_state(d):
    return _ints(d["state"]), d["squeezing"], d["index"]


_CASES = {}


def fixture_case():
    if "fx" not in _CASES:
        _CASES["fx"] = make_case(*FIXTURE_DIMS, FIXTURE_SEED, FIXTURE_SRS_SEED)
    return _CASES["fx"]


def make_fixture():
    c = fixture_case()
    nz = c["nizk"]
    return {"num_cons": c["dims"][0], "num_vars": c["dims"][1], "num_inputs": c["dims"][2], "label": LABEL.decode(),
            "seed": FIXTURE_SEED, "srs_seed": FIXTURE_SRS_SEED,
            "mats": [[[r, cc, _hx(x)] for r, cc, x in M] for M in c["mats"]],
            "vars": _hxs(c["vars"]), "inputs": _hxs(c["inputs"]), "rnd": [_hxs(r) for r in c["rnd"]],
            "comm": {"num_ops": c["comm"]["num_ops"], "num_mem_cells": c["comm"]["num_mem_cells"],
                     "comm_ops": S._pts(c["comm"]["comm_ops"]), "comm_mem": S._pts(c["comm"]["comm_mem"])},
            "c": _hx(c["c"]), "sat": enc_sat(c["proof"]["sat"]), "eval": S._enc_proof(c["proof"]["eval"]),
            "inst_evals": _hxs(c["proof"]["inst_evals"]),
            "f_end": _enc_state(c["f_end"]), "q_end": _enc_state(c["q_end"]),
            "nizk": {"digest": c["digest"].hex(), "c": _hx(nz["c"]), "proof": enc_sat(nz["proof"]),
                     "f_end": _enc_state(nz["f_end"]), "q_end": _enc_state(nz["q_end"])}}


def dump_fixture(fx):
    return json.dumps(fx, indent=0) + "\n"


def load_fixture():
    with open(GOLDEN) as f:
        d = json.load(f)
    nz = d["nizk"]
    return {"raw": d, "dims": (d["num_cons"], d["num_vars"], d["num_inputs"]), "label": d["label"].encode(),
            "seed": d["seed"], "srs_seed": d["srs_seed"],
            "mats": [[(r, c, int(x, 16)) for r, c, x in M] for M in d["mats"]],
            "vars": _ints(d["vars"]), "inputs": _ints(d["inputs"]), "rnd": [_ints(r) for r in d["rnd"]],
            "comm": {"num_ops": d["comm"]["num_ops"], "num_mem_cells": d["comm"]["num_mem_cells"],
                     "comm_ops": [H.pt_in(p) for p in d["comm"]["comm_ops"]],
                     "comm_mem": [H.pt_in(p) for p in d["comm"]["comm_mem"]]},
            "c": int(d["c"], 16),
            "proof": {"sat": dec_sat(d["sat"]), "eval": S._dec_proof(d["eval"]), "inst_evals": _ints(d["inst_evals"])},
            "f_end": _dec_state(d["f_end"]), "q_end": _dec_state(d["q_end"]),
            "nizk": {"digest": bytes.fromhex(nz["digest"]), "c": int(nz["c"], 16), "proof": dec_sat(nz["proof"]),
                     "f_end": _dec_state(nz["f_end"]), "q_end": _dec_state(nz["q_end"])}}


def fixture_bytes():
    """(SNARK proof bytes, R1CSProof bytes of the NIZK proof) of tests/golden/snark.json"""
    fx = load_fixture()
    return ser_snark_proof(fx["proof"]), ser_r1cs_proof(fx["nizk"]["proof"])


def make_wire_fixture():
    out = {}
    for name, b in zip(("snark_proof", "r1cs_proof"), fixture_bytes()):
        out[name] = {"len": len(b), "sha256": hashlib.sha256(b).hexdigest(), "hex": b.hex()}
    return out


def load_wire_fixture():
    with open(GOLDEN_WIRE) as f:
        d = json.load(f)
    return {k: bytes.fromhex(v["hex"]) for k, v in d.items()}, d


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        f.write(dump_fixture(make_fixture()))
    with open(GOLDEN_WIRE, "w") as f:
        f.write(json.dumps(make_wire_fixture(), indent=0) + "\n")
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), GOLDEN_WIRE, os.path.getsize(GOLDEN_WIRE))
