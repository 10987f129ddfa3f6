"""TEST INFRASTRUCTURE ONLY -- never imported by the product path.

First-principles restatement of R1CSEvalProof = SparseMatPolyEvalProof::{prove,
verify} (r1csinstance.rs:336-386, sparse_mlpoly.rs:1441-1569) over Python
integers: the checker of csrc/sparse_eval.hip.  The transcript and the Hyrax
opening are hyrax_ref's, the product circuits product_tree_ref's, the synthetic
instance oracle/py/r1cs.py's.  Restated here: the dense representation with its
address vectors (sparse_mlpoly.rs:358-437), AddrTimestamps::deref (:263-278),
Layers::build_hash_layer (:542-615), DensePolynomial::merge and
bound_poly_var_bot (dense_mlpoly.rs:431-444, :398-405), IdentityPolynomial
(:267-283), ProductLayerProof (:1053-1334) and HashLayerProof (:733-1040).

A proof is a dict:
  comm_derefs   the row commitments of Derefs::commit
  prod          eval_row / eval_col = (init, [read], [write], audit),
                eval_val = ([left], [right]), proof_ops / proof_mem
                (product_tree_ref proofs)
  hash          eval_row / eval_col = ([addr], [read_ts], audit_ts), eval_val,
                eval_derefs = ([row], [col]), proof_derefs / proof_ops /
                proof_mem (hyrax_ref proofs)

``python tests/sparse_eval_ref.py`` rewrites tests/golden/r1cs_eval.json.
Parity with arkworks is unpinned (no Rust toolchain): the restatement and the
verifier's equations pin the device code.
"""
from __future__ import annotations

import copy
import json
import os
import random
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import hyrax_ref as H  # noqa: E402
import product_tree_ref as PT  # noqa: E402
from hyrax_ref import Transcript, eq_evals  # noqa: E402
import r1cs as OR  # noqa: E402  (oracle/py, on the path through hyrax_ref)

R = H.R
BATCH = 3


class ProverAssert(Exception):
    """one of the assert_eq!s of ProductLayerProof::prove"""


def log2(n):
    return n.bit_length() - 1


def next_pow2(n):
    p = 1
    while p < n:
        p *= 2
    return p


# ------------------------------------------------------ dense polynomials --
def merge(polys):
    """DensePolynomial::merge (dense_mlpoly.rs:431-444)."""
    Z = [v for p in polys for v in p]
    return Z + [0] * (next_pow2(len(Z)) - len(Z))


def bound_bot(Z, r):
    """DensePolynomial::bound_poly_var_bot (dense_mlpoly.rs:398-405)."""
    return [(Z[2 * i] + (Z[2 * i + 1] - Z[2 * i]) * r) % R for i in range(len(Z) // 2)]


def identity_eval(r):
    """IdentityPolynomial::evaluate (dense_mlpoly.rs:276-282)."""
    n = len(r)
    return sum((1 << (n - i - 1)) * r[i] for i in range(n)) % R


def eq_eval(r, x):
    """EqPolynomial::evaluate (dense_mlpoly.rs:221-229)."""
    out = 1
    for a, b in zip(r, x):
        out = out * (a * b + (1 - a) * (1 - b)) % R
    return out


def n_to_1(evals, tr):
    """the n-to-1 reduction of sparse_mlpoly.rs:107-121 / 778-789: append the
    evaluations, draw log2(n) challenges, bind from the last -> (challenges,
    joint claim)."""
    tr.append_scalars(evals)
    ch = PT.challenge_vec(tr, log2(len(evals)))
    Z = list(evals)
    for c in reversed(ch):
        Z = bound_bot(Z, c)
    assert len(Z) == 1
    return ch, Z[0]


# --------------------------------------------------- dense representation --
def dims(mats, num_cons, num_vars):
    N = next_pow2(max(next_pow2(max(len(M), 1)) for M in mats))
    vx, vy = log2(num_cons), log2(2 * num_vars)
    return N, vx, vy, 1 << max(vx, vy)


def dense_rep(mats, num_cons, num_vars):
    """SparseMatPolynomial::multi_sparse_to_dense_rep (sparse_mlpoly.rs:373-437)
    with AddrTimestamps::new (:228-261)."""
    N, _vx, _vy, cells = dims(mats, num_cons, num_vars)

    def side(k):
        ops = [[e[k] for e in M] + [0] * (N - len(M)) for M in mats]
        audit, read = [0] * cells, []
        for inst in ops:
            r = []
            for a in inst:
                assert a < cells
                r.append(audit[a])
                audit[a] += 1
            read.append(r)
        return {"addr": ops, "read_ts": read, "audit_ts": audit}

    row, col = side(0), side(1)
    val = [[e[2] % R for e in M] + [0] * (N - len(M)) for M in mats]
    return {"N": N, "cells": cells, "row": row, "col": col, "val": val,
            "comb_ops": merge(row["addr"] + row["read_ts"] + col["addr"] + col["read_ts"] + val),
            "comb_mem": row["audit_ts"] + col["audit_ts"]}


def gens_setup(label, num_cons, num_vars, num_nz_entries):
    """R1CSCommitmentGens::setup (r1csinstance.rs:33-52) ->
    SparseMatPolyCommitmentGens::setup (sparse_mlpoly.rs:296-323), batch 3."""
    vx, vy = log2(num_cons), log2(2 * num_vars)
    n = log2(next_pow2(num_nz_entries))
    ell = {"ops": n + log2(next_pow2(BATCH * 5)), "mem": max(vx, vy) + 1, "derefs": n + log2(next_pow2(BATCH * 2))}
    return {"ell": ell, **{k: H.setup_gens(v, label) for k, v in ell.items()}}


def poly_commit(Z, gens, msm):
    """DensePolynomial::commit with zero blinds (dense_mlpoly.rs:349-377)."""
    ell = log2(len(Z))
    return H.commit_rows(list(Z), [0] * (1 << (ell // 2)), gens, msm)


def multi_commit(mats, num_cons, num_vars, gens, msm=H.py_msm):
    """SparseMatPolynomial::multi_commit (sparse_mlpoly.rs:490-517) -> (comm, dense)."""
    dense = dense_rep(mats, num_cons, num_vars)
    comm = {"num_ops": dense["N"], "num_mem_cells": dense["cells"],
            "comm_ops": poly_commit(dense["comb_ops"], gens["ops"], msm),
            "comm_mem": poly_commit(dense["comb_mem"], gens["mem"], msm)}
    return comm, dense


def multi_evaluate(mats, rx, ry):
    """SparseMatPolynomial::multi_evaluate (sparse_mlpoly.rs:453-460)."""
    ex, ey = eq_evals(rx), eq_evals(ry)
    return [sum(ex[r] * ey[c] * v for r, c, v in M) % R for M in mats]


# ------------------------------------------------------------- the layers --
def equalize(rx, ry):
    """SparseMatPolyEvalProof::equalize (sparse_mlpoly.rs:1452-1471)."""
    d = len(ry) - len(rx)
    return ([0] * max(d, 0) + list(rx), [0] * max(-d, 0) + list(ry))


def deref(addrs, mem):
    """AddrTimestamps::deref (sparse_mlpoly.rs:263-278)."""
    return [[mem[a] for a in inst] for inst in addrs]


def build_hash_layer(eval_table, addrs, derefs, read_ts, audit_ts, r_mem_check):
    """Layers::build_hash_layer (sparse_mlpoly.rs:542-615) -> (init, [read], [write], audit)."""
    r_hash, gamma = r_mem_check
    sq = r_hash * r_hash % R
    h = lambda addr, val, ts: (sq * ts + val * r_hash + addr - gamma) % R  # noqa: E731
    init = [h(i, eval_table[i], 0) for i in range(len(eval_table))]
    audit = [h(i, eval_table[i], audit_ts[i]) for i in range(len(eval_table))]
    read = [[h(a, d, t) for a, d, t in zip(A, Dv, T)] for A, Dv, T in zip(addrs, derefs, read_ts)]
    write = [[h(a, d, t + 1) for a, d, t in zip(A, Dv, T)] for A, Dv, T in zip(addrs, derefs, read_ts)]
    return init, read, write, audit


def _prod(v):
    out = 1
    for x in v:
        out = out * x % R
    return out


# ----------------------------------------------------------------- prover --
def _open(Z, gens, r_joint, claim, tr, rnd, msm):
    tr.append_scalar(claim)
    proof, _c = H.eval_prove(list(Z), None, r_joint, claim, None, gens, tr, rnd, msm)
    return proof


def prove(dense, rx, ry, evals, gens, tr, rnd, msm=H.py_msm):
    """SparseMatPolyEvalProof::prove (sparse_mlpoly.rs:1473-1532).  rnd = the
    three openings' draws in proving order (derefs, ops, mem).  -> (proof, aux)
    with aux = the intermediate values the fixture records."""
    assert len(evals) == BATCH
    rx_ext, ry_ext = equalize(rx, ry)
    mem_rx, mem_ry = eq_evals(rx_ext), eq_evals(ry_ext)
    row_val, col_val = deref(dense["row"]["addr"], mem_rx), deref(dense["col"]["addr"], mem_ry)
    comb_derefs = merge(row_val + col_val)
    comm_derefs = poly_commit(comb_derefs, gens["derefs"], msm)
    for p in comm_derefs:
        tr.append_point(p)
    r_mem_check = PT.challenge_vec(tr, 2)
    layers = [build_hash_layer(mem, side["addr"], dv, side["read_ts"], side["audit_ts"], r_mem_check)
              for mem, side, dv in ((mem_rx, dense["row"], row_val), (mem_ry, dense["col"], col_val))]

    # ---- ProductLayerProof::prove (:1053-1236)
    circ, ev = [], []
    for init, read, write, audit in layers:
        c = (PT.product_circuit(init), [PT.product_circuit(p) for p in read],
             [PT.product_circuit(p) for p in write], PT.product_circuit(audit))
        e = (PT.circuit_evaluate(c[0]), [PT.circuit_evaluate(x) for x in c[1]],
             [PT.circuit_evaluate(x) for x in c[2]], PT.circuit_evaluate(c[3]))
        if e[0] * _prod(e[2]) % R != _prod(e[1]) * e[3] % R:
            raise ProverAssert("subset check")
        tr.append_scalar(e[0])
        tr.append_scalars(e[1])
        tr.append_scalars(e[2])
        tr.append_scalar(e[3])
        circ.append(c)
        ev.append(e)
    dotps, left, right = [], [], []
    for i in range(BATCH):
        lh, rh = PT.dotp_split(row_val[i], col_val[i], dense["val"][i])
        el, er = PT.dotp_evaluate(*lh), PT.dotp_evaluate(*rh)
        tr.append_scalar(el)
        tr.append_scalar(er)
        if (el + er) % R != evals[i] % R:
            raise ProverAssert("evals[%d]" % i)
        left.append(el)
        right.append(er)
        dotps += [lh, rh]
    (ri, rr, rw, ra), (ci, cr, cw, ca) = circ
    proof_ops, rand_ops = PT.prove(rr + rw + cr + cw, dotps, tr)
    proof_mem, rand_mem = PT.prove([ri, ra, ci, ca], [], tr)
    prod = {"eval_row": ev[0], "eval_col": ev[1], "eval_val": (left, right), "proof_ops": proof_ops,
            "proof_mem": proof_mem}

    # ---- HashLayerProof::prove (:733-837)
    ev_at = lambda polys, r: [H.evaluate(p, r) for p in polys]  # noqa: E731
    e_row_val, e_col_val = ev_at(row_val, rand_ops), ev_at(col_val, rand_ops)
    evals_derefs = e_row_val + e_col_val
    evals_derefs += [0] * (next_pow2(len(evals_derefs)) - len(evals_derefs))
    ch, claim_derefs = n_to_1(evals_derefs, tr)
    proof_derefs = _open(comb_derefs, gens["derefs"], ch + rand_ops, claim_derefs, tr, rnd[0], msm)
    helper = lambda side: (ev_at(side["addr"], rand_ops), ev_at(side["read_ts"], rand_ops),  # noqa: E731
                           H.evaluate(side["audit_ts"], rand_mem))
    h_row, h_col = helper(dense["row"]), helper(dense["col"])
    e_val = ev_at(dense["val"], rand_ops)
    evals_ops = h_row[0] + h_row[1] + h_col[0] + h_col[1] + e_val
    evals_ops += [0] * (next_pow2(len(evals_ops)) - len(evals_ops))
    ch, claim_ops = n_to_1(evals_ops, tr)
    proof_hops = _open(dense["comb_ops"], gens["ops"], ch + rand_ops, claim_ops, tr, rnd[1], msm)
    ch, claim_mem = n_to_1([h_row[2], h_col[2]], tr)
    proof_hmem = _open(dense["comb_mem"], gens["mem"], ch + rand_mem, claim_mem, tr, rnd[2], msm)
    hash_ = {"eval_row": h_row, "eval_col": h_col, "eval_val": e_val, "eval_derefs": (e_row_val, e_col_val),
             "proof_derefs": proof_derefs, "proof_ops": proof_hops, "proof_mem": proof_hmem}
    aux = {"r_mem_check": r_mem_check, "rand_mem": rand_mem, "rand_ops": rand_ops,
           "joint_claims": [claim_derefs, claim_ops, claim_mem], "comb_derefs": comb_derefs, "layers": layers}
    return {"comm_derefs": comm_derefs, "prod": prod, "hash": hash_}, aux


# --------------------------------------------------------------- verifier --
def _verify_helper(rand_mem, claims, e_val, e_addr, e_read_ts, e_audit_ts, r, r_mem_check):
    """HashLayerProof::verify_helper (sparse_mlpoly.rs:839-894)."""
    r_hash, gamma = r_mem_check
    sq = r_hash * r_hash % R
    h = lambda addr, val, ts: (sq * ts + val * r_hash + addr - gamma) % R  # noqa: E731
    c_init, c_read, c_write, c_audit = claims
    addr0, val0 = identity_eval(rand_mem), eq_eval(r, rand_mem)
    if h(addr0, val0, 0) != c_init:
        return False
    for i in range(len(e_addr)):
        if h(e_addr[i], e_val[i], e_read_ts[i]) != c_read[i]:
            return False
        if h(e_addr[i], e_val[i], e_read_ts[i] + 1) != c_write[i]:
            return False
    return h(addr0, val0, e_audit_ts) == c_audit


def verify(comm, gens, rx, ry, evals, tr, proof, msm=H.py_msm):
    """SparseMatPolyEvalProof::verify (sparse_mlpoly.rs:1534-1568) ->
    PolyEvalNetworkProof::verify (:1377-1438); False where the reference
    asserts or returns Err."""
    rx_ext, ry_ext = equalize(rx, ry)
    num_ops, cells = comm["num_ops"], comm["num_mem_cells"]
    if 1 << len(rx_ext) != cells or len(evals) != BATCH:
        return False
    for p in proof["comm_derefs"]:
        tr.append_point(p)
    r_mem_check = PT.challenge_vec(tr, 2)
    # ---- ProductLayerProof::verify (:1238-1334)
    pd = proof["prod"]
    for init, read, write, audit in (pd["eval_row"], pd["eval_col"]):
        if len(read) != BATCH or len(write) != BATCH:
            return False
        if _prod(write) * init % R != _prod(read) * audit % R:
            return False
        tr.append_scalar(init)
        tr.append_scalars(read)
        tr.append_scalars(write)
        tr.append_scalar(audit)
    left, right = pd["eval_val"]
    if len(left) != BATCH or len(right) != BATCH:
        return False
    claims_dotp = []
    for i in range(BATCH):
        if (left[i] + right[i]) % R != evals[i] % R:
            return False
        tr.append_scalar(left[i])
        tr.append_scalar(right[i])
        claims_dotp += [left[i], right[i]]
    er, ec = pd["eval_row"], pd["eval_col"]
    res = PT.verify(pd["proof_ops"], er[1] + er[2] + ec[1] + ec[2], claims_dotp, num_ops, tr)
    if res is False:
        return False
    claims_ops, claims_dot, rand_ops = res
    res = PT.verify(pd["proof_mem"], [er[0], er[3], ec[0], ec[3]], [], cells, tr)
    if res is False:
        return False
    claims_mem, _none, rand_mem = res
    if len(claims_mem) != 4 or len(claims_ops) != 4 * BATCH or len(claims_dot) != 3 * BATCH:
        return False
    # ---- HashLayerProof::verify (:896-1040)
    hs = proof["hash"]
    e_row_val, e_col_val = hs["eval_derefs"]
    if len(e_row_val) != BATCH or len(e_col_val) != BATCH:
        return False
    evals_derefs = list(e_row_val) + list(e_col_val)
    evals_derefs += [0] * (next_pow2(len(evals_derefs)) - len(evals_derefs))
    ch, claim = n_to_1(evals_derefs, tr)
    tr.append_scalar(claim)
    if not H.eval_verify_plain(gens["derefs"], tr, ch + rand_ops, claim, proof["comm_derefs"], hs["proof_derefs"], msm):
        return False
    e_val = hs["eval_val"]
    for i in range(BATCH):
        if claims_dot[3 * i] != e_row_val[i] or claims_dot[3 * i + 1] != e_col_val[i] or claims_dot[3 * i + 2] != e_val[i]:
            return False
    h_row, h_col = hs["eval_row"], hs["eval_col"]
    evals_ops = list(h_row[0]) + list(h_row[1]) + list(h_col[0]) + list(h_col[1]) + list(e_val)
    evals_ops += [0] * (next_pow2(len(evals_ops)) - len(evals_ops))
    ch, claim = n_to_1(evals_ops, tr)
    tr.append_scalar(claim)
    if not H.eval_verify_plain(gens["ops"], tr, ch + rand_ops, claim, comm["comm_ops"], hs["proof_ops"], msm):
        return False
    ch, claim = n_to_1([h_row[2], h_col[2]], tr)
    tr.append_scalar(claim)
    if not H.eval_verify_plain(gens["mem"], tr, ch + rand_mem, claim, comm["comm_mem"], hs["proof_mem"], msm):
        return False
    B = BATCH
    rows = (claims_mem[0], claims_ops[0:B], claims_ops[B:2 * B], claims_mem[1])
    cols = (claims_mem[2], claims_ops[2 * B:3 * B], claims_ops[3 * B:4 * B], claims_mem[3])
    if not _verify_helper(rand_mem, rows, e_row_val, h_row[0], h_row[1], h_row[2], rx_ext, r_mem_check):
        return False
    return _verify_helper(rand_mem, cols, e_col_val, h_col[0], h_col[1], h_col[2], ry_ext, r_mem_check)


# ------------------------------------------------------------------ shapes --
LABEL = b"r1cs_eval"


def general_mats(num_cons, num_vars, nnz, seed, first_at_origin=False, repeats=False):
    """general matrices: nnz[m] entries of matrix m at seeded positions, values
    nonzero; repeats: every second entry reuses the previous row or column."""
    rng = random.Random(seed)
    mats = []
    for m, n in enumerate(nnz):
        M = []
        for k in range(n):
            r, c = rng.randrange(num_cons), rng.randrange(2 * num_vars)
            if repeats and k % 2 == 1:
                r, c = (M[-1][0], c) if k % 4 == 1 else (r, M[-1][1])
            if first_at_origin and m == 0 and k == 0:
                r, c = 0, 0
            M.append((r, c, rng.randrange(1, R)))
        mats.append(M)
    return mats


def shape(name):
    """-> (mats, num_cons, num_vars, num_inputs) of the issue's shapes a, b, c"""
    if name == "a":
        return general_mats(2, 2, (2, 2, 2), 0x5345_000A), 2, 2, 1
    if name == "b":
        return general_mats(8, 4, (5, 3, 7), 0x5345_000B, first_at_origin=True, repeats=True), 8, 4, 1
    if name == "c":
        return general_mats(32, 4, (9, 16, 12), 0x5345_000C), 32, 4, 1
    raise KeyError(name)


def synthetic(num_cons, num_vars, num_inputs, seed):
    mats, _v, _i = OR.synthetic_r1cs(num_cons, num_vars, num_inputs, seed)
    return [list(M) for M in mats]


def draws(gens, rng):
    """the reference's thread_rng draws of the three openings (derefs, ops, mem)"""
    out = []
    for k in ("derefs", "ops", "mem"):
        n = len(gens[k][0])
        out.append([rng.randrange(1, R) for _ in range(3 + 4 * log2(n))])
    return out


def point(num_cons, num_vars, rng):
    return ([rng.randrange(1, R) for _ in range(log2(num_cons))],
            [rng.randrange(1, R) for _ in range(log2(2 * num_vars))])


def run(mats, num_cons, num_vars, seed, msm=H.py_msm, tr=None, verify_too=True):
    """commit, prove at a seeded point, verify on a fresh transcript"""
    rng = random.Random(seed)
    gens = gens_setup(LABEL, num_cons, num_vars, max(len(M) for M in mats))
    comm, dense = multi_commit(mats, num_cons, num_vars, gens, msm)
    rx, ry = point(num_cons, num_vars, rng)
    evals = multi_evaluate(mats, rx, ry)
    rnd = draws(gens, rng)
    tr = tr or Transcript()
    start = copy.deepcopy(tr)
    proof, aux = prove(dense, rx, ry, evals, gens, tr, rnd, msm)
    if verify_too:
        vt = copy.deepcopy(start)
        assert verify(comm, gens, rx, ry, evals, vt, proof, msm)
        assert vt.state() == tr.state()
    return {"gens": gens, "comm": comm, "dense": dense, "rx": rx, "ry": ry, "evals": evals, "rnd": rnd,
            "proof": proof, "aux": aux, "transcript_end": tr.state()}


# ----------------------------------------------------------------- tampers --
def tamper_list(log_ops, log_cells):
    """every single-field tamper of a proof whose product proofs have log_ops
    and log_cells layers: (name, path) with path into the proof dict"""
    out = []
    for side in ("eval_row", "eval_col"):
        out += [("prod.%s.init" % side, ("prod", side, 0)), ("prod.%s.audit" % side, ("prod", side, 3))]
        out += [("prod.%s.read[%d]" % (side, i), ("prod", side, 1, i)) for i in range(BATCH)]
        out += [("prod.%s.write[%d]" % (side, i), ("prod", side, 2, i)) for i in range(BATCH)]
        out += [("hash.%s.audit_ts" % side, ("hash", side, 2))]
        out += [("hash.%s.addr[%d]" % (side, i), ("hash", side, 0, i)) for i in range(BATCH)]
        out += [("hash.%s.read_ts[%d]" % (side, i), ("hash", side, 1, i)) for i in range(BATCH)]
    for i in range(BATCH):
        out += [("prod.eval_val.left[%d]" % i, ("prod", "eval_val", 0, i)),
                ("prod.eval_val.right[%d]" % i, ("prod", "eval_val", 1, i)),
                ("hash.eval_val[%d]" % i, ("hash", "eval_val", i)),
                ("hash.eval_derefs.row[%d]" % i, ("hash", "eval_derefs", 0, i)),
                ("hash.eval_derefs.col[%d]" % i, ("hash", "eval_derefs", 1, i))]
    for k, layers in (("proof_ops", log_ops), ("proof_mem", log_cells)):
        last = layers - 1
        out.append(("prod.%s coefficient" % k, ("prod", k, "layers", last, "polys", 0, 1))
                   if last >= 1 else ("prod.%s left claim" % k, ("prod", k, "layers", 0, "left", 0)))
    out.append(("comm_derefs[0]", ("comm_derefs", 0)))
    for k in ("proof_derefs", "proof_ops", "proof_mem"):
        out += [("hash.%s.%s" % (k, f), ("hash", k, f, 0)) for f in ("L", "R")]
        out += [("hash.%s.%s" % (k, f), ("hash", k, f)) for f in ("delta", "beta", "z1", "z2")]
    return out


def tampered(proof, path):
    """a deep copy with the element at `path` changed: a scalar gets + 1, a
    point is doubled (still on the curve and in the subgroup)."""
    p = json.loads(json.dumps(_enc_proof(proof)))
    p = _dec_proof(p)
    node = p
    for k in path[:-1]:
        node = node[k]
    v = node[path[-1]]
    node[path[-1]] = (v + 1) % R if isinstance(v, int) else H.O.g1_add(v, v)
    return p


# ----------------------------------------------------------------- fixture --
GOLDEN = os.path.join(os.path.dirname(_HERE), "tests", "golden", "r1cs_eval.json")
SEED_B = 0x5345_0B0B


def _hx(v):
    return "%x" % v


def _hxs(v):
    return [_hx(x) for x in v]


def _ints(v):
    return [int(x, 16) for x in v]


def _pts(v):
    return [H._pt(p) for p in v]


def _enc_pt_proof(pr):
    return {"L": _pts(pr["L"]), "R": _pts(pr["R"]), "delta": H._pt(pr["delta"]), "beta": H._pt(pr["beta"]),
            "z1": _hx(pr["z1"]), "z2": _hx(pr["z2"])}


def _dec_pt_proof(d):
    return {"L": [H.pt_in(p) for p in d["L"]], "R": [H.pt_in(p) for p in d["R"]], "delta": H.pt_in(d["delta"]),
            "beta": H.pt_in(d["beta"]), "z1": int(d["z1"], 16), "z2": int(d["z2"], 16)}


def _enc_pc(pr):
    return {"layers": [{"polys": [_hxs(p) for p in L["polys"]], "left": _hxs(L["left"]), "right": _hxs(L["right"])}
                       for L in pr["layers"]], "dotp": [_hxs(v) for v in pr["dotp"]]}


def _dec_pc(d):
    return {"layers": [{"polys": [_ints(p) for p in L["polys"]], "left": _ints(L["left"]), "right": _ints(L["right"])}
                       for L in d["layers"]], "dotp": tuple(_ints(v) for v in d["dotp"])}


def _enc_proof(p):
    pd, hs = p["prod"], p["hash"]
    e4 = lambda e: [_hx(e[0]), _hxs(e[1]), _hxs(e[2]), _hx(e[3])]  # noqa: E731
    e3 = lambda e: [_hxs(e[0]), _hxs(e[1]), _hx(e[2])]  # noqa: E731
    return {"comm_derefs": _pts(p["comm_derefs"]),
            "prod": {"eval_row": e4(pd["eval_row"]), "eval_col": e4(pd["eval_col"]),
                     "eval_val": [_hxs(pd["eval_val"][0]), _hxs(pd["eval_val"][1])],
                     "proof_ops": _enc_pc(pd["proof_ops"]), "proof_mem": _enc_pc(pd["proof_mem"])},
            "hash": {"eval_row": e3(hs["eval_row"]), "eval_col": e3(hs["eval_col"]), "eval_val": _hxs(hs["eval_val"]),
                     "eval_derefs": [_hxs(hs["eval_derefs"][0]), _hxs(hs["eval_derefs"][1])],
                     "proof_derefs": _enc_pt_proof(hs["proof_derefs"]), "proof_ops": _enc_pt_proof(hs["proof_ops"]),
                     "proof_mem": _enc_pt_proof(hs["proof_mem"])}}


def _dec_proof(d):
    pd, hs = d["prod"], d["hash"]
    d4 = lambda e: [int(e[0], 16), _ints(e[1]), _ints(e[2]), int(e[3], 16)]  # noqa: E731
    d3 = lambda e: [_ints(e[0]), _ints(e[1]), int(e[2], 16)]  # noqa: E731
    return {"comm_derefs": [H.pt_in(p) for p in d["comm_derefs"]],
            "prod": {"eval_row": d4(pd["eval_row"]), "eval_col": d4(pd["eval_col"]),
                     "eval_val": [_ints(pd["eval_val"][0]), _ints(pd["eval_val"][1])],
                     "proof_ops": _dec_pc(pd["proof_ops"]), "proof_mem": _dec_pc(pd["proof_mem"])},
            "hash": {"eval_row": d3(hs["eval_row"]), "eval_col": d3(hs["eval_col"]), "eval_val": _ints(hs["eval_val"]),
                     "eval_derefs": [_ints(hs["eval_derefs"][0]), _ints(hs["eval_derefs"][1])],
                     "proof_derefs": _dec_pt_proof(hs["proof_derefs"]), "proof_ops": _dec_pt_proof(hs["proof_ops"]),
                     "proof_mem": _dec_pt_proof(hs["proof_mem"])}}


def make_fixture():
    """shape (b): every proof element, the challenges, the joint claims and the
    transcript's end state (recorded results only)"""
    mats, nc, nv, ni = shape("b")
    v = run(mats, nc, nv, SEED_B)
    st, sq, idx = v["transcript_end"]
    aux = v["aux"]
    return {"shape": "b", "label": LABEL.decode(), "num_cons": nc, "num_vars": nv, "num_inputs": ni,
            "mats": [[[r, c, _hx(x)] for r, c, x in M] for M in mats],
            "rx": _hxs(v["rx"]), "ry": _hxs(v["ry"]), "evals": _hxs(v["evals"]), "rnd": [_hxs(r) for r in v["rnd"]],
            "comm": {"num_ops": v["comm"]["num_ops"], "num_mem_cells": v["comm"]["num_mem_cells"],
                     "comm_ops": _pts(v["comm"]["comm_ops"]), "comm_mem": _pts(v["comm"]["comm_mem"])},
            "proof": _enc_proof(v["proof"]),
            "r_mem_check": _hxs(aux["r_mem_check"]), "rand_mem": _hxs(aux["rand_mem"]),
            "rand_ops": _hxs(aux["rand_ops"]), "joint_claims": _hxs(aux["joint_claims"]),
            "transcript_end": {"state": _hxs(st), "squeezing": sq, "index": idx}}


def dump_fixture(fx):
    return json.dumps(fx, indent=0) + "\n"


def load_fixture():
    with open(GOLDEN) as f:
        d = json.load(f)
    te = d["transcript_end"]
    return {"raw": d, "mats": [[(r, c, int(x, 16)) for r, c, x in M] for M in d["mats"]],
            "num_cons": d["num_cons"], "num_vars": d["num_vars"], "num_inputs": d["num_inputs"],
            "label": d["label"].encode(), "rx": _ints(d["rx"]), "ry": _ints(d["ry"]), "evals": _ints(d["evals"]),
            "rnd": [_ints(r) for r in d["rnd"]],
            "comm": {"num_ops": d["comm"]["num_ops"], "num_mem_cells": d["comm"]["num_mem_cells"],
                     "comm_ops": [H.pt_in(p) for p in d["comm"]["comm_ops"]],
                     "comm_mem": [H.pt_in(p) for p in d["comm"]["comm_mem"]]},
            "proof": _dec_proof(d["proof"]), "r_mem_check": _ints(d["r_mem_check"]), "rand_mem": _ints(d["rand_mem"]),
            "rand_ops": _ints(d["rand_ops"]), "joint_claims": _ints(d["joint_claims"]),
            "transcript_end": (_ints(te["state"]), te["squeezing"], te["index"])}


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        f.write(dump_fixture(make_fixture()))
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
