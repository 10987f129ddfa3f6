"""TEST INFRASTRUCTURE ONLY -- never imported by the product path.

First-principles restatement of the arkworks wire format (ark-serialize 0.4,
Compress::Yes) of R1CSCommitment and R1CSEvalProof, written down from the
reference's struct definitions (every one derives CanonicalSerialize: fields in
declaration order, usize and Vec lengths as u64 LE, tuples field by field, a
G: CurveGroup value as its compressed affine form).  Independent of the C++
writer (csrc/serialize.hip over csrc/wire_spark.h); tests/test_spark_wire.py
compares the two byte for byte.  Point and integer encoders: oracle/py/serialize.py.

  R1CSCommitment { num_cons, num_vars, num_inputs, comm }            r1csinstance.rs:55-61
  SparseMatPolyCommitment { batch_size, num_ops, num_mem_cells,
                            comm_comb_ops, comm_comb_mem }           sparse_mlpoly.rs:325-332
  PolyCommitment { C: Vec<G> }                                       dense_mlpoly.rs:206-208
  R1CSEvalProof { proof: SparseMatPolyEvalProof }                    r1csinstance.rs:336-339
  SparseMatPolyEvalProof { comm_derefs, poly_eval_network_proof }    sparse_mlpoly.rs:1441-1445
  DerefsCommitment { comm_ops_val: PolyCommitment }                  sparse_mlpoly.rs:52-55
  PolyEvalNetworkProof { proof_prod_layer, proof_hash_layer }        sparse_mlpoly.rs:1337-1341
  ProductLayerProof { eval_row: (F, Vec, Vec, F), eval_col, eval_val: (Vec, Vec),
                      proof_mem, proof_ops }                         sparse_mlpoly.rs:1043-1050
  HashLayerProof { eval_row: (Vec, Vec, F), eval_col, eval_val: Vec, eval_derefs: (Vec, Vec),
                   proof_ops, proof_mem: PolyEvalProof, proof_derefs: DerefsEvalProof }  :691-700
  ProductCircuitEvalProofBatched { proof: Vec<LayerProofBatched>, claims_dotp: (Vec, Vec, Vec) }
  LayerProofBatched { proof: SumcheckInstanceProof { polys: Vec<UniPoly { coeffs: Vec }> },
                      claims_prod_left, claims_prod_right }          product_tree.rs:138-170
  PolyEvalProof / DerefsEvalProof -> DotProductProofLog { BulletReductionProof { L_vec, R_vec },
                                                          delta, beta, z1, z2 }  nizk/mod.rs:31-38

The proof and the commitment are the restatement's values (tests/sparse_eval_ref.py): points as
(x, y) or None, scalars as integers.

``python tests/spark_wire_ref.py`` rewrites tests/golden/r1cs_eval_wire.json: the two byte
strings of the proof and commitment of tests/golden/r1cs_eval.json (recorded results only).
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.join(os.path.dirname(_HERE), "oracle", "py")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from serialize import _le, _u64, ser_g1  # noqa: E402  (oracle/py/serialize.py)

GOLDEN = os.path.join(_HERE, "golden", "r1cs_eval_wire.json")
BATCH_SIZE = 3


def _fr(v: int) -> bytes:
    return _le(v, 32)


def _vec_fr(v) -> bytes:
    return _u64(len(v)) + b"".join(_fr(x) for x in v)


def _vec_g1(v) -> bytes:
    return _u64(len(v)) + b"".join(ser_g1(p) for p in v)


def ser_prodcircuit(pc) -> bytes:
    """ProductCircuitEvalProofBatched: layer proof i has i round polynomials of 4 coefficients"""
    out = _u64(len(pc["layers"]))
    for layer in pc["layers"]:
        out += _u64(len(layer["polys"])) + b"".join(_vec_fr(p) for p in layer["polys"])
        out += _vec_fr(layer["left"]) + _vec_fr(layer["right"])
    return out + b"".join(_vec_fr(v) for v in pc["dotp"])


def ser_dotprod(p) -> bytes:
    """PolyEvalProof { DotProductProofLog }"""
    return _vec_g1(p["L"]) + _vec_g1(p["R"]) + ser_g1(p["delta"]) + ser_g1(p["beta"]) + _fr(p["z1"]) + _fr(p["z2"])


def ser_r1cs_eval_proof(p) -> bytes:
    pd, hs = p["prod"], p["hash"]
    out = _vec_g1(p["comm_derefs"])
    for e in (pd["eval_row"], pd["eval_col"]):          # (F, Vec<F>, Vec<F>, F)
        out += _fr(e[0]) + _vec_fr(e[1]) + _vec_fr(e[2]) + _fr(e[3])
    out += _vec_fr(pd["eval_val"][0]) + _vec_fr(pd["eval_val"][1])
    out += ser_prodcircuit(pd["proof_mem"]) + ser_prodcircuit(pd["proof_ops"])      # mem first
    for e in (hs["eval_row"], hs["eval_col"]):          # (Vec<F>, Vec<F>, F)
        out += _vec_fr(e[0]) + _vec_fr(e[1]) + _fr(e[2])
    out += _vec_fr(hs["eval_val"])
    out += _vec_fr(hs["eval_derefs"][0]) + _vec_fr(hs["eval_derefs"][1])
    return out + ser_dotprod(hs["proof_ops"]) + ser_dotprod(hs["proof_mem"]) + ser_dotprod(hs["proof_derefs"])


def ser_r1cs_commitment(num_cons: int, num_vars: int, num_inputs: int, comm) -> bytes:
    out = _u64(num_cons) + _u64(num_vars) + _u64(num_inputs)
    out += _u64(BATCH_SIZE) + _u64(comm["num_ops"]) + _u64(comm["num_mem_cells"])
    return out + _vec_g1(comm["comm_ops"]) + _vec_g1(comm["comm_mem"])


def fixture_bytes():
    """(proof bytes, commitment bytes) of tests/golden/r1cs_eval.json"""
    import sparse_eval_ref as S
    fx = S.load_fixture()
    return (ser_r1cs_eval_proof(fx["proof"]),
            ser_r1cs_commitment(fx["num_cons"], fx["num_vars"], fx["num_inputs"], fx["comm"]))


def make_fixture():
    out = {}
    for name, b in zip(("proof", "commitment"), fixture_bytes()):
        out[name] = {"len": len(b), "sha256": hashlib.sha256(b).hexdigest(), "hex": b.hex()}
    return out


def load_fixture():
    with open(GOLDEN) as f:
        d = json.load(f)
    return {k: bytes.fromhex(v["hex"]) for k, v in d.items()}, d


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        f.write(json.dumps(make_fixture(), indent=0) + "\n")
