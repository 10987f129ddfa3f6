"""arkworks wire format of the sqrt-PST objects (Compress::Yes), through the
host-only C-ABI of csrc/serialize.hip (no GPU needed).

Mirrors the reference's serialisation calls: benches/pst.rs:43-46
(`ck.serialize_with_mode(.., Compress::Yes)` -> commiter_key_size) and
:64-74 (`pst_proof` and `mipp_proof` -> proof_size).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .sqrt_pst import MippProof, _unpack, pack_proof


class SerializationError(ValueError):
    """ark_serialize::SerializationError (InvalidData / NotEnoughSpace)."""


def _lib_():
    return _lib.load()


def _u64p(a):
    return np.ascontiguousarray(a, dtype=np.uint64).ctypes.data_as(C.POINTER(C.c_uint64))


def _write(fn, *args) -> bytes:
    n = C.c_size_t(0)
    if fn(*args, None, 0, C.byref(n)) != 0:
        raise SerializationError("element not serialisable (non-canonical limbs)")
    buf = C.create_string_buffer(n.value)
    if fn(*args, buf, n.value, C.byref(n)) != 0:
        raise SerializationError("serialisation failed")
    return buf.raw[:n.value]


def ser_g1(p) -> bytes:
    out = C.create_string_buffer(48)
    if _lib_().tpst_ser_g1(_u64p(np.asarray(p, dtype=np.uint64).reshape(12)), out) != 0:
        raise SerializationError("bad G1 limbs")
    return out.raw


def ser_g2(p) -> bytes:
    out = C.create_string_buffer(96)
    if _lib_().tpst_ser_g2(_u64p(np.asarray(p, dtype=np.uint64).reshape(24)), out) != 0:
        raise SerializationError("bad G2 limbs")
    return out.raw


def de_g1(b: bytes) -> np.ndarray:
    out = np.zeros(12, dtype=np.uint64)
    if len(b) != 48 or _lib_().tpst_de_g1(b, _u64p(out)) != 0:
        raise SerializationError("invalid G1 encoding")
    return out


def de_g2(b: bytes) -> np.ndarray:
    out = np.zeros(24, dtype=np.uint64)
    if len(b) != 96 or _lib_().tpst_de_g2(b, _u64p(out)) != 0:
        raise SerializationError("invalid G2 encoding")
    return out


def ser_commitment(nv: int, g1) -> bytes:
    """ark-poly-commit Commitment { nv, g_product } (U of sqrt_pst.rs:201)."""
    g1 = np.ascontiguousarray(g1, dtype=np.uint64).reshape(12)
    return _write(_lib_().tpst_ser_commitment, nv, _u64p(g1))


def _proof_struct(pst_proof, mipp: MippProof):
    m_row, m_col = len(pst_proof), len(mipp.comms_t)
    return pack_proof(m_col + m_row, np.zeros(12, dtype=np.uint64), pst_proof, mipp)


def ser_pst_proof(pst_proof, mipp: MippProof) -> bytes:
    pr = _proof_struct(pst_proof, mipp)
    return _write(_lib_().tpst_ser_pst_proof, C.byref(pr))


def ser_mipp_proof(pst_proof, mipp: MippProof) -> bytes:
    pr = _proof_struct(pst_proof, mipp)
    return _write(_lib_().tpst_ser_mipp_proof, C.byref(pr))


def proof_size(pst_proof, mipp: MippProof) -> int:
    """benches/pst.rs:64-74: |pst_proof| + |mipp_proof| compressed."""
    return len(ser_pst_proof(pst_proof, mipp)) + len(ser_mipp_proof(pst_proof, mipp))


def de_open_proof(pst_bytes: bytes, mipp_bytes: bytes):
    """-> (pst_proof (m_row, 24), MippProof); SerializationError if invalid."""
    pr = _lib.OpenProof()
    if _lib_().tpst_de_open_proof(pst_bytes, len(pst_bytes), mipp_bytes, len(mipp_bytes), C.byref(pr)) != 0:
        raise SerializationError("invalid proof encoding")
    _, pst, mipp = _unpack(pr)
    return pst, mipp


def ser_committer_key(nv: int, srs_flat) -> bytes:
    """CommitterKey { nv, powers_of_g, powers_of_h, g, h } of the flat SRS
    (tpst_srs_export layout) -- benches/pst.rs:43-46."""
    flat = np.ascontiguousarray(srs_flat, dtype=np.uint64)
    return _write(_lib_().tpst_ser_committer_key, nv, _u64p(flat), len(flat))


# ---- SPARK objects and batched points (the readers validate on the device) ----
def _first_bad():
    return C.c_size_t(0)


def _de_batch(ctx, b: bytes, size: int, words: int, fn) -> np.ndarray:
    if len(b) % size:
        raise SerializationError("length is not a multiple of %d" % size)
    n = len(b) // size
    out, bad = np.zeros((n, words), dtype=np.uint64), _first_bad()
    rc = fn(ctx.h, bytes(b), n, _u64p(out), C.byref(bad))
    if rc == -1:
        raise SerializationError("invalid point encoding at index %d" % bad.value)
    ctx.check(rc, "batched point decompression")
    return out


def de_g1_batch(ctx, b: bytes) -> np.ndarray:
    """n x 48 compressed bytes -> (n, 12) canonical limbs, Validate::Yes on the device."""
    return _de_batch(ctx, b, 48, 12, _lib_().tpst_de_g1_batch)


def de_g2_batch(ctx, b: bytes) -> np.ndarray:
    """n x 96 compressed bytes -> (n, 24) canonical limbs, Validate::Yes on the device."""
    return _de_batch(ctx, b, 96, 24, _lib_().tpst_de_g2_batch)


def _check_batch(ctx, pts, words: int, fn):
    pts = np.ascontiguousarray(pts, dtype=np.uint64).reshape(-1, words)
    bad = _first_bad()
    rc = fn(ctx.h, _u64p(pts), len(pts), C.byref(bad))
    if rc == -5:
        return bad.value
    ctx.check(rc, "batched point check")
    return None


def check_g1_batch(ctx, pts):
    """Valid::check of (n, 12) affine points on the device: None, or the lowest rejected index."""
    return _check_batch(ctx, pts, 12, _lib_().tpst_g1_check_batch)


def check_g2_batch(ctx, pts):
    """Valid::check of (n, 24) affine points on the device: None, or the lowest rejected index."""
    return _check_batch(ctx, pts, 24, _lib_().tpst_g2_check_batch)


def ser_r1cs_commitment(comm, num_cons: int, num_vars: int, num_inputs: int) -> bytes:
    """R1CSCommitment { num_cons, num_vars, num_inputs, SparseMatPolyCommitment }
    (r1csinstance.rs:55-61) of an ``r1cs_eval.R1CSCommitment``."""
    ops = np.ascontiguousarray(comm.comm_ops, dtype=np.uint64).reshape(-1, 12)
    mem = np.ascontiguousarray(comm.comm_mem, dtype=np.uint64).reshape(-1, 12)
    return _write(_lib_().tpst_ser_r1cs_commitment, num_cons, num_vars, num_inputs, comm.num_ops, comm.num_mem_cells,
                  _u64p(ops), len(ops), _u64p(mem), len(mem))


def de_r1cs_commitment(ctx, b: bytes):
    """-> (r1cs_eval.R1CSCommitment, (num_cons, num_vars, num_inputs))."""
    from .r1cs_eval import R1CSCommitment
    lib, b = _lib_(), bytes(b)
    dims, n_ops, n_mem = (C.c_size_t * 5)(), C.c_size_t(0), C.c_size_t(0)
    if lib.tpst_de_r1cs_commitment(ctx.h, b, len(b), dims, None, 0, C.byref(n_ops), None, 0, C.byref(n_mem)) != 0:
        raise SerializationError("invalid R1CSCommitment encoding")
    ops = np.zeros((n_ops.value, 12), dtype=np.uint64)
    mem = np.zeros((n_mem.value, 12), dtype=np.uint64)
    rc = lib.tpst_de_r1cs_commitment(ctx.h, b, len(b), dims, _u64p(ops), len(ops), C.byref(n_ops), _u64p(mem),
                                     len(mem), C.byref(n_mem))
    if rc == -1:
        raise SerializationError("invalid R1CSCommitment encoding")
    ctx.check(rc, "tpst_de_r1cs_commitment")
    return R1CSCommitment(dims[3], dims[4], ops, mem), (dims[0], dims[1], dims[2])


def ser_r1cs_eval_proof(proof, sizes) -> bytes:
    """R1CSEvalProof (r1csinstance.rs:336-339) of an ``r1cs_eval.R1CSEvalProof``;
    ``sizes`` = ``r1cs_eval.sizes(num_cons, num_vars, num_nz_entries)``."""
    pr = proof.pack()
    cd = np.ascontiguousarray(proof.comm_derefs, dtype=np.uint64).reshape(-1, 12)
    if len(cd) != sizes.derefs_rows:
        raise SerializationError("comm_derefs does not match the sizes")
    po, pm = proof.proof_ops.pack(), proof.proof_mem.pack()
    if len(po) != sizes.prod_ops_len or len(pm) != sizes.prod_mem_len:
        raise SerializationError("product proofs do not match the sizes")
    return _write(_lib_().tpst_ser_r1cs_eval_proof, C.byref(sizes), C.byref(pr), _u64p(cd), _u64p(po), _u64p(pm))


def de_r1cs_eval_proof(ctx, b: bytes, sizes):
    """-> r1cs_eval.R1CSEvalProof; SerializationError if the bytes are not a
    valid proof of these sizes."""
    from .hyrax import DotProductProof
    from .product_tree import ProductCircuitProof
    from .r1cs_eval import BATCH, R1CSEvalProof
    b = bytes(b)
    pr = _lib.R1CSEvalProof()
    cd = np.zeros((sizes.derefs_rows, 12), dtype=np.uint64)
    po = np.zeros((sizes.prod_ops_len, 4), dtype=np.uint64)
    pm = np.zeros((sizes.prod_mem_len, 4), dtype=np.uint64)
    rc = _lib_().tpst_de_r1cs_eval_proof(ctx.h, b, len(b), C.byref(sizes), C.byref(pr), _u64p(cd), _u64p(po),
                                         _u64p(pm))
    if rc == -1:
        raise SerializationError("invalid R1CSEvalProof encoding")
    ctx.check(rc, "tpst_de_r1cs_eval_proof")
    a = lambda x: np.ctypeslib.as_array(x).copy()  # noqa: E731
    return R1CSEvalProof(
        comm_derefs=cd, prod_row=a(pr.prod_row), prod_col=a(pr.prod_col), prod_val=a(pr.prod_val),
        proof_ops=ProductCircuitProof.unpack(po, sizes.log_ops, 4 * BATCH, 2 * BATCH),
        proof_mem=ProductCircuitProof.unpack(pm, sizes.log_cells, 4, 0),
        hash_row=a(pr.hash_row), hash_col=a(pr.hash_col), hash_val=a(pr.hash_val), hash_derefs=a(pr.hash_derefs),
        open_derefs=DotProductProof.unpack(pr.proof_derefs), open_ops=DotProductProof.unpack(pr.proof_ops),
        open_mem=DotProductProof.unpack(pr.proof_mem))


def de_committer_key(ctx, b: bytes):
    """CommitterKey bytes -> (nv, flat SRS in the tpst_srs_export layout, which
    tpst_srs_load takes; the verifier's masks are rebuilt from the powers)."""
    lib, b = _lib_(), bytes(b)
    nv, n = C.c_int(0), C.c_size_t(0)
    if lib.tpst_de_committer_key(ctx.h, b, len(b), C.byref(nv), None, 0, C.byref(n)) != 0:
        raise SerializationError("invalid CommitterKey encoding")
    flat = np.zeros(n.value, dtype=np.uint64)
    rc = lib.tpst_de_committer_key(ctx.h, b, len(b), C.byref(nv), _u64p(flat), len(flat), C.byref(n))
    if rc == -1:
        raise SerializationError("invalid CommitterKey encoding")
    ctx.check(rc, "tpst_de_committer_key")
    return nv.value, flat
