"""SPARK grand products (csrc/product_tree.hip through the C-ABI): the mirror
of ProductCircuitEvalProofBatched::{prove, verify} (product_tree.rs:255-476),
the memory-checking argument of ProductLayerProof::prove
(sparse_mlpoly.rs:1053-1236), over a ``hyrax.FrTranscript``.

    proof, claims_prod, claims_dotp, rand = prove(ctx, polys, (left, right, weight), FrTranscript())
    res = verify(claims_prod, claims_dotp, proof, FrTranscript())
    claims_out, claims_dotp_out, rand = res      # or False if it rejects

``polys`` is P x 2^ell canonical Fr; the dot-product arrays are D x 2^(ell-1)
each (the already split circuits, D even) or None.  The verifier is host only.
No CPU fallback for the prover.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from .encoding import ptr
from .engine import Context, TpstError
from .hyrax import FrTranscript

_E_VERIFY = -5


def _fr3(a, rows, cols):
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(rows, cols, 4)


@dataclass
class ProductCircuitProof:
    """ProductCircuitEvalProofBatched { proof: Vec<LayerProofBatched>,
    claims_dotp }: layer proof i has i rounds."""
    ell: int
    P: int
    D: int
    polys: list              # ell arrays (i, 4, 4): round, coefficient (constant first), limbs
    claims_left: np.ndarray  # (ell, P, 4)
    claims_right: np.ndarray
    claims_dotp: np.ndarray  # (3, D, 4): left, right, weight

    def pack(self) -> np.ndarray:
        """the flat buffer of include/tpst.h: (tpst_prodcircuit_proof_len, 4)"""
        parts = [np.asarray(p, dtype=np.uint64).reshape(-1, 4) for p in self.polys]
        parts += [self.claims_left.reshape(-1, 4), self.claims_right.reshape(-1, 4), self.claims_dotp.reshape(-1, 4)]
        flat = np.ascontiguousarray(np.concatenate(parts), dtype=np.uint64)
        if len(flat) != proof_len(self.ell, self.P, self.D):
            raise TpstError("proof arrays do not match (ell, P, D)")
        return flat

    @staticmethod
    def unpack(flat, ell: int, P: int, D: int) -> "ProductCircuitProof":
        flat = np.ascontiguousarray(flat, dtype=np.uint64).reshape(-1, 4)
        if len(flat) != proof_len(ell, P, D):
            raise TpstError("flat proof does not match (ell, P, D)")
        polys, o = [], 0
        for i in range(ell):
            polys.append(flat[o:o + 4 * i].reshape(i, 4, 4).copy())
            o += 4 * i
        left = flat[o:o + ell * P].reshape(ell, P, 4).copy()
        right = flat[o + ell * P:o + 2 * ell * P].reshape(ell, P, 4).copy()
        return ProductCircuitProof(ell, P, D, polys, left, right,
                                   flat[o + 2 * ell * P:].reshape(3, D, 4).copy())


def proof_len(ell: int, P: int, D: int) -> int:
    """Fr count of the flat proof; raises for dimensions the library rejects."""
    n = _lib.load().tpst_prodcircuit_proof_len(ell, P, D)
    if n == 0:
        raise TpstError("bad dimensions: 1 <= ell <= 30, P >= 1, D even")
    return n


def _outputs(ell, P, D):
    z = lambda n: np.zeros((n, 4), dtype=np.uint64)  # noqa: E731
    return z(proof_len(ell, P, D)), z(P), z(max(D, 1)), z(ell)


def prove(ctx: Context, polys, dotp, transcript: FrTranscript):
    """ProductCircuitEvalProofBatched::prove -> (proof, claims_prod (P, 4),
    claims_dotp (D, 4), rand (ell, 4)).  polys: (P, 2^ell, 4); dotp: None or
    (left, right, weight), each (D, 2^(ell-1), 4)."""
    polys = np.ascontiguousarray(polys, dtype=np.uint64)
    if polys.ndim != 3 or polys.shape[2] != 4:
        raise TpstError("polys must be (P, 2^ell, 4)")
    P, n = polys.shape[0], polys.shape[1]
    ell = n.bit_length() - 1
    if n != 1 << ell:
        raise TpstError("polys must hold 2^ell entries each")
    D = 0 if dotp is None else len(dotp[0])
    lrw = [None] * 3 if not D else [_fr3(v, D, n // 2) for v in dotp]
    proof, cp, cd, rand = _outputs(ell, P, D)
    ctx.check(ctx.lib.tpst_prodcircuit_prove(ctx.h, ell, P, ptr(polys), D, *[None if v is None else ptr(v) for v in lrw],
                                             C.byref(transcript.t), ptr(proof), ptr(cp), ptr(cd) if D else None,
                                             ptr(rand)), "tpst_prodcircuit_prove")
    return ProductCircuitProof.unpack(proof, ell, P, D), cp, cd[:D], rand


def prove_dev(ctx: Context, ell: int, P: int, d_polys: int, D: int, d_left: int, d_right: int, d_weight: int,
              transcript: FrTranscript):
    """prove from device buffers on the context's device (addresses; canonical
    Fr), ordered after the work queued on the library's stream."""
    proof, cp, cd, rand = _outputs(ell, P, D)
    vp = lambda a: C.c_void_p(int(a)) if a else None  # noqa: E731
    ctx.check(ctx.lib.tpst_prodcircuit_prove_dev(ctx.h, ell, P, vp(d_polys), D, vp(d_left), vp(d_right), vp(d_weight),
                                                 C.byref(transcript.t), ptr(proof), ptr(cp), ptr(cd) if D else None,
                                                 ptr(rand)), "tpst_prodcircuit_prove_dev")
    return ProductCircuitProof.unpack(proof, ell, P, D), cp, cd[:D], rand


def verify(claims_prod, claims_dotp, proof: ProductCircuitProof, transcript: FrTranscript):
    """ProductCircuitEvalProofBatched::verify on the host -> (claims_out (P, 4),
    claims_dotp_out (3 D / 2, 4), rand (ell, 4)), or False if it rejects."""
    ell, P, D = proof.ell, proof.P, proof.D
    cp = np.ascontiguousarray(claims_prod, dtype=np.uint64).reshape(P, 4)
    cd = np.ascontiguousarray(claims_dotp, dtype=np.uint64).reshape(D, 4) if D else None
    out, rand = np.zeros((P, 4), dtype=np.uint64), np.zeros((ell, 4), dtype=np.uint64)
    dout = np.zeros((max(3 * D // 2, 1), 4), dtype=np.uint64)
    rc = _lib.load().tpst_prodcircuit_verify(ell, P, D, ptr(cp), ptr(cd) if D else None, ptr(proof.pack()),
                                             C.byref(transcript.t), ptr(out), ptr(dout) if D else None, ptr(rand))
    if rc == _E_VERIFY:
        return False
    if rc != 0:
        raise TpstError("tpst_prodcircuit_verify failed (%d): bad argument" % rc)
    return out, dout[:3 * D // 2], rand
