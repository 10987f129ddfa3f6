"""SPARK evaluation proofs (csrc/sparse_eval.hip through the C-ABI): the mirror
of R1CSCommitmentGens::setup, R1CSInstance::commit with its decommitment and
R1CSEvalProof::{prove, verify} (r1csinstance.rs:29-53, 313-386;
sparse_mlpoly.rs:1441-1569), over a ``hyrax.FrTranscript``.

    gens = R1CSCommitmentGens.setup(ctx, b"label", num_cons, num_vars, num_inputs, num_nz_entries)
    comm, decomm = commit_decomm(inst, gens)
    evals = inst.evaluate(rx, ry)
    proof = R1CSEvalProof.prove(decomm, rx, ry, evals, gens, FrTranscript(), rnd)
    assert proof.verify(comm, rx, ry, evals, gens, FrTranscript())

``rnd`` = the reference's thread_rng draws of the three openings in proving
order (derefs, ops, mem), ``sizes(...).rnd_len[k]`` Fr each.  This module only
marshals arrays; no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from .encoding import ptr
from .engine import Context, TpstError
from .hyrax import DotProductProof, FrTranscript
from .product_tree import ProductCircuitProof
from .r1cs import R1CSInstance

_E_VERIFY = -5
BATCH = 3


def _fr(a, n=None):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a.reshape(-1, 4) if n is None else a.reshape(n, 4)


def sizes(num_cons: int, num_vars: int, num_nz_entries: int) -> "_lib.R1CSEvalSizes":
    """tpst_r1cs_eval_proof_sizes (host only): the dimensions of the proof."""
    out = _lib.R1CSEvalSizes()
    if _lib.load().tpst_r1cs_eval_proof_sizes(num_cons, num_vars, num_nz_entries, C.byref(out)) != 0:
        raise TpstError("bad dimensions: powers of two, at least 2 entries")
    return out


class R1CSCommitmentGens:
    """R1CSCommitmentGens (r1csinstance.rs:29-53): the three Hyrax generator
    sets of SparseMatPolyCommitmentGens::setup, built once."""

    def __init__(self, ctx: Context, handle, num_cons, num_vars, num_inputs, num_nz_entries):
        self.ctx, self.h = ctx, handle
        self.num_cons, self.num_vars, self.num_inputs = num_cons, num_vars, num_inputs
        self.sizes = sizes(num_cons, num_vars, num_nz_entries)

    @classmethod
    def setup(cls, ctx: Context, label: bytes, num_cons, num_vars, num_inputs, num_nz_entries):
        h = C.c_void_p()
        ctx.check(ctx.lib.tpst_r1cs_gens_setup(ctx.h, bytes(label), len(label), num_cons, num_vars, num_inputs,
                                               num_nz_entries, C.byref(h)), "tpst_r1cs_gens_setup")
        return cls(ctx, h, num_cons, num_vars, num_inputs, num_nz_entries)

    def close(self):
        if self.h:
            self.ctx.lib.tpst_r1cs_gens_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class R1CSCommitment:
    """SparseMatPolyCommitment (sparse_mlpoly.rs:325-332), batch size 3."""
    num_ops: int
    num_mem_cells: int
    comm_ops: np.ndarray  # (ops_rows, 12)
    comm_mem: np.ndarray  # (mem_rows, 12)


class R1CSDecommitment:
    """R1CSDecommitment (r1csinstance.rs:72-74), resident on the device."""

    def __init__(self, ctx: Context, handle, sz):
        self.ctx, self.h, self.sizes = ctx, handle, sz

    def stages(self, rx, ry, r_mem_check=None, rand_ops=None, rand_mem=None):
        """tpst_r1cs_eval_stages: the prover's stages alone -> dict with
        ``derefs`` (8 N, 4), and with r_mem_check ``hash_ops`` (12, N, 4) and
        ``hash_mem`` (4, cells, 4), with rand_ops / rand_mem ``seg`` (23, 4)."""
        sz, ctx = self.sizes, self.ctx
        N, cells = sz.num_ops, sz.num_mem_cells
        z = lambda *s: np.zeros(s + (4,), dtype=np.uint64)  # noqa: E731
        out = {"derefs": z(8 * N)}
        rmc = None if r_mem_check is None else _fr(r_mem_check, 2)
        if rmc is not None:
            out["hash_ops"], out["hash_mem"] = z(12, N), z(4, cells)
        ro = rm = None
        if rand_ops is not None:
            ro, rm = _fr(rand_ops, sz.log_ops), _fr(rand_mem, sz.log_cells)
            out["seg"] = z(23)
        p = lambda a: None if a is None else ptr(a)  # noqa: E731
        rxa, rya = _fr(rx), _fr(ry)
        ctx.check(ctx.lib.tpst_r1cs_eval_stages(ctx.h, self.h, ptr(rxa), ptr(rya), p(rmc), p(ro), p(rm),
                                                ptr(out["derefs"]), p(out.get("hash_ops")), p(out.get("hash_mem")),
                                                p(out.get("seg"))), "tpst_r1cs_eval_stages")
        return out

    def close(self):
        if self.h:
            self.ctx.lib.tpst_r1cs_decomm_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def commit_decomm(inst: R1CSInstance, gens: R1CSCommitmentGens):
    """R1CSInstance::commit (r1csinstance.rs:313-333) -> (R1CSCommitment,
    R1CSDecommitment); the commitment equals ``inst.commit(label)``."""
    ctx, sz = inst.ctx, gens.sizes
    ops = np.zeros((sz.ops_rows, 12), dtype=np.uint64)
    mem = np.zeros((sz.mem_rows, 12), dtype=np.uint64)
    n_ops, n_mem, h = C.c_size_t(0), C.c_size_t(0), C.c_void_p()
    ctx.check(ctx.lib.tpst_r1cs_commit_decomm(ctx.h, inst.h, gens.h, ptr(ops), C.byref(n_ops), ptr(mem),
                                              C.byref(n_mem), C.byref(h)), "tpst_r1cs_commit_decomm")
    return R1CSCommitment(sz.num_ops, sz.num_mem_cells, ops, mem), R1CSDecommitment(ctx, h, sz)


@dataclass
class R1CSEvalProof:
    """R1CSEvalProof { SparseMatPolyEvalProof { comm_derefs,
    PolyEvalNetworkProof { ProductLayerProof, HashLayerProof } } }."""
    comm_derefs: np.ndarray   # (derefs_rows, 12)
    prod_row: np.ndarray      # (8, 4): init, read A B C, write A B C, audit
    prod_col: np.ndarray
    prod_val: np.ndarray      # (2, 3, 4): left, right
    proof_ops: ProductCircuitProof
    proof_mem: ProductCircuitProof
    hash_row: np.ndarray      # (7, 4): ops_addr A B C, read_ts A B C, audit_ts
    hash_col: np.ndarray
    hash_val: np.ndarray      # (3, 4)
    hash_derefs: np.ndarray   # (2, 3, 4): row_ops_val, col_ops_val
    open_derefs: DotProductProof
    open_ops: DotProductProof
    open_mem: DotProductProof

    _SCALARS = ("prod_row", "prod_col", "prod_val", "hash_row", "hash_col", "hash_val", "hash_derefs")

    @staticmethod
    def prove(decomm: R1CSDecommitment, rx, ry, evals, gens: R1CSCommitmentGens, transcript: FrTranscript, rnd):
        """SparseMatPolyEvalProof::prove (sparse_mlpoly.rs:1473-1532)."""
        ctx, sz = decomm.ctx, gens.sizes
        pr = _lib.R1CSEvalProof()
        cd = np.zeros((sz.derefs_rows, 12), dtype=np.uint64)
        po = np.zeros((sz.prod_ops_len, 4), dtype=np.uint64)
        pm = np.zeros((sz.prod_mem_len, 4), dtype=np.uint64)
        if len(rnd) != 3:
            raise TpstError("rnd = the draws of the three openings (derefs, ops, mem)")
        rn = [_fr(r, sz.rnd_len[k]) for k, r in enumerate(rnd)]
        rxa, rya, ev = _fr(rx), _fr(ry), _fr(evals, 3)
        ctx.check(ctx.lib.tpst_r1cs_eval_prove(ctx.h, decomm.h, gens.h, ptr(rxa), ptr(rya), ptr(ev),
                                               ptr(rn[0]), ptr(rn[1]), ptr(rn[2]), C.byref(transcript.t), C.byref(pr),
                                               ptr(cd), ptr(po), ptr(pm)), "tpst_r1cs_eval_prove")
        a = lambda x: np.ctypeslib.as_array(x).copy()  # noqa: E731
        return R1CSEvalProof(
            comm_derefs=cd, prod_row=a(pr.prod_row), prod_col=a(pr.prod_col), prod_val=a(pr.prod_val),
            proof_ops=ProductCircuitProof.unpack(po, sz.log_ops, 4 * BATCH, 2 * BATCH),
            proof_mem=ProductCircuitProof.unpack(pm, sz.log_cells, 4, 0),
            hash_row=a(pr.hash_row), hash_col=a(pr.hash_col), hash_val=a(pr.hash_val), hash_derefs=a(pr.hash_derefs),
            open_derefs=DotProductProof.unpack(pr.proof_derefs), open_ops=DotProductProof.unpack(pr.proof_ops),
            open_mem=DotProductProof.unpack(pr.proof_mem))

    def pack(self) -> "_lib.R1CSEvalProof":
        pr = _lib.R1CSEvalProof()
        for f in self._SCALARS:
            dst = np.ctypeslib.as_array(getattr(pr, f))
            dst[...] = np.asarray(getattr(self, f), dtype=np.uint64).reshape(dst.shape)
        pr.proof_derefs, pr.proof_ops, pr.proof_mem = self.open_derefs.pack(), self.open_ops.pack(), self.open_mem.pack()
        return pr

    def verify(self, comm: R1CSCommitment, rx, ry, evals, gens: R1CSCommitmentGens, transcript: FrTranscript) -> bool:
        """SparseMatPolyEvalProof::verify (sparse_mlpoly.rs:1534-1568); False if
        the proof does not verify, any other failure raises."""
        ctx = gens.ctx
        pr = self.pack()
        cd = np.ascontiguousarray(self.comm_derefs, dtype=np.uint64).reshape(-1, 12)
        co = np.ascontiguousarray(comm.comm_ops, dtype=np.uint64)
        cm = np.ascontiguousarray(comm.comm_mem, dtype=np.uint64)
        rxa, rya, ev = _fr(rx), _fr(ry), _fr(evals, 3)
        po, pm = self.proof_ops.pack(), self.proof_mem.pack()
        rc = ctx.lib.tpst_r1cs_eval_verify(ctx.h, ptr(co), ptr(cm), comm.num_ops, comm.num_mem_cells, gens.h, ptr(rxa),
                                           ptr(rya), ptr(ev), C.byref(transcript.t), C.byref(pr), ptr(cd), ptr(po),
                                           ptr(pm))
        if rc == _E_VERIFY:
            return False
        ctx.check(rc, "tpst_r1cs_eval_verify")
        return True
