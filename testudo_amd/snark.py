"""TestudoSnark / TestudoNizk (csrc/snark.hip through the C-ABI): the mirror of
testudo_snark.rs:22-235 and testudo_nizk.rs:22-157 -- a succinct proof that an
R1CS instance is satisfiable, end to end.

    inst = Instance.new(num_cons, num_vars, num_inputs, A, B, C)
    gens = TestudoSnarkGens.setup(ctx, num_cons, num_vars, num_inputs, num_nz_entries)
    sqrt_pst.srs_setup(ctx, gens.srs_nv, seed)                    # the SRS stays the caller's
    comm, decomm = encode(inst, gens)
    proof = TestudoSnark.prove(comm, decomm, vars_, inputs, gens, FrTranscript(), rnd)
    assert proof.verify(gens, comm, inputs, FrTranscript())
    blob = proof.to_bytes(gens); TestudoSnark.from_bytes(ctx, blob, gens)

``rnd`` = the reference's thread_rng draws of the three openings of the
evaluation proof (derefs, ops, mem), ``gens.sizes.rnd_len[k]`` Fr each.  The
protocol, with the bridge between the caller's PoseidonTranscript<Fr> and the
satisfiability proof's PoseidonTranscript<Fq>, is stated in include/tpst.h.
This module only marshals arrays; no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from .encoding import ptr
from .engine import Context, TpstError
from .hyrax import DotProductProof, FrTranscript
from .instance import Assignment, Instance, padded_dims
from .product_tree import ProductCircuitProof
from .r1cs import R1CSInstance, R1CSProof
from .r1cs_eval import BATCH, R1CSCommitment, R1CSCommitmentGens, R1CSDecommitment, R1CSEvalProof, commit_decomm
from .serialize import SerializationError, _write
from .sqrt_pst import _unpack

_E_ARG, _E_VERIFY = -1, -5
LABEL = b"gens_r1cs_eval"


def _fr(a, n=None):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a.reshape(-1, 4) if n is None else a.reshape(n, 4)


def _values(a):
    """an Assignment or an array of canonical limbs -> (n, 4) limbs"""
    return a.array() if isinstance(a, Assignment) else _fr(a)


def _p(a):
    """NULL for an empty array"""
    return ptr(a) if len(a) else None


class TestudoSnarkGens:
    """TestudoSnarkGens::setup (testudo_snark.rs:41-90): the dimensions padded as
    Instance.new pads them, R1CSCommitmentGens::setup over b"gens_r1cs_eval".
    The sqrt-PST SRS (gens_r1cs_sat) is the caller's ``sqrt_pst.srs_setup`` for
    ``srs_nv`` variables."""

    __test__ = False  # not a pytest class, whatever its name starts with

    def __init__(self, ctx: Context, eval_gens: R1CSCommitmentGens):
        self.ctx, self.gens_r1cs_eval = ctx, eval_gens
        self.num_cons, self.num_vars, self.num_inputs = eval_gens.num_cons, eval_gens.num_vars, eval_gens.num_inputs
        self.sizes = eval_gens.sizes
        self.srs_nv = (self.num_vars.bit_length() - 1 + 1) // 2

    @classmethod
    def setup(cls, ctx: Context, num_cons, num_vars, num_inputs, num_nz_entries):
        num_cons_padded, num_vars_padded = padded_dims(num_cons, num_vars, num_inputs)
        return cls(ctx, R1CSCommitmentGens.setup(ctx, LABEL, num_cons_padded, num_vars_padded, num_inputs,
                                                 num_nz_entries))

    def close(self):
        self.gens_r1cs_eval.close()


@dataclass
class ComputationCommitment:
    """ComputationCommitment (lib.rs:53-56): R1CSCommitment with its dimensions"""
    num_cons: int
    num_vars: int
    num_inputs: int
    comm: R1CSCommitment

    def struct(self):
        """(tpst_r1cs_commitment, the arrays it points into)"""
        ops = np.ascontiguousarray(self.comm.comm_ops, dtype=np.uint64).reshape(-1, 12)
        mem = np.ascontiguousarray(self.comm.comm_mem, dtype=np.uint64).reshape(-1, 12)
        c = _lib.R1CSCommitmentC(self.num_cons, self.num_vars, self.num_inputs, self.comm.num_ops,
                                 self.comm.num_mem_cells, ptr(ops), len(ops), ptr(mem), len(mem))
        return c, (ops, mem)

    def write_to_transcript(self, transcript: FrTranscript) -> None:
        """R1CSCommitment::write_to_transcript (r1csinstance.rs:63-70), host only"""
        c, _keep = self.struct()
        if _lib.load().tpst_r1cs_commitment_absorb(C.byref(c), C.byref(transcript.t)) != 0:
            raise ValueError("commitment rows do not follow from its dimensions, or a point is not canonical")


@dataclass
class ComputationDecommitment:
    """ComputationDecommitment (lib.rs:60-62) with the device instance it was made from"""
    inst: R1CSInstance
    decomm: R1CSDecommitment


def encode(inst, gens: TestudoSnarkGens):
    """TestudoSnark::encode (testudo_snark.rs:100-114): ``inst`` an
    ``instance.Instance`` (loaded onto the generators' device here) or a device
    ``r1cs.R1CSInstance``."""
    dev = inst.to_device(gens.ctx) if isinstance(inst, Instance) else inst
    comm, decomm = commit_decomm(dev, gens.gens_r1cs_eval)
    return (ComputationCommitment(dev.num_cons, dev.num_vars, dev.num_inputs, comm),
            ComputationDecommitment(dev, decomm))


def transcript_append_u64(transcript: FrTranscript, x: int) -> None:
    """PoseidonTranscript::append_u64 (poseidon_transcript.rs:65-67)"""
    if _lib.load().tpst_transcript_fr_append_u64(C.byref(transcript.t), x) != 0:
        raise ValueError("bad transcript state")


def transcript_new_from_state(transcript: FrTranscript, fr) -> None:
    """PoseidonTranscript::new_from_state (poseidon_transcript.rs:50-53)"""
    if _lib.load().tpst_transcript_fr_new_from_state(C.byref(transcript.t), ptr(_fr(fr, 1))) != 0:
        raise ValueError("scalar >= r")


def sat_from_struct(pr) -> R1CSProof:
    """a tpst_r1cs_proof as an ``r1cs.R1CSProof``"""
    a = lambda x: np.ctypeslib.as_array(x).copy()  # noqa: E731
    rxn, ryn = pr.rounds_x, pr.rounds_y
    U, pst, mipp = _unpack(pr.open)
    return R1CSProof(T=a(pr.T), initial_state=a(pr.initial_state), sc_proof_phase1=a(pr.sc1)[:rxn],
                     claims_phase2=a(pr.claims_phase2), sc_proof_phase2=a(pr.sc2)[:ryn],
                     claims_z_abc=a(pr.claims_phase2_z_abc), r_abc=a(pr.r_abc), rx=a(pr.rx)[:rxn], ry=a(pr.ry)[:ryn],
                     transcript_sat_state=a(pr.transcript_sat_state), eval_vars_at_ry=a(pr.eval_vars_at_ry), comm=U,
                     proof_eval_vars_at_ry=pst, mipp_proof=mipp)


def _eval_from_buffers(pr, cd, po, pm, sz) -> R1CSEvalProof:
    a = lambda x: np.ctypeslib.as_array(x).copy()  # noqa: E731
    return R1CSEvalProof(
        comm_derefs=cd, prod_row=a(pr.prod_row), prod_col=a(pr.prod_col), prod_val=a(pr.prod_val),
        proof_ops=ProductCircuitProof.unpack(po, sz.log_ops, 4 * BATCH, 2 * BATCH),
        proof_mem=ProductCircuitProof.unpack(pm, sz.log_cells, 4, 0),
        hash_row=a(pr.hash_row), hash_col=a(pr.hash_col), hash_val=a(pr.hash_val), hash_derefs=a(pr.hash_derefs),
        open_derefs=DotProductProof.unpack(pr.proof_derefs), open_ops=DotProductProof.unpack(pr.proof_ops),
        open_mem=DotProductProof.unpack(pr.proof_mem))


def _buffers(sz):
    return (np.zeros((sz.derefs_rows, 12), dtype=np.uint64), np.zeros((sz.prod_ops_len, 4), dtype=np.uint64),
            np.zeros((sz.prod_mem_len, 4), dtype=np.uint64))


@dataclass
class TestudoSnark:
    """(R1CSProof, R1CSEvalProof, inst_evals); rx and ry live in the R1CSProof"""
    r1cs_sat_proof: R1CSProof
    r1cs_eval_proof: R1CSEvalProof
    inst_evals: np.ndarray  # (3, 4): (A, B, C)(rx, ry)
    __test__ = False

    @staticmethod
    def prove(comm: ComputationCommitment, decomm: ComputationDecommitment, vars_, inputs, gens: TestudoSnarkGens,
              transcript: FrTranscript, rnd) -> "TestudoSnark":
        """TestudoSnark::prove (testudo_snark.rs:120-196): ``vars_`` may hold fewer
        values than the padded instance has variables."""
        ctx, sz, inst = gens.ctx, gens.sizes, decomm.inst
        if len(rnd) != 3:
            raise TpstError("rnd = the draws of the three openings (derefs, ops, mem)")
        rn = [_fr(r, sz.rnd_len[k]) for k, r in enumerate(rnd)]
        v, x = _values(vars_), _values(inputs)
        c, _keep = comm.struct()
        pr = _lib.SnarkProof()
        cd, po, pm = _buffers(sz)
        ctx.check(ctx.lib.tpst_snark_prove(ctx.h, inst.h, C.byref(c), decomm.decomm.h, gens.gens_r1cs_eval.h, _p(v),
                                           len(v), _p(x), ptr(rn[0]), ptr(rn[1]), ptr(rn[2]), C.byref(transcript.t),
                                           C.byref(pr), ptr(cd), ptr(po), ptr(pm)), "tpst_snark_prove")
        return TestudoSnark(sat_from_struct(pr.sat), _eval_from_buffers(pr.eval, cd, po, pm, sz),
                            np.ctypeslib.as_array(pr.inst_evals).copy())

    def pack(self):
        """(tpst_snark_proof, comm_derefs, prod_ops, prod_mem)"""
        pr = _lib.SnarkProof()
        pr.sat = self.r1cs_sat_proof.pack()
        pr.eval = self.r1cs_eval_proof.pack()
        np.ctypeslib.as_array(pr.inst_evals)[:] = _fr(self.inst_evals, 3)
        cd = np.ascontiguousarray(self.r1cs_eval_proof.comm_derefs, dtype=np.uint64).reshape(-1, 12)
        return pr, cd, self.r1cs_eval_proof.proof_ops.pack(), self.r1cs_eval_proof.proof_mem.pack()

    def verify(self, gens: TestudoSnarkGens, comm: ComputationCommitment, inputs, transcript: FrTranscript) -> bool:
        """TestudoSnark::verify (testudo_snark.rs:198-235): needs no instance and no
        decommitment.  False if either proof does not verify; any other failure raises."""
        ctx = gens.ctx
        pr, cd, po, pm = self.pack()
        x = _values(inputs)
        c, _keep = comm.struct()
        rc = ctx.lib.tpst_snark_verify(ctx.h, C.byref(c), gens.gens_r1cs_eval.h, _p(x), len(x), C.byref(transcript.t),
                                       C.byref(pr), ptr(cd), ptr(po), ptr(pm))
        if rc == _E_VERIFY:
            return False
        ctx.check(rc, "tpst_snark_verify")
        return True

    def to_bytes(self, gens: TestudoSnarkGens) -> bytes:
        """R1CSProof || R1CSEvalProof || Ar || Br || Cr, Compress::Yes (this library's layout)"""
        sz = gens.sizes
        pr, cd, po, pm = self.pack()
        if len(cd) != sz.derefs_rows or len(po) != sz.prod_ops_len or len(pm) != sz.prod_mem_len:
            raise SerializationError("the evaluation proof does not match the sizes")
        return _write(_lib.load().tpst_ser_snark_proof, C.byref(sz), C.byref(pr), ptr(cd), ptr(po), ptr(pm))

    @staticmethod
    def from_bytes(ctx: Context, b: bytes, gens: TestudoSnarkGens) -> "TestudoSnark":
        sz, b = gens.sizes, bytes(b)
        pr = _lib.SnarkProof()
        cd, po, pm = _buffers(sz)
        rc = ctx.lib.tpst_de_snark_proof(ctx.h, b, len(b), gens.num_cons, gens.num_vars, C.byref(sz), C.byref(pr),
                                         ptr(cd), ptr(po), ptr(pm))
        if rc == _E_ARG:
            raise SerializationError("invalid SNARK proof encoding")
        ctx.check(rc, "tpst_de_snark_proof")
        return TestudoSnark(sat_from_struct(pr.sat), _eval_from_buffers(pr.eval, cd, po, pm, sz),
                            np.ctypeslib.as_array(pr.inst_evals).copy())


def ser_r1cs_proof(proof: R1CSProof) -> bytes:
    """R1CSProof (r1csproof.rs:32-53), Compress::Yes; host only"""
    pr = proof.pack()
    return _write(_lib.load().tpst_ser_r1cs_proof, C.byref(pr))


def de_r1cs_proof(ctx: Context, b: bytes, num_cons: int, num_vars: int) -> R1CSProof:
    b, pr = bytes(b), _lib.R1CSProof()
    rc = ctx.lib.tpst_de_r1cs_proof(ctx.h, b, len(b), num_cons, num_vars, C.byref(pr))
    if rc == _E_ARG:
        raise SerializationError("invalid R1CSProof encoding")
    ctx.check(rc, "tpst_de_r1cs_proof")
    return sat_from_struct(pr)


@dataclass
class TestudoNizk:
    """TestudoNizk (testudo_nizk.rs:22-157): the satisfiability proof alone; the
    verifier evaluates (A, B, C) at (rx, ry) itself."""
    r1cs_sat_proof: R1CSProof
    __test__ = False

    @staticmethod
    def prove(inst: R1CSInstance, digest: bytes, vars_, inputs, transcript: FrTranscript) -> "TestudoNizk":
        ctx = inst.ctx
        v, x = _values(vars_), _values(inputs)
        pr = _lib.R1CSProof()
        ctx.check(ctx.lib.tpst_nizk_prove(ctx.h, inst.h, bytes(digest), len(digest), _p(v), len(v), _p(x),
                                          C.byref(transcript.t), C.byref(pr)), "tpst_nizk_prove")
        return TestudoNizk(sat_from_struct(pr))

    def verify(self, inst: R1CSInstance, digest: bytes, inputs, transcript: FrTranscript) -> bool:
        ctx = inst.ctx
        pr = self.r1cs_sat_proof.pack()
        x = _values(inputs)
        if len(x) != inst.num_inputs:
            return False
        rc = ctx.lib.tpst_nizk_verify(ctx.h, inst.h, bytes(digest), len(digest), _p(x), C.byref(transcript.t),
                                      C.byref(pr))
        if rc == _E_VERIFY:
            return False
        ctx.check(rc, "tpst_nizk_verify")
        return True

    def to_bytes(self) -> bytes:
        return ser_r1cs_proof(self.r1cs_sat_proof)

    @staticmethod
    def from_bytes(ctx: Context, b: bytes, num_cons: int, num_vars: int) -> "TestudoNizk":
        return TestudoNizk(de_r1cs_proof(ctx, b, num_cons, num_vars))
