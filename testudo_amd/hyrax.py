"""Hyrax evaluation proofs (csrc/hyrax.hip through the C-ABI): the mirror of
PolyEvalProof::{prove, verify, verify_plain} (dense_mlpoly.rs:473-575),
DotProductProofLog (nizk/mod.rs:32-180) and the PoseidonTranscript<Fr> they run
over -- the opening of the commitments of ``engine.dense_commit``.

    gens = HyraxGens.setup(ctx, ell, b"label")
    comm = dense_commit(gens.gens, Z, blinds)
    Zr = dense_evaluate(ctx, Z, r)
    proof, C_Zr = eval_prove(gens, Z, r, Zr, rnd, FrTranscript(), blinds=blinds)
    assert eval_verify(gens, r, C_Zr, comm, FrTranscript(), proof)

The reference's thread_rng draws are the argument ``rnd`` (3 + 4 log2 R Fr:
d, r_delta, r_beta, then 2 log2 R (blind_L, blind_R) pairs).  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from .encoding import ptr
from .engine import Context, Gens, TpstError

_E_VERIFY = -5


def _fr(a, n=None):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a.reshape(-1, 4) if n is None else a.reshape(n, 4)


def _g1(a, n=None):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a.reshape(-1, 12) if n is None else a.reshape(n, 12)


class FrTranscript:
    """PoseidonTranscript<Fr> (poseidon_transcript.rs) with poseidon_params();
    host only."""

    def __init__(self):
        self.lib = _lib.load()
        self.t = _lib.TranscriptFr()
        self.lib.tpst_transcript_fr_init(C.byref(self.t))

    def _ok(self, rc, what):
        if rc != 0:
            raise ValueError("%s: value out of range" % what)

    def append_scalar(self, fr) -> None:
        self._ok(self.lib.tpst_transcript_fr_append_scalar(C.byref(self.t), ptr(_fr(fr, 1))), "append_scalar")

    def append_scalars(self, frs) -> None:
        frs = _fr(frs)
        self._ok(self.lib.tpst_transcript_fr_append_scalars(C.byref(self.t), ptr(frs), len(frs)),
                 "append_scalar_vector")

    def append_point(self, g1) -> None:
        self._ok(self.lib.tpst_transcript_fr_append_point(C.byref(self.t), ptr(_g1(g1, 1))), "append_point")

    def append_bytes(self, data: bytes) -> None:
        self._ok(self.lib.tpst_transcript_fr_append_bytes(C.byref(self.t), bytes(data), len(data)), "append_bytes")

    def challenge_scalar(self) -> np.ndarray:
        out = np.zeros(4, dtype=np.uint64)
        self._ok(self.lib.tpst_transcript_fr_challenge(C.byref(self.t), ptr(out)), "challenge_scalar")
        return out

    def state(self):
        """(state (3, 4) canonical limbs, squeezing, index)"""
        return np.ctypeslib.as_array(self.t.state).copy(), int(self.t.squeezing), int(self.t.index)


class HyraxGens:
    """PolyCommitmentGens::setup(num_vars, label).gens (dense_mlpoly.rs:185-187)
    = DotProductProofGens::new(R, label), R = 2^(num_vars - num_vars/2):
    ``gens`` = the generator set over G[0..R) with h, ``Q`` = G[R]."""

    def __init__(self, ctx: Context, gens: Gens, Q: np.ndarray, num_vars: int = None):
        self.ctx, self.gens, self.Q, self.num_vars = ctx, gens, _g1(Q, 1)[0].copy(), num_vars
        self.n = gens.n

    @classmethod
    def setup(cls, ctx: Context, num_vars: int, label: bytes) -> "HyraxGens":
        return cls.new(ctx, 1 << (num_vars - num_vars // 2), label, num_vars)

    @classmethod
    def new(cls, ctx: Context, n: int, label: bytes, num_vars: int = None) -> "HyraxGens":
        """DotProductProofGens::new(n, label) (nizk/mod.rs:25-28)."""
        G = np.zeros((n + 1, 12), dtype=np.uint64)
        h = np.zeros(12, dtype=np.uint64)
        ctx.check(ctx.lib.tpst_gens_new(ctx.h, n + 1, bytes(label), len(label), ptr(G), ptr(h), None),
                  "tpst_gens_new")
        gens = Gens(ctx, G[:n], h)
        gens.G, gens.h = G[:n].copy(), h
        return cls(ctx, gens, G[n], num_vars)

    def close(self):
        self.gens.close()


@dataclass
class DotProductProof:
    """DotProductProofLog: BulletReductionProof {L_vec, R_vec}, delta, beta, z1, z2."""
    L: np.ndarray      # (rounds, 12)
    R: np.ndarray      # (rounds, 12)
    delta: np.ndarray
    beta: np.ndarray
    z1: np.ndarray
    z2: np.ndarray
    rounds: int = None

    def pack(self) -> "_lib.DotProdProof":
        pr = _lib.DotProdProof()
        k = len(self.L)
        if k > _lib.HYRAX_MAX_ROUNDS:
            raise TpstError("more than %d rounds" % _lib.HYRAX_MAX_ROUNDS)
        pr.rounds = k if self.rounds is None else self.rounds
        w = np.ctypeslib.as_array
        if k:
            w(pr.L)[:k] = _g1(self.L, k)
            w(pr.R)[:k] = _g1(self.R, k)
        w(pr.delta)[:] = _g1(self.delta, 1)[0]
        w(pr.beta)[:] = _g1(self.beta, 1)[0]
        w(pr.z1)[:] = _fr(self.z1, 1)[0]
        w(pr.z2)[:] = _fr(self.z2, 1)[0]
        return pr

    @staticmethod
    def unpack(pr: "_lib.DotProdProof") -> "DotProductProof":
        a = lambda x: np.ctypeslib.as_array(x).copy()  # noqa: E731
        k = pr.rounds
        return DotProductProof(L=a(pr.L)[:k], R=a(pr.R)[:k], delta=a(pr.delta), beta=a(pr.beta), z1=a(pr.z1),
                               z2=a(pr.z2))


def _rnd(rnd, n):
    lg = n.bit_length() - 1
    rnd = _fr(rnd)
    if len(rnd) != 3 + 4 * lg:
        raise TpstError("rnd must hold 3 + 4 log2(n) = %d scalars" % (3 + 4 * lg))
    return rnd


def _verdict(ctx, rc, what) -> bool:
    if rc == _E_VERIFY:
        return False
    ctx.check(rc, what)
    return True


def dotprod_prove(gens: HyraxGens, x, blind_x, a, y, blind_y, rnd, transcript: FrTranscript):
    """DotProductProofLog::prove (nizk/mod.rs:45-125) -> (proof, Cx, Cy)."""
    ctx = gens.ctx
    x, a = _fr(x, gens.n), _fr(a, gens.n)
    pr = _lib.DotProdProof()
    Cx, Cy = np.zeros(12, dtype=np.uint64), np.zeros(12, dtype=np.uint64)
    ctx.check(ctx.lib.tpst_dotprod_prove(ctx.h, gens.gens.handle, ptr(gens.Q), ptr(x), ptr(_fr(blind_x, 1)), ptr(a),
                                         ptr(_fr(y, 1)), ptr(_fr(blind_y, 1)), ptr(_rnd(rnd, gens.n)),
                                         C.byref(transcript.t), C.byref(pr), ptr(Cx), ptr(Cy)), "tpst_dotprod_prove")
    return DotProductProof.unpack(pr), Cx, Cy


def dotprod_verify(gens: HyraxGens, a, Cx, Cy, transcript: FrTranscript, proof: DotProductProof) -> bool:
    """DotProductProofLog::verify (nizk/mod.rs:127-179); False if it rejects."""
    ctx = gens.ctx
    pr = proof.pack()
    rc = ctx.lib.tpst_dotprod_verify(ctx.h, gens.gens.handle, ptr(gens.Q), ptr(_fr(a, gens.n)), ptr(_g1(Cx, 1)),
                                     ptr(_g1(Cy, 1)), C.byref(transcript.t), C.byref(pr))
    return _verdict(ctx, rc, "tpst_dotprod_verify")


def eval_prove(gens: HyraxGens, Z, r, Zr, rnd, transcript: FrTranscript, blinds=None, blind_Zr=None, ell: int = None):
    """PolyEvalProof::prove (dense_mlpoly.rs:482-534) -> (proof, C_Zr').  Z: the
    2^ell evaluations, or (with ``ell``) the address of a device buffer of them
    on the context's device."""
    ctx = gens.ctx
    r = _fr(r)
    pr = _lib.DotProdProof()
    C_Zr = np.zeros(12, dtype=np.uint64)
    bl = None if blinds is None else _fr(blinds, 1 << (len(r) // 2))
    bz = None if blind_Zr is None else _fr(blind_Zr, 1)
    tail = (ptr(bl) if bl is not None else None, ptr(r), ptr(_fr(Zr, 1)), ptr(bz) if bz is not None else None,
            ptr(_rnd(rnd, gens.n)), C.byref(transcript.t), C.byref(pr), ptr(C_Zr))
    if ell is not None:
        if ell != len(r):
            raise TpstError("r must have ell coordinates")
        ctx.check(ctx.lib.tpst_hyrax_eval_prove_dev(ctx.h, gens.gens.handle, ptr(gens.Q), C.c_void_p(int(Z)), ell,
                                                    *tail), "tpst_hyrax_eval_prove_dev")
    else:
        Z = _fr(Z, 1 << len(r))
        ctx.check(ctx.lib.tpst_hyrax_eval_prove(ctx.h, gens.gens.handle, ptr(gens.Q), ptr(Z), len(r), *tail),
                  "tpst_hyrax_eval_prove")
    return DotProductProof.unpack(pr), C_Zr


def eval_verify(gens: HyraxGens, r, C_Zr, comm, transcript: FrTranscript, proof: DotProductProof) -> bool:
    """PolyEvalProof::verify (dense_mlpoly.rs:536-560); comm = the row commitments."""
    ctx = gens.ctx
    r = _fr(r)
    pr = proof.pack()
    rc = ctx.lib.tpst_hyrax_eval_verify(ctx.h, gens.gens.handle, ptr(gens.Q), len(r), ptr(r), ptr(_g1(C_Zr, 1)),
                                        ptr(_g1(comm, 1 << (len(r) // 2))), C.byref(transcript.t), C.byref(pr))
    return _verdict(ctx, rc, "tpst_hyrax_eval_verify")


def eval_verify_plain(gens: HyraxGens, r, Zr, comm, transcript: FrTranscript, proof: DotProductProof) -> bool:
    """PolyEvalProof::verify_plain (dense_mlpoly.rs:562-574)."""
    ctx = gens.ctx
    r = _fr(r)
    pr = proof.pack()
    rc = ctx.lib.tpst_hyrax_eval_verify_plain(ctx.h, gens.gens.handle, ptr(gens.Q), len(r), ptr(r), ptr(_fr(Zr, 1)),
                                              ptr(_g1(comm, 1 << (len(r) // 2))), C.byref(transcript.t),
                                              C.byref(pr))
    return _verdict(ctx, rc, "tpst_hyrax_eval_verify_plain")


def dense_evaluate(ctx: Context, Z, r) -> np.ndarray:
    """DensePolynomial::evaluate (dense_mlpoly.rs:408-414) on the device."""
    r = _fr(r)
    Z = _fr(Z, 1 << len(r))
    out = np.zeros(4, dtype=np.uint64)
    ctx.check(ctx.lib.tpst_dense_evaluate(ctx.h, ptr(Z), len(r), ptr(r), ptr(out)), "tpst_dense_evaluate")
    return out
