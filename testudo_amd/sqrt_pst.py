"""Host-side mirror of Testudo's sqrt-PST surface over libtpst.

Reference: ``src/sqrt_pst.rs:14-265`` (``Polynomial``), ``src/mipp.rs``
(``MippProof``) and ``src/poseidon_transcript.rs`` (``PoseidonTranscript``).
Names and argument meaning follow the reference; every computation runs in
libtpst (HIP on gfx950) -- this module only marshals arrays:

* field elements are numpy ``uint64`` arrays of canonical little-endian limbs
  (Fr: 4, Fq: 6), G1 affine 12 limbs, G2 affine 24, GT 72 (include/tpst.h);
* errors raise ``TpstError``; ``verify`` returns ``False`` on an invalid proof
  where the reference would ``assert!`` (sqrt_pst.rs:250, mipp.rs:308-317).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from .encoding import ptr
from .engine import Context, TpstError


def _torch_ready() -> bool:
    """True when torch is importable with a GPU (stream ordering applies)."""
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


def _u64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a if shape is None else a.reshape(shape)


class PoseidonTranscript:
    """PoseidonTranscript<Fq> with get_bls12377_fq_params (parameters.rs:309-338)."""

    def __init__(self):
        self.lib = _lib.load()
        self.t = _lib.Transcript()
        self.lib.tpst_transcript_init(C.byref(self.t))

    def append_g1(self, p):
        self.lib.tpst_transcript_append_g1(C.byref(self.t), ptr(_u64(p, (12,))))

    def append_gt(self, f):
        self.lib.tpst_transcript_append_gt(C.byref(self.t), ptr(_u64(f, (72,))))

    def append_bytes(self, b: bytes):
        """append_bytes (poseidon_transcript.rs:67-69); ``append`` of a value
        is this over its Compress::No serialisation."""
        b = bytes(b)
        self.lib.tpst_transcript_append_bytes(C.byref(self.t), b, len(b))

    def challenge_scalar(self) -> np.ndarray:
        out = np.zeros(4, dtype=np.uint64)
        self.lib.tpst_transcript_challenge(C.byref(self.t), ptr(out))
        return out

    def state(self) -> np.ndarray:
        return np.ctypeslib.as_array(self.t.state).reshape(18).copy()


@dataclass
class MippProof:
    """mipp.rs:21-28."""
    comms_t: np.ndarray      # (m_col, 2, 72) GT
    comms_u: np.ndarray      # (m_col, 2, 12) G1
    final_a: np.ndarray      # (12,)
    final_h: np.ndarray      # (24,)
    pst_proof_h: np.ndarray  # (m_col, 12) ProofG1


def srs_setup(ctx: Context, nv: int, seed: int):
    """MultilinearPC::setup + trim to nv variables, trapdoor from ``seed``."""
    ctx.check(ctx.lib.tpst_srs_setup(ctx.h, nv, seed), "tpst_srs_setup")


def srs_load(ctx: Context, nv: int, flat: np.ndarray):
    flat = _u64(flat)
    if len(flat) != ctx.lib.tpst_srs_flat_len(nv):
        raise TpstError("SRS flat length mismatch")
    ctx.check(ctx.lib.tpst_srs_load(ctx.h, nv, ptr(flat)), "tpst_srs_load")


def srs_export(ctx: Context, nv: int) -> np.ndarray:
    out = np.zeros(ctx.lib.tpst_srs_flat_len(nv), dtype=np.uint64)
    ctx.check(ctx.lib.tpst_srs_export(ctx.h, ptr(out)), "tpst_srs_export")
    return out


def fr_stream(seed: int, n: int, start: int = 0):
    lib = _lib.load()
    out = np.zeros((n, 4), dtype=np.uint64)
    nxt = lib.tpst_fr_stream(seed, n, start, ptr(out))
    return out, nxt


def _nv(evals) -> int:
    """log2 of the evaluation count; a non-power-of-two vector is an error
    (the reference's MultilinearExtension always has 2^nv evaluations)."""
    nv = len(evals).bit_length() - 1
    if len(evals) == 0 or 1 << nv != len(evals):
        raise TpstError("evaluation count must be a power of two")
    return nv


class MultilinearPC:
    """The ark-poly-commit fork's MultilinearPC<Bls12_377> calls the reference
    makes, against the SRS loaded in ``ctx``.  Points are
    LSB-first (MultilinearPC's order); ``check``/``check_2`` return bool."""

    @staticmethod
    def commit(ctx: Context, evals) -> np.ndarray:
        """sqrt_pst.rs:124 -> g_product (12,)."""
        evals = _u64(evals).reshape(-1, 4)
        nv = _nv(evals)
        out = np.zeros(12, dtype=np.uint64)
        ctx.check(ctx.lib.tpst_mlpc_commit(ctx.h, ptr(evals), nv, ptr(out)), "MultilinearPC::commit")
        return out

    @staticmethod
    def commit_g2(ctx: Context, evals) -> np.ndarray:
        """mipp.rs:133 -> h_product (24,)."""
        evals = _u64(evals).reshape(-1, 4)
        nv = _nv(evals)
        out = np.zeros(24, dtype=np.uint64)
        ctx.check(ctx.lib.tpst_mlpc_commit_g2(ctx.h, ptr(evals), nv, ptr(out)), "MultilinearPC::commit_g2")
        return out

    @staticmethod
    def open(ctx: Context, evals, point) -> np.ndarray:
        """sqrt_pst.rs:225 -> Proof (nv, 24) G2."""
        evals = _u64(evals).reshape(-1, 4)
        nv = _nv(evals)
        point = _u64(point, (nv, 4))
        out = np.zeros((nv, 24), dtype=np.uint64)
        ctx.check(ctx.lib.tpst_mlpc_open(ctx.h, ptr(evals), nv, ptr(point), ptr(out)), "MultilinearPC::open")
        return out

    @staticmethod
    def open_g1(ctx: Context, evals, point) -> np.ndarray:
        """mipp.rs:144 -> ProofG1 (nv, 12)."""
        evals = _u64(evals).reshape(-1, 4)
        nv = _nv(evals)
        point = _u64(point, (nv, 4))
        out = np.zeros((nv, 12), dtype=np.uint64)
        ctx.check(ctx.lib.tpst_mlpc_open_g1(ctx.h, ptr(evals), nv, ptr(point), ptr(out)), "MultilinearPC::open_g1")
        return out

    @staticmethod
    def _chk(ctx, fn, nv, comm, point, value, proofs, what):
        rc = fn(ctx.h, nv, ptr(comm), ptr(point), ptr(value), ptr(proofs))
        if rc == -5:
            return False
        ctx.check(rc, what)
        return True

    @staticmethod
    def check(ctx: Context, comm, point, value, proofs) -> bool:
        """sqrt_pst.rs:261."""
        point = _u64(point).reshape(-1, 4)
        nv = len(point)
        return MultilinearPC._chk(ctx, ctx.lib.tpst_mlpc_check, nv, _u64(comm, (12,)), point, _u64(value, (4,)),
                                  _u64(proofs, (nv, 24)) if nv else np.zeros(24, np.uint64),
                                  "MultilinearPC::check")

    @staticmethod
    def check_2(ctx: Context, comm_h, point, value, proofs) -> bool:
        """mipp.rs:307."""
        point = _u64(point).reshape(-1, 4)
        nv = len(point)
        return MultilinearPC._chk(ctx, ctx.lib.tpst_mlpc_check_2, nv, _u64(comm_h, (24,)), point, _u64(value, (4,)),
                                  _u64(proofs, (nv, 12)) if nv else np.zeros(12, np.uint64), "MultilinearPC::check_2")


class Polynomial:
    """sqrt_pst.rs:14-20 -- 2^n evaluations viewed as 2^m_col rows of 2^m_row."""

    def __init__(self, ctx: Context, handle, n: int, keep=None):
        self.ctx = ctx
        self.h = handle
        self.n = n
        self.m_col = n // 2
        self.m_row = n - self.m_col
        self.odd = n % 2
        self._keep = keep

    @classmethod
    def from_evaluations(cls, ctx: Context, Z: np.ndarray) -> "Polynomial":
        """sqrt_pst.rs:32-75."""
        Z = _u64(Z).reshape(-1, 4)
        n = int(len(Z)).bit_length() - 1
        if 1 << n != len(Z):
            raise TpstError("evaluation count must be a power of two")
        h = C.c_void_p()
        ctx.check(ctx.lib.tpst_poly_from_evaluations(ctx.h, ptr(Z), n, C.byref(h)), "from_evaluations")
        return cls(ctx, h, n)

    @classmethod
    def from_evaluations_cols(cls, ctx: Context, Z: np.ndarray, c0: int, c1: int) -> "Polynomial":
        """This rank's column block [c0, c1) of the strided view only (one 2D
        copy); serves commit_rows / commit_rows_partial for rows in [c0, c1)."""
        Z = _u64(Z).reshape(-1, 4)
        n = int(len(Z)).bit_length() - 1
        if 1 << n != len(Z):
            raise TpstError("evaluation count must be a power of two")
        h = C.c_void_p()
        ctx.check(ctx.lib.tpst_poly_from_evaluations_cols(ctx.h, ptr(Z), n, c0, c1, C.byref(h)),
                  "from_evaluations_cols")
        return cls(ctx, h, n)

    @classmethod
    def from_device(cls, ctx: Context, d_ptr: int, n: int, keep=None) -> "Polynomial":
        h = C.c_void_p()
        if _torch_ready():
            ctx.torch_to_lib()  # d_ptr may be a torch tensor written on torch's stream
        ctx.check(ctx.lib.tpst_poly_from_evaluations_dev(ctx.h, C.c_void_p(d_ptr), n, C.byref(h)),
                  "from_evaluations_dev")
        return cls(ctx, h, n, keep)

    def __del__(self):
        try:
            if self.h:
                self.ctx.lib.tpst_poly_free(self.h)
                self.h = None
        except Exception:
            pass

    def eval(self, point) -> np.ndarray:
        """sqrt_pst.rs:105-115 (computes and caches q on first use)."""
        point = _u64(point, (self.n, 4))
        out = np.zeros(4, dtype=np.uint64)
        self.ctx.check(self.ctx.lib.tpst_poly_eval(self.ctx.h, self.h, ptr(point), ptr(out)), "eval")
        return out

    def commit(self):
        """sqrt_pst.rs:117-149 -> (comm_list (2^m_col, 12), T (72,))."""
        comms = np.zeros((1 << self.m_col, 12), dtype=np.uint64)
        T = np.zeros(72, dtype=np.uint64)
        self.ctx.check(self.ctx.lib.tpst_poly_commit(self.ctx.h, self.h, ptr(comms), ptr(T)), "commit")
        return comms, T

    def commit_rows(self, r0: int, r1: int) -> np.ndarray:
        """Row MSMs of rows [r0, r1) only (one rank's shard of sqrt_pst.rs:121-125)."""
        out = np.zeros((r1 - r0, 12), dtype=np.uint64)
        self.ctx.check(self.ctx.lib.tpst_poly_commit_rows(self.ctx.h, self.h, r0, r1, ptr(out)), "commit_rows")
        return out

    def commit_rows_partial(self, r0: int, r1: int):
        """Rows [r0, r1) of sqrt_pst.rs:121-125 plus their share of the IPP
        (sqrt_pst.rs:128-143) as an unreduced Miller-loop product (72,)."""
        out = np.zeros((r1 - r0, 12), dtype=np.uint64)
        ml = np.zeros(72, dtype=np.uint64)
        self.ctx.check(self.ctx.lib.tpst_poly_commit_rows_partial(self.ctx.h, self.h, r0, r1, ptr(out), ptr(ml)),
                       "commit_rows_partial")
        return out, ml

    def commit_rows_partial_into(self, r0: int, r1: int, out) -> None:
        """commit_rows_partial written into the int64 tensor ``out`` (R * 12 +
        72 words, [comms | Miller partial]): straight from device memory when
        ``out`` is a GPU tensor (the RCCL all-gather buffer), else via host."""
        if out.is_cuda:
            self.ctx.torch_to_lib()  # `out` may come from torch's caching allocator
            self.ctx.check(self.ctx.lib.tpst_poly_commit_rows_partial_dev(self.ctx.h, self.h, r0, r1,
                                                                          C.c_void_p(out.data_ptr())),
                           "commit_rows_partial_dev")
            self.ctx.lib_to_torch()  # the all-gather reads it on torch's stream
            return
        import torch
        cm, ml = self.commit_rows_partial(r0, r1)
        out.copy_(torch.from_numpy(np.concatenate([cm.reshape(-1), ml]).view(np.int64)))

    def get_q_partial(self, point, r0: int, r1: int) -> np.ndarray:
        """Rows [r0, r1)'s share of get_q (sqrt_pst.rs:92-95): (2^m_row, 4) canonical Fr."""
        point = _u64(point, (self.n, 4))
        out = np.zeros((1 << self.m_row, 4), dtype=np.uint64)
        self.ctx.check(self.ctx.lib.tpst_poly_get_q_partial(self.ctx.h, self.h, ptr(point), r0, r1, ptr(out)),
                       "get_q_partial")
        return out

    def get_q_partial_into(self, point, r0: int, r1: int, out) -> None:
        """get_q_partial into the int64 tensor ``out`` (device-side when it is a GPU tensor)."""
        if out.is_cuda:
            point = _u64(point, (self.n, 4))
            self.ctx.torch_to_lib()
            self.ctx.check(self.ctx.lib.tpst_poly_get_q_partial_dev(self.ctx.h, self.h, ptr(point), r0, r1,
                                                                    C.c_void_p(out.data_ptr())),
                           "get_q_partial_dev")
            self.ctx.lib_to_torch()
            return
        import torch
        out.copy_(torch.from_numpy(self.get_q_partial(point, r0, r1).reshape(-1).view(np.int64)))

    @classmethod
    def from_q(cls, ctx: Context, n: int, point, zq, U=None) -> "Polynomial":
        """Opening-only Polynomial from the combined q (an int64 tensor of 2^m_row
        canonical Fr, moved to the device if needed) and optionally the combined
        c_u: serves eval and open; no evaluations resident."""
        import torch
        point = _u64(point, (n, 4))
        if not zq.is_cuda:
            zq = zq.to(torch.device("cuda", ctx.device))
        zq = zq.contiguous()
        ctx.torch_to_lib()  # zq was produced on torch's stream
        Up = ptr(_u64(U, (12,))) if U is not None else None
        h = C.c_void_p()
        ctx.check(ctx.lib.tpst_poly_from_q_dev(ctx.h, n, ptr(point), C.c_void_p(zq.data_ptr()), Up, C.byref(h)),
                  "from_q")
        return cls(ctx, h, n, keep=zq)

    def commit_dev(self, d_comms: int, d_T: int):
        self.ctx.check(self.ctx.lib.tpst_poly_commit_dev(self.ctx.h, self.h, C.c_void_p(d_comms),
                                                         C.c_void_p(d_T)), "commit_dev")

    @classmethod
    def lincomb(cls, polys, w) -> "Polynomial":
        """tpst_poly_lincomb: Z* = sum_j w_j Z_j on the device, a new whole
        Polynomial.  ``polys``: Polynomials of one context and one n; ``w``:
        (B, 4) canonical Fr."""
        polys = list(polys)
        if not polys:
            raise TpstError("lincomb needs at least one polynomial")
        ctx = polys[0].ctx
        w = _u64(w, (len(polys), 4))
        hs = (C.c_void_p * len(polys))(*[p.h for p in polys])
        h = C.c_void_p()
        ctx.check(ctx.lib.tpst_poly_lincomb(ctx.h, hs, len(polys), ptr(w), C.byref(h)), "poly_lincomb")
        return cls(ctx, h, polys[0].n)

    def evaluations(self) -> np.ndarray:
        """tpst_poly_evaluations: the (2^n, 4) canonical Fr of a whole polynomial."""
        out = np.zeros((1 << self.n, 4), dtype=np.uint64)
        self.ctx.check(self.ctx.lib.tpst_poly_evaluations(self.ctx.h, self.h, ptr(out)), "evaluations")
        return out

    def open(self, transcript: PoseidonTranscript, comm_list, point, T):
        """sqrt_pst.rs:168-230 -> (U, pst_proof (m_row, 24), MippProof)."""
        comm_list = _u64(comm_list, (1 << self.m_col, 12))
        point = _u64(point, (self.n, 4))
        T = _u64(T, (72,))
        pr = _lib.OpenProof()
        self.ctx.check(self.ctx.lib.tpst_poly_open(self.ctx.h, self.h, C.byref(transcript.t), ptr(comm_list),
                                                   ptr(point), ptr(T), C.byref(pr)), "open")
        return _unpack(pr)


def open_sharded(ctx: Context, p, transcript: PoseidonTranscript, n: int, comm_list, point, U, exchange):
    """Row-sharded Polynomial::open (tpst_poly_open_sharded):
    every rank calls it with the whole comm_list, the point, c_u and its own
    transcript copy; rank 0 passes its opening handle `p` and gets (U,
    pst_proof, MippProof); the other ranks pass p = None and get None.
    `exchange` is a testudo_amd.distributed.TorchExchange (or any object with
    a ctypes `struct` attribute of type _lib.Exchange)."""
    comm_list = _u64(comm_list, (1 << (n // 2), 12))
    point = _u64(point, (n, 4))
    U = _u64(U, (12,))
    lead = exchange.struct.rank == 0
    pr = _lib.OpenProof() if lead else None
    if _torch_ready():
        ctx.torch_to_lib()  # the exchange arena is a torch allocation
    ctx.check(ctx.lib.tpst_poly_open_sharded(ctx.h, p.h if p is not None else None, C.byref(transcript.t), n,
                                             ptr(comm_list), ptr(point), ptr(U), C.byref(exchange.struct),
                                             C.byref(pr) if lead else None), "open_sharded")
    return _unpack(pr) if lead else None


def _unpack(pr):
    mc, mr = pr.m_col, pr.m_row
    arr = lambda x: np.ctypeslib.as_array(x).copy()  # noqa: E731
    U = arr(pr.U)
    pst = arr(pr.pst_proof)[:mr]
    mipp = MippProof(comms_t=arr(pr.comms_t)[:mc], comms_u=arr(pr.comms_u)[:mc], final_a=arr(pr.final_a),
                     final_h=arr(pr.final_h), pst_proof_h=arr(pr.pst_proof_h)[:mc])
    return U, pst, mipp


def pack_proof(n, U, pst_proof, mipp: MippProof):
    pr = _lib.OpenProof()
    pr.m_col, pr.m_row = n // 2, n - n // 2
    np.ctypeslib.as_array(pr.U)[:] = _u64(U, (12,))
    np.ctypeslib.as_array(pr.pst_proof)[:pr.m_row] = _u64(pst_proof, (pr.m_row, 24))
    np.ctypeslib.as_array(pr.comms_t)[:pr.m_col] = _u64(mipp.comms_t, (pr.m_col, 2, 72))
    np.ctypeslib.as_array(pr.comms_u)[:pr.m_col] = _u64(mipp.comms_u, (pr.m_col, 2, 12))
    np.ctypeslib.as_array(pr.final_a)[:] = _u64(mipp.final_a, (12,))
    np.ctypeslib.as_array(pr.final_h)[:] = _u64(mipp.final_h, (24,))
    np.ctypeslib.as_array(pr.pst_proof_h)[:pr.m_col] = _u64(mipp.pst_proof_h, (pr.m_col, 12))
    return pr


def ipp(ctx: Context, n: int, comms) -> np.ndarray:
    """T = prod e(C_i, h_i) for a full (gathered) commitment list."""
    T = np.zeros(72, dtype=np.uint64)
    ctx.check(ctx.lib.tpst_poly_ipp(ctx.h, n, ptr(_u64(comms, (-1, 12))), ptr(T)), "ipp")
    return T


def gt_final_exp_product_gathered(ctx: Context, gathered, R: int) -> np.ndarray:
    """T = FE(prod of the Miller partials) of an all-gathered (world, R * 12 +
    72) int64 tensor of commit_rows_partial shares, read in place on the device."""
    import torch
    if not gathered.is_cuda:
        gathered = gathered.to(torch.device("cuda", ctx.device))
    gathered = gathered.contiguous()
    ctx.torch_to_lib()  # the all-gather / copy wrote it on torch's stream
    k, w = gathered.shape
    T = np.zeros(72, dtype=np.uint64)
    ctx.check(ctx.lib.tpst_gt_final_exp_product_dev(ctx.h, C.c_void_p(gathered.data_ptr() + 96 * R), 8 * w, k,
                                                    ptr(T)), "gt_final_exp_product_dev")
    return T


def fr_sum(ctx: Context, gathered):
    """Mod-r sum of the rows of a (k, n * 4) int64 tensor of canonical Fr (the C3
    combine): an (n * 4,) int64 tensor on the context's device."""
    import torch
    if not gathered.is_cuda:
        gathered = gathered.to(torch.device("cuda", ctx.device))
    gathered = gathered.contiguous()
    k, w = gathered.shape
    out = torch.empty(w, dtype=torch.int64, device=gathered.device)
    ctx.torch_to_lib()  # gathered (all-gather / stack / contiguous) and out's previous users
    ctx.check(ctx.lib.tpst_fr_sum_dev(ctx.h, C.c_void_p(gathered.data_ptr()), k, w // 4, C.c_void_p(out.data_ptr())),
              "fr_sum_dev")
    ctx.lib_to_torch()
    return out


def cu_partial(ctx: Context, n: int, point, r0: int, r1: int, comms_rows) -> np.ndarray:
    """Rows [r0, r1)'s share of c_u = MSM(comm_list, chi(b)) (sqrt_pst.rs:198), (12,)."""
    point = _u64(point, (n, 4))
    comms_rows = _u64(comms_rows, (r1 - r0, 12)) if r1 > r0 else np.zeros((1, 12), dtype=np.uint64)
    out = np.zeros(12, dtype=np.uint64)
    ctx.check(ctx.lib.tpst_poly_cu_partial(ctx.h, n, ptr(point), r0, r1, ptr(comms_rows), ptr(out)), "cu_partial")
    return out


def g1_sum(ctx: Context, points) -> np.ndarray:
    """Sum of canonical affine G1 points (the c_u combine): an MSM with unit scalars."""
    points = _u64(points).reshape(-1, 12)
    ones = np.zeros((len(points), 4), dtype=np.uint64)
    ones[:, 0] = 1
    return ctx.g1_msm(points, ones)


def gt_final_exp_product(ctx: Context, partials) -> np.ndarray:
    """T = final_exponentiation(prod of the ranks' Miller-loop partials)."""
    partials = _u64(partials, (-1, 72))
    T = np.zeros(72, dtype=np.uint64)
    ctx.check(ctx.lib.tpst_gt_final_exp_product(ctx.h, ptr(partials), len(partials), ptr(T)), "gt_final_exp_product")
    return T


def verify(ctx: Context, transcript: PoseidonTranscript, U, point, v, pst_proof, mipp: MippProof, T) -> bool:
    """Polynomial::verify (sqrt_pst.rs:232-264)."""
    point = _u64(point).reshape(-1, 4)
    n = len(point)
    pr = pack_proof(n, U, pst_proof, mipp)
    rc = ctx.lib.tpst_pst_verify(ctx.h, C.byref(transcript.t), n, ptr(point), ptr(_u64(v, (4,))),
                                 ptr(_u64(T, (72,))), C.byref(pr))
    if rc == -5:
        return False
    ctx.check(rc, "verify")
    return True


def pack_items(items):
    """(transcript, U, point, v, pst_proof, mipp, T) tuples -> (n, the
    tpst_verify_item array, the arrays it points into -- keep them alive for
    the call)."""
    B = len(items)
    n = len(_u64(items[0][2]).reshape(-1, 4))
    arr = (_lib.VerifyItem * B)()
    keep = []
    for j, (tr, U, point, v, pst_proof, mipp, T) in enumerate(items):
        point = _u64(point).reshape(-1, 4)
        if len(point) != n:
            raise TpstError("items of one batch share the number of variables")
        v, T = _u64(v, (4,)), _u64(T, (72,))
        pr = pack_proof(n, U, pst_proof, mipp)
        keep.append((point, v, T, pr, tr))
        arr[j].point, arr[j].v, arr[j].T = ptr(point), ptr(v), ptr(T)
        arr[j].proof = C.pointer(pr)
        arr[j].tr = C.pointer(tr.t)
    return n, arr, keep


def verify_batch(ctx: Context, items, rho=None):
    """tpst_pst_verify_batch: one combined check of many openings against the
    SRS loaded in ``ctx``.  ``items``: a sequence of (transcript, U, point, v,
    pst_proof, mipp, T) -- the arguments of ``verify``, one PoseidonTranscript
    per item.  ``rho``: (B, 4, 2) uint64, the 128-bit multipliers (rho_T,
    rho_2, rho_1, rho_U) of every item; None draws them here with ``secrets``.
    A caller that passes its own must draw them uniformly at random after all
    proofs of the batch are fixed (include/tpst.h).  Returns (all valid, ok)
    with ok a (B,) uint8 array of per-item verdicts; valid items' transcripts
    are advanced as ``verify`` advances them, invalid ones are untouched."""
    items = list(items)
    B = len(items)
    if B == 0:
        return True, np.zeros(0, dtype=np.uint8)
    if rho is None:
        import secrets
        rho = np.zeros((B, 4, 2), dtype=np.uint64)
        for j in range(B):
            for k in range(4):
                x = 0
                while x == 0:
                    x = secrets.randbits(128)
                rho[j, k] = (x & (2**64 - 1), x >> 64)
    rho = _u64(rho, (B, 4, 2))
    n, arr, _keep = pack_items(items)
    ok = np.zeros(B, dtype=np.uint8)
    rc = ctx.lib.tpst_pst_verify_batch(ctx.h, n, C.cast(arr, C.c_void_p), B, ptr(rho),
                                       ok.ctypes.data_as(C.POINTER(C.c_uint8)))
    if rc == -5:
        return False, ok
    ctx.check(rc, "verify_batch")
    return True, ok


def _ptr_array(arrs):
    """u64 arrays -> a ctypes array of their pointers (keep ``arrs`` alive for the call)."""
    return (C.POINTER(C.c_uint64) * len(arrs))(*[ptr(a) for a in arrs])


def g1_lincomb_rows(ctx: Context, lists, w) -> np.ndarray:
    """tpst_g1_lincomb_rows: out[i] = sum_j w_j lists[j][i]; ``lists``: B
    arrays of (C, 12) canonical affine G1, ``w``: (B, 4) Fr -> (C, 12)."""
    lists = [_u64(x).reshape(-1, 12) for x in lists]
    B = len(lists)
    Cn = len(lists[0]) if B else 0
    if any(len(x) != Cn for x in lists):
        raise TpstError("lists of one combination share their length")
    w = _u64(w, (B, 4)) if B else np.zeros((1, 4), dtype=np.uint64)
    out = np.zeros((max(Cn, 1), 12), dtype=np.uint64)
    ctx.check(ctx.lib.tpst_g1_lincomb_rows(ctx.h, _ptr_array(lists), B, Cn, ptr(w), ptr(out)), "g1_lincomb_rows")
    return out[:Cn]


def commit_lincomb(ctx: Context, n: int, comm_lists, Ts, w):
    """tpst_commit_lincomb: (comm_list*, T*) of the combination with weights
    ``w``; ``comm_lists`` or ``Ts`` may be None (its output is then None)."""
    B = len(comm_lists if comm_lists is not None else Ts)
    w = _u64(w, (B, 4))
    cl = [_u64(x, (1 << (n // 2), 12)) for x in comm_lists] if comm_lists is not None else None
    tl = [_u64(x, (72,)) for x in Ts] if Ts is not None else None
    comms = np.zeros((1 << (n // 2), 12), dtype=np.uint64) if cl is not None else None
    T = np.zeros(72, dtype=np.uint64) if tl is not None else None
    ctx.check(ctx.lib.tpst_commit_lincomb(ctx.h, n, _ptr_array(cl) if cl is not None else None,
                                          _ptr_array(tl) if tl is not None else None, B, ptr(w),
                                          ptr(comms) if cl is not None else None,
                                          ptr(T) if tl is not None else None), "commit_lincomb")
    return comms, T


def combine_challenge(transcript: PoseidonTranscript, point, Ts, vs) -> np.ndarray:
    """tpst_pst_combine_challenge: the Fiat-Shamir weights of a combined
    opening, (B, 4) Fr with w_j = rho^j; ``transcript`` absorbs every T_j, the
    point and every v_j and is squeezed once."""
    point = _u64(point).reshape(-1, 4)
    tl = [_u64(x, (72,)) for x in Ts]
    vs = _u64(vs, (len(tl), 4))
    w = np.zeros((len(tl), 4), dtype=np.uint64)
    rc = transcript.lib.tpst_pst_combine_challenge(C.byref(transcript.t), len(point), ptr(point), _ptr_array(tl),
                                                   ptr(vs), len(tl), ptr(w))
    if rc:
        raise TpstError("combine_challenge: rc=%d" % rc)
    return w


def open_combined(polys, commitments, transcript: PoseidonTranscript, point, w=None):
    """tpst_poly_open_combined: one opening for B polynomials at ``point``.
    ``commitments``: their (comm_list, T) pairs.  ``w`` None: every polynomial
    is evaluated and the weights come from ``combine_challenge`` on
    ``transcript`` (the verifier repeats that call).  Returns (w, comm_list*,
    T*, v*, (U, pst_proof, MippProof))."""
    polys = list(polys)
    ctx, n, B = polys[0].ctx, polys[0].n, len(polys)
    point = _u64(point, (n, 4))
    cl = [_u64(c, (1 << (n // 2), 12)) for c, _ in commitments]
    tl = [_u64(T, (72,)) for _, T in commitments]
    if w is None:
        w = combine_challenge(transcript, point, tl, np.stack([p.eval(point) for p in polys]))
    w = _u64(w, (B, 4))
    hs = (C.c_void_p * B)(*[p.h for p in polys])
    comms = np.zeros((1 << (n // 2), 12), dtype=np.uint64)
    T, v = np.zeros(72, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    pr = _lib.OpenProof()
    ctx.check(ctx.lib.tpst_poly_open_combined(ctx.h, hs, _ptr_array(cl), _ptr_array(tl), B, ptr(w),
                                              C.byref(transcript.t), ptr(point), ptr(comms), ptr(T), ptr(v),
                                              C.byref(pr)), "open_combined")
    return w, comms, T, v, _unpack(pr)


def verify_combined(ctx: Context, transcript: PoseidonTranscript, U, point, vs, pst_proof, mipp: MippProof, Ts,
                    w) -> bool:
    """tpst_pst_verify_combined: ``verify`` of one combined opening against
    the B commitments ``Ts`` and claimed values ``vs`` under the weights ``w``."""
    point = _u64(point).reshape(-1, 4)
    n = len(point)
    tl = [_u64(x, (72,)) for x in Ts]
    B = len(tl)
    pr = pack_proof(n, U, pst_proof, mipp)
    rc = ctx.lib.tpst_pst_verify_combined(ctx.h, C.byref(transcript.t), n, ptr(point), ptr(_u64(vs, (B, 4))),
                                          _ptr_array(tl), B, ptr(_u64(w, (B, 4))), C.byref(pr))
    if rc == -5:
        return False
    ctx.check(rc, "verify_combined")
    return True


@dataclass
class MultiOpenProof:
    """The proof of a multi-point opening (include/tpst.h): the sum-check's
    round coefficients, the B values at rho and one opening."""
    rounds: np.ndarray       # (n, 3, 4) Fr: c0, c1, c2 of every round
    u: np.ndarray            # (B, 4) Fr: u_j = f_j(rho)
    U: np.ndarray            # (12,)
    pst_proof: np.ndarray    # (m_row, 24)
    mipp: MippProof


def _claims(claims, n):
    """[(poly_index, point, value)] -> the three arrays of the C-ABI (kept alive by the caller)"""
    claims = list(claims)
    if not claims:
        raise TpstError("a multi-point opening needs at least one claim")
    for j, _, _ in claims:
        if int(j) < 0 or int(j) >= 2**32:
            raise TpstError("claim on a polynomial index out of range")
    idx = np.ascontiguousarray([int(j) for j, _, _ in claims], dtype=np.uint32)
    pts = np.ascontiguousarray(np.stack([_u64(p, (n, 4)) for _, p, _ in claims]))
    vals = np.ascontiguousarray(np.stack([_u64(v, (4,)) for _, _, v in claims]))
    return idx, pts, vals


def _u32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def open_multi(polys, commitments, transcript: PoseidonTranscript, claims):
    """tpst_poly_open_multi: one proof for K claims (poly_index, point, value)
    on B committed polynomials of one size; ``commitments``: their (comm_list,
    T) pairs.  The values are not checked: a wrong one yields a proof that
    ``verify_multi`` rejects.  Returns (MultiOpenProof, rho (n, 4), comm_list*,
    T*, v*); the last three are what ``open_combined`` at rho returns."""
    polys = list(polys)
    ctx, n, B = polys[0].ctx, polys[0].n, len(polys)
    idx, pts, vals = _claims(claims, n)
    cl = [_u64(c, (1 << (n // 2), 12)) for c, _ in commitments]
    tl = [_u64(T, (72,)) for _, T in commitments]
    hs = (C.c_void_p * B)(*[p.h for p in polys])
    rounds = np.zeros((n, 3, 4), dtype=np.uint64)
    u, rho = np.zeros((B, 4), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64)
    comms = np.zeros((1 << (n // 2), 12), dtype=np.uint64)
    T, v = np.zeros(72, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    pr = _lib.OpenProof()
    ctx.check(ctx.lib.tpst_poly_open_multi(ctx.h, hs, _ptr_array(cl), _ptr_array(tl), B, _u32p(idx), ptr(pts),
                                           ptr(vals), len(idx), C.byref(transcript.t), ptr(rounds), ptr(u), ptr(rho),
                                           ptr(comms), ptr(T), ptr(v), C.byref(pr)), "open_multi")
    U, pst_proof, mipp = _unpack(pr)
    return MultiOpenProof(rounds, u, U, pst_proof, mipp), rho, comms, T, v


def multi_reduce(transcript: PoseidonTranscript, n: int, claims, Ts, rounds, u):
    """tpst_pst_multi_reduce (host only): the verifier's statement absorb,
    round checks and final identity.  Returns rho (n, 4) with ``transcript``
    where the combined opening starts, or None (transcript unchanged) when a
    check fails; misuse raises."""
    idx, pts, vals = _claims(claims, n)
    tl = [_u64(x, (72,)) for x in Ts]
    B = len(tl)
    rho = np.zeros((n, 4), dtype=np.uint64)
    rc = transcript.lib.tpst_pst_multi_reduce(C.byref(transcript.t), n, _ptr_array(tl), B, _u32p(idx), ptr(pts),
                                              ptr(vals), len(idx), ptr(_u64(rounds, (n, 3, 4))), ptr(_u64(u, (B, 4))),
                                              ptr(rho))
    if rc == -5:
        return None
    if rc:
        raise TpstError("multi_reduce: rc=%d" % rc)
    return rho


def verify_multi(ctx: Context, transcript: PoseidonTranscript, claims, Ts, proof: MultiOpenProof) -> bool:
    """tpst_pst_verify_multi: the K claims (poly_index, point, value) against
    the B commitments ``Ts`` and one MultiOpenProof."""
    n = len(proof.rounds)
    idx, pts, vals = _claims(claims, n)
    tl = [_u64(x, (72,)) for x in Ts]
    B = len(tl)
    pr = pack_proof(n, proof.U, proof.pst_proof, proof.mipp)
    rc = ctx.lib.tpst_pst_verify_multi(ctx.h, C.byref(transcript.t), n, _ptr_array(tl), B, _u32p(idx), ptr(pts),
                                       ptr(vals), len(idx), ptr(_u64(proof.rounds, (n, 3, 4))),
                                       ptr(_u64(proof.u, (B, 4))), C.byref(pr))
    if rc == -5:
        return False
    ctx.check(rc, "verify_multi")
    return True


def multi_sumcheck_stages(polys, claims, a, rho):
    """tpst_poly_multi_sumcheck_stages (test entry): the device reduction
    alone under the caller's weights ``a`` (K, 4) and challenges ``rho`` (n,
    4); the claims' values are not used.  Returns (sums (n, 2, 4): s_i(0) and
    s_i(2), u (B, 4))."""
    polys = list(polys)
    ctx, n, B = polys[0].ctx, polys[0].n, len(polys)
    idx, pts, _ = _claims(claims, n)
    hs = (C.c_void_p * B)(*[p.h for p in polys])
    sums, u = np.zeros((n, 2, 4), dtype=np.uint64), np.zeros((B, 4), dtype=np.uint64)
    ctx.check(ctx.lib.tpst_poly_multi_sumcheck_stages(ctx.h, hs, B, _u32p(idx), ptr(pts), ptr(_u64(a, (len(idx), 4))),
                                                      len(idx), ptr(_u64(rho, (n, 4))), ptr(sums), ptr(u)),
              "multi_sumcheck_stages")
    return sums, u


@dataclass
class SumcheckOpenProof:
    """The proof of a product sum-check (include/tpst.h): the round
    coefficients, the B values at rho and one opening."""
    rounds: np.ndarray       # (n, D + 1, 4) Fr: the coefficients of every round, constant first
    u: np.ndarray            # (B, 4) Fr: u_j = f_j(rho)
    U: np.ndarray            # (12,)
    pst_proof: np.ndarray    # (m_row, 24)
    mipp: MippProof
    rho: np.ndarray = None   # (n, 4): the prover's challenges; not part of the proof, the verifier derives them


def _sc_terms(terms, has_tau):
    """[(coeff, [indices])] -> (the tpst_sc_term array, the round degree D); the library validates the rest"""
    terms = list(terms)
    if not terms:
        raise TpstError("a product sum-check needs at least one term")
    arr = (_lib.ScTerm * len(terms))()
    for t, (coeff, idx) in enumerate(terms):
        idx = [int(j) for j in idx]
        if len(idx) > 3 or any(j < 0 or j >= 2**32 for j in idx):
            raise TpstError("a term has at most 3 factors, each a polynomial index")
        arr[t].deg = len(idx)
        for k, j in enumerate(idx):
            arr[t].idx[k] = j
        for k, limb in enumerate(_u64(coeff, (4,))):
            arr[t].coeff[k] = int(limb)
    return arr, max(max(len(idx) for _, idx in terms) + (1 if has_tau else 0), 2)


def sumcheck_open(polys, commitments, transcript: PoseidonTranscript, terms, tau=None):
    """tpst_poly_sumcheck_open: proves e0 = sum_x [eq(tau, x)] sum_t c_t prod_i
    f_idx_t[i](x) over B committed polynomials of one size with a sum-check and
    one combined opening.  ``terms``: [(coeff (4,), [indices])], 1..3 indices
    each; ``tau``: (n, 4) or None; ``commitments``: the (comm_list, T) pairs.
    Returns (e0 (4,), SumcheckOpenProof, comm_list*, T*, v*); the last three
    are what ``open_combined`` at the proof's ``rho`` returns."""
    polys = list(polys)
    ctx, n, B = polys[0].ctx, polys[0].n, len(polys)
    arr, D = _sc_terms(terms, tau is not None)
    tau = None if tau is None else _u64(tau, (n, 4))
    cl = [_u64(c, (1 << (n // 2), 12)) for c, _ in commitments]
    tl = [_u64(T, (72,)) for _, T in commitments]
    hs = (C.c_void_p * B)(*[p.h for p in polys])
    e0, rounds = np.zeros(4, dtype=np.uint64), np.zeros((n, min(D, 3) + 1, 4), dtype=np.uint64)
    u, rho = np.zeros((B, 4), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64)
    comms = np.zeros((1 << (n // 2), 12), dtype=np.uint64)
    T, v = np.zeros(72, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    pr = _lib.OpenProof()
    ctx.check(ctx.lib.tpst_poly_sumcheck_open(ctx.h, hs, _ptr_array(cl), _ptr_array(tl), B, C.addressof(arr), len(arr),
                                              None if tau is None else ptr(tau), C.addressof(transcript.t), ptr(e0),
                                              ptr(rounds), ptr(u), ptr(rho), ptr(comms), ptr(T), ptr(v), C.byref(pr)),
              "sumcheck_open")
    U, pst_proof, mipp = _unpack(pr)
    return e0, SumcheckOpenProof(rounds, u, U, pst_proof, mipp, rho), comms, T, v


def sumcheck_reduce(transcript: PoseidonTranscript, n: int, terms, tau, Ts, e0, rounds, u):
    """tpst_pst_sumcheck_reduce (host only): the verifier's statement absorb,
    round checks and final identity on the claimed ``e0``.  Returns rho (n, 4)
    with ``transcript`` where the combined opening starts, or None (transcript
    unchanged) when a check fails; misuse raises."""
    arr, D = _sc_terms(terms, tau is not None)
    tau = None if tau is None else _u64(tau, (n, 4))
    tl = [_u64(x, (72,)) for x in Ts]
    B = len(tl)
    rho = np.zeros((n, 4), dtype=np.uint64)
    rc = transcript.lib.tpst_pst_sumcheck_reduce(C.addressof(transcript.t), n, _ptr_array(tl), B, C.addressof(arr),
                                                 len(arr), None if tau is None else ptr(tau), ptr(_u64(e0, (4,))),
                                                 ptr(_u64(rounds, (n, min(D, 3) + 1, 4))), ptr(_u64(u, (B, 4))),
                                                 ptr(rho))
    if rc == -5:
        return None
    if rc:
        raise TpstError("sumcheck_reduce: rc=%d" % rc)
    return rho


def verify_sumcheck(ctx: Context, transcript: PoseidonTranscript, terms, tau, Ts, e0,
                    proof: SumcheckOpenProof) -> bool:
    """tpst_pst_verify_sumcheck: the claim ``e0`` on the terms (and ``tau``)
    against the B commitments ``Ts`` and one SumcheckOpenProof."""
    n = len(proof.rounds)
    arr, D = _sc_terms(terms, tau is not None)
    tau = None if tau is None else _u64(tau, (n, 4))
    tl = [_u64(x, (72,)) for x in Ts]
    B = len(tl)
    pr = pack_proof(n, proof.U, proof.pst_proof, proof.mipp)
    rc = ctx.lib.tpst_pst_verify_sumcheck(ctx.h, C.addressof(transcript.t), n, _ptr_array(tl), B, C.addressof(arr),
                                          len(arr), None if tau is None else ptr(tau), ptr(_u64(e0, (4,))),
                                          ptr(_u64(proof.rounds, (n, min(D, 3) + 1, 4))), ptr(_u64(proof.u, (B, 4))),
                                          C.byref(pr))
    if rc == -5:
        return False
    ctx.check(rc, "verify_sumcheck")
    return True


def sumcheck_stages(polys, terms, tau, rho):
    """tpst_poly_sumcheck_stages (test entry): the device rounds alone on the
    caller's challenges ``rho`` (n, 4).  Returns (sums (n, D + 1, 4):
    s_i(0..D), u (B, 4))."""
    polys = list(polys)
    ctx, n, B = polys[0].ctx, polys[0].n, len(polys)
    arr, D = _sc_terms(terms, tau is not None)
    tau = None if tau is None else _u64(tau, (n, 4))
    hs = (C.c_void_p * B)(*[p.h for p in polys])
    sums, u = np.zeros((n, min(D, 3) + 1, 4), dtype=np.uint64), np.zeros((B, 4), dtype=np.uint64)
    ctx.check(ctx.lib.tpst_poly_sumcheck_stages(ctx.h, hs, B, C.addressof(arr), len(arr),
                                                None if tau is None else ptr(tau), ptr(_u64(rho, (n, 4))), ptr(sums),
                                                ptr(u)), "sumcheck_stages")
    return sums, u


@dataclass
class LookupProof:
    """The proof of a lookup argument (include/tpst.h): the helper
    commitments, the product sum-check, the values at the 1/2 point, the
    multi-point reduction and one opening."""
    T_m: np.ndarray          # (72,) GT
    T_h: np.ndarray          # (L + 1, 72) GT: T_{h_0}..T_{h_{L-1}}, T_{h_t}
    rounds: np.ndarray       # (n, 4, 4) Fr: the sum-check's coefficients, constant first
    u: np.ndarray            # (2L + 3, 4) Fr: u_j = f_j(rho)
    s: np.ndarray            # (L + 1, 4) Fr: s_0..s_{L-1}, s_t
    mp_rounds: np.ndarray    # (n, 3, 4) Fr: the multi-point reduction's coefficients
    mp_u: np.ndarray         # (2L + 3, 4) Fr: its final values f_j(rho')
    U: np.ndarray            # (12,)
    pst_proof: np.ndarray    # (m_row, 24)
    mipp: MippProof
    rho: np.ndarray = None   # (n, 4): rho', the combined opening's point; not part of the proof

    def T_helpers(self) -> np.ndarray:
        """T_m, then every T_h: (L + 2, 72), the C-ABI's layout"""
        return np.ascontiguousarray(np.concatenate([_u64(self.T_m, (1, 72)), _u64(self.T_h).reshape(-1, 72)]))


def range_table(ctx: Context, n: int) -> Polynomial:
    """The table of a range check: t(y) = y for y < 2^n."""
    Z = np.zeros((1 << n, 4), dtype=np.uint64)
    Z[:, 0] = np.arange(1 << n, dtype=np.uint64)
    return Polynomial.from_evaluations(ctx, Z)


def lookup_open(witnesses, table: Polynomial, commitments, transcript: PoseidonTranscript):
    """tpst_poly_lookup_open: proves that every entry of every witness
    polynomial occurs in ``table``, with one opening.  ``commitments``: the
    (comm_list, T) pairs of the witnesses, then of the table.  A witness entry
    that is not in the table raises.  Returns (LookupProof, comm_list*, T*,
    v*); the last three are what the combined opening at the proof's ``rho``
    returns."""
    wits = list(witnesses)
    ctx, n, L = table.ctx, table.n, len(wits)
    B = 2 * L + 3
    cl = [_u64(c, (1 << (n // 2), 12)) for c, _ in commitments]
    tl = [_u64(T, (72,)) for _, T in commitments]
    if len(cl) != L + 1:
        raise TpstError("lookup_open: one commitment per witness, then the table's")
    hs = (C.c_void_p * max(L, 1))(*[p.h for p in wits])
    Th = np.zeros((L + 2, 72), dtype=np.uint64)
    rounds, mp_rounds = np.zeros((n, 4, 4), dtype=np.uint64), np.zeros((n, 3, 4), dtype=np.uint64)
    u, mp_u = np.zeros((B, 4), dtype=np.uint64), np.zeros((B, 4), dtype=np.uint64)
    s, rho = np.zeros((L + 1, 4), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64)
    comms = np.zeros((1 << (n // 2), 12), dtype=np.uint64)
    T, v = np.zeros(72, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    pr = _lib.OpenProof()
    ctx.check(ctx.lib.tpst_poly_lookup_open(ctx.h, hs, L, table.h, _ptr_array(cl), _ptr_array(tl),
                                            C.addressof(transcript.t), ptr(Th), ptr(rounds), ptr(u), ptr(s),
                                            ptr(mp_rounds), ptr(mp_u), ptr(rho), ptr(comms), ptr(T), ptr(v),
                                            C.byref(pr)), "lookup_open")
    U, pst_proof, mipp = _unpack(pr)
    return LookupProof(Th[0].copy(), Th[1:].copy(), rounds, u, s, mp_rounds, mp_u, U, pst_proof, mipp, rho), comms, T, v


def _lookup_args(n, Ts, proof: LookupProof):
    tl = [_u64(x, (72,)) for x in Ts]
    L = len(tl) - 1
    B = 2 * L + 3
    return tl, L, (proof.T_helpers().reshape(L + 2, 72), _u64(proof.rounds, (n, 4, 4)), _u64(proof.u, (B, 4)),
                   _u64(proof.s, (L + 1, 4)), _u64(proof.mp_rounds, (n, 3, 4)), _u64(proof.mp_u, (B, 4)))


def lookup_reduce(transcript: PoseidonTranscript, n: int, Ts, proof: LookupProof):
    """tpst_pst_lookup_reduce (host only): the verifier's transcript steps,
    the product sum-check, sum_l s_l = s_t and the multi-point reduction.
    ``Ts``: the T of every witness, then the table's.  Returns rho' (n, 4) with
    ``transcript`` where the combined opening's challenge starts, or None
    (transcript unchanged) when a check fails; misuse raises."""
    tl, L, arrs = _lookup_args(n, Ts, proof)
    rho = np.zeros((n, 4), dtype=np.uint64)
    rc = transcript.lib.tpst_pst_lookup_reduce(C.addressof(transcript.t), n, L, _ptr_array(tl),
                                               *[ptr(a) for a in arrs], ptr(rho))
    if rc == -5:
        return None
    if rc:
        raise TpstError("lookup_reduce: rc=%d" % rc)
    return rho


def verify_lookup(ctx: Context, transcript: PoseidonTranscript, Ts, proof: LookupProof) -> bool:
    """tpst_pst_verify_lookup: every entry of the polynomials behind
    ``Ts[:-1]`` occurs in the table behind ``Ts[-1]``."""
    n = len(proof.rounds)
    tl, L, arrs = _lookup_args(n, Ts, proof)
    pr = pack_proof(n, proof.U, proof.pst_proof, proof.mipp)
    rc = ctx.lib.tpst_pst_verify_lookup(ctx.h, C.addressof(transcript.t), n, L, _ptr_array(tl),
                                        *[ptr(a) for a in arrs], C.byref(pr))
    if rc == -5:
        return False
    ctx.check(rc, "verify_lookup")
    return True


def lookup_stages(witnesses, table: Polynomial, beta):
    """tpst_poly_lookup_stages (test entry): the device stages alone on the
    caller's ``beta`` (4,).  Returns (m (2^n, 4), h (L + 1, 2^n, 4): h_0..
    h_{L-1}, h_t, s (L + 1, 4))."""
    wits = list(witnesses)
    ctx, n, L = table.ctx, table.n, len(wits)
    hs = (C.c_void_p * max(L, 1))(*[p.h for p in wits])
    m = np.zeros((1 << n, 4), dtype=np.uint64)
    h = np.zeros((L + 1, 1 << n, 4), dtype=np.uint64)
    s = np.zeros((L + 1, 4), dtype=np.uint64)
    ctx.check(ctx.lib.tpst_poly_lookup_stages(ctx.h, hs, L, table.h, ptr(_u64(beta, (4,))), ptr(m), ptr(h), ptr(s)),
              "lookup_stages")
    return m, h, s


def g1_msm_partial_into(ctx: Context, d_bases: int, d_scalars: int, i0: int, i1: int, out) -> None:
    """Points [i0, i1) of a device-resident MSM (Montgomery bases, canonical Fr
    scalars) summed into the int64 tensor ``out`` (24 words, raw XYZZ; a host
    tensor -- the gloo path -- is filled through a device staging tensor)."""
    import torch
    dst = out if out.is_cuda else torch.empty(24, dtype=torch.int64, device=torch.device("cuda", ctx.device))
    ctx.torch_to_lib()
    ctx.g1_msm_xyzz_dev(d_bases + 96 * i0, d_scalars + 32 * i0, i1 - i0, dst.data_ptr())
    ctx.lib_to_torch()
    if dst is not out:
        out.copy_(dst.cpu())


def g1_xyzz_combine(ctx: Context, gathered):
    """Sum of a gathered (k, 24) int64 tensor of XYZZ shares on the device ->
    (12,) canonical affine G1 as an int64 tensor."""
    import torch
    if not gathered.is_cuda:
        gathered = gathered.to(torch.device("cuda", ctx.device))
    gathered = gathered.contiguous()
    out = torch.empty(12, dtype=torch.int64, device=gathered.device)
    ctx.torch_to_lib()
    ctx.g1_xyzz_sum_dev(gathered.data_ptr(), gathered.shape[0], 8 * gathered.shape[1], out.data_ptr())
    ctx.lib_to_torch()
    return out
