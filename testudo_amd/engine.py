"""Python handle on a libtpst context (one per GPU / process).

Thin, typed wrappers over the C-ABI primitives; every call goes to the HIP
library.  Errors raise ``TpstError`` with the library's message.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .encoding import ptr


class TpstError(RuntimeError):
    pass


class Context:
    def __init__(self, device: int = 0):
        self.lib = _lib.load()
        h = C.c_void_p()
        rc = self.lib.tpst_create(device, C.byref(h))
        if rc != 0:
            raise TpstError("tpst_create(%d) failed: %d" % (device, rc))
        self.h = h
        self.device = device

    def close(self):
        if self.h:
            self.lib.tpst_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc: int, what: str):
        if rc != 0:
            msg = self.lib.tpst_last_error(self.h)
            raise TpstError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else ""))

    # ------------------------------------------------------------ MSM ----
    def g1_msm(self, bases: np.ndarray, scalars: np.ndarray) -> np.ndarray:
        bases = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, 12)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros(12, dtype=np.uint64)
        self.check(self.lib.tpst_g1_msm(self.h, ptr(bases), len(bases), ptr(scalars), len(scalars), ptr(out)),
                   "tpst_g1_msm")
        return out

    def g2_msm(self, bases: np.ndarray, scalars: np.ndarray) -> np.ndarray:
        bases = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, 24)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros(24, dtype=np.uint64)
        self.check(self.lib.tpst_g2_msm(self.h, ptr(bases), len(bases), ptr(scalars), len(scalars), ptr(out)),
                   "tpst_g2_msm")
        return out

    def multiexp(self, bases: np.ndarray, scalars: np.ndarray, g2: bool = False) -> np.ndarray:
        """mipp.rs:385-394 `multiexponentiation`: raises on a length mismatch
        (the reference's Err(InvalidIPVectorLength))."""
        w = 24 if g2 else 12
        bases = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, w)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros(w, dtype=np.uint64)
        fn = self.lib.tpst_g2_multiexp if g2 else self.lib.tpst_g1_multiexp
        self.check(fn(self.h, ptr(bases), len(bases), ptr(scalars), len(scalars), ptr(out)), "multiexponentiation")
        return out

    def msm_fixed(self, bases: np.ndarray, scalars: np.ndarray, L: int = 0, D: int = 0, g2: bool = False):
        """Grouped fixed-base MSM (include/tpst.h tpst_g*_msm_fixed): (L/D, 12|24)."""
        w = 24 if g2 else 12
        bases = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, w)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        n = len(bases)
        L = L or n
        D = D or L
        out = np.zeros((L // D, w), dtype=np.uint64)
        fn = self.lib.tpst_g2_msm_fixed if g2 else self.lib.tpst_g1_msm_fixed
        self.check(fn(self.h, ptr(bases), n, ptr(scalars), L, D, ptr(out)), "tpst_msm_fixed")
        return out

    def multi_pairing(self, g1: np.ndarray, g2: np.ndarray) -> np.ndarray:
        g1 = np.ascontiguousarray(g1, dtype=np.uint64).reshape(-1, 12)
        g2 = np.ascontiguousarray(g2, dtype=np.uint64).reshape(-1, 24)
        assert len(g1) == len(g2)
        out = np.zeros(72, dtype=np.uint64)
        self.check(self.lib.tpst_multi_pairing(self.h, ptr(g1), ptr(g2), len(g1), ptr(out)), "tpst_multi_pairing")
        return out

    def g1_mul_generator(self, scalars: np.ndarray) -> np.ndarray:
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros((len(scalars), 12), dtype=np.uint64)
        self.check(self.lib.tpst_g1_mul_generator(self.h, ptr(scalars), len(scalars), ptr(out)),
                   "tpst_g1_mul_generator")
        return out

    def g2_mul_generator(self, scalars: np.ndarray) -> np.ndarray:
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros((len(scalars), 24), dtype=np.uint64)
        self.check(self.lib.tpst_g2_mul_generator(self.h, ptr(scalars), len(scalars), ptr(out)),
                   "tpst_g2_mul_generator")
        return out

    def _lincomb(self, fn, w, P, s, Q, t, what):
        P = np.ascontiguousarray(P, dtype=np.uint64).reshape(-1, w)
        s = np.ascontiguousarray(s, dtype=np.uint64).reshape(-1, 4)
        if (Q is None) != (t is None) or len(s) != len(P):
            raise TpstError(what + ": Q and t go together; one scalar per point")
        if Q is not None:
            Q = np.ascontiguousarray(Q, dtype=np.uint64).reshape(-1, w)
            t = np.ascontiguousarray(t, dtype=np.uint64).reshape(-1, 4)
            if len(Q) != len(P) or len(t) != len(P):
                raise TpstError(what + ": length mismatch")
        out = np.zeros((len(P), w), dtype=np.uint64)
        self.check(fn(self.h, ptr(P), ptr(s), None if Q is None else ptr(Q), None if t is None else ptr(t), len(P),
                      ptr(out)), what)
        return out

    def g1_lincomb_batch(self, P, s, Q=None, t=None) -> np.ndarray:
        """out[i] = s_i P_i + t_i Q_i on G1 (tpst_g1_lincomb_batch); Q = t = None: s_i P_i.  (n, 12)."""
        return self._lincomb(self.lib.tpst_g1_lincomb_batch, 12, P, s, Q, t, "tpst_g1_lincomb_batch")

    def g2_lincomb_batch(self, P, s, Q=None, t=None) -> np.ndarray:
        """out[i] = s_i P_i + t_i Q_i on G2 (tpst_g2_lincomb_batch).  (n, 24)."""
        return self._lincomb(self.lib.tpst_g2_lincomb_batch, 24, P, s, Q, t, "tpst_g2_lincomb_batch")

    # ------------------------------------------------------- profiling ---
    STAGES = ("decompose", "sort", "bounds", "bucket_acc", "reduce", "combine", "batch_sort",
              # sqrt-PST stages under the reference's Timer labels (sqrt_pst.rs:33-262), device spans
              "build_q", "sqrt_commit", "comm_list", "ipp", "sqrt_open", "msm", "mipp_prove", "pst_open",
              # tpst_r1cs_evaluate: the two eq tables; the reduction kernel and its partial sum
              "r1cs_eval_eq", "r1cs_eval",
              # tpst_hyrax_eval_prove: the L / R eq tables; bound; the dot-product proof (host work included)
              "hyrax_eq", "hyrax_bound", "hyrax_rounds",
              "prodtree_build", "prodtree_rounds", "prodtree_round0", "prodtree_round1",
              # tpst_r1cs_eval_prove: k_deref; k_hash_ops; k_hash_mem; k_seg_eval (both groups, with their sums)
              "sparse_deref", "sparse_hash_ops", "sparse_hash_mem", "sparse_seg_eval",
              # point_codec.hip: batched point decompression / validation
              "point_codec",
              # k_lincomb2 launches; tpst_pst_verify_batch's multi-pairing call and its GT powers
              "lincomb", "verify_batch_pairing", "verify_batch_gt_pow",
              # poly_lincomb.hip: k_fr_lincomb; k_g1_lincomb_rows and the sum of its chains
              "fr_lincomb", "lincomb_rows",
              # poly_multi.hip: round 0, round 1, and the later rounds with the closing bind of the multi-point reduction
              "multi_round0", "multi_round1", "multi_rounds",
              # poly_sumcheck.hip: round 0, round 1, and the later rounds with the closing bind of the product sum-check
              "sumcheck_round0", "sumcheck_round1", "sumcheck_rounds",
              # lookup.hip: the table's index; probes and counts; the batched inversions; the sums of the h tables
              "lookup_index", "lookup_count", "lookup_inverse", "lookup_sums")

    def profile(self, on: bool):
        self.check(self.lib.tpst_profile_enable(self.h, 1 if on else 0), "tpst_profile_enable")

    def profile_reset(self):
        self.check(self.lib.tpst_profile_reset(self.h), "tpst_profile_reset")

    def profile_read(self) -> dict:
        out = {}
        for i, name in enumerate(self.STAGES):
            ms, cnt = C.c_double(), C.c_uint64()
            self.check(self.lib.tpst_profile_read(self.h, i, C.byref(ms), C.byref(cnt)), "tpst_profile_read")
            out[name] = (ms.value, cnt.value)
        return out

    def synchronize(self):
        self.check(self.lib.tpst_synchronize(self.h), "tpst_synchronize")

    # ------------------------------------------- ordering against torch ---
    # The library runs on its own non-blocking stream.  A device buffer that
    # torch produced (all-gather output, a .contiguous() copy, torch.empty from
    # the caching allocator) is handed to a _dev call only after torch_to_lib();
    # a buffer the library filled is used by torch only after lib_to_torch().
    @staticmethod
    def _torch_stream(device):
        import torch
        return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)

    def torch_to_lib(self):
        """Library work queued from now on waits for torch's current stream."""
        self.check(self.lib.tpst_wait_stream(self.h, self._torch_stream(self.device)), "tpst_wait_stream")

    def lib_to_torch(self):
        """Torch work queued from now on (current stream) waits for the library."""
        self.check(self.lib.tpst_join_stream(self.h, self._torch_stream(self.device)), "tpst_join_stream")

    def g1_msm_dev(self, d_bases: int, d_scalars: int, n: int, d_out: int):
        """Stream-ordered device MSM: later work on the library stream sees d_out."""
        self.check(self.lib.tpst_g1_msm_dev(self.h, C.c_void_p(d_bases), C.c_void_p(d_scalars), n,
                                            C.c_void_p(d_out)), "tpst_g1_msm_dev")

    def g1_msm_dev_async(self, d_bases: int, d_scalars: int, n: int, d_out: int):
        """Pipelined device MSM (tpst_g1_msm_dev_async): consecutive calls overlap.
        The buffers must stay alive and untouched until synchronize() /
        lib_to_torch() or the next call of another entry point."""
        self.check(self.lib.tpst_g1_msm_dev_async(self.h, C.c_void_p(d_bases), C.c_void_p(d_scalars), n,
                                                  C.c_void_p(d_out)), "tpst_g1_msm_dev_async")

    def g1_msm_xyzz_dev(self, d_bases: int, d_scalars: int, n: int, d_out: int):
        """One rank's share of a split MSM: the raw XYZZ sum (24 u64, Montgomery) at d_out."""
        self.check(self.lib.tpst_g1_msm_xyzz_dev(self.h, C.c_void_p(d_bases), C.c_void_p(d_scalars), n,
                                                 C.c_void_p(d_out)), "tpst_g1_msm_xyzz_dev")

    def g1_xyzz_sum_dev(self, d_parts: int, k: int, stride_bytes: int, d_out: int):
        """Sum of k XYZZ shares (stride_bytes apart) -> one canonical affine G1 (12 u64) at d_out."""
        self.check(self.lib.tpst_g1_xyzz_sum_dev(self.h, C.c_void_p(d_parts), k, stride_bytes, C.c_void_p(d_out)),
                   "tpst_g1_xyzz_sum_dev")

    def g1_mul_generator_dev(self, d_scalars: int, n: int, d_out: int):
        self.check(self.lib.tpst_g1_mul_generator_dev(self.h, C.c_void_p(d_scalars), n, C.c_void_p(d_out)),
                   "tpst_g1_mul_generator_dev")

    def microbench(self, kind: int, threads: int, iters: int) -> float:
        ms = C.c_double()
        self.check(self.lib.tpst_microbench(self.h, kind, threads, iters, C.byref(ms)), "tpst_microbench")
        return ms.value

    def selftest_inv(self, vals: np.ndarray):
        """device Fq inverses of Montgomery-form values (n x 6 words) by the
        lone-lane and the wave-cooperative routine"""
        vals = np.ascontiguousarray(vals, dtype=np.uint64).reshape(-1, 6)
        ol = np.zeros_like(vals)
        ow = np.zeros_like(vals)
        self.check(self.lib.tpst_selftest_inv(self.h, len(vals), ptr(vals), ptr(ol), ptr(ow)), "tpst_selftest_inv")
        return ol, ow

    def selftest_field(self, op: int, a: np.ndarray, b: np.ndarray = None) -> np.ndarray:
        """one device field operation per row of a (and b): `op` and the u32
        words per operand / result are SELFTEST_FIELD's (csrc/selftest_ops.h);
        rows are u32 words, the result is (n, out words) u32"""
        wi, wo = selftest_field_words(op)
        a = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1, wi)
        b = a if b is None else np.ascontiguousarray(b, dtype=np.uint32).reshape(-1, wi)
        assert a.shape == b.shape
        out = np.zeros((len(a), wo), dtype=np.uint32)
        self.check(self.lib.tpst_selftest_field(self.h, op, len(a), _u32ptr(a), _u32ptr(b), _u32ptr(out)),
                   "tpst_selftest_field")
        return out

    def selftest_curve(self, op: int, p: np.ndarray, q: np.ndarray = None) -> np.ndarray:
        """one device curve operation (or glv_split) per row of p (and q), XYZZ
        words in and out: `op` = SELFTEST_CURVE_FORMS[form] * 16 +
        SELFTEST_CURVE_OPS[name] (csrc/selftest_ops.h)"""
        w = selftest_curve_words(op)
        p = np.ascontiguousarray(p, dtype=np.uint32).reshape(-1, w)
        if q is not None:
            q = np.ascontiguousarray(q, dtype=np.uint32).reshape(-1, w)
            assert p.shape == q.shape
        out = np.zeros((len(p), w), dtype=np.uint32)
        self.check(self.lib.tpst_selftest_curve(self.h, op, len(p), _u32ptr(p), None if q is None else _u32ptr(q),
                                                _u32ptr(out)), "tpst_selftest_curve")
        return out

    def selftest_tower(self, op: int, a: np.ndarray, b: np.ndarray = None):
        """one operation of the pairing's RNS or wave Fq12 engine per row of a
        (and b): `op` = selftest_tower_op(engine, name, cin, cout), rows are
        u32 words (selftest_tower_words), the result is (n, out words) u32;
        gt_pow returns (result, ok) with ok (n,) u32"""
        wa, wb, wo = selftest_tower_words(op)
        a = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1, wa)
        n = len(a)
        if wb:
            b = np.ascontiguousarray(b, dtype=np.uint32).reshape(-1, wb)
            assert len(b) == n
        nok = n + (n & 1) if (op & 63) == SELFTEST_TOWER_OPS["gt_pow"] else 0
        out = np.zeros(n * wo + nok, dtype=np.uint32)
        self.check(self.lib.tpst_selftest_tower(self.h, op, n, _u32ptr(a), _u32ptr(b) if wb else None, _u32ptr(out)),
                   "tpst_selftest_tower")
        res = out[:n * wo].reshape(n, wo)
        return (res, out[n * wo:n * wo + n]) if nok else res

    def selftest_fbt(self, bases: np.ndarray, scalars: np.ndarray = None, *, g2: bool = False, glv: bool = False,
                     groups: int = 1, members: int = 0, L: int = 1, D: int = 1, seg=None, sets: int = 1,
                     set_stride: int = 0, table: bool = False) -> np.ndarray:
        """the fixed-base table engine (csrc/fbt.h) on a caller-chosen FbGroups
        (include/tpst.h tpst_selftest_fbt): (sets * groups, 12|24) canonical
        affine sums, or with table=True the (n * nw * 8, 12|24) table entries.
        The group shape is not checked here: the library validates it and a
        violation raises TpstError."""
        w = 24 if g2 else 12
        bases = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, w)
        n = len(bases)
        if table:
            out = np.zeros((n * (32 if glv else 64) * 8, w), dtype=np.uint64)
            s_ptr, ns = None, 0
        else:
            scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
            s_ptr, ns = ptr(scalars), len(scalars)
            out = np.zeros((max(sets * groups, 0), w), dtype=np.uint64)
        seg_ptr = None
        if seg is not None:
            seg = np.ascontiguousarray(seg, dtype=np.uint32)
            assert seg.shape == (groups + 1,)  # what the library will read
            seg_ptr = seg.ctypes.data_as(C.POINTER(C.c_uint32))
        self.check(self.lib.tpst_selftest_fbt(self.h, 2 if g2 else 1, int(glv), int(table), ptr(bases), n, s_ptr, ns,
                                              groups, members, L, D, seg_ptr, sets, set_stride, ptr(out)),
                   "tpst_selftest_fbt")
        return out


def _u32ptr(a: np.ndarray):
    assert a.dtype == np.uint32 and a.flags["C_CONTIGUOUS"] and a.size % 2 == 0
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


# Op numbers and word counts of tpst_selftest_field / tpst_selftest_curve.  The
# single source is csrc/selftest_ops.h (the enums, field_in_words /
# field_out_words / curve_words, field_op_valid / curve_op_valid); these
# tables restate it for Python, and tests/test_selftest_ops.py compares them
# with the header's values, read through the compiled host dispatch.
SELFTEST_FIELD_FAMILIES = {"fq": 0, "fr": 1, "fq29": 2, "fq2": 3, "fq2p": 4}
SELFTEST_FIELD = {}
for _i, _n in enumerate(("mul", "sqr", "add", "sub", "neg", "to_mont", "from_mont")):
    SELFTEST_FIELD["fq." + _n] = _i
    SELFTEST_FIELD["fr." + _n] = 32 + _i
for _i, _n in enumerate(("mul", "sqr", "mul_sum", "mul_sub", "add", "sub", "cneg", "p_minus", "to_std", "to_std_mul",
                         "from_std", "roundtrip", "mul_sum4", "mul_sub4")):
    SELFTEST_FIELD["fq29." + _n] = 64 + _i
for _i, _n in enumerate(("mul", "sqr")):
    SELFTEST_FIELD["fq2." + _n] = 96 + _i
for _i, _n in enumerate(("mul", "is_zero", "eq")):
    SELFTEST_FIELD["fq2p." + _n] = 128 + _i
SELFTEST_CURVE_FORMS = {"fq": 0, "fq29_acc": 1, "fq29_pk": 2, "fq2": 3, "coop_fq29_acc": 4, "coop_fq2_acc": 5,
                        "pair": 6, "glv": 7, "coop_fq29_pk": 8, "fq2_acc": 9}
SELFTEST_CURVE_OPS = {"add_affine": 0, "add": 1, "dbl": 2, "dbl_affine": 3, "sub_affine": 4, "to_affine": 5}
SELFTEST_GLV_SPLIT = 7 * 16
# chain-start forms (add_affine_unit: p infinity or ZZ = ZZZ = 1): form
# SELFTEST_CURVE_UNIT + a lane form, op add_affine only
SELFTEST_CURVE_UNIT = 16
SELFTEST_CURVE_UNIT_FORMS = ("fq", "fq29_acc", "fq29_pk", "fq2")


def selftest_curve_unit_op(form: str) -> int:
    assert form in SELFTEST_CURVE_UNIT_FORMS
    return (SELFTEST_CURVE_UNIT + SELFTEST_CURVE_FORMS[form]) * 16 + SELFTEST_CURVE_OPS["add_affine"]


def selftest_field_words(op: int):
    """(u32 words per operand, per result) of a tpst_selftest_field op"""
    fam, idx = op >> 5, op & 31
    if fam == 1:
        return 8, 8
    if fam == 3:
        return 24, 24
    if fam == 4:
        return 24, (24 if idx == 0 else 2)
    return (24 if fam == 2 and idx in (12, 13) else 12), 12


def selftest_curve_words(op: int) -> int:
    """u32 words per element of p, q and the result of a tpst_selftest_curve op"""
    form = op >> 4
    if SELFTEST_CURVE_UNIT <= form <= SELFTEST_CURVE_UNIT + 3:
        form -= SELFTEST_CURVE_UNIT
    return 8 if form == 7 else 96 if form in (3, 5, 6, 9) else 48


# tpst_selftest_tower: op = engine << 8 | in codec << 7 | out codec << 6 | index (csrc/selftest_ops.h's tower_*
# functions are the source; tests/test_tower_vectors.py compares these tables with the compiled header)
SELFTEST_TOWER_ENGINES = {"rns": 0, "wave": 1}
SELFTEST_TOWER_CODECS = {"fq": 0, "res": 1}
SELFTEST_TOWER_OPS = {"f12_mul": 0, "f12_sqr": 1, "cyc_sqr": 2, "frob1": 3, "frob2": 4, "frob3": 5, "conj": 6,
                      "copy": 7, "inv": 8, "final_exp": 9, "g2_prepare": 10, "gt_pow": 11, "pass": 12}
# what each engine runs; final_exp and g2_prepare take the fq codec only
SELFTEST_TOWER_ENGINE_OPS = {
    "rns": ("f12_mul", "f12_sqr", "cyc_sqr", "frob1", "frob2", "frob3", "conj", "copy", "inv", "final_exp",
            "g2_prepare", "pass"),
    "wave": ("f12_mul", "cyc_sqr", "frob1", "frob2", "conj", "inv", "gt_pow"),
}


def selftest_tower_op(engine: str, name: str, cin: str = "fq", cout: str = "fq") -> int:
    assert name in SELFTEST_TOWER_ENGINE_OPS[engine]
    assert (cin == "fq" and cout == "fq") or (engine == "rns" and name not in ("final_exp", "g2_prepare"))
    return (SELFTEST_TOWER_ENGINES[engine] << 8 | SELFTEST_TOWER_CODECS[cin] << 7 | SELFTEST_TOWER_CODECS[cout] << 6 |
            SELFTEST_TOWER_OPS[name])


def selftest_tower_valid(op: int) -> bool:
    if op < 0:
        return False
    eng, idx, fq = op >> 8, op & 63, (op >> 6) & 3 == 0
    names = {v: k for k, v in SELFTEST_TOWER_OPS.items()}
    for e, num in SELFTEST_TOWER_ENGINES.items():
        if eng == num:
            return (idx in names and names[idx] in SELFTEST_TOWER_ENGINE_OPS[e] and
                    (fq or (e == "rns" and names[idx] not in ("final_exp", "g2_prepare"))))
    return False


def selftest_tower_words(op: int):
    """u32 words per element of a, of b (0: not read) and of the result (gt_pow:
    without the trailing membership words) of a tpst_selftest_tower op"""
    idx = op & 63
    if idx == SELFTEST_TOWER_OPS["g2_prepare"]:
        return 48, 0, 69 * 72
    wa = 384 if (op >> 7) & 1 else 144
    wb = 8 if idx == SELFTEST_TOWER_OPS["gt_pow"] else wa if idx == SELFTEST_TOWER_OPS["f12_mul"] else 0
    return wa, wb, (384 if (op >> 6) & 1 else 144)


class Gens:
    """MultiCommitGens {n, G, h} (commitments.rs:9-15) resident on the device,
    with PedersenCommit::commit_slice (commitments.rs:79-86), the Hyrax row
    commitments of DensePolynomial::commit_inner (dense_mlpoly.rs:314-329) and
    the strided shared-base batch MSM."""

    def __init__(self, ctx: Context, G: np.ndarray, h: np.ndarray = None):
        self.ctx = ctx
        G = np.ascontiguousarray(G, dtype=np.uint64).reshape(-1, 12)
        self.n = len(G)
        hh = None if h is None else np.ascontiguousarray(h, dtype=np.uint64).reshape(12)
        handle = C.c_void_p()
        ctx.check(ctx.lib.tpst_gens_load(ctx.h, ptr(G), self.n, ptr(hh) if hh is not None else None,
                                         C.byref(handle)), "tpst_gens_load")
        self.handle = handle

    @classmethod
    def new(cls, ctx: Context, n: int, label: bytes) -> "Gens":
        """MultiCommitGens::new (commitments.rs:17-39): the generators of a
        label, derived on the device (tpst_gens_new); .G (n, 12), .h (12,)."""
        G = np.zeros((n, 12), dtype=np.uint64)
        h = np.zeros(12, dtype=np.uint64)
        handle = C.c_void_p()
        ctx.check(ctx.lib.tpst_gens_new(ctx.h, n, bytes(label), len(label), ptr(G), ptr(h), C.byref(handle)),
                  "tpst_gens_new")
        obj = cls.__new__(cls)
        obj.ctx, obj.n, obj.handle, obj.G, obj.h = ctx, n, handle, G, h
        return obj

    def close(self):
        if self.handle:
            self.ctx.lib.tpst_gens_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def msm_batch(self, scalars: np.ndarray, rows: int, row_stride: int, col_stride: int) -> np.ndarray:
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros((rows, 12), dtype=np.uint64)
        if rows and self.n:
            need = (rows - 1) * row_stride + (self.n - 1) * col_stride + 1
            if len(scalars) < need:
                raise TpstError("scalar buffer shorter than the strided view")
        self.ctx.check(self.ctx.lib.tpst_g1_msm_batch(self.ctx.h, self.handle, ptr(scalars), rows, self.n,
                                                      row_stride, col_stride, ptr(out)), "tpst_g1_msm_batch")
        return out

    def commit_slice(self, scalars: np.ndarray, blind: np.ndarray) -> np.ndarray:
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        blind = np.ascontiguousarray(blind, dtype=np.uint64).reshape(4)
        out = np.zeros(12, dtype=np.uint64)
        self.ctx.check(self.ctx.lib.tpst_pedersen_commit_slice(self.ctx.h, self.handle, ptr(scalars), len(scalars),
                                                               ptr(blind), ptr(out)), "commit_slice")
        return out

    def commit_rows(self, Z: np.ndarray, blinds: np.ndarray) -> np.ndarray:
        Z = np.ascontiguousarray(Z, dtype=np.uint64).reshape(-1, 4)
        blinds = np.ascontiguousarray(blinds, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros((len(blinds), 12), dtype=np.uint64)
        self.ctx.check(self.ctx.lib.tpst_pedersen_commit_rows(self.ctx.h, self.handle, ptr(Z), len(Z), ptr(blinds),
                                                              len(blinds), ptr(out)), "commit_inner")
        return out


def dense_commit(gens: Gens, Z: np.ndarray, blinds: np.ndarray = None) -> np.ndarray:
    """DensePolynomial::commit (dense_mlpoly.rs:349-377), the Hyrax commitment:
    ell = log2 |Z|, L = 2^(ell/2) rows of R = 2^(ell - ell/2) contiguous
    evaluations, row i -> commit_slice(Z[R i .. R (i+1)], blinds[i]) with
    gens.n == R; blinds default to zero (random_blinds = false, as in
    Derefs::commit sparse_mlpoly.rs:75-81 and SparseMatPolynomial::multi_commit)."""
    Z = np.ascontiguousarray(Z, dtype=np.uint64).reshape(-1, 4)
    ell = len(Z).bit_length() - 1
    if len(Z) != 1 << ell:
        raise TpstError("|Z| must be a power of two")
    L, R = 1 << (ell // 2), 1 << (ell - ell // 2)
    if gens.n != R:
        raise TpstError("gens.n must be 2^(ell - ell/2)")
    if blinds is None:
        blinds = np.zeros((L, 4), dtype=np.uint64)
    return gens.commit_rows(Z, blinds)
