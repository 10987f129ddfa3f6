// Self-tests of the device arithmetic below the kernels (tpst_selftest_field /
// tpst_selftest_curve): element-wise runs of the building blocks
// (selftest_ops.h) on caller-chosen operands; and of the pairing's two Fq12
// engines (tpst_selftest_tower); and of the fixed-base table engine
// (tpst_selftest_fbt, at the end).  64-thread blocks, every lane
// active: the threads past the last element recompute it and store nothing,
// which keeps the quads of coop.h and the pairs of pair_fq2.h whole.
//
// A translation unit of its own, with the Fq2 products out of line as in
// msm_g2.hip: test-only code that builds beside the product's files instead
// of lengthening one of them.
#define TPST_FQ2_ATTR __host__ __device__ inline __attribute__((noinline))
#include "../../include/tpst.h"
#include "ctx.h"
#include "device_util.h"
#include "acc_field.h"
#include "coop.h"
#include "fbt.h"
#include "pair_fq2.h"
#include "glv.h"
#include "pairing_kernels.h"
#include "pairing_rns_chain.h"
#include "pairing_wave_fe.h"
#include "selftest_ops.h"

using namespace tpst;
namespace st = tpst::selftest;

template <int FAM>
__global__ void __launch_bounds__(64) k_selftest_field(int idx, size_t n, const uint32_t* __restrict__ a,
                                                       const uint32_t* __restrict__ b, uint32_t* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
  if constexpr (FAM == st::FAM_FQ2P) {
    // a holds (a_i, b_i) as the (x, y) of affine point i (b unused): one lane pair per element
    const size_t e = t >> 1;
    const bool live = e < n;
    const size_t i = live ? e : n - 1;
    const int h = threadIdx.x & 1;
    const Affine<Fq2P> ab = load_affine_pair(a, i);
    if (idx == st::F2P_MUL) {
      const Fq2P r = mul(ab.x, ab.y);
      if (live) store_f<Fq>(out + 24 * i + 12 * h, r.v);
    } else {
      const bool f = idx == st::F2P_IS_ZERO ? is_zero(ab.x) : eq(ab.x, ab.y);
      if (live) out[2 * i + h] = f ? 1u : 0u;
    }
  } else {
    constexpr int WO = FAM == st::FAM_FR ? 8 : FAM == st::FAM_FQ2 ? 24 : 12;
    const bool live = t < n;
    const size_t i = live ? t : n - 1;
    const int wi = st::field_in_words(FAM * 32 + idx);
    uint32_t r[WO];
    if constexpr (FAM == st::FAM_FQ)
      st::fp_op<FqCfg>(idx, a + wi * i, b + wi * i, r);
    else if constexpr (FAM == st::FAM_FR)
      st::fp_op<FrCfg>(idx, a + wi * i, b + wi * i, r);
    else if constexpr (FAM == st::FAM_F29)
      st::f29_op(idx, a + wi * i, b + wi * i, r);
    else
      st::fq2_op(idx, a + wi * i, b + wi * i, r);
    if (live) {
#pragma unroll
      for (int k = 0; k < WO; k++) out[WO * i + k] = r[k];
    }
  }
}

extern "C" int tpst_selftest_field(tpst_ctx* ctx, int op, size_t n, const uint64_t* a, const uint64_t* b,
                                   uint64_t* out) {
  if (!ctx || !n || n > ((size_t)1 << 24) || !a || !b || !out || !st::field_op_valid(op))
    return fail(ctx, TPST_E_ARG, "bad argument");
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  const int fam = st::field_family(op), idx = st::field_index(op);
  const size_t wi = st::field_in_words(op), wo = st::field_out_words(op);
  const bool pair = fam == st::FAM_FQ2P;
  ctx->io.reset();
  TPST_HIP(ctx, ctx->io.reserve(2 * Arena::need(n * wi * (pair ? 2 : 1), 4) + Arena::need(n * wo, 4)));
  uint32_t* d_a = ctx->io.take<uint32_t>(n * wi * (pair ? 2 : 1));
  uint32_t* d_b = ctx->io.take<uint32_t>(n * wi);
  uint32_t* d_o = ctx->io.take<uint32_t>(n * wo);
  if (pair) {  // interleave to affine points (a_i, b_i), the layout load_affine_pair reads
    TPST_HIP(ctx, hipMemcpy2DAsync(d_a, 192, a, 96, 96, n, hipMemcpyHostToDevice, ctx->stream));
    TPST_HIP(ctx, hipMemcpy2DAsync(d_a + 24, 192, b, 96, 96, n, hipMemcpyHostToDevice, ctx->stream));
  } else {
    TPST_HIP(ctx, hipMemcpyAsync(d_a, a, n * wi * 4, hipMemcpyHostToDevice, ctx->stream));
    TPST_HIP(ctx, hipMemcpyAsync(d_b, b, n * wi * 4, hipMemcpyHostToDevice, ctx->stream));
  }
  const unsigned grid = grid_for(n * (pair ? 2 : 1), 64);
  switch (fam) {
    case st::FAM_FQ: k_selftest_field<st::FAM_FQ><<<grid, 64, 0, ctx->stream>>>(idx, n, d_a, d_b, d_o); break;
    case st::FAM_FR: k_selftest_field<st::FAM_FR><<<grid, 64, 0, ctx->stream>>>(idx, n, d_a, d_b, d_o); break;
    case st::FAM_F29: k_selftest_field<st::FAM_F29><<<grid, 64, 0, ctx->stream>>>(idx, n, d_a, d_b, d_o); break;
    case st::FAM_FQ2: k_selftest_field<st::FAM_FQ2><<<grid, 64, 0, ctx->stream>>>(idx, n, d_a, d_b, d_o); break;
    default: k_selftest_field<st::FAM_FQ2P><<<grid, 64, 0, ctx->stream>>>(idx, n, d_a, d_b, d_o); break;
  }
  TPST_HIP(ctx, hipGetLastError());
  TPST_HIP(ctx, hipMemcpyAsync(out, d_o, n * wo * 4, hipMemcpyDeviceToHost, ctx->stream));
  TPST_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return TPST_OK;
}

// coop.h: every lane of the quad holds the operands
template <int COP, class T>
__device__ __forceinline__ Xyzz<T> coop_op(const Xyzz<T>& a, const Xyzz<T>& b) {
  const int qi = (int)(threadIdx.x & 3);
  if constexpr (COP == st::C_ADD_AFFINE)
    return add_affine_quad(a, Affine<T>{b.X, b.Y}, qi);
  else if constexpr (COP == st::C_ADD)
    return add_quad(a, b, qi);
  else
    return dbl_quad(a, qi);
}

// a lane form's operation: add_affine_unit for the chain-start forms
template <bool UNIT, int COP, class F>
__device__ __forceinline__ Xyzz<F> lane_op(const Xyzz<F>& a, const Xyzz<F>& b) {
  if constexpr (UNIT)
    return st::curve_op_unit(a, b);
  else
    return st::curve_op<COP>(a, b);
}

template <int OPFORM, int COP>
__global__ void __launch_bounds__(64) k_selftest_curve(size_t n, const uint32_t* __restrict__ p,
                                                       const uint32_t* __restrict__ q, uint32_t* __restrict__ out) {
  constexpr bool UNIT = OPFORM >= st::FORM_UNIT;  // FORM_UNIT + a lane form
  constexpr int FORM = UNIT ? OPFORM - st::FORM_UNIT : OPFORM;
  constexpr bool COOP = FORM == st::FORM_COOP_FQ29_ACC || FORM == st::FORM_COOP_FQ29_PK || FORM == st::FORM_COOP_FQ2_ACC;
  constexpr int T = COOP ? 4 : FORM == st::FORM_PAIR ? 2 : 1;
  const size_t e = ((size_t)blockIdx.x * 64 + threadIdx.x) / T;
  const bool live = e < n;
  const size_t i = live ? e : n - 1;
  // a quad's storing lane rotates with the element
  const bool store = live && (!COOP || (threadIdx.x & 3) == (e & 3));
  if constexpr (FORM == st::FORM_GLV) {
    uint32_t k1[4], k2[4];
    glv_split(p + 8 * i, k1, k2);
    if (live) {
#pragma unroll
      for (int k = 0; k < 4; k++) {
        out[8 * i + k] = k1[k];
        out[8 * i + 4 + k] = k2[k];
      }
    }
  } else if constexpr (FORM == st::FORM_PAIR || FORM == st::FORM_FQ2 || FORM == st::FORM_FQ2_ACC ||
                       FORM == st::FORM_COOP_FQ2_ACC) {
    const Xyzz<Fq2>* P = reinterpret_cast<const Xyzz<Fq2>*>(p);
    const Xyzz<Fq2>* Q = reinterpret_cast<const Xyzz<Fq2>*>(q);
    Xyzz<Fq2>* O = reinterpret_cast<Xyzz<Fq2>*>(out);
    if constexpr (FORM == st::FORM_PAIR) {
      const Xyzz<Fq2P> r = st::curve_op<COP>(load_xyzz_pair(P, i), load_xyzz_pair(Q, i));
      if (live) store_xyzz_pair(O, i, r);
    } else if constexpr (FORM == st::FORM_FQ2) {
      const Xyzz<Fq2> r = lane_op<UNIT, COP>(load_xyzz(P, i), load_xyzz(Q, i));
      if (store) store_xyzz(O, i, r);
    } else if constexpr (FORM == st::FORM_FQ2_ACC) {  // Fq2x29, converted as the G2 tail kernels do
      const Xyzz<Fq2x29> r = st::curve_op<COP>(load_acc(P, i), load_acc(Q, i));
      if (store) store_acc(O, i, r);
    } else {
      const Xyzz<Fq2x29> r = coop_op<COP>(load_acc(P, i), load_acc(Q, i));
      if (store) store_acc(O, i, r);
    }
  } else {
    const Xyzz<Fq>* P = reinterpret_cast<const Xyzz<Fq>*>(p);
    const Xyzz<Fq>* Q = reinterpret_cast<const Xyzz<Fq>*>(q);
    Xyzz<Fq>* O = reinterpret_cast<Xyzz<Fq>*>(out);
    if constexpr (FORM == st::FORM_FQ) {
      const Xyzz<Fq> r = lane_op<UNIT, COP>(load_xyzz(P, i), load_xyzz(Q, i));
      if (store) store_xyzz(O, i, r);
    } else if constexpr (FORM == st::FORM_FQ29_ACC) {  // field.h words, converted as the tail kernels do
      const Xyzz<Fq29> r = lane_op<UNIT, COP>(load_acc(P, i), load_acc(Q, i));
      if (store) store_acc(O, i, r);
    } else if constexpr (FORM == st::FORM_FQ29_PK) {  // the accumulation kernels' packed buckets
      const Xyzz<Fq29> r = lane_op<UNIT, COP>(load_pk(P, i), load_pk(Q, i));
      if (store) store_pk(O, i, r);
    } else if constexpr (FORM == st::FORM_COOP_FQ29_ACC) {
      const Xyzz<Fq29> r = coop_op<COP>(load_acc(P, i), load_acc(Q, i));
      if (store) store_acc(O, i, r);
    } else {
      const Xyzz<Fq29> r = coop_op<COP>(load_pk(P, i), load_pk(Q, i));
      if (store) store_pk(O, i, r);
    }
  }
}

extern "C" int tpst_selftest_curve(tpst_ctx* ctx, int op, size_t n, const uint64_t* p, const uint64_t* q,
                                   uint64_t* out) {
  if (!ctx || !n || n > ((size_t)1 << 24) || !p || !out || !st::curve_op_valid(op))
    return fail(ctx, TPST_E_ARG, "bad argument");
  const int form = st::curve_form(op);
  if (!q && form != st::FORM_GLV) return fail(ctx, TPST_E_ARG, "bad argument");
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  const size_t w = st::curve_words(op);
  const size_t T = st::curve_form_coop(form) ? 4 : form == st::FORM_PAIR ? 2 : 1;
  ctx->io.reset();
  TPST_HIP(ctx, ctx->io.reserve(3 * Arena::need(n * w, 4)));
  uint32_t* d_p = ctx->io.take<uint32_t>(n * w);
  uint32_t* d_q = ctx->io.take<uint32_t>(n * w);
  uint32_t* d_o = ctx->io.take<uint32_t>(n * w);
  TPST_HIP(ctx, hipMemcpyAsync(d_p, p, n * w * 4, hipMemcpyHostToDevice, ctx->stream));
  if (q) TPST_HIP(ctx, hipMemcpyAsync(d_q, q, n * w * 4, hipMemcpyHostToDevice, ctx->stream));
  const unsigned grid = grid_for(n * T, 64);
  hipStream_t s = ctx->stream;
#define TPST_ST_CURVE(F, C) \
  case (F) * 16 + C: k_selftest_curve<(F), C><<<grid, 64, 0, s>>>(n, d_p, d_q, d_o); break;
#define TPST_ST_LANE(F)                                                                       \
  TPST_ST_CURVE(F, st::C_ADD_AFFINE) TPST_ST_CURVE(F, st::C_ADD) TPST_ST_CURVE(F, st::C_DBL) \
  TPST_ST_CURVE(F, st::C_DBL_AFFINE) TPST_ST_CURVE(F, st::C_SUB_AFFINE)
#define TPST_ST_COOP(F) \
  TPST_ST_CURVE(F, st::C_ADD_AFFINE) TPST_ST_CURVE(F, st::C_ADD) TPST_ST_CURVE(F, st::C_DBL)
  switch (op) {
    TPST_ST_LANE(st::FORM_FQ) TPST_ST_CURVE(st::FORM_FQ, st::C_TO_AFFINE)
    TPST_ST_LANE(st::FORM_FQ29_ACC) TPST_ST_CURVE(st::FORM_FQ29_ACC, st::C_TO_AFFINE)
    TPST_ST_LANE(st::FORM_FQ29_PK) TPST_ST_CURVE(st::FORM_FQ29_PK, st::C_TO_AFFINE)
    TPST_ST_LANE(st::FORM_FQ2) TPST_ST_CURVE(st::FORM_FQ2, st::C_TO_AFFINE)
    TPST_ST_CURVE(st::FORM_UNIT + st::FORM_FQ, st::C_ADD_AFFINE)
    TPST_ST_CURVE(st::FORM_UNIT + st::FORM_FQ29_ACC, st::C_ADD_AFFINE)
    TPST_ST_CURVE(st::FORM_UNIT + st::FORM_FQ29_PK, st::C_ADD_AFFINE)
    TPST_ST_CURVE(st::FORM_UNIT + st::FORM_FQ2, st::C_ADD_AFFINE)
    TPST_ST_LANE(st::FORM_FQ2_ACC)
    TPST_ST_LANE(st::FORM_PAIR)
    TPST_ST_COOP(st::FORM_COOP_FQ29_ACC)
    TPST_ST_COOP(st::FORM_COOP_FQ29_PK)
    TPST_ST_COOP(st::FORM_COOP_FQ2_ACC)
    TPST_ST_CURVE(st::FORM_GLV, st::C_GLV_SPLIT)
    default: return fail(ctx, TPST_E_ARG, "bad argument");
  }
#undef TPST_ST_COOP
#undef TPST_ST_LANE
#undef TPST_ST_CURVE
  TPST_HIP(ctx, hipGetLastError());
  TPST_HIP(ctx, hipMemcpyAsync(out, d_o, n * w * 4, hipMemcpyDeviceToHost, ctx->stream));
  TPST_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return TPST_OK;
}

// ---- the pairing's Fq12 engines (tpst_selftest_tower) ----------------------
// The engines' own code on caller-chosen operands: rns::load / load_res /
// stage<OP> / store / store_res and rc_inv in the production kernels' shape
// (12 waves, two elements per workgroup, an odd n's last workgroup running
// its lone element in both halves as k_g2_prepare_rns does), wave::run with
// the FE op set and fe_inv, one wave per element.  No arithmetic of its own.
constexpr int TW_SLOTS = rns::N_CONSTS + 36 + 24;  // constants, A, B, C, rc_inv's temporaries

template <int TOP>
__device__ __forceinline__ void tower_rns_op(const rns::Eng& e, const rns::Lane& L, int A, int B, int C, int I,
                                             Fq* sh_n) {
  if constexpr (TOP == st::T_F12_MUL)
    rns::stage<rns::OP_F12_MUL>(e, L, A, B, C);
  else if constexpr (TOP == st::T_F12_SQR)
    rns::stage<rns::OP_F12_SQR>(e, L, A, 0, C);
  else if constexpr (TOP == st::T_CYC_SQR)
    rns::stage<rns::OP_CYC_SQR>(e, L, A, 0, C);
  else if constexpr (TOP == st::T_FROB1)
    rns::stage<rns::OP_FROB1>(e, L, A, 0, C);
  else if constexpr (TOP == st::T_FROB2)
    rns::stage<rns::OP_FROB2>(e, L, A, 0, C);
  else if constexpr (TOP == st::T_FROB3)
    rns::stage<rns::OP_FROB3>(e, L, A, 0, C);
  else if constexpr (TOP == st::T_CONJ)
    rns::stage<rns::OP_CONJ>(e, L, A, 0, C);
  else if constexpr (TOP == st::T_COPY)
    rns::stage<rns::OP_COPY>(e, L, A, 0, C);
  else
    rc_inv(e, L, A, I, C, sh_n);
}

template <int TOP>
__global__ void __launch_bounds__(64 * RC_WAVES) k_selftest_rns(int cin, int cout, size_t n,
                                                                const uint32_t* __restrict__ a,
                                                                const uint32_t* __restrict__ b,
                                                                uint32_t* __restrict__ out) {
  __shared__ uint32_t s_slots[TW_SLOTS * rns::SLOT];
  __shared__ uint32_t s_xch[RC_WAVES * rns::XCH];
  __shared__ Fq sh_n[2];
  const size_t p0 = 2 * (size_t)blockIdx.x, p1 = p0 + 1 < n ? p0 + 1 : p0;
  rns::load_consts((rns::lds_t*)s_slots);
  const rns::Lane L = rns::load_lane();
  const rns::Eng e{(rns::lds_t*)s_slots, (rns::lds_t*)s_xch + rns::wave_id() * rns::XCH, 0};
  __syncthreads();
  const int A = rns::N_CONSTS, B = A + 12, C = TOP == st::T_PASS ? A : A + 24, I = A + 36;
  constexpr size_t WF = st::TOWER_FQ_WORDS, WR = st::TOWER_RES_WORDS;
  if (cin == st::TW_FQ) {
    rns::load(e, L, reinterpret_cast<const Fq*>(a + WF * p0), reinterpret_cast<const Fq*>(a + WF * p1), A, 12);
    if constexpr (TOP == st::T_F12_MUL)
      rns::load(e, L, reinterpret_cast<const Fq*>(b + WF * p0), reinterpret_cast<const Fq*>(b + WF * p1), B, 12);
  } else {
    rns::load_res(e, a + WR * p0, a + WR * p1, A, 12);
    if constexpr (TOP == st::T_F12_MUL) rns::load_res(e, b + WR * p0, b + WR * p1, B, 12);
  }
  if constexpr (TOP != st::T_PASS) tower_rns_op<TOP>(e, L, A, B, C, I, sh_n);
  if (cout == st::TW_FQ)
    rns::store(e, L, C, reinterpret_cast<Fq*>(out + WF * p0), reinterpret_cast<Fq*>(out + WF * p1), 12);
  else
    rns::store_res(e, C, out + WR * p0, out + WR * p1, 12);
}

constexpr size_t TWV_LDS = (size_t)(FW_PROG + (wave::N_CONSTS + 64 + 36 + 24) * wave::SLOT) * 4;
static_assert(TWV_LDS <= 65536, "tower self-test wave kernel LDS");

// fe: index into FE_SET of a single stage, or < 0 for fe_inv
__global__ void __launch_bounds__(64) k_selftest_wave(int fe, size_t n, const Fq12* __restrict__ a,
                                                      const Fq12* __restrict__ b, Fq12* __restrict__ out) {
  extern __shared__ uint4 smem4[];
  wave::lds_t* prog = (wave::lds_t*)(smem4);
  wave::lds_t* vals = prog + FW_PROG;
  wave::load_set(prog, FE_SET);
  wave::load_consts(vals, 0);
  __syncthreads();
  const size_t i = blockIdx.x;
  if (i >= n) return;
  const wave::Eng e{vals, wave::N_CONSTS, 0};
  const int A = wave::N_CONSTS + 64, B = A + 12, C = A + 24, I = A + 36;
  wave::load_f12(vals, A, a + i);
  wave::load_f12(vals, B, (b ? b : a) + i);
  if (fe < 0)
    fe_inv(e, prog, A, I, C);
  else
    wave::run(e, prog + FE_SET.off[fe], A, B, C);
  wave::store_f12(vals, C, out + i);
}

static int tower_fe_index(int idx) {
  switch (idx) {
    case st::T_F12_MUL: return FE_MUL;
    case st::T_CYC_SQR: return FE_CYC;
    case st::T_FROB1: return FE_FROB1;
    case st::T_FROB2: return FE_FROB2;
    case st::T_CONJ: return FE_CONJ;
    default: return -1;  // T_INV
  }
}

extern "C" int tpst_selftest_tower(tpst_ctx* ctx, int op, size_t n, const uint64_t* a, const uint64_t* b,
                                   uint64_t* out) {
  if (!ctx || !n || n > ((size_t)1 << 16) || !a || !out || !st::tower_op_valid(op))
    return fail(ctx, TPST_E_ARG, "bad argument");
  if (!b && st::tower_reads_b(op)) return fail(ctx, TPST_E_ARG, "bad argument");
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  const int eng = st::tower_engine(op), idx = st::tower_index(op);
  const int cin = st::tower_codec_in(op), cout = st::tower_codec_out(op);
  const size_t wa = st::tower_a_words(op), wb = st::tower_b_words(op), wo = st::tower_out_words(op);
  const size_t nok = idx == st::T_GT_POW ? n + (n & 1) : 0;  // trailing membership words
  hipStream_t s = ctx->stream;
  ctx->io.reset();
  TPST_HIP(ctx, ctx->io.reserve(Arena::need(n * wa, 4) + Arena::need(n * wb + 2, 4) + Arena::need(n * wo + nok, 4) +
                                (idx == st::T_G2_PREPARE ? Arena::need(plan::prepare_words(n), 4) : 0)));
  uint32_t* d_a = ctx->io.take<uint32_t>(n * wa);
  uint32_t* d_b = ctx->io.take<uint32_t>(n * wb + 2);
  uint32_t* d_o = ctx->io.take<uint32_t>(n * wo + nok);
  TPST_HIP(ctx, hipMemcpyAsync(d_a, a, n * wa * 4, hipMemcpyHostToDevice, s));
  if (wb) TPST_HIP(ctx, hipMemcpyAsync(d_b, b, n * wb * 4, hipMemcpyHostToDevice, s));
  const Fq12* fa = reinterpret_cast<const Fq12*>(d_a);
  Fq12* fo = reinterpret_cast<Fq12*>(d_o);
  if (idx == st::T_G2_PREPARE) {
    uint32_t* prep = ctx->io.take<uint32_t>(plan::prepare_words(n));
    TPST_HIP(ctx, g2_prepare_batch(s, d_a, n, reinterpret_cast<LineCoeff*>(d_o), prep));
  } else if (idx == st::T_FINAL_EXP) {
    TPST_HIP(ctx, gt_prod_final(s, fa, 1, n, fo));
  } else if (idx == st::T_GT_POW) {
    TPST_HIP(ctx, hipMemsetAsync(d_o, 0, (n * wo + nok) * 4, s));
    TPST_HIP(ctx, gt_pow_wave(s, fa, reinterpret_cast<const uint64_t*>(d_b), n, fo, d_o + n * wo));
  } else if (eng == st::TE_WAVE) {
    k_selftest_wave<<<(unsigned)n, 64, TWV_LDS, s>>>(tower_fe_index(idx), n, fa,
                                                     wb ? reinterpret_cast<const Fq12*>(d_b) : nullptr, fo);
    TPST_HIP(ctx, hipGetLastError());
  } else {
    const unsigned grid = (unsigned)((n + 1) / 2);
#define TPST_ST_TOWER(T) \
  case T: k_selftest_rns<T><<<grid, 64 * RC_WAVES, 0, s>>>(cin, cout, n, d_a, d_b, d_o); break;
    switch (idx) {
      TPST_ST_TOWER(st::T_F12_MUL) TPST_ST_TOWER(st::T_F12_SQR) TPST_ST_TOWER(st::T_CYC_SQR)
      TPST_ST_TOWER(st::T_FROB1) TPST_ST_TOWER(st::T_FROB2) TPST_ST_TOWER(st::T_FROB3)
      TPST_ST_TOWER(st::T_CONJ) TPST_ST_TOWER(st::T_COPY) TPST_ST_TOWER(st::T_INV) TPST_ST_TOWER(st::T_PASS)
      default: return fail(ctx, TPST_E_ARG, "bad argument");
    }
#undef TPST_ST_TOWER
    TPST_HIP(ctx, hipGetLastError());
  }
  TPST_HIP(ctx, hipMemcpyAsync(out, d_o, (n * wo + nok) * 4, hipMemcpyDeviceToHost, s));
  TPST_HIP(ctx, hipStreamSynchronize(s));
  return TPST_OK;
}

// ---- the fixed-base table engine (tpst_selftest_fbt) ------------------------
// fbt_build / fbt_msm (fbt.h) themselves on a caller-chosen FbGroups: no kernel
// of its own.  Every index a kernel will form is checked here first.
constexpr size_t ST_FBT_MAX_N = (size_t)1 << 14;        // bases (a table is 48 KiB per G1 base, 96 KiB per G2 base)
constexpr size_t ST_FBT_MAX_SCALARS = (size_t)1 << 20;  // scalars, and the bound on set_stride
constexpr size_t ST_FBT_MAX_TERMS = (size_t)1 << 16;    // sets * groups * max(members, 1)

// true when every (set, group, member) reads a base below n and a scalar below n_scalars
static bool fbt_groups_in_bounds(size_t n, size_t n_scalars, const FbGroups& g, const uint32_t* seg) {
  if (!g.groups || !g.sets || g.groups > ST_FBT_MAX_TERMS || g.sets > ST_FBT_MAX_TERMS ||
      g.members > ST_FBT_MAX_TERMS)
    return false;
  if (g.sets * g.groups > ST_FBT_MAX_TERMS || g.sets * g.groups * (g.members ? g.members : 1) > ST_FBT_MAX_TERMS)
    return false;
  if (g.set_stride > ST_FBT_MAX_SCALARS) return false;
  size_t kmax = 0;  // largest base index any member reads
  bool any = false;
  if (seg) {
    for (size_t i = 0; i < g.groups; i++) {
      if (seg[i] > seg[i + 1] || (size_t)seg[i + 1] - seg[i] > g.members) return false;
    }
    if (seg[g.groups] > n) return false;
    any = seg[g.groups] > seg[0];
    if (any) kmax = (size_t)seg[g.groups] - 1;
  } else {
    if (!g.L || !g.D || g.L > ST_FBT_MAX_N || g.D > ST_FBT_MAX_N) return false;
    for (size_t i = 0; i < g.groups; i++)
      for (size_t m = 0; m < g.members; m++) {
        const size_t k = (m / g.D) * g.L + i * g.D + m % g.D;
        if (k >= n) return false;
        if (k > kmax) kmax = k;
        any = true;
      }
  }
  return !any || kmax + (g.sets - 1) * g.set_stride < n_scalars;
}

template <class F>
static int selftest_fbt(tpst_ctx* ctx, bool glv, int mode, const uint64_t* bases, size_t n, const uint64_t* scalars,
                        size_t n_scalars, const FbGroups& g0, const uint32_t* seg, uint64_t* out) {
  constexpr size_t PW = 2 * Words<F>::n;
  const size_t nw = glv ? FBT_WG : FBT_W;
  const size_t entries = n * nw * FBT_M, G = mode ? 0 : g0.groups * g0.sets;
  const size_t nout = mode ? entries : G;
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  ctx->io.reset();
  TPST_HIP(ctx, ctx->io.reserve(Arena::need(n * PW, 4) * 2 + Arena::need(n_scalars * 8, 4) +
                                Arena::need(g0.groups + 1, 4) + Arena::need(G, sizeof(Xyzz<F>)) +
                                Arena::need(nout * PW, 4) + Arena::need(entries * PW, 4) + 4096));
  uint32_t* d_b = ctx->io.take<uint32_t>(n * PW);
  uint32_t* d_bm = ctx->io.take<uint32_t>(n * PW);
  uint32_t* d_s = ctx->io.take<uint32_t>(n_scalars * 8);
  uint32_t* d_seg = ctx->io.take<uint32_t>(g0.groups + 1);
  Xyzz<F>* d_r = ctx->io.take<Xyzz<F>>(G);
  uint32_t* d_o = ctx->io.take<uint32_t>(nout * PW);
  uint32_t* d_t = ctx->io.take<uint32_t>(entries * PW);
  hipStream_t s = ctx->stream;
  TPST_HIP(ctx, hipMemcpyAsync(d_b, bases, n * PW * 4, hipMemcpyHostToDevice, s));
  TPST_HIP(ctx, points_to_mont<F>(s, d_b, d_bm, n));
  TPST_HIP(ctx, fbt_build<F>(ctx->arena, s, d_bm, n, d_t, glv));
  if (mode) {
    TPST_HIP(ctx, affine_from_mont<F>(s, d_t, d_o, entries));
  } else {
    FbGroups g = g0;
    TPST_HIP(ctx, hipMemcpyAsync(d_s, scalars, n_scalars * 32, hipMemcpyHostToDevice, s));
    if (seg) {
      TPST_HIP(ctx, hipMemcpyAsync(d_seg, seg, (g.groups + 1) * 4, hipMemcpyHostToDevice, s));
      g.d_seg = d_seg;
    }
    TPST_HIP(ctx, fbt_msm<F>(ctx->arena, s, d_t, d_s, g, d_r));
    TPST_HIP(ctx, xyzz_to_affine_canonical<F>(s, d_r, d_o, G));
  }
  TPST_HIP(ctx, hipMemcpyAsync(out, d_o, nout * PW * 4, hipMemcpyDeviceToHost, s));
  TPST_HIP(ctx, hipStreamSynchronize(s));
  return TPST_OK;
}

extern "C" int tpst_selftest_fbt(tpst_ctx* ctx, int group, int glv, int mode, const uint64_t* bases, size_t n,
                                 const uint64_t* scalars, size_t n_scalars, size_t groups, size_t members, size_t L,
                                 size_t D, const uint32_t* seg, size_t sets, size_t set_stride, uint64_t* out) {
  if (!ctx || !bases || !out || !n || n > ST_FBT_MAX_N || (group != 1 && group != 2) || (glv != 0 && glv != 1) ||
      (mode != 0 && mode != 1) || (glv && group == 2))
    return fail(ctx, TPST_E_ARG, "bad argument");
  FbGroups g;
  g.glv = glv != 0;
  if (mode == 0) {
    g.groups = groups;
    g.members = members;
    g.L = L;
    g.D = D;
    g.sets = sets;
    g.set_stride = set_stride;
    if (!scalars || !n_scalars || n_scalars > ST_FBT_MAX_SCALARS || !fbt_groups_in_bounds(n, n_scalars, g, seg))
      return fail(ctx, TPST_E_ARG, "bad group shape");
  } else {
    n_scalars = 0;
    seg = nullptr;
  }
  return group == 2 ? selftest_fbt<Fq2>(ctx, false, mode, bases, n, scalars, n_scalars, g, seg, out)
                    : selftest_fbt<Fq>(ctx, g.glv, mode, bases, n, scalars, n_scalars, g, seg, out);
}
