// Self-tests of the device arithmetic below the kernels (tpst_selftest_field /
// tpst_selftest_curve): element-wise runs of the building blocks
// (selftest_ops.h) on caller-chosen operands.  64-thread blocks, every lane
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
#include "pair_fq2.h"
#include "glv.h"
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
