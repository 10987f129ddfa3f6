// One sqrt-PST proof for B polynomials opened at one point (include/tpst.h,
// "combined opening"): the commitment is linear in the polynomial, so for
// weights w_j fixed after every T_j, the point and every v_j,
//   Z* = sum_j w_j Z_j,  comm_list*[i] = sum_j w_j comm_list_j[i],
//   T* = prod_j T_j^(w_j),  v* = sum_j w_j v_j
// is a committed polynomial with its value, and one opening of Z* covers all
// B.  Two kernels of this unit and the verifier's GT powers build it:
//
//   k_fr_lincomb       out[i] = sum_j w_j Z_j[i] mod r over canonical tables.
//                      The weights are uploaded in Montgomery form: a
//                      Montgomery product of a Montgomery and a canonical
//                      operand is the canonical product, so no conversion pass
//                      runs.  Two 128-bit loads per entry and term, grid-stride,
//                      one lane per entry: no atomics, the value does not
//                      depend on the grid.  (B + 1) 2^n 32 B of traffic.
//   k_g1_lincomb_rows  out[i] = sum_j w_j P_j[i]: one quad of lanes per row
//                      (lincomb_quad.h), one joint double-and-add over the bits
//                      of the longest weight.  The weights are the same for
//                      every row, so the schedule -- which terms to add after
//                      which doubling -- is a table built on the host and read
//                      by a uniform index: no per-lane bit test.  C rows are
//                      far fewer than the chip has lanes and a chain of B terms
//                      is nbits (1 + B / 2) serial additions, so the terms are
//                      dealt to G chains per row (grid y) that repeat the
//                      doublings and share the additions; k_g1_rows_sum adds
//                      the G partial sums.  Every special case is the formulas'
//                      own (infinity in the input, acc = +-P_j[i], a result at
//                      infinity): lc_madd_quad / lc_add_quad / lc_dbl_quad.
//   GT                 gt_pow_wave (membership test and T_j^(w_j)), then the
//                      product of the B powers on the host, as
//                      pst_verify_batch.hip does.
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/tpst.h"
#include "acc_field.h"
#include "ctx.h"
#include "device_util.h"
#include "host_curve.h"
#include "lincomb_quad.h"
#include "pairing_kernels.h"
#include "poly_lincomb.h"
#include "poseidon_host.h"
#include "pst_state.h"

namespace tpst {

// ------------------------------------------------------------ k_fr_lincomb --
constexpr int FL_BS = 256;

__device__ __forceinline__ Fr ld_fr16(const uint32_t* p) {
  const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
  Fr r;
  r.v[0] = a.x, r.v[1] = a.y, r.v[2] = a.z, r.v[3] = a.w;
  r.v[4] = b.x, r.v[5] = b.y, r.v[6] = b.z, r.v[7] = b.w;
  return r;
}

__global__ void __launch_bounds__(FL_BS) k_fr_lincomb(const uint32_t* const* __restrict__ tabs,
                                                      const uint32_t* __restrict__ w, int B, size_t n,
                                                      uint32_t* __restrict__ out) {
  const size_t stride = (size_t)gridDim.x * FL_BS;
  for (size_t i = (size_t)blockIdx.x * FL_BS + threadIdx.x; i < n; i += stride) {
    Fr acc = Fr::zero();
    for (int j = 0; j < B; j++)  // tabs[j], w[j]: uniform over the wave
      acc = add(acc, mul(load_f<Fr>(w + 8 * j), ld_fr16(tabs[j] + 8 * i)));
    uint4* o = reinterpret_cast<uint4*>(out + 8 * i);
    o[0] = make_uint4(acc.v[0], acc.v[1], acc.v[2], acc.v[3]);
    o[1] = make_uint4(acc.v[4], acc.v[5], acc.v[6], acc.v[7]);
  }
}

hipError_t fr_lincomb(hipStream_t s, const uint32_t* const* d_tabs, const uint32_t* d_w, size_t B, size_t n,
                      uint32_t* d_out) {
  if (!n) return hipSuccess;
  if (!d_tabs || !d_w || !d_out || B < 1 || B > LINCOMB_MAX_TERMS) return hipErrorInvalidValue;
  // a few resident workgroups per CU keep the loads in flight; the stride loop covers the rest
  const unsigned grid = (unsigned)std::min<size_t>(grid_for(n, FL_BS), 256 * 8);
  k_fr_lincomb<<<grid, FL_BS, 0, s>>>(d_tabs, d_w, (int)B, n, d_out);
  return hipGetLastError();
}

// ------------------------------------------------------- k_g1_lincomb_rows --
// Quads that one pass of the chip takes at two waves per SIMD (256 CUs x 4
// SIMDs x 16 quads x 2): the row chains are latency-bound, so the terms are
// split over chains up to that many
constexpr size_t ROW_QUADS = 32768;
constexpr int ROW_MAX_CHAINS = 16;

RowSchedule row_schedule(const uint64_t* w, size_t B, size_t C) {
  RowSchedule rs;
  uint64_t m[4] = {1, 0, 0, 0};
  for (size_t j = 0; j < B; j++)
    for (int k = 0; k < 4; k++) m[k] |= w[4 * j + k];
  for (int k = 3; k >= 0; k--)
    if (m[k]) {
      rs.nbits = 64 * k + 64 - __builtin_clzll(m[k]);
      break;
    }
  rs.G = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(B, ROW_MAX_CHAINS), ROW_QUADS / C));
  // TPST_ROW_CHAINS=g: that many chains whatever the size (1 = the plain joint chain; tests, A/B timing)
  if (const char* e = getenv("TPST_ROW_CHAINS"))
    if (atoi(e) >= 1) rs.G = (int)std::min<size_t>(std::min<size_t>(B, ROW_MAX_CHAINS), (size_t)atoi(e));
  const size_t heads = (size_t)rs.G * (rs.nbits + 1);
  rs.words.assign(heads, 0);
  for (int g = 0; g < rs.G; g++)
    for (int t = 0; t <= rs.nbits; t++) {
      rs.words[(size_t)g * (rs.nbits + 1) + t] = (uint32_t)(rs.words.size() - heads);
      if (t == rs.nbits) break;
      const int bit = rs.nbits - 1 - t;
      for (size_t j = g; j < B; j += rs.G)
        if ((w[4 * j + (bit >> 6)] >> (bit & 63)) & 1) rs.words.push_back((uint32_t)j);
    }
  return rs;
}

__global__ void __launch_bounds__(64) k_g1_lincomb_rows(const uint32_t* __restrict__ P, size_t C,
                                                        const uint32_t* __restrict__ sched, int nbits,
                                                        Xyzz<Fq>* __restrict__ out) {
  using A = AccField<Fq>;  // the chain computes in the accumulation field (acc_field.h), like k_lincomb2
  using T = typename A::T;
  const uint32_t* off = sched + (size_t)blockIdx.y * (nbits + 1);  // this chain's steps
  const uint32_t* idx = sched + (size_t)gridDim.y * (nbits + 1);
  const size_t q = ((size_t)blockIdx.x * 64 + threadIdx.x) >> 2;
  const int qi = threadIdx.x & 3;
  // the quads past the end redo the last row and store nothing: whole quads (the DPP exchanges)
  const size_t i = q < C ? q : C - 1;
  Xyzz<T> acc = Xyzz<T>::inf();
  uint32_t k = off[0];
  for (int t = 0; t < nbits; t++) {
    acc = lc_dbl_quad(acc, qi);
    for (const uint32_t e = off[t + 1]; k < e; k++)  // uniform over the grid's x
      acc = lc_madd_quad(acc, A::in(load_affine<Fq>(P, (size_t)idx[k] * C + i)), qi);
  }
  if (q < C && qi == 0) store_acc(out, (size_t)blockIdx.y * C + q, acc);
}

// out[i] = sum_g part[g C + i]
__global__ void __launch_bounds__(64) k_g1_rows_sum(const Xyzz<Fq>* __restrict__ part, size_t C, int G,
                                                    Xyzz<Fq>* __restrict__ out) {
  const size_t q = ((size_t)blockIdx.x * 64 + threadIdx.x) >> 2;
  const int qi = threadIdx.x & 3;
  const size_t i = q < C ? q : C - 1;
  auto acc = load_acc(part, i);
  for (int g = 1; g < G; g++) acc = lc_add_quad(acc, load_acc(part, (size_t)g * C + i), qi);
  if (q < C && qi == 0) store_acc(out, q, acc);
}

hipError_t g1_lincomb_rows(hipStream_t s, const uint32_t* d_P, size_t C, const uint32_t* d_sched, int nbits, int G,
                           Xyzz<Fq>* d_part, Xyzz<Fq>* d_out) {
  if (!C) return hipSuccess;
  if (!d_P || !d_sched || !d_out || nbits < 1 || nbits > 256 || G < 1 || G > ROW_MAX_CHAINS || (G > 1 && !d_part))
    return hipErrorInvalidValue;
  const dim3 grid(grid_for(4 * C, 64), (unsigned)G);
  k_g1_lincomb_rows<<<grid, 64, 0, s>>>(d_P, C, d_sched, nbits, G > 1 ? d_part : d_out);
  TPST_TRY(hipGetLastError());
  if (G > 1) {
    k_g1_rows_sum<<<grid_for(4 * C, 64), 64, 0, s>>>(d_part, C, G, d_out);
    TPST_TRY(hipGetLastError());
  }
  return hipSuccess;
}

}  // namespace tpst

using namespace tpst;

namespace {

bool fr_is_zero(const uint64_t* a) { return !(a[0] | a[1] | a[2] | a[3]); }

int weights_ok(tpst_ctx* ctx, const uint64_t* w, size_t B) {
  if (B < 1 || B > LINCOMB_MAX_TERMS) return fail(ctx, TPST_E_ARG, "the number of terms must be 1..256");
  for (size_t j = 0; j < B; j++)
    if (!fr_ok(w + 4 * j)) return fail(ctx, TPST_E_ARG, "weight >= r");
  return TPST_OK;
}

// out = sum_j w_j lists[j] over C rows; arguments validated
int rows_combine(tpst_ctx* ctx, const uint64_t* const* lists, size_t B, size_t C, const uint64_t* w, uint64_t* out) {
  std::atomic<bool> bad(false);
  host::parallel_for(B * ((C + 255) / 256), [&](size_t c) {
    const size_t j = c / ((C + 255) / 256), i0 = 256 * (c % ((C + 255) / 256));
    for (size_t i = i0; i < C && i < i0 + 256; i++)
      if (!point_on_curve<Fq>(lists[j] + 12 * i)) bad.store(true);
  });
  if (bad.load()) return fail(ctx, TPST_E_ARG, "non-canonical coordinate or point off the curve");
  const RowSchedule rs = row_schedule(w, B, C);
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  ctx->io.reset();
  TPST_HIP(ctx, ctx->io.reserve(Arena::need(B * C * 24, 4) + Arena::need(rs.words.size(), 4) +
                                Arena::need((size_t)rs.G * C, sizeof(Xyzz<Fq>)) + Arena::need(C, sizeof(Xyzz<Fq>)) +
                                Arena::need(C * 24, 4)));
  uint32_t* d_p = ctx->io.take<uint32_t>(B * C * 24);
  uint32_t* d_s = ctx->io.take<uint32_t>(rs.words.size());
  Xyzz<Fq>* d_part = ctx->io.take<Xyzz<Fq>>((size_t)rs.G * C);
  Xyzz<Fq>* d_r = ctx->io.take<Xyzz<Fq>>(C);
  uint32_t* d_o = ctx->io.take<uint32_t>(C * 24);
  for (size_t j = 0; j < B; j++)
    TPST_HIP(ctx, hipMemcpyAsync(d_p + j * C * 24, lists[j], C * 96, hipMemcpyHostToDevice, st));
  TPST_HIP(ctx, hipMemcpyAsync(d_s, rs.words.data(), rs.words.size() * 4, hipMemcpyHostToDevice, st));
  TPST_HIP(ctx, points_to_mont<Fq>(st, d_p, d_p, B * C));
  ctx->prof.begin(ST_LINCOMB_ROWS, st);
  TPST_HIP(ctx, g1_lincomb_rows(st, d_p, C, d_s, rs.nbits, rs.G, d_part, d_r));
  ctx->prof.end(ST_LINCOMB_ROWS, st);
  TPST_HIP(ctx, xyzz_to_affine_canonical<Fq>(st, d_r, d_o, C));
  TPST_HIP(ctx, hipMemcpyAsync(out, d_o, C * 96, hipMemcpyDeviceToHost, st));
  TPST_HIP(ctx, hipStreamSynchronize(st));
  return TPST_OK;
}

// T_out = prod_j Ts[j]^(w_j) after a GT membership test of every T_j (canonical coefficients: the caller);
// *in_gt = every T_j is in GT (T_out is written only then)
int gt_combine(tpst_ctx* ctx, const uint64_t* const* Ts, size_t B, const uint64_t* w, uint64_t* T_out, bool* in_gt) {
  std::vector<Fq12> bases(B), pw(B);
  std::vector<uint64_t> dg(4 * B);
  std::vector<uint32_t> okv(B);
  for (size_t j = 0; j < B; j++) {
    Fq* c = reinterpret_cast<Fq*>(&bases[j]);
    for (int q = 0; q < 12; q++) c[q] = fq_canon(Ts[j] + 6 * q);
    base_x_digits(w + 4 * j, &dg[4 * j]);
  }
  {
    std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
    TPST_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    ctx->io.reset();
    TPST_HIP(ctx, ctx->io.reserve(2 * Arena::need(B, sizeof(Fq12)) + Arena::need(B * 4, 8) + Arena::need(B, 4)));
    Fq12* d_b = ctx->io.take<Fq12>(B);
    Fq12* d_o = ctx->io.take<Fq12>(B);
    uint64_t* d_e = ctx->io.take<uint64_t>(B * 4);
    uint32_t* d_ok = ctx->io.take<uint32_t>(B);
    TPST_HIP(ctx, hipMemcpyAsync(d_b, bases.data(), B * sizeof(Fq12), hipMemcpyHostToDevice, st));
    TPST_HIP(ctx, hipMemcpyAsync(d_e, dg.data(), B * 32, hipMemcpyHostToDevice, st));
    TPST_HIP(ctx, gt_pow_wave(st, d_b, d_e, B, d_o, d_ok));
    TPST_HIP(ctx, hipMemcpyAsync(pw.data(), d_o, B * sizeof(Fq12), hipMemcpyDeviceToHost, st));
    TPST_HIP(ctx, hipMemcpyAsync(okv.data(), d_ok, B * 4, hipMemcpyDeviceToHost, st));
    TPST_HIP(ctx, hipStreamSynchronize(st));
  }
  *in_gt = true;
  Fq12 acc = Fq12::one();
  for (size_t j = 0; j < B; j++) {
    if (!okv[j]) *in_gt = false;
    if (okv[j] && !fr_is_zero(w + 4 * j)) acc = mul(acc, pw[j]);
  }
  if (!*in_gt) return TPST_OK;
  const Fq* c = reinterpret_cast<const Fq*>(&acc);
  for (int q = 0; q < 12; q++) fq_out(c[q], T_out + 6 * q);
  return TPST_OK;
}

}  // namespace

extern "C" int tpst_poly_lincomb(tpst_ctx* ctx, tpst_poly* const* polys, size_t B, const uint64_t* w,
                                 tpst_poly** out) {
  if (!ctx) return TPST_E_ARG;
  if (!polys || !w || !out) return fail(ctx, TPST_E_ARG, "null argument");
  if (int rc = weights_ok(ctx, w, B)) return rc;
  for (size_t j = 0; j < B; j++) {
    if (!polys[j]) return fail(ctx, TPST_E_ARG, "null polynomial " + std::to_string(j));
    if (polys[j]->ctx != ctx) return fail(ctx, TPST_E_ARG, "polynomial of another context");
    if (polys[j]->n != polys[0]->n) return fail(ctx, TPST_E_ARG, "polynomials differ in num_vars");
  }
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  std::vector<const uint32_t*> tabs(B);
  for (size_t j = 0; j < B; j++) {
    tabs[j] = polys[j]->q_only ? nullptr : poly_evals(polys[j]);
    if (!tabs[j]) return fail(ctx, TPST_E_STATE, "operation needs whole polynomials (a column slice or q-only handle)");
    if ((uintptr_t)tabs[j] & 15) return fail(ctx, TPST_E_ARG, "evaluation table not 16-byte aligned");
  }
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  const tpst_poly* p0 = polys[0];
  const size_t N = (size_t)1 << p0->n;
  auto p = std::make_unique<tpst_poly>();
  p->ctx = ctx;
  p->n = p0->n;
  p->m_col = p0->m_col;
  p->m_row = p0->m_row;
  p->odd = p0->odd;
  TPST_HIP(ctx, p->Zown.alloc(N * 32));
  std::vector<Fr> wm(B);
  for (size_t j = 0; j < B; j++) wm[j] = fr_canon(w + 4 * j);
  hipStream_t st = ctx->stream;
  ctx->io.reset();
  TPST_HIP(ctx, ctx->io.reserve(Arena::need(B, sizeof(void*)) + Arena::need(B, sizeof(Fr))));
  const uint32_t** d_tabs = ctx->io.take<const uint32_t*>(B);
  uint32_t* d_w = ctx->io.take<uint32_t>(B * 8);
  TPST_HIP(ctx, hipMemcpyAsync(d_tabs, tabs.data(), B * sizeof(void*), hipMemcpyHostToDevice, st));
  TPST_HIP(ctx, hipMemcpyAsync(d_w, wm.data(), B * sizeof(Fr), hipMemcpyHostToDevice, st));
  ctx->prof.begin(ST_FR_LINCOMB, st);
  TPST_HIP(ctx, fr_lincomb(st, d_tabs, d_w, B, N, p->Zown.u()));
  ctx->prof.end(ST_FR_LINCOMB, st);
  TPST_HIP(ctx, hipStreamSynchronize(st));
  p->d_Z = p->Zown.u();
  *out = p.release();
  return TPST_OK;
}

extern "C" int tpst_poly_evaluations(tpst_ctx* ctx, const tpst_poly* p, uint64_t* Z) {
  if (!ctx) return TPST_E_ARG;
  if (!p || !Z) return fail(ctx, TPST_E_ARG, "null argument");
  if (p->ctx != ctx) return fail(ctx, TPST_E_ARG, "polynomial of another context");
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  const uint32_t* d_Z = p->q_only ? nullptr : poly_evals(p);
  if (!d_Z) return fail(ctx, TPST_E_STATE, "operation needs a whole polynomial (a column slice or q-only handle)");
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  TPST_HIP(ctx, hipMemcpyAsync(Z, d_Z, ((size_t)1 << p->n) * 32, hipMemcpyDeviceToHost, ctx->stream));
  TPST_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return TPST_OK;
}

extern "C" int tpst_g1_lincomb_rows(tpst_ctx* ctx, const uint64_t* const* lists, size_t B, size_t C,
                                    const uint64_t* w, uint64_t* out) {
  if (!ctx) return TPST_E_ARG;
  if (!lists || !w || !out) return fail(ctx, TPST_E_ARG, "null argument");
  if (int rc = weights_ok(ctx, w, B)) return rc;
  for (size_t j = 0; j < B; j++)
    if (!lists[j]) return fail(ctx, TPST_E_ARG, "null list " + std::to_string(j));
  if (C < 1 || C > ((size_t)1 << 26) / B) return fail(ctx, TPST_E_ARG, "rows out of range (1 .. 2^26 / B)");
  return rows_combine(ctx, lists, B, C, w, out);
}

extern "C" int tpst_commit_lincomb(tpst_ctx* ctx, int n, const uint64_t* const* comms, const uint64_t* const* Ts,
                                   size_t B, const uint64_t* w, uint64_t* comms_out, uint64_t* T_out) {
  if (!ctx) return TPST_E_ARG;
  if (!w || (!comms && !Ts) || (comms && !comms_out) || (Ts && !T_out)) return fail(ctx, TPST_E_ARG, "null argument");
  int m_col, m_row, odd;
  if (poly_dims(n, m_col, m_row, odd)) return fail(ctx, TPST_E_ARG, "bad num_vars");
  if (int rc = weights_ok(ctx, w, B)) return rc;
  const size_t C = (size_t)1 << m_col;
  if (C > ((size_t)1 << 26) / B) return fail(ctx, TPST_E_ARG, "more than 2^26 row commitments: split the combination");
  for (size_t j = 0; j < B; j++) {
    if ((comms && !comms[j]) || (Ts && !Ts[j])) return fail(ctx, TPST_E_ARG, "null commitment " + std::to_string(j));
    if (Ts && !gt_ok(Ts[j])) return fail(ctx, TPST_E_ARG, "non-canonical T " + std::to_string(j));
  }
  if (Ts) {  // first: a T outside GT fails the call before anything is written
    bool in_gt = false;
    uint64_t T[72];
    if (int rc = gt_combine(ctx, Ts, B, w, T, &in_gt)) return rc;
    if (!in_gt) return fail(ctx, TPST_E_ARG, "T outside GT");
    if (comms)
      if (int rc = rows_combine(ctx, comms, B, C, w, comms_out)) return rc;
    memcpy(T_out, T, 576);
    return TPST_OK;
  }
  return rows_combine(ctx, comms, B, C, w, comms_out);
}

extern "C" int tpst_pst_combine_challenge(tpst_transcript* tr, int n, const uint64_t* point, const uint64_t* const* Ts,
                                          const uint64_t* vs, size_t B, uint64_t* w_out) {
  if (!tr || !point || !Ts || !vs || !w_out || n < 0 || B < 1 || B > LINCOMB_MAX_TERMS) return TPST_E_ARG;
  for (size_t j = 0; j < B; j++)
    if (!Ts[j] || !fr_ok(vs + 4 * j)) return TPST_E_ARG;
  for (int i = 0; i < n; i++)
    if (!fr_ok(point + 4 * i)) return TPST_E_ARG;
  Sponge sp;
  sp.load(tr);
  for (size_t j = 0; j < B; j++) sp.absorb_bytes((const uint8_t*)Ts[j], 576);  // append_gt
  auto append_fr = [&](const uint64_t* fr) {  // tpst_transcript_append_fr
    const uint64_t l[6] = {fr[0], fr[1], fr[2], fr[3], 0, 0};
    sp.absorb(std::vector<Fq>{fq_canon(l)});
  };
  for (int i = 0; i < n; i++) append_fr(point + 4 * i);
  for (size_t j = 0; j < B; j++) append_fr(vs + 4 * j);
  uint64_t rho[4];
  sp.challenge(rho);
  sp.store(tr);
  const Fr r = fr_canon(rho);
  Fr p = Fr::one();
  for (size_t j = 0; j < B; j++) {  // w_j = rho^j
    fr_out(p, w_out + 4 * j);
    p = mul(p, r);
  }
  return TPST_OK;
}

extern "C" int tpst_poly_open_combined(tpst_ctx* ctx, tpst_poly* const* polys, const uint64_t* const* comms,
                                       const uint64_t* const* Ts, size_t B, const uint64_t* w, tpst_transcript* tr,
                                       const uint64_t* point, uint64_t* comms_out, uint64_t* T_out, uint64_t* v_out,
                                       tpst_open_proof* proof) {
  if (!ctx) return TPST_E_ARG;
  if (!polys || !comms || !Ts || !w || !tr || !point || !comms_out || !T_out || !v_out || !proof)
    return fail(ctx, TPST_E_ARG, "null argument");
  if (int rc = weights_ok(ctx, w, B)) return rc;
  for (size_t j = 0; j < B; j++)
    if (fr_is_zero(w + 4 * j)) return fail(ctx, TPST_E_ARG, "zero weight: polynomial " + std::to_string(j) + " would not be bound");
  tpst_poly* z = nullptr;
  if (int rc = tpst_poly_lincomb(ctx, polys, B, w, &z)) return rc;
  std::unique_ptr<tpst_poly> hold(z);
  if (int rc = tpst_commit_lincomb(ctx, z->n, comms, Ts, B, w, comms_out, T_out)) return rc;
  if (int rc = tpst_poly_eval(ctx, z, point, v_out)) return rc;
  return tpst_poly_open(ctx, z, tr, comms_out, point, T_out, proof);
}

extern "C" int tpst_pst_verify_combined(tpst_ctx* ctx, tpst_transcript* tr, int n, const uint64_t* point,
                                        const uint64_t* vs, const uint64_t* const* Ts, size_t B, const uint64_t* w,
                                        const tpst_open_proof* proof) {
  if (!ctx) return TPST_E_ARG;
  if (!tr || !point || !vs || !Ts || !w || !proof) return fail(ctx, TPST_E_ARG, "null argument");
  if (B < 1 || B > LINCOMB_MAX_TERMS) return fail(ctx, TPST_E_ARG, "the number of terms must be 1..256");
  for (size_t j = 0; j < B; j++)
    if (!Ts[j]) return fail(ctx, TPST_E_ARG, "null commitment " + std::to_string(j));
  // every element is validated before the sponge absorbs anything
  for (size_t j = 0; j < B; j++) {
    if (!fr_ok(vs + 4 * j) || !fr_ok(w + 4 * j)) return fail(ctx, TPST_E_VERIFY, "value or weight >= r");
    if (fr_is_zero(w + 4 * j)) return fail(ctx, TPST_E_VERIFY, "zero weight");
    if (!gt_ok(Ts[j])) return fail(ctx, TPST_E_VERIFY, "non-canonical T " + std::to_string(j));
  }
  bool in_gt = false;
  uint64_t T[72], v[4];
  if (int rc = gt_combine(ctx, Ts, B, w, T, &in_gt)) return rc;
  if (!in_gt) return fail(ctx, TPST_E_VERIFY, "T outside GT");
  Fr acc = Fr::zero();
  for (size_t j = 0; j < B; j++) acc = add(acc, mul(fr_canon(w + 4 * j), fr_canon(vs + 4 * j)));
  fr_out(acc, v);
  tpst_transcript t = *tr;
  const int rc = tpst_pst_verify(ctx, &t, n, point, v, T, proof);
  if (rc == TPST_OK) *tr = t;
  return rc;
}
