// Batched double-scalar multiplication out[i] = s_i P_i + t_i Q_i (lincomb.h).
//
// One quad of lanes (coop.h) per output, 16 outputs per wave.  The batches
// this serves are a few hundred to a few thousand outputs (the batch
// verifier's pairing inputs), far fewer than the chip has lanes, so the
// launch is bound by the latency of one chain, not by throughput: the quad
// forms cut a doubling from 9 serial field products to 3 and an addition from
// 12 to 4, and four times as many waves still leave most SIMDs idle.
//
// Joint double-and-add (Shamir): the quad tabulates P, Q and P + Q as XYZZ in
// LDS (lane 0, 1, 2 of the quad write one entry each; word-major, so the 16
// quads of the wave read 16 different banks), then walks the scalars from bit
// nbits - 1 down: one quad doubling per bit and, where (s, t) has a bit set,
// one quad addition of the selected entry.  The three entries go through the
// same addition, so quads of one wave that select different entries do not
// serialise three additions.  Every special case is the formulas' own: the
// addition returns the other operand for infinity, doubles on equal operands
// and gives infinity on opposite ones (add-2008-s as curve.h has it), so P = Q (the entry
// P + Q is a doubling), P = -Q (it is infinity), an input at infinity, zero
// scalars and a result at infinity need no code here.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/tpst.h"
#include "acc_field.h"
#include "coop.h"
#include "ctx.h"
#include "device_util.h"
#include "host_curve.h"
#include "lincomb.h"
#include "lincomb_quad.h"
#include "pst_state.h"  // fr_ok, point_on_curve

namespace tpst {

// p + (table entry `col`), lc_add_quad with the entry left in LDS: a lane
// reads only the two coordinates its own products take (L1: ZZ2, X2, ZZZ2, Y2
// for lane 0..3; L2: ZZ2, ZZZ2 for lane 2, 3) instead of holding all four,
// which is what keeps the G2 chain inside the register file.  Row W of the
// table is the entry's infinity flag.
template <class F, int W>
__device__ __forceinline__ F tab_coord(const uint32_t (*tab)[48], int col, int c) {
  F r;
  uint32_t* d = reinterpret_cast<uint32_t*>(&r);
#pragma unroll
  for (int k = 0; k < Words<F>::n; k++) d[k] = tab[c * Words<F>::n + k][col];
  return r;
}
template <class F, int W>
__device__ __forceinline__ Xyzz<F> lc_add_tab(const Xyzz<F>& p, const uint32_t (*tab)[48], int col, int qi) {
  if (tab[W][col]) return p;
  if (is_zero(p.ZZ))
    return {tab_coord<F, W>(tab, col, 0), tab_coord<F, W>(tab, col, 1), tab_coord<F, W>(tab, col, 2),
            tab_coord<F, W>(tab, col, 3)};
  const F e1 = tab_coord<F, W>(tab, col, qi == 0 ? 2 : qi == 1 ? 0 : qi == 2 ? 3 : 1);
  const F e2 = tab_coord<F, W>(tab, col, qi == 3 ? 3 : 2);
  // L1: U1 = X1 ZZ2, U2 = X2 ZZ1, S1 = Y1 ZZZ2, S2 = Y2 ZZZ1
  F r = mul(pick4(qi, p.X, p.ZZ, p.Y, p.ZZZ), e1);
  const F U1 = quad_bcast<0>(r), U2 = quad_bcast<1>(r), S1 = quad_bcast<2>(r), S2 = quad_bcast<3>(r);
  const F P = sub(U2, U1), R = sub(S2, S1);
  if (is_zero(P)) {
    if (is_zero(R)) return lc_dbl_quad(p, qi);
    return Xyzz<F>::inf();
  }
  // L2: PP = P^2, RR = R^2, Z12 = ZZ1 ZZ2, T12 = ZZZ1 ZZZ2
  const F l2 = pick4(qi, P, R, p.ZZ, p.ZZZ);
  r = mul(l2, pick(qi < 2, l2, e2));
  const F PP = quad_bcast<0>(r), RR = quad_bcast<1>(r), Z12 = quad_bcast<2>(r), T12 = quad_bcast<3>(r);
  // L3: PPP = P PP, Q = U1 PP, ZZ' = Z12 PP
  r = mul(pick4(qi, P, U1, Z12, Z12), PP);
  const F PPP = quad_bcast<0>(r), Q = quad_bcast<1>(r);
  Xyzz<F> o;
  o.ZZ = quad_bcast<2>(r);
  o.X = sub(sub(RR, PPP), dbl(Q));
  // L4: R (Q - X'), S1 PPP, ZZZ' = T12 PPP
  r = mul(pick4(qi, R, S1, T12, T12), pick(qi == 0, sub(Q, o.X), PPP));
  o.Y = sub(quad_bcast<0>(r), quad_bcast<1>(r));
  o.ZZZ = quad_bcast<2>(r);
  return o;
}

template <class F>
__global__ void __launch_bounds__(64) k_lincomb2(const uint32_t* __restrict__ P, const uint32_t* __restrict__ s,
                                                 const uint32_t* __restrict__ Q, const uint32_t* __restrict__ t,
                                                 size_t n, int nbits, Xyzz<F>* __restrict__ out) {
  using A = AccField<F>;  // the chain computes in the accumulation field (acc_field.h), like the MSM's tails
  using T = typename A::T;
  constexpr int W = 4 * Words<T>::n;  // u32 per XYZZ entry
  // [word][3 quad + entry]: P, Q, P + Q of the wave's 16 quads; row W: the entry is infinity
  __shared__ uint32_t tab[W + 1][48];
  const size_t q = ((size_t)blockIdx.x * 64 + threadIdx.x) >> 2;
  const int qi = threadIdx.x & 3, slot = 3 * (int)(threadIdx.x >> 2);
  // the quads past the end redo the last output and store nothing: whole
  // quads (the DPP exchanges) and the whole wave at the barrier
  const size_t i = q < n ? q : n - 1;
  const Affine<F> p = load_affine<F>(P, i);
  const Affine<F> pq = Q ? load_affine<F>(Q, i) : Affine<F>::inf();
  {
    const Xyzz<T> xp = to_xyzz(A::in(p)), xq = to_xyzz(A::in(pq));
    Xyzz<T> e = lc_add_quad(xp, xq, qi);
    if (qi == 0) e = xp;
    if (qi == 1) e = xq;
    if (qi < 3) {
      const uint32_t* w = reinterpret_cast<const uint32_t*>(&e);
#pragma unroll
      for (int k = 0; k < W; k++) tab[k][slot + qi] = w[k];
      tab[W][slot + qi] = is_zero(e.ZZ) ? 1u : 0u;
    }
  }
  __syncthreads();
  Xyzz<T> acc = Xyzz<T>::inf();
  const int top = (nbits - 1) >> 5;
  for (int wd = top; wd >= 0; wd--) {
    const uint32_t sw = s[8 * i + wd], tw = t ? t[8 * i + wd] : 0u;
    for (int b = wd == top ? (nbits - 1) & 31 : 31; b >= 0; b--) {
      acc = lc_dbl_quad(acc, qi);
      const int sel = (int)((sw >> b) & 1u) | ((int)((tw >> b) & 1u) << 1);
      if (sel) acc = lc_add_tab<T, W>(acc, tab, slot + sel - 1, qi);  // quad-uniform
    }
  }
  if (q < n && qi == 0) store_acc(out, q, acc);
}

template <class F>
hipError_t lincomb2(hipStream_t s, const uint32_t* d_P, const uint32_t* d_s, const uint32_t* d_Q,
                    const uint32_t* d_t, size_t n, int nbits, Xyzz<F>* d_out) {
  if (!n) return hipSuccess;
  if (!d_P || !d_s || !d_out || (d_Q == nullptr) != (d_t == nullptr) || nbits < 1 || nbits > 256)
    return hipErrorInvalidValue;
  k_lincomb2<F><<<grid_for(4 * n, 64), 64, 0, s>>>(d_P, d_s, d_Q, d_t, n, nbits, d_out);
  return hipGetLastError();
}

template hipError_t lincomb2<Fq>(hipStream_t, const uint32_t*, const uint32_t*, const uint32_t*, const uint32_t*,
                                 size_t, int, Xyzz<Fq>*);
template hipError_t lincomb2<Fq2>(hipStream_t, const uint32_t*, const uint32_t*, const uint32_t*, const uint32_t*,
                                  size_t, int, Xyzz<Fq2>*);

}  // namespace tpst

using namespace tpst;

namespace {

// bits of the longest scalar (at least 1)
int scalar_bits(const uint64_t* s, size_t n) {
  uint64_t m[4] = {1, 0, 0, 0};
  for (size_t i = 0; i < n; i++)
    for (int k = 0; k < 4; k++) m[k] |= s[4 * i + k];
  for (int k = 3; k >= 0; k--)
    if (m[k]) return 64 * k + 64 - __builtin_clzll(m[k]);
  return 1;
}

template <class F>
int lincomb_host(tpst_ctx* ctx, const uint64_t* P, const uint64_t* s, const uint64_t* Q, const uint64_t* t, size_t n,
                 uint64_t* out) {
  if (!ctx) return TPST_E_ARG;
  if (n == 0) return TPST_OK;
  if (!P || !s || !out || (Q == nullptr) != (t == nullptr)) return fail(ctx, TPST_E_ARG, "null argument");
  if (n > ((size_t)1 << 26)) return fail(ctx, TPST_E_ARG, "more than 2^26 outputs: split the batch");
  constexpr size_t PW = 2 * Words<F>::n, P64 = PW / 2;  // u32 / u64 per affine point
  std::atomic<bool> bad(false);
  host::parallel_for((n + 255) / 256, [&](size_t c) {
    for (size_t i = 256 * c; i < n && i < 256 * (c + 1); i++) {
      bool ok = fr_ok(s + 4 * i) && point_on_curve<F>(P + P64 * i);
      if (Q) ok = ok && fr_ok(t + 4 * i) && point_on_curve<F>(Q + P64 * i);
      if (!ok) bad.store(true);
    }
  });
  if (bad.load()) return fail(ctx, TPST_E_ARG, "scalar >= r, non-canonical coordinate or point off its curve");
  const int nbits = std::max(scalar_bits(s, n), Q ? scalar_bits(t, n) : 1);
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t np = Q ? 2 * n : n;  // points and scalars uploaded: P then Q, s then t
  ctx->io.reset();
  TPST_HIP(ctx, ctx->io.reserve(Arena::need(np * PW, 4) + Arena::need(np * 8, 4) + Arena::need(n, sizeof(Xyzz<F>)) +
                                Arena::need(n * PW, 4)));
  uint32_t* d_p = ctx->io.take<uint32_t>(np * PW);
  uint32_t* d_s = ctx->io.take<uint32_t>(np * 8);
  Xyzz<F>* d_r = ctx->io.take<Xyzz<F>>(n);
  uint32_t* d_o = ctx->io.take<uint32_t>(n * PW);
  TPST_HIP(ctx, hipMemcpyAsync(d_p, P, n * PW * 4, hipMemcpyHostToDevice, st));
  TPST_HIP(ctx, hipMemcpyAsync(d_s, s, n * 32, hipMemcpyHostToDevice, st));
  if (Q) {
    TPST_HIP(ctx, hipMemcpyAsync(d_p + n * PW, Q, n * PW * 4, hipMemcpyHostToDevice, st));
    TPST_HIP(ctx, hipMemcpyAsync(d_s + n * 8, t, n * 32, hipMemcpyHostToDevice, st));
  }
  TPST_HIP(ctx, points_to_mont<F>(st, d_p, d_p, np));
  ctx->prof.begin(ST_LINCOMB, st);
  TPST_HIP(ctx, lincomb2<F>(st, d_p, d_s, Q ? d_p + n * PW : nullptr, Q ? d_s + n * 8 : nullptr, n, nbits, d_r));
  ctx->prof.end(ST_LINCOMB, st);
  TPST_HIP(ctx, xyzz_to_affine_canonical<F>(st, d_r, d_o, n));
  TPST_HIP(ctx, hipMemcpyAsync(out, d_o, n * PW * 4, hipMemcpyDeviceToHost, st));
  TPST_HIP(ctx, hipStreamSynchronize(st));
  return TPST_OK;
}

}  // namespace

extern "C" int tpst_g1_lincomb_batch(tpst_ctx* ctx, const uint64_t* P, const uint64_t* s, const uint64_t* Q,
                                     const uint64_t* t, size_t n, uint64_t* out) {
  return lincomb_host<Fq>(ctx, P, s, Q, t, n, out);
}

extern "C" int tpst_g2_lincomb_batch(tpst_ctx* ctx, const uint64_t* P, const uint64_t* s, const uint64_t* Q,
                                     const uint64_t* t, size_t n, uint64_t* out) {
  return lincomb_host<Fq2>(ctx, P, s, Q, t, n, out);
}
