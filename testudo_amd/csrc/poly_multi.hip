// One sqrt-PST proof for B polynomials opened at many points (include/tpst.h,
// "multi-point opening"; this project's own protocol, no counterpart in the
// reference).  K claims f_{j_k}(r_k) = v_k are reduced by a sum-check to B
// claims at one point rho, which the combined opening (poly_lincomb.hip) then
// proves.  With a_k = gamma^k the summand is
//   g(x) = sum_j D_j(x) f_j(x),   D_j(x) = sum_{k: j_k = j} a_k eq(r_k, x),
// D_j multilinear: 2B tables are bound however many claims there are.
//
//   k_multi_eq_halves  per claim the chi tables of its point's two halves
//                      (2^ceil(n/2) and 2^floor(n/2) entries, a_k folded into
//                      the first): eq(r_k, x) = EH_k[x >> lo] EL_k[x & mask] as
//                      k_eq_outer forms it, so no 2^n eq table is ever made.
//   k_multi_round<0>   round 0: F_j straight from the handles (never written),
//                      D_j on the fly from the half tables.
//   k_multi_round<1>   round 1: binds rho_0 while reading the same sources and
//                      writes the first scratch tables, 2B of 2^(n-1) Fr.
//   k_multi_round<2>   later rounds: bind in place.  Lane i reads entries i,
//                      i + h/2, i + h, i + h + h/2 of a table of length 2h and
//                      writes i and i + h/2: no other lane touches those four,
//                      in the grid-stride loop either, so no lane reads what
//                      another has overwritten.
//   k_multi_reduce     the workgroups' partial sums -> s(0), s(2).
// D is kept in Montgomery form and F canonical: a Montgomery product of the
// two is the canonical product, a bind r (b - a) with r in Montgomery form
// keeps either form (k_fr_lincomb's trick), so no conversion pass runs and the
// sums come out canonical.  One lane per index pair, two 128-bit accesses per
// entry, grid-stride over a bounded grid, LDS tree per workgroup, no atomics:
// exact field sums, independent of the grid.  Claim and polynomial indices are
// uniform over the wave.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/tpst.h"
#include "ctx.h"
#include "device_util.h"
#include "fr_mem.h"
#include "poly_lincomb.h"
#include "poly_multi.h"
#include "poseidon_host.h"
#include "pst_state.h"
#include "r1cs_state.h"

namespace tpst {

namespace {

constexpr int MP_BS = 256;
// a few resident workgroups per CU keep the loads in flight; the stride loop covers the rest
constexpr unsigned MP_MAX_GRID = 256 * 8;

// thread t < K (2^hi + 2^lo): entry i of claim c's high table (i < 2^hi) or of its low table
__global__ void __launch_bounds__(MP_BS) k_multi_eq_halves(const uint32_t* __restrict__ pts,
                                                           const uint32_t* __restrict__ a, int n, int hi, size_t K,
                                                           uint32_t* __restrict__ eh, uint32_t* __restrict__ el) {
  const int lo = n - hi;
  const size_t nh = (size_t)1 << hi, per = nh + ((size_t)1 << lo);
  const size_t t = (size_t)blockIdx.x * MP_BS + threadIdx.x;
  if (t >= K * per) return;
  const size_t c = t / per, i = t % per;
  const bool high = i < nh;
  const size_t x = high ? i : i - nh;
  const int ell = high ? hi : lo;
  const uint32_t* r = pts + 8 * (c * (size_t)n + (high ? 0 : hi));
  Fr prod = high ? ld_fr16(a + 8 * c) : Fr::one();
  for (int j = 0; j < ell; j++) {  // MSB-first, as k_eq_evals
    const Fr rj = ld_fr16(r + 8 * j);
    prod = mul(prod, ((x >> (ell - 1 - j)) & 1) ? rj : sub(Fr::one(), rj));
  }
  st_fr16(high ? eh + 8 * ((c << hi) + x) : el + 8 * ((c << lo) + x), prod);
}

// D_j(x) for the claims [c0, c1) of polynomial j (uniform over the wave), Montgomery
__device__ __forceinline__ Fr d_at(const MultiSrc& s, uint32_t c0, uint32_t c1, size_t x) {
  const size_t xh = x >> s.lo, xl = x & (((size_t)1 << s.lo) - 1);
  Fr acc = Fr::zero();
  for (uint32_t c = c0; c < c1; c++)
    acc = add(acc, mul(ld_fr16(s.eh + 8 * (((size_t)c << s.hi) + xh)), ld_fr16(s.el + 8 * (((size_t)c << s.lo) + xl))));
  return acc;
}

// MODE 0: the tables (src) have length h, nothing is bound.
// MODE 1: src has length 2h; X'[y] = X[y] + r (X[y + h] - X[y]) is written to the scratch tables (length h).
// MODE 2: the same bind in the scratch tables in place.
// Then, unless h == 1 (the closing bind), the sums over the pairs (i, i + h/2), i < h/2, of the tables of length h.
template <int MODE>
__global__ void __launch_bounds__(MP_BS) k_multi_round(MultiSrc src, uint32_t* scr, size_t scr_stride, int B, size_t h,
                                                       const uint32_t* __restrict__ r, int do_sum,
                                                       uint32_t* __restrict__ partial) {
  __shared__ Fr sh[2][MP_BS];
  const size_t half = h >> 1;
  const size_t npairs = half ? half : 1;
  const size_t stride = (size_t)gridDim.x * MP_BS;
  Fr rr = Fr::zero();
  if (MODE != 0) rr = ld_fr16(r);
  Fr s0 = Fr::zero(), s2 = Fr::zero();
  for (size_t i = (size_t)blockIdx.x * MP_BS + threadIdx.x; i < npairs; i += stride) {
    const size_t i1 = i + half;
    for (int j = 0; j < B; j++) {
      Fr dlo, dhi = Fr::zero(), flo, fhi = Fr::zero();
      uint32_t* D = scr + 8 * (size_t)j * scr_stride;
      uint32_t* F = scr + 8 * (size_t)(B + j) * scr_stride;
      if (MODE == 2) {
        dlo = bind_top(rr, ld_fr16(D + 8 * i), ld_fr16(D + 8 * (i + h)));
        flo = bind_top(rr, ld_fr16(F + 8 * i), ld_fr16(F + 8 * (i + h)));
        if (half) {
          dhi = bind_top(rr, ld_fr16(D + 8 * i1), ld_fr16(D + 8 * (i1 + h)));
          fhi = bind_top(rr, ld_fr16(F + 8 * i1), ld_fr16(F + 8 * (i1 + h)));
        }
      } else {
        const uint32_t c0 = src.cptr[j], c1 = src.cptr[j + 1];
        const uint32_t* Z = src.tabs[j];
        if (MODE == 0) {
          dlo = d_at(src, c0, c1, i);
          flo = ld_fr16(Z + 8 * i);
          if (half) {
            dhi = d_at(src, c0, c1, i1);
            fhi = ld_fr16(Z + 8 * i1);
          }
        } else {
          dlo = bind_top(rr, d_at(src, c0, c1, i), d_at(src, c0, c1, i + h));
          flo = bind_top(rr, ld_fr16(Z + 8 * i), ld_fr16(Z + 8 * (i + h)));
          if (half) {
            dhi = bind_top(rr, d_at(src, c0, c1, i1), d_at(src, c0, c1, i1 + h));
            fhi = bind_top(rr, ld_fr16(Z + 8 * i1), ld_fr16(Z + 8 * (i1 + h)));
          }
        }
      }
      if (MODE != 0) {
        st_fr16(D + 8 * i, dlo);
        st_fr16(F + 8 * i, flo);
        if (half) {
          st_fr16(D + 8 * i1, dhi);
          st_fr16(F + 8 * i1, fhi);
        }
      }
      if (do_sum && half) {
        s0 = add(s0, mul(dlo, flo));
        s2 = add(s2, mul(sub(dbl(dhi), dlo), sub(dbl(fhi), flo)));  // at t = 2: 2 hi - lo
      }
    }
  }
  if (!do_sum) return;
  sh[0][threadIdx.x] = s0;
  sh[1][threadIdx.x] = s2;
  __syncthreads();
  for (int w = MP_BS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
      for (int k = 0; k < 2; k++) sh[k][threadIdx.x] = add(sh[k][threadIdx.x], sh[k][threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x < 2) st_fr16(partial + 8 * (2 * (size_t)blockIdx.x + threadIdx.x), sh[threadIdx.x][0]);
}

// sum nblk partial pairs -> out[2] (canonical, as the partials are)
__global__ void __launch_bounds__(MP_BS) k_multi_reduce(const uint32_t* __restrict__ partial, unsigned nblk,
                                                        uint32_t* __restrict__ out) {
  __shared__ Fr sh[2][MP_BS];
  Fr a[2] = {Fr::zero(), Fr::zero()};
  for (unsigned b = threadIdx.x; b < nblk; b += MP_BS)
    for (int k = 0; k < 2; k++) a[k] = add(a[k], ld_fr16(partial + 8 * (2 * (size_t)b + k)));
  for (int k = 0; k < 2; k++) sh[k][threadIdx.x] = a[k];
  __syncthreads();
  for (int w = MP_BS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
      for (int k = 0; k < 2; k++) sh[k][threadIdx.x] = add(sh[k][threadIdx.x], sh[k][threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x < 2) st_fr16(out + 8 * threadIdx.x, sh[threadIdx.x][0]);
}

// u[j] = entry 0 of table F_j
__global__ void k_multi_finals(const uint32_t* __restrict__ scr, size_t scr_stride, int B, uint32_t* __restrict__ u) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < B) st_fr16(u + 8 * j, ld_fr16(scr + 8 * (size_t)(B + j) * scr_stride));
}

}  // namespace

hipError_t multi_eq_halves(hipStream_t s, const uint32_t* d_pts, const uint32_t* d_a, int n, size_t K, uint32_t* d_eh,
                           uint32_t* d_el) {
  if (!d_pts || !d_a || !d_eh || !d_el || n < 2 || n > 40 || K < 1 || K > MULTI_MAX_CLAIMS) return hipErrorInvalidValue;
  const int hi = n - n / 2;
  const size_t total = K * (((size_t)1 << hi) + ((size_t)1 << (n - hi)));
  k_multi_eq_halves<<<grid_for(total, MP_BS), MP_BS, 0, s>>>(d_pts, d_a, n, hi, K, d_eh, d_el);
  return hipGetLastError();
}

unsigned multi_round_grid(size_t pairs) {
  size_t cap = MP_MAX_GRID;
  // TPST_MULTI_GRID=g: at most g workgroups whatever the size (tests: the sums do not depend on the grid)
  if (const char* e = getenv("TPST_MULTI_GRID"))
    if (atoi(e) >= 1) cap = std::min<size_t>((size_t)atoi(e), MP_MAX_GRID);
  return (unsigned)std::min<size_t>(std::max<size_t>(grid_for(pairs, MP_BS), 1), cap);
}

hipError_t multi_round(hipStream_t s, int round, const MultiSrc& src, uint32_t* d_scr, size_t scr_stride, int B,
                       size_t h, const uint32_t* d_r, int do_sum, uint32_t* d_partial, uint32_t* d_sums) {
  if (B < 1 || B > (int)LINCOMB_MAX_TERMS || h < 1 || round < 0 || (round && (!d_r || !d_scr || scr_stride < h)) ||
      (round < 2 && (!src.tabs || !src.cptr || !src.eh || !src.el)) || (do_sum && (!d_partial || !d_sums || h < 2)))
    return hipErrorInvalidValue;
  const unsigned grid = multi_round_grid(h >> 1);
  if (round == 0)
    k_multi_round<0><<<grid, MP_BS, 0, s>>>(src, d_scr, scr_stride, B, h, d_r, do_sum, d_partial);
  else if (round == 1)
    k_multi_round<1><<<grid, MP_BS, 0, s>>>(src, d_scr, scr_stride, B, h, d_r, do_sum, d_partial);
  else
    k_multi_round<2><<<grid, MP_BS, 0, s>>>(src, d_scr, scr_stride, B, h, d_r, do_sum, d_partial);
  TPST_TRY(hipGetLastError());
  if (!do_sum) return hipSuccess;
  k_multi_reduce<<<1, MP_BS, 0, s>>>(d_partial, grid, d_sums);
  return hipGetLastError();
}

int multi_sumcheck(tpst_ctx* ctx, const uint32_t* const* tabs, size_t B, int n, const uint32_t* claim_poly,
                   const uint64_t* points, const uint64_t* a, size_t K, const MultiChallenge& challenge, uint64_t* u) {
  const int lo = n / 2, hi = n - lo;
  const size_t N = (size_t)1 << n, half = N >> 1;
  // the claims sorted by polynomial (stable), Montgomery points and weights
  std::vector<uint32_t> cptr(B + 1, 0), order(K);
  for (size_t k = 0; k < K; k++) cptr[claim_poly[k] + 1]++;
  for (size_t j = 0; j < B; j++) cptr[j + 1] += cptr[j];
  {
    std::vector<uint32_t> at(cptr.begin(), cptr.end() - 1);
    for (size_t k = 0; k < K; k++) order[at[claim_poly[k]]++] = (uint32_t)k;
  }
  std::vector<Fr> pm(K * (size_t)n), am(K);
  for (size_t c = 0; c < K; c++) {
    am[c] = fr_canon(a + 4 * (size_t)order[c]);
    for (int i = 0; i < n; i++) pm[c * n + i] = fr_canon(points + 4 * ((size_t)order[c] * n + i));
  }

  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  // everything the rounds touch is reserved here, before the first launch
  if (int rc = ensure_pinned(ctx, 4096)) return rc;
  uint64_t(*hs)[4] = reinterpret_cast<uint64_t(*)[4]>(ctx->pinned);  // the round's sums down
  uint32_t* rpin = reinterpret_cast<uint32_t*>((char*)ctx->pinned + 1024);  // the challenge up
  const unsigned grid0 = multi_round_grid(half);
  Arena& ar = ctx->arena;
  ar.reset();
  TPST_HIP(ctx, ar.reserve(Arena::need(B, sizeof(void*)) + Arena::need(B + 1, 4) + Arena::need(pm.size(), sizeof(Fr)) +
                           Arena::need(K, sizeof(Fr)) + Arena::need(K << hi, sizeof(Fr)) +
                           Arena::need(K << lo, sizeof(Fr)) + Arena::need(2 * B * half, sizeof(Fr)) +
                           Arena::need(2 * (size_t)grid0, sizeof(Fr)) + Arena::need(2, sizeof(Fr)) +
                           Arena::need(1, sizeof(Fr)) + Arena::need(B, sizeof(Fr))));
  const uint32_t** d_tabs = ar.take<const uint32_t*>(B);
  uint32_t* d_cptr = ar.take<uint32_t>(B + 1);
  uint32_t* d_pts = ar.take<uint32_t>(pm.size() * 8);
  uint32_t* d_a = ar.take<uint32_t>(K * 8);
  uint32_t* d_eh = ar.take<uint32_t>((K << hi) * 8);
  uint32_t* d_el = ar.take<uint32_t>((K << lo) * 8);
  uint32_t* d_scr = ar.take<uint32_t>(2 * B * half * 8);
  uint32_t* d_partial = ar.take<uint32_t>(2 * (size_t)grid0 * 8);
  uint32_t* d_sums = ar.take<uint32_t>(2 * 8);
  uint32_t* d_r = ar.take<uint32_t>(8);
  uint32_t* d_u = ar.take<uint32_t>(B * 8);
  TPST_HIP(ctx, hipMemcpyAsync(d_tabs, tabs, B * sizeof(void*), hipMemcpyHostToDevice, st));
  TPST_HIP(ctx, hipMemcpyAsync(d_cptr, cptr.data(), (B + 1) * 4, hipMemcpyHostToDevice, st));
  TPST_HIP(ctx, hipMemcpyAsync(d_pts, pm.data(), pm.size() * sizeof(Fr), hipMemcpyHostToDevice, st));
  TPST_HIP(ctx, hipMemcpyAsync(d_a, am.data(), K * sizeof(Fr), hipMemcpyHostToDevice, st));
  TPST_HIP(ctx, multi_eq_halves(st, d_pts, d_a, n, K, d_eh, d_el));
  const MultiSrc src{d_tabs, d_cptr, d_eh, d_el, lo, hi};
  for (int i = 0; i < n; i++) {
    const size_t h = N >> i;  // table length once the previous challenge is bound
    const int stage = i == 0 ? ST_MULTI_ROUND0 : i == 1 ? ST_MULTI_ROUND1 : ST_MULTI_ROUNDS;
    ctx->prof.begin(stage, st);
    TPST_HIP(ctx, multi_round(st, i, src, d_scr, half, (int)B, h, d_r, 1, d_partial, d_sums));
    ctx->prof.end(stage, st);
    TPST_HIP(ctx, hipMemcpyAsync(hs, d_sums, 64, hipMemcpyDeviceToHost, st));
    TPST_HIP(ctx, hipStreamSynchronize(st));
    uint64_t rho[4];
    if (int rc = challenge(i, hs[0], hs[1], rho)) return rc;
    const Fr rm = fr_canon(rho);
    memcpy(rpin, rm.v, 32);
    TPST_HIP(ctx, hipMemcpyAsync(d_r, rpin, 32, hipMemcpyHostToDevice, st));
  }
  // the closing bind: length 2 -> 1; u_j is entry 0 of table F_j
  ctx->prof.begin(ST_MULTI_ROUNDS, st);
  TPST_HIP(ctx, multi_round(st, n, src, d_scr, half, (int)B, 1, d_r, 0, nullptr, nullptr));
  k_multi_finals<<<grid_for(B, MP_BS), MP_BS, 0, st>>>(d_scr, half, (int)B, d_u);
  ctx->prof.end(ST_MULTI_ROUNDS, st);
  TPST_HIP(ctx, hipGetLastError());
  TPST_HIP(ctx, hipMemcpyAsync(u, d_u, B * 32, hipMemcpyDeviceToHost, st));
  TPST_HIP(ctx, hipStreamSynchronize(st));
  return TPST_OK;
}

// the whole polynomials' tables under the context's lock, or an error
int whole_tables(tpst_ctx* ctx, tpst_poly* const* polys, size_t B, std::vector<const uint32_t*>& tabs) {
  for (size_t j = 0; j < B; j++) {
    if (!polys[j]) return fail(ctx, TPST_E_ARG, "null polynomial " + std::to_string(j));
    if (polys[j]->ctx != ctx) return fail(ctx, TPST_E_ARG, "polynomial of another context");
    if (polys[j]->n != polys[0]->n) return fail(ctx, TPST_E_ARG, "polynomials differ in num_vars");
  }
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  tabs.resize(B);
  for (size_t j = 0; j < B; j++) {
    tabs[j] = polys[j]->q_only ? nullptr : poly_evals(polys[j]);
    if (!tabs[j]) return fail(ctx, TPST_E_STATE, "operation needs whole polynomials (a column slice or q-only handle)");
    if ((uintptr_t)tabs[j] & 15) return fail(ctx, TPST_E_ARG, "evaluation table not 16-byte aligned");
  }
  return TPST_OK;
}

}  // namespace tpst

using namespace tpst;

namespace {

void append_fr(Sponge& sp, const uint64_t* fr) {  // tpst_transcript_append_fr
  const uint64_t l[6] = {fr[0], fr[1], fr[2], fr[3], 0, 0};
  sp.absorb(std::vector<Fq>{fq_canon(l)});
}

void append_int(Sponge& sp, uint64_t x) {
  const uint64_t l[4] = {x, 0, 0, 0};
  append_fr(sp, l);
}

// what prover and verifier ask of the claims' shape; 0 or a message
const char* claims_shape(int n, size_t B, const uint32_t* claim_poly, size_t K) {
  int m_col, m_row, odd;
  if (poly_dims(n, m_col, m_row, odd)) return "bad num_vars";
  if (B < 1 || B > LINCOMB_MAX_TERMS) return "the number of polynomials must be 1..256";
  if (K < 1 || K > MULTI_MAX_CLAIMS) return "the number of claims must be 1..4096";
  std::vector<uint8_t> seen(B, 0);
  for (size_t k = 0; k < K; k++) {
    if (claim_poly[k] >= B) return "claim on a polynomial index >= B";
    seen[claim_poly[k]] = 1;
  }
  for (size_t j = 0; j < B; j++)
    if (!seen[j]) return "a polynomial without a claim";
  return nullptr;
}

bool claims_canonical(int n, const uint64_t* points, const uint64_t* vals, size_t K) {
  for (size_t k = 0; k < K; k++) {
    if (!fr_ok(vals + 4 * k)) return false;
    for (int i = 0; i < n; i++)
      if (!fr_ok(points + 4 * (k * (size_t)n + i))) return false;
  }
  return true;
}

// step 1: the statement, then gamma
void absorb_statement(tpst_transcript* tr, int n, size_t B, const uint64_t* const* Ts, const uint32_t* claim_poly,
                      const uint64_t* points, const uint64_t* vals, size_t K, uint64_t* gamma) {
  Sponge sp;
  sp.load(tr);
  append_int(sp, B);
  append_int(sp, K);
  append_int(sp, (uint64_t)n);
  for (size_t j = 0; j < B; j++) sp.absorb_bytes((const uint8_t*)Ts[j], 576);  // append_gt
  for (size_t k = 0; k < K; k++) {
    append_int(sp, claim_poly[k]);
    for (int i = 0; i < n; i++) append_fr(sp, points + 4 * (k * (size_t)n + i));
    append_fr(sp, vals + 4 * k);
  }
  sp.challenge(gamma);
  sp.store(tr);
}

// a_k = gamma^k (canonical out) and e_0 = sum_k a_k v_k
Fr claim_weights(const uint64_t* gamma, const uint64_t* vals, size_t K, std::vector<uint64_t>& a) {
  a.resize(4 * K);
  const Fr g = fr_canon(gamma);
  Fr p = Fr::one(), e = Fr::zero();
  for (size_t k = 0; k < K; k++) {
    fr_out(p, &a[4 * k]);
    e = add(e, mul(p, fr_canon(vals + 4 * k)));
    p = mul(p, g);
  }
  return e;
}

}  // namespace

extern "C" int tpst_poly_multi_sumcheck_stages(tpst_ctx* ctx, tpst_poly* const* polys, size_t B,
                                               const uint32_t* claim_poly, const uint64_t* points, const uint64_t* a,
                                               size_t K, const uint64_t* rho, uint64_t* sums, uint64_t* u) {
  if (!ctx) return TPST_E_ARG;
  if (!polys || !claim_poly || !points || !a || !rho || !sums || !u) return fail(ctx, TPST_E_ARG, "null argument");
  if (B < 1 || B > LINCOMB_MAX_TERMS) return fail(ctx, TPST_E_ARG, "the number of polynomials must be 1..256");
  std::vector<const uint32_t*> tabs;
  if (int rc = whole_tables(ctx, polys, B, tabs)) return rc;
  const int n = polys[0]->n;
  if (const char* m = claims_shape(n, B, claim_poly, K)) return fail(ctx, TPST_E_ARG, m);
  if (!claims_canonical(n, points, a, K)) return fail(ctx, TPST_E_ARG, "coordinate or weight >= r");
  for (int i = 0; i < n; i++)
    if (!fr_ok(rho + 4 * i)) return fail(ctx, TPST_E_ARG, "challenge >= r");
  return multi_sumcheck(ctx, tabs.data(), B, n, claim_poly, points, a, K,
                        [&](int i, const uint64_t* s0, const uint64_t* s2, uint64_t* r) {
                          memcpy(sums + 8 * (size_t)i, s0, 32);
                          memcpy(sums + 8 * (size_t)i + 4, s2, 32);
                          memcpy(r, rho + 4 * i, 32);
                          return TPST_OK;
                        },
                        u);
}

extern "C" int tpst_poly_open_multi(tpst_ctx* ctx, tpst_poly* const* polys, const uint64_t* const* comms,
                                    const uint64_t* const* Ts, size_t B, const uint32_t* claim_poly,
                                    const uint64_t* points, const uint64_t* vals, size_t K, tpst_transcript* tr,
                                    uint64_t* rounds, uint64_t* u, uint64_t* rho, uint64_t* comms_out, uint64_t* T_out,
                                    uint64_t* v_out, tpst_open_proof* proof) {
  if (!ctx) return TPST_E_ARG;
  if (!polys || !comms || !Ts || !claim_poly || !points || !vals || !tr || !rounds || !u || !rho || !comms_out ||
      !T_out || !v_out || !proof)
    return fail(ctx, TPST_E_ARG, "null argument");
  if (B < 1 || B > LINCOMB_MAX_TERMS) return fail(ctx, TPST_E_ARG, "the number of polynomials must be 1..256");
  for (size_t j = 0; j < B; j++)
    if (!comms[j] || !Ts[j]) return fail(ctx, TPST_E_ARG, "null commitment " + std::to_string(j));
  std::vector<const uint32_t*> tabs;
  if (int rc = whole_tables(ctx, polys, B, tabs)) return rc;
  const int n = polys[0]->n;
  if (const char* m = claims_shape(n, B, claim_poly, K)) return fail(ctx, TPST_E_ARG, m);
  if (!claims_canonical(n, points, vals, K)) return fail(ctx, TPST_E_ARG, "coordinate or value >= r");
  {
    std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
    if (!srs_of(ctx)) return fail(ctx, TPST_E_STATE, "no SRS loaded");
  }
  tpst_transcript t = *tr;  // tr changes only on success
  uint64_t gamma[4];
  absorb_statement(&t, n, B, Ts, claim_poly, points, vals, K, gamma);
  std::vector<uint64_t> a;
  Fr e = claim_weights(gamma, vals, K, a);
  const int rc = multi_sumcheck(ctx, tabs.data(), B, n, claim_poly, points, a.data(), K,
                                [&](int i, const uint64_t* s0, const uint64_t* s2, uint64_t* r) {
                                  // evaluations at 0, 1 (= e_i - s_i(0)), 2 -> coefficients (sumcheck.rs:127-128, 424)
                                  Fr ev[3] = {fr_canon(s0), Fr::zero(), fr_canon(s2)}, cs[3];
                                  ev[1] = sub(e, ev[0]);
                                  from_evals(ev, 3, cs);
                                  for (int c = 0; c < 3; c++) {
                                    uint64_t* out = rounds + 4 * (3 * (size_t)i + c);
                                    fr_out(cs[c], out);
                                    if (tpst_transcript_append_fr(&t, out) != TPST_OK)
                                      return fail(ctx, TPST_E_ARG, "transcript append");
                                  }
                                  tpst_transcript_challenge(&t, r);
                                  memcpy(rho + 4 * (size_t)i, r, 32);
                                  e = uni_eval(cs, 3, fr_canon(r));
                                  return (int)TPST_OK;
                                },
                                u);
  if (rc) return rc;
  std::vector<uint64_t> w(4 * B);
  if (tpst_pst_combine_challenge(&t, n, rho, Ts, u, B, w.data()) != TPST_OK)
    return fail(ctx, TPST_E_ARG, "combine challenge");
  if (int rc2 = tpst_poly_open_combined(ctx, polys, comms, Ts, B, w.data(), &t, rho, comms_out, T_out, v_out, proof))
    return rc2;
  *tr = t;
  return TPST_OK;
}

extern "C" int tpst_pst_multi_reduce(tpst_transcript* tr, int n, const uint64_t* const* Ts, size_t B,
                                     const uint32_t* claim_poly, const uint64_t* points, const uint64_t* vals, size_t K,
                                     const uint64_t* rounds, const uint64_t* u, uint64_t* rho) {
  if (!tr || !Ts || !claim_poly || !points || !vals || !rounds || !u || !rho) return TPST_E_ARG;
  if (claims_shape(n, B, claim_poly, K)) return TPST_E_ARG;
  for (size_t j = 0; j < B; j++)
    if (!Ts[j]) return TPST_E_ARG;
  // every scalar is validated before the sponge absorbs anything
  if (!claims_canonical(n, points, vals, K)) return TPST_E_VERIFY;
  for (size_t j = 0; j < B; j++)
    if (!fr_ok(u + 4 * j) || !gt_ok(Ts[j])) return TPST_E_VERIFY;
  for (int i = 0; i < 3 * n; i++)
    if (!fr_ok(rounds + 4 * (size_t)i)) return TPST_E_VERIFY;
  tpst_transcript t = *tr;  // tr changes only on success
  uint64_t gamma[4];
  absorb_statement(&t, n, B, Ts, claim_poly, points, vals, K, gamma);
  std::vector<uint64_t> a;
  Fr e = claim_weights(gamma, vals, K, a);
  std::vector<Fr> rs(n);
  std::vector<uint64_t> rc(4 * (size_t)n);
  for (int i = 0; i < n; i++) {
    Fr cs[3];
    for (int c = 0; c < 3; c++) cs[c] = fr_canon(rounds + 4 * (3 * (size_t)i + c));
    // s_i(0) + s_i(1) = 2 c0 + c1 + c2 = e_i
    if (!eq(add(add(dbl(cs[0]), cs[1]), cs[2]), e)) return TPST_E_VERIFY;
    for (int c = 0; c < 3; c++) tpst_transcript_append_fr(&t, rounds + 4 * (3 * (size_t)i + c));
    tpst_transcript_challenge(&t, &rc[4 * (size_t)i]);
    rs[i] = fr_canon(&rc[4 * (size_t)i]);
    e = uni_eval(cs, 3, rs[i]);
  }
  // e_n = sum_j u_j D_j(rho),  D_j(rho) = sum_{k: j_k = j} a_k prod_i (r_ki rho_i + (1 - r_ki)(1 - rho_i))
  std::vector<Fr> D(B, Fr::zero());
  for (size_t k = 0; k < K; k++) {
    Fr p = fr_canon(&a[4 * k]);
    for (int i = 0; i < n; i++) {
      const Fr x = fr_canon(points + 4 * (k * (size_t)n + i));
      p = mul(p, add(mul(x, rs[i]), mul(sub(Fr::one(), x), sub(Fr::one(), rs[i]))));
    }
    D[claim_poly[k]] = add(D[claim_poly[k]], p);
  }
  Fr sum = Fr::zero();
  for (size_t j = 0; j < B; j++) sum = add(sum, mul(fr_canon(u + 4 * j), D[j]));
  if (!eq(sum, e)) return TPST_E_VERIFY;
  memcpy(rho, rc.data(), 32 * (size_t)n);
  *tr = t;
  return TPST_OK;
}

extern "C" int tpst_pst_verify_multi(tpst_ctx* ctx, tpst_transcript* tr, int n, const uint64_t* const* Ts, size_t B,
                                     const uint32_t* claim_poly, const uint64_t* points, const uint64_t* vals, size_t K,
                                     const uint64_t* rounds, const uint64_t* u, const tpst_open_proof* proof) {
  if (!ctx) return TPST_E_ARG;
  if (!tr || !Ts || !claim_poly || !points || !vals || !rounds || !u || !proof)
    return fail(ctx, TPST_E_ARG, "null argument");
  int m_col, m_row, odd;
  if (poly_dims(n, m_col, m_row, odd)) return fail(ctx, TPST_E_ARG, "bad num_vars");
  {
    std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
    SrsState* st = srs_of(ctx);
    if (!st) return fail(ctx, TPST_E_STATE, "no SRS loaded");
    if (st->nv != m_row || proof->m_col != m_col || proof->m_row != m_row) return fail(ctx, TPST_E_ARG, "size mismatch");
  }
  tpst_transcript t = *tr;  // tr changes only on TPST_OK
  std::vector<uint64_t> rho(4 * (size_t)n), w(4 * (B ? B : 1));
  int rc = tpst_pst_multi_reduce(&t, n, Ts, B, claim_poly, points, vals, K, rounds, u, rho.data());
  if (rc == TPST_E_ARG) return fail(ctx, rc, "multi-point claims: bad polynomial index, a polynomial without a claim, or sizes out of range");
  if (rc) return fail(ctx, rc, "multi-point reduction rejected (a round check, the final identity or a scalar >= r)");
  if (tpst_pst_combine_challenge(&t, n, rho.data(), Ts, u, B, w.data()) != TPST_OK)
    return fail(ctx, TPST_E_ARG, "combine challenge");
  rc = tpst_pst_verify_combined(ctx, &t, n, rho.data(), u, Ts, B, w.data(), proof);
  if (rc == TPST_OK) *tr = t;
  return rc;
}
