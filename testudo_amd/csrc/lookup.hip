// Lookup argument on committed polynomials (include/tpst.h, "lookup argument";
// this project's own protocol, no counterpart in the reference): every entry
// of the witness tables a_0..a_{L-1} occurs in the table t.  LogUp: with
//   m(y)   = #{(l, x) : a_l(x) = t(y)}  at the first y holding the value,
//   h_l(x) = 1 / (beta + a_l(x)),  h_t(y) = m(y) / (beta + t(y))
// the claim is sum_l sum_x h_l(x) = sum_y h_t(y).  The device work:
//
//   k_lk_index     an open-addressing index of t: a slot holds a table INDEX,
//                  claimed with a 32-bit CAS; a repeat of the slot's value
//                  lowers it with atomicMin, so the first occurrence wins
//                  whatever the arrival order.  A key's slot is the first free
//                  one on its probe path and no path is ever passed while
//                  free, so equal values always meet in one slot.  Keys are
//                  compared on all 8 words read from t, never on the hash.
//   k_lk_count     one probe per witness entry, then atomicAdd on a u32 count;
//                  the lanes of a wave that hit the same index are combined
//                  first (one atomic with their number), so an all-equal
//                  witness costs one atomic per wave, not one per entry.
//   k_lk_counts_fr the counts as canonical Fr: the table of m.
//   k_lk_inverse   out = num / (beta + f) by Montgomery's trick, one inversion
//                  (Fermat, in registers) per lane over its grid-strided
//                  (coalesced) entries; the prefix products wait in `out`, the
//                  second pass walks back.
//   k_lk_sum       exact field sums of the h tables (LDS tree, no atomics):
//                  2^-n sum_x h(x) is h at the point (1/2, .., 1/2).
// m is a function of (a, t) alone and every h and sum is exact: nothing
// depends on the grid, the slot count or the arrival order.  The host driver
// and the C ABI (tpst_poly_lookup_open and its parts) follow.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/tpst.h"
#include "ctx.h"
#include "device_util.h"
#include "fr_mem.h"
#include "lookup.h"
#include "poly_multi.h"
#include "poly_sumcheck.h"
#include "pst_state.h"

namespace tpst {

namespace {

constexpr int LK_BS = 256;
// a few resident workgroups per CU, the stride loops cover the rest
constexpr unsigned LK_MAX_GRID = 256 * 8;
// entries one lane of k_lk_inverse takes at least (when there are enough): the inversion's share per entry
constexpr size_t LK_INV_CHUNK = 32;

// all 8 words of the key, finished as murmur3 does
__device__ __forceinline__ uint32_t key_hash(const Fr& k) {
  uint32_t h = 0x9E3779B9u;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    h = (h ^ k.v[i]) * 0x85EBCA6Bu;
    h = (h << 13) | (h >> 19);
  }
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  return h ^ (h >> 16);
}

__device__ __forceinline__ bool key_eq(const Fr& a, const Fr& b) {
  uint32_t acc = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) acc |= a.v[i] ^ b.v[i];
  return acc == 0;
}

// a slot's value only ever names an entry of t (< N) whose value is the slot's key
__global__ void __launch_bounds__(LK_BS) k_lk_index(const uint32_t* __restrict__ t, size_t N, uint32_t* slots,
                                                   uint32_t mask) {
  const size_t stride = (size_t)gridDim.x * LK_BS;
  for (size_t y = (size_t)blockIdx.x * LK_BS + threadIdx.x; y < N; y += stride) {
    const Fr key = ld_fr16(t + 8 * y);
    uint32_t pos = key_hash(key) & mask;
    // at most mask + 1 slots: N <= mask + 1 distinct keys always find one
    for (uint32_t probes = 0; probes <= mask; probes++) {
      uint32_t cur = __hip_atomic_load(slots + pos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cur == LK_EMPTY) {
        cur = atomicCAS(slots + pos, LK_EMPTY, (uint32_t)y);
        if (cur == LK_EMPTY) break;
      }
      if (key_eq(key, ld_fr16(t + 8 * (size_t)cur))) {
        if ((uint32_t)y < cur) atomicMin(slots + pos, (uint32_t)y);  // the slot only ever decreases
        break;
      }
      pos = (pos + 1) & mask;
    }
  }
}

__global__ void __launch_bounds__(LK_BS) k_lk_count(const uint32_t* const* __restrict__ wits, size_t total, int n,
                                                   const uint32_t* __restrict__ t, const uint32_t* __restrict__ slots,
                                                   uint32_t mask, uint32_t* cnt, unsigned long long* miss) {
  const size_t stride = (size_t)gridDim.x * LK_BS;
  const size_t xmask = ((size_t)1 << n) - 1;
  for (size_t id = (size_t)blockIdx.x * LK_BS + threadIdx.x; id < total; id += stride) {
    const Fr key = ld_fr16(wits[id >> n] + 8 * (id & xmask));
    uint32_t pos = key_hash(key) & mask, dest = LK_EMPTY;
    for (uint32_t probes = 0; probes <= mask; probes++) {  // a full index holds no empty slot to stop at
      const uint32_t cur = slots[pos];
      if (cur == LK_EMPTY) break;
      if (key_eq(key, ld_fr16(t + 8 * (size_t)cur))) {
        dest = cur;
        break;
      }
      pos = (pos + 1) & mask;
    }
    if (dest == LK_EMPTY) {
      if (id < *(volatile unsigned long long*)miss) atomicMin(miss, (unsigned long long)id);
      continue;
    }
    // the lanes with the first pending lane's destination leave together, one atomic for all of them
    bool pending = true;
    while (pending) {
      const uint32_t lead = __builtin_amdgcn_readfirstlane(dest);
      const bool mine = dest == lead;
      const unsigned long long grp = __ballot(mine);
      if (mine) {
        if ((int)__lane_id() == __ffsll((long long)grp) - 1) atomicAdd(cnt + lead, (uint32_t)__popcll(grp));
        pending = false;
      }
    }
  }
}

__global__ void __launch_bounds__(LK_BS) k_lk_counts_fr(const uint32_t* __restrict__ cnt, size_t N,
                                                       uint32_t* __restrict__ m) {
  const size_t stride = (size_t)gridDim.x * LK_BS;
  for (size_t y = (size_t)blockIdx.x * LK_BS + threadIdx.x; y < N; y += stride) {
    Fr v = Fr::zero();
    v.v[0] = cnt[y];
    st_fr16(m + 8 * y, v);
  }
}

// 1 / a by Fermat, a^(r - 2), Montgomery in and out (0 for a = 0): 253 squarings and a product per set bit, all
// in registers.  field.h's inv() is a call with a stack frame -- private scratch, which these kernels do not use --
// and one inversion per lane is spread over the lane's whole chunk.  The exponent's words are compile-time
// constants; every branch is uniform.
__device__ __forceinline__ Fr inv_fermat(const Fr& a) {
  Fr acc = Fr::one();
#pragma unroll
  for (int w = 7; w >= 0; w--) {
    const uint32_t e = params::FR_PM2[w];
#pragma unroll 1
    for (int b = 31; b >= 0; b--) {
      acc = sqr(acc);
      if ((e >> b) & 1) acc = mul(acc, a);
    }
  }
  return acc;
}

// beta + f[i], and whether it was zero (then 1 stands in for it)
__device__ __forceinline__ Fr denominator(const Fr& beta, const uint32_t* f, size_t i, bool& zero) {
  const Fr d = add(beta, ld_fr16(f + 8 * i));
  zero = is_zero(d);
  return zero ? Fr::one() : d;
}

// The tables are canonical and stay so: a canonical d is read as the Montgomery form of d / R.  With P the
// Montgomery form of prod_k d_k / R, inv(P) is that of its inverse; one product by the plain 1 divides by R.
// Scaled by R^-1 (NUM) or R^-2, the running inverse times the prefix product is R / d_k or 1 / d_k as a plain
// number, and one more product by the canonical num[i] gives num[i] / d_k.
template <bool NUM>
__global__ void __launch_bounds__(LK_BS) k_lk_inverse(const uint32_t* __restrict__ f, const uint32_t* __restrict__ num,
                                                     const uint32_t* __restrict__ beta, size_t N, uint32_t* out,
                                                     unsigned long long* zero_at) {
  const size_t stride = (size_t)gridDim.x * LK_BS;
  const size_t i0 = (size_t)blockIdx.x * LK_BS + threadIdx.x;
  if (i0 >= N) return;
  const Fr b = ld_fr16(beta);
  Fr p = Fr::one();
  for (size_t i = i0; i < N; i += stride) {
    bool zero;
    const Fr d = denominator(b, f, i, zero);
    if (zero && i < *(volatile unsigned long long*)zero_at) atomicMin(zero_at, (unsigned long long)i);
    st_fr16(out + 8 * i, p);
    p = mul(p, d);
  }
  Fr plain1 = Fr::zero();
  plain1.v[0] = 1;
  Fr run = mul(inv_fermat(p), plain1);
  if (!NUM) run = mul(run, plain1);
  for (size_t k = (N - 1 - i0) / stride + 1; k-- > 0;) {
    const size_t i = i0 + k * stride;
    bool zero;
    const Fr d = denominator(b, f, i, zero);
    Fr v = mul(run, ld_fr16(out + 8 * i));
    if (NUM) v = mul(v, ld_fr16(num + 8 * i));
    st_fr16(out + 8 * i, v);
    run = mul(run, d);
  }
}

// the workgroup's sum of the lanes' v, in lane 0; sh: LK_BS Fr
__device__ __forceinline__ Fr block_sum(Fr* sh, const Fr& v) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int w = LK_BS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] = add(sh[threadIdx.x], sh[threadIdx.x + w]);
    __syncthreads();
  }
  return sh[0];
}

// out[blockIdx.x] = the sum of the workgroup's grid-strided entries of x (n entries), canonical
__global__ void __launch_bounds__(LK_BS) k_lk_sum(const uint32_t* __restrict__ x, size_t n,
                                                 uint32_t* __restrict__ out) {
  __shared__ Fr sh[LK_BS];
  const size_t stride = (size_t)gridDim.x * LK_BS;
  Fr a = Fr::zero();
  for (size_t i = (size_t)blockIdx.x * LK_BS + threadIdx.x; i < n; i += stride) a = add(a, ld_fr16(x + 8 * i));
  a = block_sum(sh, a);
  if (threadIdx.x == 0) st_fr16(out + 8 * (size_t)blockIdx.x, a);
}

}  // namespace

unsigned lookup_grid(size_t items) {
  size_t cap = LK_MAX_GRID;
  // TPST_LOOKUP_GRID=g: at most g workgroups whatever the size (tests: no output depends on the grid)
  if (const char* e = getenv("TPST_LOOKUP_GRID"))
    if (atoi(e) >= 1) cap = std::min<size_t>((size_t)atoi(e), LK_MAX_GRID);
  return (unsigned)std::min<size_t>(std::max<size_t>(grid_for(items, LK_BS), 1), cap);
}

hipError_t lookup_index_build(hipStream_t s, const uint32_t* d_t, size_t N, uint32_t* d_slots, int slots_log2) {
  if (!d_t || !d_slots || !N || slots_log2 < 1 || slots_log2 > 31 || N > ((size_t)1 << slots_log2))
    return hipErrorInvalidValue;
  k_lk_index<<<lookup_grid(N), LK_BS, 0, s>>>(d_t, N, d_slots, (uint32_t)(((uint64_t)1 << slots_log2) - 1));
  return hipGetLastError();
}

hipError_t lookup_count(hipStream_t s, const uint32_t* const* d_wits, int L, size_t N, const uint32_t* d_t,
                        const uint32_t* d_slots, int slots_log2, uint32_t* d_cnt, unsigned long long* d_miss) {
  int n = 0;
  while (((size_t)1 << n) < N) n++;
  if (!d_wits || !d_t || !d_slots || !d_cnt || !d_miss || L < 1 || L > (int)LOOKUP_MAX_WITNESSES || !N ||
      ((size_t)1 << n) != N || slots_log2 < 1 || slots_log2 > 31 || N > ((size_t)1 << slots_log2) ||
      (uint64_t)L * N >= ((uint64_t)1 << 32))
    return hipErrorInvalidValue;
  k_lk_count<<<lookup_grid((size_t)L * N), LK_BS, 0, s>>>(d_wits, (size_t)L * N, n, d_t, d_slots,
                                                         (uint32_t)(((uint64_t)1 << slots_log2) - 1), d_cnt, d_miss);
  return hipGetLastError();
}

hipError_t lookup_counts_fr(hipStream_t s, const uint32_t* d_cnt, size_t N, uint32_t* d_m) {
  if (!d_cnt || !d_m || !N) return hipErrorInvalidValue;
  k_lk_counts_fr<<<lookup_grid(N), LK_BS, 0, s>>>(d_cnt, N, d_m);
  return hipGetLastError();
}

hipError_t lookup_inverse(hipStream_t s, const uint32_t* d_f, const uint32_t* d_num, const uint32_t* d_beta, size_t N,
                          uint32_t* d_out, unsigned long long* d_zero) {
  if (!d_f || !d_beta || !d_out || !d_zero || !N || d_out == d_f || d_out == d_num) return hipErrorInvalidValue;
  const unsigned grid = lookup_grid((N + LK_INV_CHUNK - 1) / LK_INV_CHUNK);
  if (d_num)
    k_lk_inverse<true><<<grid, LK_BS, 0, s>>>(d_f, d_num, d_beta, N, d_out, d_zero);
  else
    k_lk_inverse<false><<<grid, LK_BS, 0, s>>>(d_f, nullptr, d_beta, N, d_out, d_zero);
  return hipGetLastError();
}

hipError_t lookup_sum(hipStream_t s, const uint32_t* d_x, size_t N, uint32_t* d_partial, uint32_t* d_out) {
  if (!d_x || !d_partial || !d_out || !N) return hipErrorInvalidValue;
  const unsigned grid = lookup_grid(N);
  k_lk_sum<<<grid, LK_BS, 0, s>>>(d_x, N, d_partial);
  TPST_TRY(hipGetLastError());
  k_lk_sum<<<1, LK_BS, 0, s>>>(d_partial, grid, d_out);
  return hipGetLastError();
}

}  // namespace tpst

using namespace tpst;

namespace {

// the helper polynomials of one lookup, freed with it
struct Helpers {
  std::unique_ptr<tpst_poly> m;
  std::vector<std::unique_ptr<tpst_poly>> h;  // h_0..h_{L-1}, h_t
};

// a whole-polynomial handle owning 2^n Fr, contents undefined; the caller holds the context's lock
int new_table(tpst_ctx* ctx, int n, std::unique_ptr<tpst_poly>& out) {
  auto p = std::make_unique<tpst_poly>();
  if (poly_dims(n, p->m_col, p->m_row, p->odd)) return fail(ctx, TPST_E_ARG, "bad num_vars");
  p->ctx = ctx;
  p->n = n;
  TPST_HIP(ctx, p->Zown.alloc(((size_t)1 << n) * 32));
  p->d_Z = p->Zown.u();
  out = std::move(p);
  return TPST_OK;
}

// the index capacity: TPST_LOOKUP_SLOTS_LOG2, or twice the table
int slots_log2_for(tpst_ctx* ctx, int n, int& out) {
  out = n + 1;
  if (const char* e = getenv("TPST_LOOKUP_SLOTS_LOG2")) {
    out = atoi(e);
    if (out < n || out > 31) return fail(ctx, TPST_E_ARG, "TPST_LOOKUP_SLOTS_LOG2 must be n..31");
  }
  return TPST_OK;
}

// what the prover and the stages entry ask alike; tabs: a_0..a_{L-1}, t
int lookup_args(tpst_ctx* ctx, tpst_poly* const* wits, size_t L, tpst_poly* table, std::vector<tpst_poly*>& polys,
                std::vector<const uint32_t*>& tabs, int& n) {
  if (L < 1 || L > LOOKUP_MAX_WITNESSES) return fail(ctx, TPST_E_ARG, "the number of witness polynomials must be 1..8");
  polys.assign(wits, wits + L);
  polys.push_back(table);
  if (int rc = whole_tables(ctx, polys.data(), L + 1, tabs)) return rc;
  n = table->n;
  if (n + 3 > 32 || ((uint64_t)L << n) >= ((uint64_t)1 << 32))
    return fail(ctx, TPST_E_ARG, "n + 3 must be <= 32 and L 2^n < 2^32 (the u32 counts)");
  return TPST_OK;
}

// m from (a, t): index, probes, counts.  TPST_E_ARG with the least (l, x) when a witness entry is not in the table.
int build_m(tpst_ctx* ctx, const std::vector<const uint32_t*>& tabs, size_t L, int n, Helpers& hp) {
  int slog;
  if (int rc = slots_log2_for(ctx, n, slog)) return rc;
  const size_t N = (size_t)1 << n, S = (size_t)1 << slog;
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (int rc = new_table(ctx, n, hp.m)) return rc;
  if (int rc = ensure_pinned(ctx, 4096)) return rc;
  Arena& ar = ctx->arena;
  ar.reset();
  TPST_HIP(ctx, ar.reserve(Arena::need(L, sizeof(void*)) + Arena::need(S, 4) + Arena::need(N, 4) + Arena::need(1, 8)));
  const uint32_t** d_wits = ar.take<const uint32_t*>(L);
  uint32_t* d_slots = ar.take<uint32_t>(S);
  uint32_t* d_cnt = ar.take<uint32_t>(N);
  unsigned long long* d_miss = ar.take<unsigned long long>(1);
  memcpy(ctx->pinned, tabs.data(), L * sizeof(void*));
  TPST_HIP(ctx, hipMemcpyAsync(d_wits, ctx->pinned, L * sizeof(void*), hipMemcpyHostToDevice, st));
  ctx->prof.begin(ST_LK_INDEX, st);
  TPST_HIP(ctx, hipMemsetAsync(d_slots, 0xFF, S * 4, st));
  TPST_HIP(ctx, lookup_index_build(st, tabs[L], N, d_slots, slog));
  ctx->prof.end(ST_LK_INDEX, st);
  ctx->prof.begin(ST_LK_COUNT, st);
  TPST_HIP(ctx, hipMemsetAsync(d_cnt, 0, N * 4, st));
  TPST_HIP(ctx, hipMemsetAsync(d_miss, 0xFF, 8, st));
  TPST_HIP(ctx, lookup_count(st, d_wits, (int)L, N, tabs[L], d_slots, slog, d_cnt, d_miss));
  TPST_HIP(ctx, lookup_counts_fr(st, d_cnt, N, hp.m->Zown.u()));
  ctx->prof.end(ST_LK_COUNT, st);
  unsigned long long* miss = reinterpret_cast<unsigned long long*>((char*)ctx->pinned + 1024);
  TPST_HIP(ctx, hipMemcpyAsync(miss, d_miss, 8, hipMemcpyDeviceToHost, st));
  TPST_HIP(ctx, hipStreamSynchronize(st));
  if (*miss != LK_NONE)
    return fail(ctx, TPST_E_ARG, "lookup: witness " + std::to_string(*miss >> n) + " entry " +
                                     std::to_string(*miss & (N - 1)) + " is not in the table");
  return TPST_OK;
}

// every h from (a, t, m, beta) and s = their values at the 1/2 point (L + 1 canonical Fr).  TPST_E_ARG when a
// denominator is zero.
int build_h(tpst_ctx* ctx, const std::vector<const uint32_t*>& tabs, size_t L, int n, const uint64_t* beta, Helpers& hp,
            uint64_t* s) {
  const size_t N = (size_t)1 << n;
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  hp.h.resize(L + 1);
  for (size_t k = 0; k <= L; k++)
    if (int rc = new_table(ctx, n, hp.h[k])) return rc;
  if (int rc = ensure_pinned(ctx, 4096)) return rc;
  const unsigned grid = lookup_grid(N);
  Arena& ar = ctx->arena;
  ar.reset();
  TPST_HIP(ctx, ar.reserve(Arena::need(1, sizeof(Fr)) + Arena::need(L + 1, 8) + Arena::need(grid, sizeof(Fr)) +
                           Arena::need(L + 1, sizeof(Fr))));
  uint32_t* d_beta = ar.take<uint32_t>(8);
  unsigned long long* d_zero = ar.take<unsigned long long>(L + 1);
  uint32_t* d_partial = ar.take<uint32_t>(8 * (size_t)grid);
  uint32_t* d_sums = ar.take<uint32_t>(8 * (L + 1));
  memcpy(ctx->pinned, beta, 32);
  TPST_HIP(ctx, hipMemcpyAsync(d_beta, ctx->pinned, 32, hipMemcpyHostToDevice, st));
  TPST_HIP(ctx, hipMemsetAsync(d_zero, 0xFF, 8 * (L + 1), st));
  ctx->prof.begin(ST_LK_INVERSE, st);
  for (size_t k = 0; k <= L; k++)
    TPST_HIP(ctx, lookup_inverse(st, tabs[k], k == L ? hp.m->d_Z : nullptr, d_beta, N, hp.h[k]->Zown.u(), d_zero + k));
  ctx->prof.end(ST_LK_INVERSE, st);
  ctx->prof.begin(ST_LK_SUMS, st);
  for (size_t k = 0; k <= L; k++) TPST_HIP(ctx, lookup_sum(st, hp.h[k]->d_Z, N, d_partial, d_sums + 8 * k));
  ctx->prof.end(ST_LK_SUMS, st);
  unsigned long long* zero = reinterpret_cast<unsigned long long*>((char*)ctx->pinned + 1024);
  uint64_t* sums = reinterpret_cast<uint64_t*>((char*)ctx->pinned + 2048);
  TPST_HIP(ctx, hipMemcpyAsync(zero, d_zero, 8 * (L + 1), hipMemcpyDeviceToHost, st));
  TPST_HIP(ctx, hipMemcpyAsync(sums, d_sums, 32 * (L + 1), hipMemcpyDeviceToHost, st));
  TPST_HIP(ctx, hipStreamSynchronize(st));
  for (size_t k = 0; k <= L; k++)
    if (zero[k] != LK_NONE)
      return fail(ctx, TPST_E_ARG, "lookup: beta + value = 0 at index " + std::to_string(zero[k]) + " of " +
                                       (k == L ? std::string("the table") : "witness " + std::to_string(k)));
  // h(1/2, .., 1/2) = 2^-n sum_x h(x)
  const Fr half = inv(add(Fr::one(), Fr::one()));
  Fr scale = Fr::one();
  for (int i = 0; i < n; i++) scale = mul(scale, half);
  for (size_t k = 0; k <= L; k++) fr_out(mul(fr_canon(sums + 4 * k), scale), s + 4 * k);
  return TPST_OK;
}

int append_int(tpst_transcript* t, uint64_t x) {
  const uint64_t l[4] = {x, 0, 0, 0};
  return tpst_transcript_append_fr(t, l);
}

// Steps 1-3 on t: L, n and the statement's T (a_0..a_{L-1}, t); T_m, then beta; every T_h, then tau and lambda.
// The prover interleaves its device work, the verifier runs them in a row.  Non-zero: a T with a coefficient >= p.
int step1(tpst_transcript* t, size_t L, int n, const uint64_t* const* Ts) {
  int rc = append_int(t, L) | append_int(t, (uint64_t)n);
  for (size_t j = 0; j <= L; j++) rc |= tpst_transcript_append_gt(t, Ts[j]);
  return rc;
}
int step2(tpst_transcript* t, const uint64_t* T_m, uint64_t* beta) {
  if (int rc = tpst_transcript_append_gt(t, T_m)) return rc;
  return tpst_transcript_challenge(t, beta);
}
int step3(tpst_transcript* t, size_t L, int n, const uint64_t* T_h, uint64_t* tau, uint64_t* lambda) {
  int rc = 0;
  for (size_t k = 0; k <= L; k++) rc |= tpst_transcript_append_gt(t, T_h + 72 * k);
  if (rc) return rc;
  for (int i = 0; i < n; i++) tpst_transcript_challenge(t, tau + 4 * (size_t)i);
  return tpst_transcript_challenge(t, lambda);
}

// Step 4's statement in the polynomial order a_0..a_{L-1}, t, m, h_0..h_{L-1}, h_t: the 2L + 3 terms and the claim
// e_0 = sum_{l < L} lambda^l
void lookup_terms(size_t L, const uint64_t* beta, const uint64_t* lambda, std::vector<tpst_sc_term>& terms,
                  uint64_t* e0) {
  const Fr b = fr_canon(beta), lam = fr_canon(lambda);
  terms.assign(2 * L + 3, tpst_sc_term{});
  Fr pw = Fr::one(), e = Fr::zero();
  for (size_t l = 0; l <= L; l++) {
    const uint32_t h = (uint32_t)(L + 2 + l), f = (uint32_t)l;  // l == L: h_t and t
    tpst_sc_term& prod = terms[2 * l];
    prod.deg = 2, prod.idx[0] = h, prod.idx[1] = f;
    fr_out(pw, prod.coeff);
    tpst_sc_term& lin = terms[2 * l + 1];
    lin.deg = 1, lin.idx[0] = h;
    fr_out(mul(pw, b), lin.coeff);
    if (l < L) {
      e = add(e, pw);
      pw = mul(pw, lam);
    }
  }
  tpst_sc_term& mt = terms[2 * L + 2];
  mt.deg = 1, mt.idx[0] = (uint32_t)(L + 1);
  fr_out(sub(Fr::zero(), pw), mt.coeff);
  fr_out(e, e0);
}

// Step 6's claims: f_j(rho) = u_j for every j, then h_l(1/2^n) = s_l, then h_t(1/2^n) = s_t
void lookup_claims(size_t L, int n, const uint64_t* rho, const uint64_t* u, const uint64_t* s,
                   std::vector<uint32_t>& claim_poly, std::vector<uint64_t>& points, std::vector<uint64_t>& vals) {
  const size_t B = 2 * L + 3, K = 3 * L + 4;
  uint64_t half[4];
  fr_out(inv(add(Fr::one(), Fr::one())), half);
  claim_poly.resize(K);
  points.resize(4 * (size_t)n * K);
  vals.resize(4 * K);
  for (size_t k = 0; k < K; k++) {
    claim_poly[k] = (uint32_t)(k < B ? k : L + 2 + (k - B));
    for (int i = 0; i < n; i++)
      memcpy(&points[4 * ((size_t)n * k + i)], k < B ? rho + 4 * (size_t)i : half, 32);
    memcpy(&vals[4 * k], k < B ? u + 4 * k : s + 4 * (k - B), 32);
  }
}

}  // namespace

extern "C" int tpst_poly_lookup_stages(tpst_ctx* ctx, tpst_poly* const* wits, size_t L, tpst_poly* table,
                                       const uint64_t* beta, uint64_t* m, uint64_t* h, uint64_t* s) {
  if (!ctx) return TPST_E_ARG;
  if (!wits || !table || !beta || !m || !h || !s) return fail(ctx, TPST_E_ARG, "null argument");
  std::vector<tpst_poly*> polys;
  std::vector<const uint32_t*> tabs;
  int n;
  if (int rc = lookup_args(ctx, wits, L, table, polys, tabs, n)) return rc;
  if (!fr_ok(beta)) return fail(ctx, TPST_E_ARG, "beta >= r");
  Helpers hp;
  if (int rc = build_m(ctx, tabs, L, n, hp)) return rc;
  if (int rc = build_h(ctx, tabs, L, n, beta, hp, s)) return rc;
  const size_t N = (size_t)1 << n;
  if (int rc = tpst_poly_evaluations(ctx, hp.m.get(), m)) return rc;
  for (size_t k = 0; k <= L; k++)
    if (int rc = tpst_poly_evaluations(ctx, hp.h[k].get(), h + 4 * N * k)) return rc;
  return TPST_OK;
}

extern "C" int tpst_poly_lookup_open(tpst_ctx* ctx, tpst_poly* const* wits, size_t L, tpst_poly* table,
                                     const uint64_t* const* comms, const uint64_t* const* Ts, tpst_transcript* tr,
                                     uint64_t* T_helpers, uint64_t* sc_rounds, uint64_t* u, uint64_t* s,
                                     uint64_t* mp_rounds, uint64_t* mp_u, uint64_t* rho, uint64_t* comms_out,
                                     uint64_t* T_out, uint64_t* v_out, tpst_open_proof* proof) {
  if (!ctx) return TPST_E_ARG;
  if (!wits || !table || !comms || !Ts || !tr || !T_helpers || !sc_rounds || !u || !s || !mp_rounds || !mp_u || !rho ||
      !comms_out || !T_out || !v_out || !proof)
    return fail(ctx, TPST_E_ARG, "null argument");
  std::vector<tpst_poly*> polys;
  std::vector<const uint32_t*> tabs;
  int n;
  if (int rc = lookup_args(ctx, wits, L, table, polys, tabs, n)) return rc;
  for (size_t j = 0; j <= L; j++)
    if (!comms[j] || !Ts[j]) return fail(ctx, TPST_E_ARG, "null commitment " + std::to_string(j));
  {
    std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
    if (!srs_of(ctx)) return fail(ctx, TPST_E_STATE, "no SRS loaded");
  }
  const size_t B = 2 * L + 3, C = (size_t)1 << (n / 2);
  tpst_transcript t = *tr;  // tr changes only on success
  if (step1(&t, L, n, Ts) != TPST_OK) return fail(ctx, TPST_E_ARG, "a T_j with a coefficient >= p");
  // m, committed before beta exists
  Helpers hp;
  if (int rc = build_m(ctx, tabs, L, n, hp)) return rc;
  std::vector<uint64_t> hc(12 * C * (L + 2)), hT(72 * (L + 2)), beta(4), tau(4 * (size_t)n), lambda(4);
  if (int rc = tpst_poly_commit(ctx, hp.m.get(), hc.data(), hT.data())) return rc;
  if (step2(&t, hT.data(), beta.data()) != TPST_OK) return fail(ctx, TPST_E_ARG, "transcript append");
  // every h, committed before tau and lambda exist
  if (int rc = build_h(ctx, tabs, L, n, beta.data(), hp, s)) return rc;
  for (size_t k = 0; k <= L; k++)
    if (int rc = tpst_poly_commit(ctx, hp.h[k].get(), &hc[12 * C * (k + 1)], &hT[72 * (k + 1)])) return rc;
  if (step3(&t, L, n, &hT[72], tau.data(), lambda.data()) != TPST_OK)
    return fail(ctx, TPST_E_ARG, "transcript append");
  // the B polynomials in the protocol's order
  std::vector<tpst_poly*> all(polys);
  std::vector<const uint64_t*> call(comms, comms + L + 1), Tall(Ts, Ts + L + 1);
  all.push_back(hp.m.get());
  for (size_t k = 0; k <= L; k++) all.push_back(hp.h[k].get());
  for (size_t k = 0; k < L + 2; k++) {
    call.push_back(&hc[12 * C * k]);
    Tall.push_back(&hT[72 * k]);
  }
  std::vector<const uint32_t*> alltabs;
  if (int rc = whole_tables(ctx, all.data(), B, alltabs)) return rc;
  // step 4: the product sum-check on the claim the verifier computes
  std::vector<tpst_sc_term> terms;
  uint64_t e0[4];
  lookup_terms(L, beta.data(), lambda.data(), terms, e0);
  const std::vector<PscTerm> dt = psc_device_terms(terms.data(), terms.size());
  std::vector<uint64_t> rsc(4 * (size_t)n);
  int rc = psc_sumcheck(ctx, alltabs.data(), B, n, dt.data(), dt.size(), tau.data(), 3,
                        [&](int i, const uint64_t*, const uint64_t* coeffs, uint64_t* r) {
                          if (i == 0 && psc_absorb_statement(&t, n, B, Tall.data(), terms.data(), terms.size(),
                                                             tau.data(), e0) != TPST_OK)
                            return fail(ctx, TPST_E_ARG, "transcript append");
                          uint64_t* out = sc_rounds + 16 * (size_t)i;
                          memcpy(out, coeffs, 128);
                          for (int c = 0; c < 4; c++)
                            if (tpst_transcript_append_fr(&t, out + 4 * c) != TPST_OK)
                              return fail(ctx, TPST_E_ARG, "transcript append");
                          tpst_transcript_challenge(&t, r);
                          memcpy(&rsc[4 * (size_t)i], r, 32);
                          return (int)TPST_OK;
                        },
                        u);
  if (rc) return rc;
  // step 6 (step 5's values are build_h's): one multi-point opening of all B polynomials
  std::vector<uint32_t> claim_poly;
  std::vector<uint64_t> points, vals;
  lookup_claims(L, n, rsc.data(), u, s, claim_poly, points, vals);
  rc = tpst_poly_open_multi(ctx, all.data(), call.data(), Tall.data(), B, claim_poly.data(), points.data(), vals.data(),
                            claim_poly.size(), &t, mp_rounds, mp_u, rho, comms_out, T_out, v_out, proof);
  if (rc) return rc;
  memcpy(T_helpers, hT.data(), 72 * 8 * (L + 2));
  *tr = t;
  return TPST_OK;
}

extern "C" int tpst_pst_lookup_reduce(tpst_transcript* tr, int n, size_t L, const uint64_t* const* Ts,
                                      const uint64_t* T_helpers, const uint64_t* sc_rounds, const uint64_t* u,
                                      const uint64_t* s, const uint64_t* mp_rounds, const uint64_t* mp_u,
                                      uint64_t* rho) {
  if (!tr || !Ts || !T_helpers || !sc_rounds || !u || !s || !mp_rounds || !mp_u || !rho) return TPST_E_ARG;
  int m_col, m_row, odd;
  if (poly_dims(n, m_col, m_row, odd) || n + 3 > 32 || L < 1 || L > LOOKUP_MAX_WITNESSES) return TPST_E_ARG;
  for (size_t j = 0; j <= L; j++)
    if (!Ts[j]) return TPST_E_ARG;
  const size_t B = 2 * L + 3;
  // every scalar and every T is validated before the sponge absorbs anything
  for (size_t j = 0; j <= L; j++)
    if (!gt_ok(Ts[j])) return TPST_E_VERIFY;
  for (size_t k = 0; k < L + 2; k++)
    if (!gt_ok(T_helpers + 72 * k)) return TPST_E_VERIFY;
  for (size_t i = 0; i < 4 * (size_t)n; i++)
    if (!fr_ok(sc_rounds + 4 * i)) return TPST_E_VERIFY;
  for (size_t i = 0; i < 3 * (size_t)n; i++)
    if (!fr_ok(mp_rounds + 4 * i)) return TPST_E_VERIFY;
  for (size_t j = 0; j < B; j++)
    if (!fr_ok(u + 4 * j) || !fr_ok(mp_u + 4 * j)) return TPST_E_VERIFY;
  for (size_t k = 0; k <= L; k++)
    if (!fr_ok(s + 4 * k)) return TPST_E_VERIFY;
  tpst_transcript t = *tr;  // tr changes only on success
  std::vector<uint64_t> beta(4), tau(4 * (size_t)n), lambda(4), rsc(4 * (size_t)n);
  if (step1(&t, L, n, Ts) != TPST_OK || step2(&t, T_helpers, beta.data()) != TPST_OK ||
      step3(&t, L, n, T_helpers + 72, tau.data(), lambda.data()) != TPST_OK)
    return TPST_E_VERIFY;
  std::vector<const uint64_t*> Tall(Ts, Ts + L + 1);
  for (size_t k = 0; k < L + 2; k++) Tall.push_back(T_helpers + 72 * k);
  std::vector<tpst_sc_term> terms;
  uint64_t e0[4];
  lookup_terms(L, beta.data(), lambda.data(), terms, e0);
  if (tpst_pst_sumcheck_reduce(&t, n, Tall.data(), B, terms.data(), terms.size(), tau.data(), e0, sc_rounds, u,
                               rsc.data()) != TPST_OK)
    return TPST_E_VERIFY;
  // step 5: sum_l s_l = s_t
  Fr sum = Fr::zero();
  for (size_t l = 0; l < L; l++) sum = add(sum, fr_canon(s + 4 * l));
  if (!eq(sum, fr_canon(s + 4 * L))) return TPST_E_VERIFY;
  std::vector<uint32_t> claim_poly;
  std::vector<uint64_t> points, vals;
  lookup_claims(L, n, rsc.data(), u, s, claim_poly, points, vals);
  if (tpst_pst_multi_reduce(&t, n, Tall.data(), B, claim_poly.data(), points.data(), vals.data(), claim_poly.size(),
                            mp_rounds, mp_u, rho) != TPST_OK)
    return TPST_E_VERIFY;
  *tr = t;
  return TPST_OK;
}

extern "C" int tpst_pst_verify_lookup(tpst_ctx* ctx, tpst_transcript* tr, int n, size_t L, const uint64_t* const* Ts,
                                      const uint64_t* T_helpers, const uint64_t* sc_rounds, const uint64_t* u,
                                      const uint64_t* s, const uint64_t* mp_rounds, const uint64_t* mp_u,
                                      const tpst_open_proof* proof) {
  if (!ctx) return TPST_E_ARG;
  if (!tr || !Ts || !T_helpers || !sc_rounds || !u || !s || !mp_rounds || !mp_u || !proof)
    return fail(ctx, TPST_E_ARG, "null argument");
  int m_col, m_row, odd;
  if (poly_dims(n, m_col, m_row, odd)) return fail(ctx, TPST_E_ARG, "bad num_vars");
  {
    std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
    SrsState* st = srs_of(ctx);
    if (!st) return fail(ctx, TPST_E_STATE, "no SRS loaded");
    if (st->nv != m_row || proof->m_col != m_col || proof->m_row != m_row)
      return fail(ctx, TPST_E_ARG, "size mismatch");
  }
  tpst_transcript t = *tr;  // tr changes only on TPST_OK
  std::vector<uint64_t> rho(4 * (size_t)n);
  int rc = tpst_pst_lookup_reduce(&t, n, L, Ts, T_helpers, sc_rounds, u, s, mp_rounds, mp_u, rho.data());
  if (rc == TPST_E_ARG) return fail(ctx, rc, "lookup: a null commitment, L not in 1..8 or n + 3 > 32");
  if (rc)
    return fail(ctx, rc, "lookup rejected (a sum-check, the identity sum_l s_l = s_t, the multi-point reduction, "
                         "a scalar >= r or a T coefficient >= p)");
  const size_t B = 2 * L + 3;
  std::vector<const uint64_t*> Tall(Ts, Ts + L + 1);
  for (size_t k = 0; k < L + 2; k++) Tall.push_back(T_helpers + 72 * k);
  std::vector<uint64_t> w(4 * B);
  if (tpst_pst_combine_challenge(&t, n, rho.data(), Tall.data(), mp_u, B, w.data()) != TPST_OK)
    return fail(ctx, TPST_E_ARG, "combine challenge");
  rc = tpst_pst_verify_combined(ctx, &t, n, rho.data(), mp_u, Tall.data(), B, w.data(), proof);
  if (rc == TPST_OK) *tr = t;
  return rc;
}
