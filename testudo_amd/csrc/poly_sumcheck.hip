// Sum-check over a sum of products of committed polynomials, closed by one
// combined opening (include/tpst.h, "product sum-check"; this project's own
// protocol, no counterpart in the reference).  With
//   g(x) = sum_t c_t prod_{i < deg_t} f_{idx_t[i]}(x)
// over B whole polynomials the claim e_0 = sum_x [eq(tau, x)] g(x) is reduced
// to the B values f_j(rho), which the combined opening (poly_lincomb.hip) then
// proves.  The shape is poly_multi.hip's:
//
//   k_psc_round<0, D>   round 0: the factors straight from the handles (never
//                      written), eq(tau, x) = EH[x >> lo] EL[x & mask] from
//                      the half tables of multi_eq_halves, so no 2^n eq table
//                      exists; sums t = 0, 1, 2 (, 3).
//   k_psc_round<1, D>   round 1: binds rho_0 while reading the same sources and
//                      writes the scratch tables, B (+ 1 for eq) of 2^(n-1) Fr.
//   k_psc_round<2, D>   later rounds: bind in place.  Lane i reads entries i,
//                      i + h/2, i + h, i + h + h/2 of a table of length 2h and
//                      writes i and i + h/2: no other lane touches those four,
//                      in the grid-stride loop either.
//   k_psc_reduce        the workgroups' partial sums -> s(0..3).
//   k_psc_finals        the closing bind of the tables of length 2: u_j.
// (k_sc_round is r1cs.hip's, welded to its four tables; hence the prefix.)
// A binding round first binds every table at the lane's pair and stores it,
// then walks the term list and loads each factor back -- its own stores, in
// program order -- so a polynomial that occurs in k factors is loaded k times
// (from cache) and no per-lane array of B values exists.  The term list is a
// small device array read by a wave-uniform index: every lane runs the same
// terms.  The tables are canonical, rho and eq Montgomery, c_t is pre-scaled
// by R^deg_t (poly_sumcheck.h): every partial sum is canonical and no
// conversion pass runs.  One lane per index pair, two 128-bit accesses per
// entry, grid-stride over a bounded grid, LDS tree per workgroup, no atomics:
// exact field sums, independent of the grid.
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
#include "poly_sumcheck.h"
#include "pst_state.h"
#include "r1cs_state.h"

namespace tpst {

namespace {

constexpr int PSC_BS = 256;
// as poly_multi.hip's: a few resident workgroups per CU, the stride loop covers the rest
constexpr unsigned PSC_MAX_GRID = 256 * 8;

// eq(tau, x), Montgomery
__device__ __forceinline__ Fr eq_at(const PscSrc& s, size_t x) {
  return mul(ld_fr16(s.eh + 8 * (x >> s.lo)), ld_fr16(s.el + 8 * (x & (((size_t)1 << s.lo) - 1))));
}

// the workgroup's sum of v, in every lane; sh: PSC_BS Fr
__device__ __forceinline__ Fr block_sum(Fr* sh, const Fr& v) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int w = PSC_BS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] = add(sh[threadIdx.x], sh[threadIdx.x + w]);
    __syncthreads();
  }
  const Fr out = sh[0];
  __syncthreads();
  return out;
}

// MODE 0: the tables (src) have length h, nothing is bound.
// MODE 1: src has length 2h; X'[y] = X[y] + r (X[y + h] - X[y]) is written to the scratch tables (length h).
// MODE 2: the same bind in the scratch tables in place.
// Then the sums over the pairs (i, i + h/2), i < h/2, of the tables of length h (h >= 2) at t = 0, 2, for DEG == 3
// also 3, for MODE 0 also 1.
template <int MODE, int DEG>
__global__ void __launch_bounds__(PSC_BS) k_psc_round(PscSrc src, const PscTerm* __restrict__ terms, int M, uint32_t* scr,
                                                    size_t scr_stride, int B, size_t h, const uint32_t* __restrict__ r,
                                                    uint32_t* __restrict__ partial) {
  __shared__ Fr sh[PSC_BS];
  const size_t half = h >> 1;
  const size_t stride = (size_t)gridDim.x * PSC_BS;
  const bool has_eq = src.eh != nullptr;
  uint32_t* E = scr + 8 * (size_t)B * scr_stride;  // the eq table (MODE != 0, has_eq)
  Fr rr = Fr::zero();
  if (MODE != 0) rr = ld_fr16(r);
  Fr s0 = Fr::zero(), s1 = Fr::zero(), s2 = Fr::zero(), s3 = Fr::zero();
  for (size_t i = (size_t)blockIdx.x * PSC_BS + threadIdx.x; i < half; i += stride) {
    const size_t i1 = i + half;
    Fr elo = Fr::zero(), ehi = Fr::zero();
    if (MODE != 0) {
      for (int j = 0; j < B; j++) {
        uint32_t* T = scr + 8 * (size_t)j * scr_stride;
        const uint32_t* Z = MODE == 1 ? src.tabs[j] : T;
        st_fr16(T + 8 * i, bind_top(rr, ld_fr16(Z + 8 * i), ld_fr16(Z + 8 * (i + h))));
        st_fr16(T + 8 * i1, bind_top(rr, ld_fr16(Z + 8 * i1), ld_fr16(Z + 8 * (i1 + h))));
      }
    }
    if (has_eq) {
      if (MODE == 0) {
        elo = eq_at(src, i);
        ehi = eq_at(src, i1);
      } else {
        if (MODE == 1) {
          elo = bind_top(rr, eq_at(src, i), eq_at(src, i + h));
          ehi = bind_top(rr, eq_at(src, i1), eq_at(src, i1 + h));
        } else {
          elo = bind_top(rr, ld_fr16(E + 8 * i), ld_fr16(E + 8 * (i + h)));
          ehi = bind_top(rr, ld_fr16(E + 8 * i1), ld_fr16(E + 8 * (i1 + h)));
        }
        st_fr16(E + 8 * i, elo);
        st_fr16(E + 8 * i1, ehi);
      }
    }
    // g at t = 0..3 for this pair; a factor is lo + t (hi - lo)
    Fr g0 = Fr::zero(), g1 = Fr::zero(), g2 = Fr::zero(), g3 = Fr::zero();
    for (int t = 0; t < M; t++) {
      const uint32_t deg = terms[t].deg;
      Fr p0, p1, p2, p3;
      for (uint32_t k = 0; k < deg; k++) {
        const uint32_t j = terms[t].idx[k];
        const uint32_t* T = MODE == 0 ? src.tabs[j] : scr + 8 * (size_t)j * scr_stride;
        const Fr lo = ld_fr16(T + 8 * i), hi = ld_fr16(T + 8 * i1);
        const Fr d = sub(hi, lo), v2 = add(hi, d);
        if (k == 0) {
          p0 = lo;
          if (MODE == 0) p1 = hi;
          p2 = v2;
          if (DEG == 3) p3 = add(v2, d);
        } else {
          p0 = mul(p0, lo);
          if (MODE == 0) p1 = mul(p1, hi);
          p2 = mul(p2, v2);
          if (DEG == 3) p3 = mul(p3, add(v2, d));
        }
      }
      const Fr c = terms[t].c;
      g0 = add(g0, mul(p0, c));
      if (MODE == 0) g1 = add(g1, mul(p1, c));
      g2 = add(g2, mul(p2, c));
      if (DEG == 3) g3 = add(g3, mul(p3, c));
    }
    if (has_eq) {
      const Fr d = sub(ehi, elo), e2 = add(ehi, d);
      g0 = mul(elo, g0);
      if (MODE == 0) g1 = mul(ehi, g1);
      g2 = mul(e2, g2);
      if (DEG == 3) g3 = mul(add(e2, d), g3);
    }
    s0 = add(s0, g0);
    if (MODE == 0) s1 = add(s1, g1);
    s2 = add(s2, g2);
    if (DEG == 3) s3 = add(s3, g3);
  }
  s0 = block_sum(sh, s0);
  if (MODE == 0) s1 = block_sum(sh, s1);
  s2 = block_sum(sh, s2);
  if (DEG == 3) s3 = block_sum(sh, s3);
  if (threadIdx.x == 0) {
    uint32_t* out = partial + 8 * (PSC_SUMS * (size_t)blockIdx.x);
    st_fr16(out, s0);
    st_fr16(out + 8, s1);
    st_fr16(out + 16, s2);
    st_fr16(out + 24, s3);
  }
}

// sum nblk partial quadruples -> out[PSC_SUMS] (canonical, as the partials are); lane (k, b) sums slot k
__global__ void __launch_bounds__(PSC_BS) k_psc_reduce(const uint32_t* __restrict__ partial, unsigned nblk,
                                                     uint32_t* __restrict__ out) {
  __shared__ Fr sh[PSC_BS];
  const unsigned k = threadIdx.x % PSC_SUMS;
  Fr a = Fr::zero();
  for (unsigned b = threadIdx.x / PSC_SUMS; b < nblk; b += PSC_BS / PSC_SUMS)
    a = add(a, ld_fr16(partial + 8 * (PSC_SUMS * (size_t)b + k)));
  sh[threadIdx.x] = a;
  __syncthreads();
  for (int w = PSC_BS / 2; w >= PSC_SUMS; w >>= 1) {  // threadIdx.x + w keeps the slot: w is a multiple of PSC_SUMS
    if ((int)threadIdx.x < w) sh[threadIdx.x] = add(sh[threadIdx.x], sh[threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x < PSC_SUMS) st_fr16(out + 8 * threadIdx.x, sh[threadIdx.x]);
}

// the closing bind of the tables of length 2: u[j] = f_j(rho)
__global__ void k_psc_finals(const uint32_t* __restrict__ scr, size_t scr_stride, int B, const uint32_t* __restrict__ r,
                            uint32_t* __restrict__ u) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= B) return;
  const uint32_t* T = scr + 8 * (size_t)j * scr_stride;
  st_fr16(u + 8 * j, bind_top(ld_fr16(r), ld_fr16(T), ld_fr16(T + 8)));
}

template <int DEG>
void launch_round(hipStream_t s, unsigned grid, int round, const PscSrc& src, const PscTerm* d_terms, int M,
                  uint32_t* d_scr, size_t scr_stride, int B, size_t h, const uint32_t* d_r, uint32_t* d_partial) {
  if (round == 0)
    k_psc_round<0, DEG><<<grid, PSC_BS, 0, s>>>(src, d_terms, M, d_scr, scr_stride, B, h, d_r, d_partial);
  else if (round == 1)
    k_psc_round<1, DEG><<<grid, PSC_BS, 0, s>>>(src, d_terms, M, d_scr, scr_stride, B, h, d_r, d_partial);
  else
    k_psc_round<2, DEG><<<grid, PSC_BS, 0, s>>>(src, d_terms, M, d_scr, scr_stride, B, h, d_r, d_partial);
}

}  // namespace

unsigned psc_round_grid(size_t pairs) {
  size_t cap = PSC_MAX_GRID;
  // TPST_SUMCHECK_GRID=g: at most g workgroups whatever the size (tests: the sums do not depend on the grid)
  if (const char* e = getenv("TPST_SUMCHECK_GRID"))
    if (atoi(e) >= 1) cap = std::min<size_t>((size_t)atoi(e), PSC_MAX_GRID);
  return (unsigned)std::min<size_t>(std::max<size_t>(grid_for(pairs, PSC_BS), 1), cap);
}

hipError_t psc_finals(hipStream_t s, const uint32_t* d_scr, size_t scr_stride, int B, const uint32_t* d_r, uint32_t* d_u) {
  if (B < 1 || B > (int)LINCOMB_MAX_TERMS || !d_scr || scr_stride < 2 || !d_r || !d_u) return hipErrorInvalidValue;
  k_psc_finals<<<grid_for(B, PSC_BS), PSC_BS, 0, s>>>(d_scr, scr_stride, B, d_r, d_u);
  return hipGetLastError();
}

hipError_t psc_round(hipStream_t s, int round, int deg, const PscSrc& src, const PscTerm* d_terms, int M, uint32_t* d_scr,
                    size_t scr_stride, int B, size_t h, const uint32_t* d_r, uint32_t* d_partial, uint32_t* d_sums) {
  // a binding round reads entries up to 2h - 1: of src in round 1 (its tables have 2h entries), of d_scr later
  if (B < 1 || B > (int)LINCOMB_MAX_TERMS || M < 1 || M > (int)PSC_MAX_TERMS || !d_terms || (deg != 2 && deg != 3) ||
      h < 2 || round < 0 || (round && (!d_r || !d_scr || scr_stride < (round == 1 ? h : 2 * h))) ||
      (round < 2 && (!src.tabs || (src.eh && !src.el))) || !d_partial || !d_sums)
    return hipErrorInvalidValue;
  const unsigned grid = psc_round_grid(h >> 1);
  if (deg == 2)
    launch_round<2>(s, grid, round, src, d_terms, M, d_scr, scr_stride, B, h, d_r, d_partial);
  else
    launch_round<3>(s, grid, round, src, d_terms, M, d_scr, scr_stride, B, h, d_r, d_partial);
  TPST_TRY(hipGetLastError());
  k_psc_reduce<<<1, PSC_BS, 0, s>>>(d_partial, grid, d_sums);
  return hipGetLastError();
}

int psc_sumcheck(tpst_ctx* ctx, const uint32_t* const* tabs, size_t B, int n, const PscTerm* terms, size_t M,
                const uint64_t* tau, int deg, const PscChallenge& challenge, uint64_t* u) {
  const int lo = n / 2, hi = n - lo;
  const size_t N = (size_t)1 << n, half = N >> 1;
  const size_t ntab = B + (tau ? 1 : 0);
  std::vector<Fr> tm(tau ? n + 1 : 0);  // tau, then the weight 1 of its one "claim", Montgomery
  for (int i = 0; tau && i < n; i++) tm[i] = fr_canon(tau + 4 * (size_t)i);
  if (tau) tm[n] = Fr::one();

  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  // everything the rounds touch is reserved here, before the first launch
  if (int rc = ensure_pinned(ctx, 4096)) return rc;
  uint64_t(*hs)[4] = reinterpret_cast<uint64_t(*)[4]>(ctx->pinned);  // the round's sums down
  uint32_t* rpin = reinterpret_cast<uint32_t*>((char*)ctx->pinned + 1024);  // the challenge up
  const unsigned grid0 = psc_round_grid(half);
  Arena& ar = ctx->arena;
  ar.reset();
  TPST_HIP(ctx, ar.reserve(Arena::need(B, sizeof(void*)) + Arena::need(M, sizeof(PscTerm)) +
                           Arena::need((size_t)n + 1, sizeof(Fr)) + Arena::need((size_t)1 << hi, sizeof(Fr)) +
                           Arena::need((size_t)1 << lo, sizeof(Fr)) + Arena::need(ntab * half, sizeof(Fr)) +
                           Arena::need(PSC_SUMS * (size_t)grid0, sizeof(Fr)) + Arena::need(PSC_SUMS, sizeof(Fr)) +
                           Arena::need(1, sizeof(Fr)) + Arena::need(B, sizeof(Fr))));
  const uint32_t** d_tabs = ar.take<const uint32_t*>(B);
  PscTerm* d_terms = ar.take<PscTerm>(M);
  uint32_t* d_tau = ar.take<uint32_t>(((size_t)n + 1) * 8);
  uint32_t* d_eh = ar.take<uint32_t>(((size_t)1 << hi) * 8);
  uint32_t* d_el = ar.take<uint32_t>(((size_t)1 << lo) * 8);
  uint32_t* d_scr = ar.take<uint32_t>(ntab * half * 8);
  uint32_t* d_partial = ar.take<uint32_t>(PSC_SUMS * (size_t)grid0 * 8);
  uint32_t* d_sums = ar.take<uint32_t>(PSC_SUMS * 8);
  uint32_t* d_r = ar.take<uint32_t>(8);
  uint32_t* d_u = ar.take<uint32_t>(B * 8);
  TPST_HIP(ctx, hipMemcpyAsync(d_tabs, tabs, B * sizeof(void*), hipMemcpyHostToDevice, st));
  TPST_HIP(ctx, hipMemcpyAsync(d_terms, terms, M * sizeof(PscTerm), hipMemcpyHostToDevice, st));
  if (tau) {
    TPST_HIP(ctx, hipMemcpyAsync(d_tau, tm.data(), tm.size() * sizeof(Fr), hipMemcpyHostToDevice, st));
    TPST_HIP(ctx, multi_eq_halves(st, d_tau, d_tau + 8 * (size_t)n, n, 1, d_eh, d_el));
  }
  const PscSrc src{d_tabs, tau ? d_eh : nullptr, tau ? d_el : nullptr, lo, hi};
  Fr e = Fr::zero();  // e_i, known from round 0 on
  for (int i = 0; i < n; i++) {
    const size_t h = N >> i;  // table length once the previous challenge is bound
    const int stage = i == 0 ? ST_SC_ROUND0 : i == 1 ? ST_SC_ROUND1 : ST_SC_ROUNDS;
    ctx->prof.begin(stage, st);
    TPST_HIP(ctx, psc_round(st, i, deg, src, d_terms, (int)M, d_scr, half, (int)B, h, d_r, d_partial, d_sums));
    ctx->prof.end(stage, st);
    TPST_HIP(ctx, hipMemcpyAsync(hs, d_sums, PSC_SUMS * 32, hipMemcpyDeviceToHost, st));
    TPST_HIP(ctx, hipStreamSynchronize(st));
    // s_i(0..deg): round 0 summed s(1) itself, later rounds take it from e_i; then the coefficients
    Fr ev[4], cs[4];
    for (int t = 0; t <= deg; t++) ev[t] = fr_canon(hs[t]);
    if (i) ev[1] = sub(e, ev[0]);
    from_evals(ev, deg + 1, cs);
    uint64_t evals[16], coeffs[16], rho[4];
    for (int t = 0; t <= deg; t++) {
      fr_out(ev[t], evals + 4 * t);
      fr_out(cs[t], coeffs + 4 * t);
    }
    if (int rc = challenge(i, evals, coeffs, rho)) return rc;
    const Fr rm = fr_canon(rho);
    e = uni_eval(cs, deg + 1, rm);
    memcpy(rpin, rm.v, 32);
    TPST_HIP(ctx, hipMemcpyAsync(d_r, rpin, 32, hipMemcpyHostToDevice, st));
  }
  // the closing bind: length 2 -> 1
  ctx->prof.begin(ST_SC_ROUNDS, st);
  TPST_HIP(ctx, psc_finals(st, d_scr, half, (int)B, d_r, d_u));
  ctx->prof.end(ST_SC_ROUNDS, st);
  TPST_HIP(ctx, hipMemcpyAsync(u, d_u, B * 32, hipMemcpyDeviceToHost, st));
  TPST_HIP(ctx, hipStreamSynchronize(st));
  return TPST_OK;
}

}  // namespace tpst

using namespace tpst;

namespace {

int append_int(tpst_transcript* t, uint64_t x) {
  const uint64_t l[4] = {x, 0, 0, 0};
  return tpst_transcript_append_fr(t, l);
}

// What prover and verifier ask of the statement's shape: 0 and the round degree D, or a message.
const char* terms_shape(int n, size_t B, const tpst_sc_term* terms, size_t M, bool has_tau, int& D) {
  int m_col, m_row, odd;
  if (poly_dims(n, m_col, m_row, odd)) return "bad num_vars";
  if (B < 1 || B > LINCOMB_MAX_TERMS) return "the number of polynomials must be 1..256";
  if (M < 1 || M > PSC_MAX_TERMS) return "the number of terms must be 1..64";
  std::vector<uint8_t> seen(B, 0);
  uint32_t maxdeg = 0;
  for (size_t t = 0; t < M; t++) {
    if (terms[t].deg < 1 || terms[t].deg > 3) return "a term's degree must be 1..3";
    maxdeg = std::max(maxdeg, terms[t].deg);
    for (uint32_t k = 0; k < terms[t].deg; k++) {
      if (terms[t].idx[k] >= B) return "a term on a polynomial index >= B";
      seen[terms[t].idx[k]] = 1;
    }
  }
  for (size_t j = 0; j < B; j++)
    if (!seen[j]) return "a polynomial in no term";
  D = (int)maxdeg + (has_tau ? 1 : 0);
  if (D > 3) return "round degree above 3 (a cubic term under eq)";
  if (D < 2) D = 2;  // UniPoly::from_evals takes 3 or 4 evaluations
  return nullptr;
}

bool statement_canonical(int n, const tpst_sc_term* terms, size_t M, const uint64_t* tau) {
  for (size_t t = 0; t < M; t++)
    if (!fr_ok(terms[t].coeff)) return false;
  for (int i = 0; tau && i < n; i++)
    if (!fr_ok(tau + 4 * (size_t)i)) return false;
  return true;
}

}  // namespace

// step 1: the statement
int tpst::psc_absorb_statement(tpst_transcript* t, int n, size_t B, const uint64_t* const* Ts, const tpst_sc_term* terms,
                               size_t M, const uint64_t* tau, const uint64_t* e0) {
  int rc = append_int(t, B) | append_int(t, M) | append_int(t, (uint64_t)n) | append_int(t, tau ? 1 : 0);
  for (size_t j = 0; j < B; j++) rc |= tpst_transcript_append_gt(t, Ts[j]);
  for (size_t k = 0; k < M; k++) {
    rc |= append_int(t, terms[k].deg);
    for (uint32_t i = 0; i < terms[k].deg; i++) rc |= append_int(t, terms[k].idx[i]);
    rc |= tpst_transcript_append_fr(t, terms[k].coeff);
  }
  for (int i = 0; tau && i < n; i++) rc |= tpst_transcript_append_fr(t, tau + 4 * (size_t)i);
  rc |= tpst_transcript_append_fr(t, e0);
  return rc;
}

// the kernels' terms: c_t R^deg_t (poly_sumcheck.h)
std::vector<PscTerm> tpst::psc_device_terms(const tpst_sc_term* terms, size_t M) {
  std::vector<PscTerm> out(M);
  for (size_t t = 0; t < M; t++) {
    out[t].deg = terms[t].deg;
    for (int k = 0; k < 3; k++) out[t].idx[k] = k < (int)terms[t].deg ? terms[t].idx[k] : 0;
    Fr c;
    memcpy(c.v, terms[t].coeff, 32);
    for (uint32_t k = 0; k < terms[t].deg; k++) c = to_mont(c);
    out[t].c = c;
  }
  return out;
}

namespace {

// what prover and stages entry check alike; n and D out
int prover_args(tpst_ctx* ctx, tpst_poly* const* polys, size_t B, const tpst_sc_term* terms, size_t M,
                const uint64_t* tau, std::vector<const uint32_t*>& tabs, int& n, int& D) {
  if (B < 1 || B > LINCOMB_MAX_TERMS) return fail(ctx, TPST_E_ARG, "the number of polynomials must be 1..256");
  if (int rc = whole_tables(ctx, polys, B, tabs)) return rc;
  n = polys[0]->n;
  if (const char* m = terms_shape(n, B, terms, M, tau != nullptr, D)) return fail(ctx, TPST_E_ARG, m);
  if (!statement_canonical(n, terms, M, tau)) return fail(ctx, TPST_E_ARG, "coefficient or coordinate >= r");
  return TPST_OK;
}

}  // namespace

extern "C" int tpst_poly_sumcheck_stages(tpst_ctx* ctx, tpst_poly* const* polys, size_t B, const tpst_sc_term* terms,
                                         size_t M, const uint64_t* tau, const uint64_t* rho, uint64_t* sums,
                                         uint64_t* u) {
  if (!ctx) return TPST_E_ARG;
  if (!polys || !terms || !rho || !sums || !u) return fail(ctx, TPST_E_ARG, "null argument");
  std::vector<const uint32_t*> tabs;
  int n, D;
  if (int rc = prover_args(ctx, polys, B, terms, M, tau, tabs, n, D)) return rc;
  for (int i = 0; i < n; i++)
    if (!fr_ok(rho + 4 * i)) return fail(ctx, TPST_E_ARG, "challenge >= r");
  const std::vector<PscTerm> dt = psc_device_terms(terms, M);
  return psc_sumcheck(ctx, tabs.data(), B, n, dt.data(), M, tau, D,
                     [&](int i, const uint64_t* evals, const uint64_t*, uint64_t* r) {
                       memcpy(sums + 4 * (size_t)(D + 1) * i, evals, 32 * (size_t)(D + 1));
                       memcpy(r, rho + 4 * i, 32);
                       return TPST_OK;
                     },
                     u);
}

extern "C" int tpst_poly_sumcheck_open(tpst_ctx* ctx, tpst_poly* const* polys, const uint64_t* const* comms,
                                       const uint64_t* const* Ts, size_t B, const tpst_sc_term* terms, size_t M,
                                       const uint64_t* tau, tpst_transcript* tr, uint64_t* e0, uint64_t* rounds,
                                       uint64_t* u, uint64_t* rho, uint64_t* comms_out, uint64_t* T_out,
                                       uint64_t* v_out, tpst_open_proof* proof) {
  if (!ctx) return TPST_E_ARG;
  if (!polys || !comms || !Ts || !terms || !tr || !e0 || !rounds || !u || !rho || !comms_out || !T_out || !v_out ||
      !proof)
    return fail(ctx, TPST_E_ARG, "null argument");
  if (B < 1 || B > LINCOMB_MAX_TERMS) return fail(ctx, TPST_E_ARG, "the number of polynomials must be 1..256");
  for (size_t j = 0; j < B; j++)
    if (!comms[j] || !Ts[j]) return fail(ctx, TPST_E_ARG, "null commitment " + std::to_string(j));
  std::vector<const uint32_t*> tabs;
  int n, D;
  if (int rc = prover_args(ctx, polys, B, terms, M, tau, tabs, n, D)) return rc;
  {
    std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
    if (!srs_of(ctx)) return fail(ctx, TPST_E_STATE, "no SRS loaded");
  }
  const std::vector<PscTerm> dt = psc_device_terms(terms, M);
  tpst_transcript t = *tr;  // tr changes only on success
  const int rc = psc_sumcheck(ctx, tabs.data(), B, n, dt.data(), M, tau, D,
                             [&](int i, const uint64_t* evals, const uint64_t* coeffs, uint64_t* r) {
                               if (i == 0) {  // the claim is known now: e_0 = s_0(0) + s_0(1); then step 1
                                 fr_out(add(fr_canon(evals), fr_canon(evals + 4)), e0);
                                 if (psc_absorb_statement(&t, n, B, Ts, terms, M, tau, e0) != TPST_OK)
                                   return fail(ctx, TPST_E_ARG, "a T_j with a coefficient >= p");
                               }
                               uint64_t* out = rounds + 4 * (size_t)(D + 1) * i;
                               memcpy(out, coeffs, 32 * (size_t)(D + 1));
                               for (int c = 0; c <= D; c++)
                                 if (tpst_transcript_append_fr(&t, out + 4 * c) != TPST_OK)
                                   return fail(ctx, TPST_E_ARG, "transcript append");
                               tpst_transcript_challenge(&t, r);
                               memcpy(rho + 4 * (size_t)i, r, 32);
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

extern "C" int tpst_pst_sumcheck_reduce(tpst_transcript* tr, int n, const uint64_t* const* Ts, size_t B,
                                        const tpst_sc_term* terms, size_t M, const uint64_t* tau, const uint64_t* e0,
                                        const uint64_t* rounds, const uint64_t* u, uint64_t* rho) {
  if (!tr || !Ts || !terms || !e0 || !rounds || !u || !rho) return TPST_E_ARG;
  int D;
  if (terms_shape(n, B, terms, M, tau != nullptr, D)) return TPST_E_ARG;
  for (size_t j = 0; j < B; j++)
    if (!Ts[j]) return TPST_E_ARG;
  // every scalar is validated before the sponge absorbs anything
  if (!statement_canonical(n, terms, M, tau) || !fr_ok(e0)) return TPST_E_VERIFY;
  for (size_t j = 0; j < B; j++)
    if (!fr_ok(u + 4 * j) || !gt_ok(Ts[j])) return TPST_E_VERIFY;
  for (int i = 0; i < (D + 1) * n; i++)
    if (!fr_ok(rounds + 4 * (size_t)i)) return TPST_E_VERIFY;
  tpst_transcript t = *tr;  // tr changes only on success
  if (psc_absorb_statement(&t, n, B, Ts, terms, M, tau, e0) != TPST_OK) return TPST_E_VERIFY;
  Fr e = fr_canon(e0);
  std::vector<Fr> rs(n);
  std::vector<uint64_t> rc(4 * (size_t)n);
  for (int i = 0; i < n; i++) {
    const uint64_t* rd = rounds + 4 * (size_t)(D + 1) * i;
    Fr cs[4], s01 = Fr::zero();
    for (int c = 0; c <= D; c++) {
      cs[c] = fr_canon(rd + 4 * c);
      s01 = add(s01, cs[c]);
    }
    // s_i(0) + s_i(1) = 2 c0 + c1 + .. + cD = e_i
    if (!eq(add(s01, cs[0]), e)) return TPST_E_VERIFY;
    for (int c = 0; c <= D; c++) tpst_transcript_append_fr(&t, rd + 4 * c);
    tpst_transcript_challenge(&t, &rc[4 * (size_t)i]);
    rs[i] = fr_canon(&rc[4 * (size_t)i]);
    e = uni_eval(cs, D + 1, rs[i]);
  }
  // e_n = [prod_i (tau_i rho_i + (1 - tau_i)(1 - rho_i))] sum_t c_t prod_i u_{idx_t[i]}
  Fr g = Fr::zero();
  for (size_t k = 0; k < M; k++) {
    Fr p = fr_canon(terms[k].coeff);
    for (uint32_t i = 0; i < terms[k].deg; i++) p = mul(p, fr_canon(u + 4 * (size_t)terms[k].idx[i]));
    g = add(g, p);
  }
  for (int i = 0; tau && i < n; i++) {
    const Fr x = fr_canon(tau + 4 * (size_t)i);
    g = mul(g, add(mul(x, rs[i]), mul(sub(Fr::one(), x), sub(Fr::one(), rs[i]))));
  }
  if (!eq(g, e)) return TPST_E_VERIFY;
  memcpy(rho, rc.data(), 32 * (size_t)n);
  *tr = t;
  return TPST_OK;
}

extern "C" int tpst_pst_verify_sumcheck(tpst_ctx* ctx, tpst_transcript* tr, int n, const uint64_t* const* Ts, size_t B,
                                        const tpst_sc_term* terms, size_t M, const uint64_t* tau, const uint64_t* e0,
                                        const uint64_t* rounds, const uint64_t* u, const tpst_open_proof* proof) {
  if (!ctx) return TPST_E_ARG;
  if (!tr || !Ts || !terms || !e0 || !rounds || !u || !proof) return fail(ctx, TPST_E_ARG, "null argument");
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
  int rc = tpst_pst_sumcheck_reduce(&t, n, Ts, B, terms, M, tau, e0, rounds, u, rho.data());
  if (rc == TPST_E_ARG)
    return fail(ctx, rc, "product sum-check: sizes or a degree out of range, an index >= B or a polynomial in no term");
  if (rc) return fail(ctx, rc, "product sum-check rejected (a round check, the final identity or a scalar >= r)");
  if (tpst_pst_combine_challenge(&t, n, rho.data(), Ts, u, B, w.data()) != TPST_OK)
    return fail(ctx, TPST_E_ARG, "combine challenge");
  rc = tpst_pst_verify_combined(ctx, &t, n, rho.data(), u, Ts, B, w.data(), proof);
  if (rc == TPST_OK) *tr = t;
  return rc;
}
