// Multi-point opening (poly_multi.hip): the sum-check that reduces K claims
// f_{j_k}(r_k) = v_k on B committed polynomials of n variables to B claims at
// one point rho, which one combined opening then proves (include/tpst.h,
// "multi-point opening").  Internal interface of the device reduction.
#pragma once
#include <hip/hip_runtime.h>
#include <functional>
#include <vector>
#include "msm.h"

struct tpst_ctx;
struct tpst_poly;

namespace tpst {

// most claims of one reduction (include/tpst.h)
constexpr size_t MULTI_MAX_CLAIMS = 4096;

// What rounds 0 and 1 read: the handles' tables and, per claim, the tables of
// its point's two halves.  The claims are sorted by polynomial: those of
// polynomial j are [cptr[j], cptr[j + 1]).  For x = (xh << lo) | xl
//   D_j(x) = sum_c eh[c][xh] el[c][xl],  eh[c] = a_c eq(r_c[0..hi), .),  el[c] = eq(r_c[hi..n), .)
// (MSB-first, Montgomery); no table of 2^n eq values exists.
struct MultiSrc {
  const uint32_t* const* tabs;  // device array: B tables of 2^n canonical Fr, 16-byte aligned, never written
  const uint32_t* cptr;         // B + 1
  const uint32_t* eh;           // claim c at eh + 8 (c << hi)
  const uint32_t* el;           // claim c at el + 8 (c << lo)
  int lo, hi;                   // lo = n / 2, hi = n - lo
};

// eh / el of K sorted claims from their points (d_pts: K x n Montgomery Fr) and weights (d_a: K Montgomery Fr)
hipError_t multi_eq_halves(hipStream_t s, const uint32_t* d_pts, const uint32_t* d_a, int n, size_t K, uint32_t* d_eh,
                           uint32_t* d_el);

// One round over the 2B tables D_0..D_{B-1}, F_0..F_{B-1} (k_sc_round's contract: bind the previous challenge,
// then the sums of sum_j D_j F_j over the index pairs at t = 0 and t = 2), then the reduce launch:
// d_sums[0..1] = s(0), s(2), canonical.
//   round 0      no bind; reads src; the tables have length h = 2^n
//   round 1      binds *d_r while reading src (length 2h), writes the scratch tables (length h)
//   round >= 2   binds *d_r in the scratch tables in place (length 2h -> h); h == 1 with do_sum == 0 is the
//                closing bind, after which table F_j holds f_j(rho) in entry 0
// d_scr: table t (D_j: t = j, F_j: t = B + j) at d_scr + 8 t scr_stride.  d_r: the challenge, Montgomery.
// d_partial: 2 multi_round_grid(...) Fr.  The sums are exact field sums: they do not depend on the grid.
unsigned multi_round_grid(size_t pairs);
hipError_t multi_round(hipStream_t s, int round, const MultiSrc& src, uint32_t* d_scr, size_t scr_stride, int B,
                       size_t h, const uint32_t* d_r, int do_sum, uint32_t* d_partial, uint32_t* d_sums);

// The round loop of the reduction over B whole polynomials (tabs: host array of their device tables).  Claim k is
// (claim_poly[k], points + 4 n k, weight a + 4 k), all canonical.  After round i `challenge` receives the round's
// s_i(0) and s_i(2) (canonical) and returns the challenge rho_i (canonical) -- drawn from a transcript (the prover)
// or read from a caller's array (tpst_poly_multi_sumcheck_stages); a non-zero return ends the call with that code.
// u: B canonical Fr, u_j = f_j(rho).  Takes the context's lock once; every device buffer is reserved before the
// first launch.  Arguments validated by the caller.
using MultiChallenge = std::function<int(int round, const uint64_t* s0, const uint64_t* s2, uint64_t* rho)>;
int multi_sumcheck(tpst_ctx* ctx, const uint32_t* const* tabs, size_t B, int n, const uint32_t* claim_poly,
                   const uint64_t* points, const uint64_t* a, size_t K, const MultiChallenge& challenge, uint64_t* u);

// The device tables of B whole polynomials of one context and one n, read under the context's lock (also
// poly_sumcheck.hip's).  TPST_E_ARG: a null handle, another context, differing n, a table not 16-byte aligned;
// TPST_E_STATE: a column slice or q-only handle.
int whole_tables(tpst_ctx* ctx, tpst_poly* const* polys, size_t B, std::vector<const uint32_t*>& tabs);

}  // namespace tpst
