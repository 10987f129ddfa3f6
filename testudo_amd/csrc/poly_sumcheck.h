// Sum-check over a sum of products of committed polynomials, closed by one
// combined opening (poly_sumcheck.hip; include/tpst.h, "product sum-check").
// With g(x) = sum_t c_t prod_i f_{idx_t[i]}(x) over B whole polynomials of n
// variables the summand is g(x), or eq(tau, x) g(x) when tau is given.
// Internal interface of the device rounds.
#pragma once
#include <hip/hip_runtime.h>
#include <functional>
#include <vector>
#include "../../include/tpst.h"
#include "msm.h"

struct tpst_ctx;

namespace tpst {

// most terms of one sum-check (include/tpst.h)
constexpr size_t PSC_MAX_TERMS = 64;
// slots of a round's sums: slot t holds s(t), t = 0..3 (a slot the round does not compute holds 0)
constexpr int PSC_SUMS = 4;

// One term as the kernels read it.  The tables are canonical, so a chain of deg Montgomery products -- deg - 1
// between the factors, one by c -- divides R^deg out: c is handed over as c R^deg and the term comes out canonical.
struct PscTerm {
  uint32_t deg;     // 1..3
  uint32_t idx[3];  // the first deg are used, each < B
  Fr c;             // c_t R^deg
};

// What rounds 0 and 1 read: the handles' tables and, with tau, the tables of its two halves (multi_eq_halves with
// one claim of weight 1): for x = (xh << lo) | xl, eq(tau, x) = eh[xh] el[xl], Montgomery.  No table of 2^n eq
// values exists before round 1.
struct PscSrc {
  const uint32_t* const* tabs;  // device array: B tables of 2^n canonical Fr, 16-byte aligned, never written
  const uint32_t* eh;           // 2^hi Fr, or null: no eq factor
  const uint32_t* el;           // 2^lo Fr
  int lo, hi;                   // lo = n / 2, hi = n - lo
};

// One round: bind the previous challenge, then the sums over the index pairs (i, i + h/2), i < h/2, of the
// summand at t = 0, 2 and, for deg == 3, 3 (a factor's value at t = 2 is 2 hi - lo, at t = 3 it is 3 hi - 2 lo);
// round 0 also sums t = 1.  Then the reduce launch: d_sums[t] = s(t), canonical, PSC_SUMS slots.
//   round 0      no bind; reads src; the tables have length h = 2^n
//   round 1      binds *d_r while reading src (length 2h), writes the scratch tables (length h)
//   round >= 2   binds *d_r in the scratch tables in place (length 2h -> h)
// h >= 2; the closing bind of the tables of length 2 is psc_finals: d_u[j] = f_j(rho), canonical.
// d_scr: table j < B at d_scr + 8 j scr_stride (canonical), the eq table, if any, at j = B (Montgomery).
// deg: 2 or 3, the round degree D.  d_r: the challenge, Montgomery.  d_partial: PSC_SUMS psc_round_grid(...) Fr.
// The sums are exact field sums: they do not depend on the grid.
unsigned psc_round_grid(size_t pairs);
hipError_t psc_round(hipStream_t s, int round, int deg, const PscSrc& src, const PscTerm* d_terms, int M, uint32_t* d_scr,
                    size_t scr_stride, int B, size_t h, const uint32_t* d_r, uint32_t* d_partial, uint32_t* d_sums);
hipError_t psc_finals(hipStream_t s, const uint32_t* d_scr, size_t scr_stride, int B, const uint32_t* d_r, uint32_t* d_u);

// The round loop over B whole polynomials (tabs: host array of their device tables).  terms: M validated terms
// with canonical coefficients; tau: n canonical Fr or null; deg: the round degree D, 2 or 3.  After round i
// `challenge` receives s_i(0..D) (canonical, (D + 1) x 4 limbs) and the coefficients of s_i (UniPoly::from_evals
// of them, constant first, canonical) and returns the challenge rho_i (canonical) -- drawn from a transcript (the
// prover) or read from a caller's array (tpst_poly_sumcheck_stages); a non-zero return ends the call with that
// code.  Round 0 sums s_0(1) on the device (s_0(0) + s_0(1) is the claim e_0); later rounds take
// s_i(1) = e_i - s_i(0) with e_i = s_{i-1}(rho_{i-1}).  u: B canonical Fr, u_j = f_j(rho).  Takes the context's
// lock once; every device buffer is reserved before the first launch.  Arguments validated by the caller.
using PscChallenge = std::function<int(int round, const uint64_t* evals, const uint64_t* coeffs, uint64_t* rho)>;
int psc_sumcheck(tpst_ctx* ctx, const uint32_t* const* tabs, size_t B, int n, const PscTerm* terms, size_t M,
                const uint64_t* tau, int deg, const PscChallenge& challenge, uint64_t* u);

// For a prover that runs psc_sumcheck inside a protocol of its own (lookup.hip): step 1 of the product sum-check on
// t (non-zero: a T_j with a coefficient >= p), and the kernels' terms c_t R^deg_t of validated public terms.
int psc_absorb_statement(tpst_transcript* t, int n, size_t B, const uint64_t* const* Ts, const tpst_sc_term* terms,
                         size_t M, const uint64_t* tau, const uint64_t* e0);
std::vector<PscTerm> psc_device_terms(const tpst_sc_term* terms, size_t M);

}  // namespace tpst
