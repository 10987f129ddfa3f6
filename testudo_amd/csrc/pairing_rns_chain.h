// RNS-engine device pieces shared by the pairing units (pairing_kernels.h
// lists them): the workgroup shape of the Fq12 kernels, the Fq12 inversion,
// the final exponentiation and the short product chain.
//
// An Fq12 kernel on the RNS engine (rns_engine.h) runs two values per
// workgroup (the two halves of every wave) on twelve waves, one per Fq12
// output coefficient, so a stage is a dozen parallel RNS Montgomery
// reductions.  The Fq inversion of the final exponentiation runs
// wave-cooperatively on waves 0 / 1 between two stages.
#pragma once
#include "pairing.h"
#include "rns_engine.h"
#include "inv_wave.h"

namespace tpst {

constexpr int RC_WAVES = 12;
// constants, three work registers, the ten registers and the inversion
// temporaries of rc_final_exp
constexpr int RC_SLOTS = rns::N_CONSTS + 36 + 10 * 12 + 24;
static_assert((size_t)(RC_SLOTS * rns::SLOT + RC_WAVES * rns::XCH) * 4 <= 65536, "RNS chain LDS");

// src^x (x = BLS_X) by square-and-multiply through registers r1, r2; returns
// the register holding it
__device__ __forceinline__ int rc_exp_by_x(const rns::Eng& e, const rns::Lane& L, int src, int r1, int r2) {
  int cur = src;
  for (int b = X_BITS - 2; b >= 0; b--) {
    int nxt = cur == r1 ? r2 : r1;
    rns::stage<rns::OP_CYC_SQR>(e, L, cur, 0, nxt);
    cur = nxt;
    if ((params::BLS_X >> b) & 1) {
      nxt = cur == r1 ? r2 : r1;
      rns::stage<rns::OP_F12_MUL>(e, L, cur, src, nxt);
      cur = nxt;
    }
  }
  return cur;
}

// f (register F) -> f^-1 in the twelve slots from D, through the tower norms
// and one Fq inversion (field.h inv(Fq12)).  I: 24 slots of temporaries, sh_n:
// the two chains' Fq-norms handed to the inverting waves and back.  f = 0
// gives 0: the norm is 0 and inv_w(0) = 0.  Contains __syncthreads.
__device__ __forceinline__ void rc_inv(const rns::Eng& e, const rns::Lane& L, int F, int I, int D, Fq* sh_n) {
  using namespace rns;
  stage<OP_INV1>(e, L, F, 0, I + 0);         // t = c0^2 - v c1^2
  stage<OP_INV2>(e, L, I + 0, 0, I + 6);     // Fq6 adjugate c'
  stage<OP_INV3>(e, L, I + 6, I + 0, I + 12);  // Fq6 norm t'
  stage<OP_INV4>(e, L, I + 12, 0, I + 14);   // Fq2 norm n
  store(e, L, I + 14, sh_n, sh_n + 1, 1);
  const int lane = threadIdx.x & 63;
  if (wave_id() < 2) {  // one chain's norm per wave, wave-cooperative inverse
    const Fq ni = inv_w(sh_n[wave_id()]);
    if (lane == 0) sh_n[wave_id()] = ni;
  }
  __syncthreads();
  load(e, L, sh_n, sh_n + 1, I + 15, 1);
  stage<OP_INV5>(e, L, I + 12, I + 15, I + 16);  // t'^-1
  stage<OP_INV6>(e, L, I + 6, I + 16, I + 18);   // t^-1
  stage<OP_INV7>(e, L, F, I + 18, D);            // f^-1
}

// f (register F) -> f^(3(p^12-1)/r); returns the result register.  Same chain
// as final_exponentiation() in pairing.h (eprint 2020/875).  regs: ten Fq12
// registers, I and sh_n: rc_inv's.  Contains __syncthreads.
// Inlined into exactly two kernels, k_chain_final_rns and k_prod_final_rns
// (pairing.hip says what a third cost).
__device__ __forceinline__ int rc_final_exp(const rns::Eng& e, const rns::Lane& L, int F, int regs, int I, Fq* sh_n) {
  using namespace rns;
#define R(i) (regs + 12 * (i))
  rc_inv(e, L, F, I, R(0), sh_n);
  // easy part
  stage<OP_CONJ>(e, L, F, 0, R(1));
  stage<OP_F12_MUL>(e, L, R(1), R(0), R(2));  // r = conj(f) f^-1
  stage<OP_FROB2>(e, L, R(2), 0, R(1));
  stage<OP_F12_MUL>(e, L, R(1), R(2), R(3));  // r = r^(p^2) r
  // hard part
  stage<OP_CYC_SQR>(e, L, R(3), 0, R(4));  // y0
  int t = rc_exp_by_x(e, L, R(3), R(5), R(6));
  stage<OP_CONJ>(e, L, R(3), 0, R(7));      // y2 = conj(r)
  stage<OP_F12_MUL>(e, L, t, R(7), R(8));   // y1 = y1 y2
  t = rc_exp_by_x(e, L, R(8), R(5), R(6));  // y2
  stage<OP_CONJ>(e, L, R(8), 0, R(7));
  stage<OP_F12_MUL>(e, L, R(7), t, R(9));   // y1 = conj(y1) y2
  t = rc_exp_by_x(e, L, R(9), R(5), R(6));  // y2
  stage<OP_FROB1>(e, L, R(9), 0, R(7));
  stage<OP_F12_MUL>(e, L, R(7), t, R(8));   // y1 = frob(y1) y2
  stage<OP_F12_MUL>(e, L, R(3), R(4), R(0));  // r = r y0
  const int y0 = rc_exp_by_x(e, L, R(8), R(5), R(6));
  const int y2 = rc_exp_by_x(e, L, y0, y0 == R(5) ? R(6) : R(5), R(1));
  stage<OP_FROB2>(e, L, R(8), 0, R(2));  // y0 = frob2(y1)
  stage<OP_CONJ>(e, L, R(8), 0, R(3));
  stage<OP_F12_MUL>(e, L, R(3), y2, R(4));   // y1 = conj(y1) y2
  stage<OP_F12_MUL>(e, L, R(4), R(2), R(7));  // y1 = y1 y0
  stage<OP_F12_MUL>(e, L, R(0), R(7), R(9));  // r = r y1
  return R(9);
#undef R
}

// workgroups for a persistent RNS kernel over `pairs` work items
static inline unsigned rns_grid(size_t pairs) {
  const size_t cap = (size_t)256 * 2;  // two workgroups per CU
  return (unsigned)(pairs < cap ? pairs : cap);
}

// product of CH factors already fetched into slots X + 12 i; returns the slot
template <int CH>
__device__ int rns_product(const rns::Eng& e, const rns::Lane& L, int X, int W) {
  int acc = X, tmp = W;
#pragma unroll
  for (int i = 1; i < CH; i++) {
    rns::stage<rns::OP_F12_MUL>(e, L, acc, X + 12 * i, tmp);
    acc = tmp;
    tmp = tmp == W ? W + 12 : W;
  }
  return acc;
}

}  // namespace tpst
