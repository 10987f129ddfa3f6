// Quad-cooperative XYZZ doubling and addition (coop.h's dbl_quad / add_quad /
// add_affine_quad level for level) with the operands of every product level
// picked by value, for the joint double-and-add chains of lincomb.hip
// (k_lincomb2) and poly_lincomb.hip (k_g1_lincomb_rows).
#pragma once
#include "acc_field.h"
#include "coop.h"
#include "device_util.h"

namespace tpst {

// b ? x : y by value.  coop.h's levels pick their operands with lvalue
// conditionals; in k_lincomb2's loop the compiler turned one of them into a
// select between two private-memory addresses, which kept both operands in
// scratch (104 B / lane).  The quad forms below are coop.h's dbl_quad /
// add_quad level for level, with this pick in place of those conditionals.
template <class F>
__device__ __forceinline__ F pick(bool b, const F& x, const F& y) {
  F r;
  const uint32_t* xs = reinterpret_cast<const uint32_t*>(&x);
  const uint32_t* ys = reinterpret_cast<const uint32_t*>(&y);
  uint32_t* d = reinterpret_cast<uint32_t*>(&r);
#pragma unroll
  for (int i = 0; i < Words<F>::n; i++) d[i] = b ? xs[i] : ys[i];
  return r;
}
template <class F>
__device__ __forceinline__ F pick4(int qi, const F& a, const F& b, const F& c, const F& d) {
  return pick(qi < 2, pick(qi == 0, a, b), pick(qi == 2, c, d));
}

// dbl-2008-s-1 (a = 0) in three product levels, one product per lane per level
template <class F>
__device__ __forceinline__ Xyzz<F> lc_dbl_quad(const Xyzz<F>& p, int qi) {
  if (is_zero(p.ZZ)) return p;
  const F U = dbl(p.Y);
  const F a1 = pick(qi == 0, U, p.X);
  F r = mul(a1, a1);
  const F V = quad_bcast<0>(r), XX = quad_bcast<1>(r);
  const F M = mul3(XX);
  r = mul(pick4(qi, U, p.X, p.ZZ, M), pick(qi == 3, M, V));
  const F W = quad_bcast<0>(r), S = quad_bcast<1>(r), ZZ3 = quad_bcast<2>(r), MM = quad_bcast<3>(r);
  Xyzz<F> q;
  q.X = sub(MM, dbl(S));
  r = mul(pick(qi == 2, M, W), pick4(qi, p.Y, p.ZZZ, sub(S, q.X), sub(S, q.X)));
  q.Y = sub(quad_bcast<2>(r), quad_bcast<0>(r));
  q.ZZ = ZZ3;
  q.ZZZ = quad_bcast<1>(r);
  return q;
}

// add-2008-s in four product levels; equal operands double, opposite ones give infinity
template <class F>
__device__ __forceinline__ Xyzz<F> lc_add_quad(const Xyzz<F>& p, const Xyzz<F>& q, int qi) {
  if (is_zero(q.ZZ)) return p;
  if (is_zero(p.ZZ)) return q;
  // L1: U1 = X1 ZZ2, U2 = X2 ZZ1, S1 = Y1 ZZZ2, S2 = Y2 ZZZ1
  F r = mul(pick4(qi, p.X, q.X, p.Y, q.Y), pick4(qi, q.ZZ, p.ZZ, q.ZZZ, p.ZZZ));
  const F U1 = quad_bcast<0>(r), U2 = quad_bcast<1>(r), S1 = quad_bcast<2>(r), S2 = quad_bcast<3>(r);
  const F P = sub(U2, U1), R = sub(S2, S1);
  if (is_zero(P)) {
    if (is_zero(R)) return lc_dbl_quad(p, qi);
    return Xyzz<F>::inf();
  }
  // L2: PP = P^2, RR = R^2, Z12 = ZZ1 ZZ2, T12 = ZZZ1 ZZZ2
  r = mul(pick4(qi, P, R, p.ZZ, p.ZZZ), pick4(qi, P, R, q.ZZ, q.ZZZ));
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

// madd-2008-s in four product levels, q affine; equal operands double, opposite ones give infinity
template <class F>
__device__ __forceinline__ Xyzz<F> lc_madd_quad(const Xyzz<F>& p, const Affine<F>& q, int qi) {
  if (is_inf(q)) return p;
  if (is_zero(p.ZZ)) return {q.x, q.y, F::one(), F::one()};
  // L1: U2 = x2 ZZ1, S2 = y2 ZZZ1
  F r = mul(pick(qi == 0, q.x, q.y), pick(qi == 0, p.ZZ, p.ZZZ));
  const F P = sub(quad_bcast<0>(r), p.X), R = sub(quad_bcast<1>(r), p.Y);
  if (is_zero(P)) {
    if (is_zero(R)) return lc_dbl_quad(Xyzz<F>{q.x, q.y, F::one(), F::one()}, qi);
    return Xyzz<F>::inf();
  }
  // L2: PP = P^2, RR = R^2
  const F l2 = pick(qi == 0, P, R);
  r = mul(l2, l2);
  const F PP = quad_bcast<0>(r), RR = quad_bcast<1>(r);
  // L3: PPP = P PP, Q = X1 PP, ZZ' = ZZ1 PP
  r = mul(pick4(qi, P, p.X, p.ZZ, p.ZZ), PP);
  const F PPP = quad_bcast<0>(r), Q = quad_bcast<1>(r);
  Xyzz<F> o;
  o.ZZ = quad_bcast<2>(r);
  o.X = sub(sub(RR, PPP), dbl(Q));
  // L4: R (Q - X'), Y1 PPP, ZZZ' = ZZZ1 PPP
  r = mul(pick4(qi, R, p.Y, p.ZZZ, p.ZZZ), pick(qi == 0, sub(Q, o.X), PPP));
  o.Y = sub(quad_bcast<0>(r), quad_bcast<1>(r));
  o.ZZZ = quad_bcast<2>(r);
  return o;
}

}  // namespace tpst
