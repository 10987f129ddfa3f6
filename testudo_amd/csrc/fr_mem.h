// 128-bit loads and stores of one Fr (two per element, 16-byte aligned) and
// the bind of a table's top variable: what the round kernels of the device
// sum-checks over whole tables share (poly_multi.hip, poly_sumcheck.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "field.h"

namespace tpst {

__device__ __forceinline__ Fr ld_fr16(const uint32_t* p) {
  const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
  Fr r;
  r.v[0] = a.x, r.v[1] = a.y, r.v[2] = a.z, r.v[3] = a.w;
  r.v[4] = b.x, r.v[5] = b.y, r.v[6] = b.z, r.v[7] = b.w;
  return r;
}

__device__ __forceinline__ void st_fr16(uint32_t* p, const Fr& a) {
  uint4* o = reinterpret_cast<uint4*>(p);
  o[0] = make_uint4(a.v[0], a.v[1], a.v[2], a.v[3]);
  o[1] = make_uint4(a.v[4], a.v[5], a.v[6], a.v[7]);
}

// a + r (b - a): r Montgomery; a, b both Montgomery or both canonical, the result as they are
__device__ __forceinline__ Fr bind_top(const Fr& r, const Fr& a, const Fr& b) { return add(a, mul(r, sub(b, a))); }

}  // namespace tpst
