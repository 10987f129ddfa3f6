// Batched double-scalar multiplication on the device (lincomb.hip):
//   out[i] = s_i P_i + t_i Q_i,   F = Fq (G1), Fq2 (G2).
// The batch verifier (pst_verify_batch.hip) builds every G1 / G2 point of its
// combined pairing check with it; tpst_g1_lincomb_batch / tpst_g2_lincomb_batch
// are the host-pointer forms.
#pragma once
#include <hip/hip_runtime.h>
#include "msm.h"

namespace tpst {

// d_P, d_Q: n affine Montgomery points (24 / 48 u32 each, all-zero = infinity);
// d_s, d_t: n canonical Fr (8 u32 each), every one below 2^nbits (1 <= nbits
// <= 256: the chain walks nbits bits, so 128-bit multipliers cost half of a
// full scalar).  d_Q == d_t == nullptr: out[i] = s_i P_i.  d_out: n XYZZ
// (Montgomery), written by the launch; no other buffer is used.
template <class F>
hipError_t lincomb2(hipStream_t s, const uint32_t* d_P, const uint32_t* d_s, const uint32_t* d_Q,
                    const uint32_t* d_t, size_t n, int nbits, Xyzz<F>* d_out);

}  // namespace tpst
