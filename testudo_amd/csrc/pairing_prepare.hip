// G2Prepared on the RNS engine (pairing_kernels.h lists the pairing units).
//
// The doubling / addition chain of pairing.h per G2 point (one 44-slot region
// per point, the two halves of a 12-wave workgroup holding two points):
// G2_DBL1-4 / G2_ADD1-4 (tools/gen_rns_ops.py) as RNS stages, each step's line
// (region slots 6..11) dumped in residue form, then k_rns_to_fq converts every
// coefficient to field.h form in bulk -- about 280 stages per point.
#include "device_util.h"
#include "pairing_kernels.h"
#include "rns_engine.h"

namespace tpst {

__global__ void __launch_bounds__(768, 2) k_g2_prepare_rns(const uint32_t* __restrict__ g2, size_t n,
                                                           uint32_t* __restrict__ lres) {
  __shared__ uint32_t s_slots[(rns::N_CONSTS + 44) * rns::SLOT];
  __shared__ uint32_t s_xch[12 * rns::XCH];
  __shared__ uint32_t s_rows[2 * rns::NB * 32];
  rns::load_consts((rns::lds_t*)s_slots);
  const rns::LaneL L = rns::load_lane_lds((rns::lds_t*)s_rows);
  const rns::Eng e{(rns::lds_t*)s_slots, (rns::lds_t*)s_xch + rns::wave_id() * rns::XCH, 0};
  const int w = rns::wave_id(), lane = threadIdx.x & 63;
  const size_t p0 = 2 * (size_t)blockIdx.x, p1 = p0 + 1 < n ? p0 + 1 : p0;
  const int R = rns::N_CONSTS;
  __syncthreads();
  // x, y (and the copy of Q at 26..29); z = 1
  const Fq* q0 = reinterpret_cast<const Fq*>(g2 + p0 * 48);
  const Fq* q1 = reinterpret_cast<const Fq*>(g2 + p1 * 48);
  rns::load(e, L, q0, q1, R, 4);
  if (w < 4) e.slots[(R + 26 + w) * rns::SLOT + lane] = e.slots[(R + w) * rns::SLOT + lane];
  if (w == 4) e.slots[(R + 4) * rns::SLOT + lane] = e.slots[e.kon * rns::SLOT + lane];
  if (w == 5) e.slots[(R + 5) * rns::SLOT + lane] = 0;
  __syncthreads();
  const size_t p = (lane & 32) ? p1 : p0;
  size_t idx = 0;
  auto dump = [&]() {  // line (c0, c1, c2) of step idx
    if (w < 6) lres[((idx * n + p) * 6 + w) * 32 + (lane & 31)] = e.slots[(R + 6 + w) * rns::SLOT + lane];
    __syncthreads();
    idx++;
  };
  for (int b = X_BITS - 2; b >= 0; b--) {
    rns::stage<rns::OP_G2_DBL1, rns::OP_RW[rns::OP_G2_DBL1] != 0>(e, L, R, R, R);
    rns::stage<rns::OP_G2_DBL2, rns::OP_RW[rns::OP_G2_DBL2] != 0>(e, L, R, R, R);
    rns::stage<rns::OP_G2_DBL3, rns::OP_RW[rns::OP_G2_DBL3] != 0>(e, L, R, R, R);
    rns::stage<rns::OP_G2_DBL4, rns::OP_RW[rns::OP_G2_DBL4] != 0>(e, L, R, R, R);
    dump();
    if ((params::BLS_X >> b) & 1) {
      rns::stage<rns::OP_G2_ADD1, rns::OP_RW[rns::OP_G2_ADD1] != 0>(e, L, R, R, R);
      rns::stage<rns::OP_G2_ADD2, rns::OP_RW[rns::OP_G2_ADD2] != 0>(e, L, R, R, R);
      rns::stage<rns::OP_G2_ADD3, rns::OP_RW[rns::OP_G2_ADD3] != 0>(e, L, R, R, R);
      rns::stage<rns::OP_G2_ADD4, rns::OP_RW[rns::OP_G2_ADD4] != 0>(e, L, R, R, R);
      dump();
    }
  }
}

// count M-domain residue vectors (32 u32 each) -> field.h Montgomery Fq,
// two per wave and pass
__global__ void __launch_bounds__(256) k_rns_to_fq(const uint32_t* __restrict__ res, size_t count,
                                                   Fq* __restrict__ out) {
  __shared__ uint32_t s_slots[rns::N_CONSTS * rns::SLOT];
  __shared__ uint32_t s_xch[4 * rns::XCH];
  rns::load_consts((rns::lds_t*)s_slots);
  const rns::Lane L = rns::load_lane();
  const rns::Eng e{(rns::lds_t*)s_slots, (rns::lds_t*)s_xch + (threadIdx.x >> 6) * rns::XCH, 0};
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const size_t pairs = (count + 1) / 2;
  for (size_t pw = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); pw < pairs; pw += (size_t)gridDim.x * 4) {
    const size_t v0 = 2 * pw, v1 = v0 + 1 < count ? v0 + 1 : v0;
    const uint32_t x = res[((lane & 32) ? v1 : v0) * 32 + (lane & 31)];
    rns::to_fq_wave(e, L, x, out + v0, out + v1);
  }
}

// scratch: g2_prepare_scratch(n) bytes, one 32-word residue vector per Fq of
// the n x N_LINE_COEFFS line coefficients
hipError_t g2_prepare_batch(hipStream_t s, const uint32_t* d_g2, size_t n, LineCoeff* d_coeffs, uint32_t* scratch) {
  if (!n) return hipSuccess;
  if (!scratch) return hipErrorInvalidValue;
  k_g2_prepare_rns<<<(unsigned)((n + 1) / 2), 768, 0, s>>>(d_g2, n, scratch);
  TPST_TRY(hipGetLastError());
  const size_t count = n * N_LINE_COEFFS * 6;
  const size_t waves = (count + 1) / 2;
  const unsigned grid = (unsigned)(waves / 4 < 2048 ? (waves + 3) / 4 : 2048);
  k_rns_to_fq<<<grid, 256, 0, s>>>(scratch, count, reinterpret_cast<Fq*>(d_coeffs));
  return hipGetLastError();
}

}  // namespace tpst
