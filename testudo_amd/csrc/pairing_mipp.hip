// The opening's look-ahead combination by squaring tables, on the RNS engine
// (pairing_kernels.h lists the pairing units).
//
// The combination t_l = A0 A3 A1^(c^-1) A2^c (and t_r from B0 .. B3) needs
// four look-ahead values raised to 253-bit exponents, known only once the
// challenge c is.  Their squarings do not depend on c: right after the
// look-ahead (off the critical path) the table S_b[k] = X_b^(2^k), k < 64, is
// stored for the four bases X_b = la8[{2, 3, 6, 7}[b]] (63 cyclotomic
// squarings each).  With the base-x digits e = sum_i e_i x^i of the exponent
// (f^p = f^x in GT, each digit < 2^64),
//     X^e = prod_i frob^i( prod_{bit k of e_i} S[k] ),
// a product of <= 64 table entries per (base, digit), then frob^i, and one
// product of ten factors per side finishes t_l = A0 A3 X_A1 X_A2 and
// t_r = B0 B3 X_B1 X_B2.
//
// Tables and partial products stay in RNS form (rns::RES_WORDS u32 per Fq12):
//   k_gt_sq_table_rns   blocks 0, 1: two bases each (the two halves), 63
//                       cyclotomic squarings, every power stored; block 2
//                       converts the plain copies (A0 A3 B0 B3) into G
//   k_gt_tab_prod1_rns  (base, digit, byte j): product of the 8 selected
//                       powers 8j .. 8j+7 (ones where the digit bit is 0)
//   k_gt_tab_prod2_rns  (base, digit): product of its 8 partials, then
//                       frob^digit -- both halves share the digit index, so
//                       they share the Frobenius stages
//   k_gt_final_rns      t_l, t_r = product of the 10 factors of each group,
//                       back to field.h Montgomery form
// about 25 stages on the critical path after the challenge.
#include "device_util.h"
#include "pairing_kernels.h"
#include "pairing_rns_chain.h"

namespace tpst {

static_assert(MIPP_TAB_F12_BYTES == rns::RES_WORDS * sizeof(uint32_t), "table entries are RNS-form Fq12");

// k_gt_sq_table_rns: tables of the bases src[sel[b]], b < n (two per block);
// the last block copies src[cp.src[j]] to G[cp.dst[j]] in RNS form
struct SqPlan {
  int n;
  int sel[12];
};
struct CopyPlan {
  int n;
  int src[12], dst[12];
};

// k_gt_tab_prod1/2_rns: exponent b has the base-x digits digits[4 tp.dig[b] + i]
// (4 x u64 per exponent) and its four factors frob^i(..), i < 4, go to
// G[tp.out[b] + i]
struct TpPlan {
  int n;
  int dig[12], out[12];
};

__global__ void __launch_bounds__(64 * RC_WAVES) k_gt_sq_table_rns(const Fq12* __restrict__ src, SqPlan sp,
                                                                   uint32_t* __restrict__ tab, CopyPlan cp,
                                                                   uint32_t* __restrict__ G) {
  __shared__ uint32_t s_slots[(rns::N_CONSTS + 24) * rns::SLOT];
  __shared__ uint32_t s_xch[RC_WAVES * rns::XCH];
  rns::load_consts((rns::lds_t*)s_slots);
  const rns::Lane L = rns::load_lane();
  const rns::Eng e{(rns::lds_t*)s_slots, (rns::lds_t*)s_xch + rns::wave_id() * rns::XCH, 0};
  __syncthreads();
  int cur = rns::N_CONSTS, nxt = cur + 12;
  if (blockIdx.x < 2) {
    const int b0 = 2 * blockIdx.x, b1 = b0 + 1;
    rns::load(e, L, reinterpret_cast<const Fq*>(src + sp.sel[b0]), reinterpret_cast<const Fq*>(src + sp.sel[b1]),
              cur, 12);
    for (int k = 0; k < 64; k++) {
      rns::store_res(e, cur, tab + (size_t)(b0 * 64 + k) * rns::RES_WORDS,
                     tab + (size_t)(b1 * 64 + k) * rns::RES_WORDS, 12);
      if (k == 63) break;
      rns::stage<rns::OP_CYC_SQR>(e, L, cur, 0, nxt);
      const int t = cur;
      cur = nxt;
      nxt = t;
    }
    return;
  }
  for (int j = 0; j < cp.n; j += 2) {
    const int j1 = j + 1 < cp.n ? j + 1 : j;
    rns::load(e, L, reinterpret_cast<const Fq*>(src + cp.src[j]), reinterpret_cast<const Fq*>(src + cp.src[j1]),
              cur, 12);
    rns::store_res(e, cur, G + (size_t)cp.dst[j] * rns::RES_WORDS, G + (size_t)cp.dst[j1] * rns::RES_WORDS, 12);
    __syncthreads();
  }
}

__global__ void __launch_bounds__(64 * RC_WAVES) k_gt_tab_prod1_rns(const uint32_t* __restrict__ tab,
                                                                    const uint64_t* __restrict__ digits, TpPlan tp,
                                                                    uint32_t* __restrict__ L1) {
  __shared__ uint32_t s_slots[(rns::N_CONSTS + 12 * 10) * rns::SLOT];
  __shared__ uint32_t s_xch[RC_WAVES * rns::XCH];
  rns::load_consts((rns::lds_t*)s_slots);
  const rns::Lane L = rns::load_lane();
  const rns::Eng e{(rns::lds_t*)s_slots, (rns::lds_t*)s_xch + rns::wave_id() * rns::XCH, 0};
  const int w = rns::wave_id(), lane = threadIdx.x & 63;
  const int q = 2 * blockIdx.x + (lane >> 5);  // (base, digit, byte) = (q / 32, q / 8 % 4, q % 8)
  const int b = q >> 5, i = (q >> 3) & 3, j = q & 7;
  const uint64_t ei = digits[4 * tp.dig[b] + i];
  const uint32_t one = w == 0 ? e.slots[e.kon * rns::SLOT + lane] : 0u;
  uint32_t v[8];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int bit = 8 * j + k;
    v[k] = ((ei >> bit) & 1) ? tab[(size_t)(b * 64 + bit) * rns::RES_WORDS + w * 32 + (lane & 31)] : one;
  }
  const int X = rns::N_CONSTS;
#pragma unroll
  for (int k = 0; k < 8; k++) e.slots[(X + 12 * k + w) * rns::SLOT + lane] = v[k];
  __syncthreads();
  const int r = rns_product<8>(e, L, X, X + 96);
  rns::store_res(e, r, L1 + (size_t)(2 * blockIdx.x) * rns::RES_WORDS, L1 + (size_t)(2 * blockIdx.x + 1) * rns::RES_WORDS,
                 12);
}

__global__ void __launch_bounds__(64 * RC_WAVES) k_gt_tab_prod2_rns(const uint32_t* __restrict__ L1, TpPlan tp,
                                                                    uint32_t* __restrict__ G) {
  __shared__ uint32_t s_slots[(rns::N_CONSTS + 12 * 10) * rns::SLOT];
  __shared__ uint32_t s_xch[RC_WAVES * rns::XCH];
  rns::load_consts((rns::lds_t*)s_slots);
  const rns::Lane L = rns::load_lane();
  const rns::Eng e{(rns::lds_t*)s_slots, (rns::lds_t*)s_xch + rns::wave_id() * rns::XCH, 0};
  const int w = rns::wave_id(), lane = threadIdx.x & 63;
  const int i = blockIdx.x >> 1, b = 2 * (blockIdx.x & 1) + (lane >> 5);  // both halves: digit i
  const int X = rns::N_CONSTS;
#pragma unroll
  for (int j = 0; j < 8; j++)
    e.slots[(X + 12 * j + w) * rns::SLOT + lane] = L1[(size_t)((b * 4 + i) * 8 + j) * rns::RES_WORDS + w * 32 + (lane & 31)];
  __syncthreads();
  int r = rns_product<8>(e, L, X, X + 96);
  const int o = r == X + 96 ? X + 108 : X + 96;
  if (i == 1) {
    rns::stage<rns::OP_FROB1>(e, L, r, 0, o);
    r = o;
  } else if (i == 2) {
    rns::stage<rns::OP_FROB2>(e, L, r, 0, o);
    r = o;
  } else if (i == 3) {
    rns::stage<rns::OP_FROB3>(e, L, r, 0, o);
    r = o;
  }
  const int b0 = 2 * (blockIdx.x & 1);
  rns::store_res(e, r, G + (size_t)(tp.out[b0] + i) * rns::RES_WORDS, G + (size_t)(tp.out[b0 + 1] + i) * rns::RES_WORDS,
                 12);
}

__global__ void __launch_bounds__(64 * RC_WAVES) k_gt_final_rns(const uint32_t* __restrict__ G, Fq12* __restrict__ out2) {
  __shared__ uint32_t s_slots[(rns::N_CONSTS + 12 * 12) * rns::SLOT];
  __shared__ uint32_t s_xch[RC_WAVES * rns::XCH];
  rns::load_consts((rns::lds_t*)s_slots);
  const rns::Lane L = rns::load_lane();
  const rns::Eng e{(rns::lds_t*)s_slots, (rns::lds_t*)s_xch + rns::wave_id() * rns::XCH, 0};
  const int w = rns::wave_id(), lane = threadIdx.x & 63, h = lane >> 5;
  const int X = rns::N_CONSTS;
#pragma unroll
  for (int f = 0; f < 10; f++)
    e.slots[(X + 12 * f + w) * rns::SLOT + lane] = G[(size_t)(10 * h + f) * rns::RES_WORDS + w * 32 + (lane & 31)];
  __syncthreads();
  const int r = rns_product<10>(e, L, X, X + 120);
  rns::store(e, L, r, reinterpret_cast<Fq*>(out2), reinterpret_cast<Fq*>(out2 + 1), 12);
}

hipError_t mipp_sq_tables(hipStream_t s, const Fq12* d_la8, Fq12* d_tab, Fq12* d_G) {
  // tables of A1 A2 B1 B2; A0 A3 / B0 B3 into slots 0, 1 of the two product lists
  const SqPlan sp{4, {2, 3, 6, 7}};
  const CopyPlan cp{4, {0, 1, 4, 5}, {0, 1, 10, 11}};
  k_gt_sq_table_rns<<<3, 64 * RC_WAVES, 0, s>>>(d_la8, sp, reinterpret_cast<uint32_t*>(d_tab), cp,
                                                reinterpret_cast<uint32_t*>(d_G));
  return hipGetLastError();
}

hipError_t mipp_combine_tab(hipStream_t s, const Fq12* d_tab, const uint64_t* d_digits, Fq12* d_G, Fq12* d_mid,
                            Fq12* d_out2) {
  const TpPlan tp{4, {0, 1, 2, 3}, {2, 6, 12, 16}};
  uint32_t* L1 = reinterpret_cast<uint32_t*>(d_mid);  // 128 partials
  k_gt_tab_prod1_rns<<<64, 64 * RC_WAVES, 0, s>>>(reinterpret_cast<const uint32_t*>(d_tab), d_digits, tp, L1);
  TPST_TRY(hipGetLastError());
  k_gt_tab_prod2_rns<<<8, 64 * RC_WAVES, 0, s>>>(L1, tp, reinterpret_cast<uint32_t*>(d_G));
  TPST_TRY(hipGetLastError());
  k_gt_final_rns<<<1, 64 * RC_WAVES, 0, s>>>(reinterpret_cast<const uint32_t*>(d_G), d_out2);
  return hipGetLastError();
}

}  // namespace tpst
