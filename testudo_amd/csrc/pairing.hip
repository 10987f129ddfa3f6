// K4: optimal-ate multi-pairing on gfx950, by line products on the RNS engine
// (pairing_kernels.h lists the pairing units).
//
// Prepared line coefficients are coefficient-major (all pairs' step-idx
// coefficients contiguous) so the line evaluation's loads are coalesced across
// threads.  With m_{p,b} the line value(s) of pair p at bit b (b = 62..0), the
// Miller product of a group is
//     prod_p f_p = prod_b M_b^(2^b),   M_b = prod_p m_{p,b}.
// The M_b do not depend on f, so they are a parallel tree over the pairs:
// k_line_pair multiplies the lines of two pairs (one lane per product), then
// k_chunk_prod_rns levels of TREE_CHUNK factors each run down to one value per
// (group, line).  The only serial chain left is Horner over the bits: per
// block of LB bits a block multiplier
//     MB_j = prod_{b in block} M_b^(2^(b - lo_j))
// (k_miller_blocks_rns, all blocks in parallel), then F = MB_top,
// F = F^(2^LB) MB_j for the lower blocks, and the final exponentiation in the
// same workgroup (k_chain_final_rns): 56 squarings + 7 products instead of
// 63 x (square + line product) per pair.
// G1 operands may be XYZZ: the line of column j is scaled by
// lambda = ZZ ZZZ in Fq (c0 Y ZZ, c1 X ZZZ, c2 ZZ ZZZ), a factor the final
// exponentiation removes, so no inversion is needed before pairing.
#include "device_util.h"
#include "pairing_kernels.h"
#include "pairing_rns_chain.h"
#include <cstdlib>

namespace tpst {

constexpr int LB = 8;                                     // bits per block
constexpr int N_BITS = X_BITS - 1;                        // 63 Miller bits
constexpr int NBLK = (N_BITS + LB - 1) / LB;              // 8 blocks
constexpr int TREE_CHUNK = (int)plan::TREE_CHUNK;

static_assert(plan::F12_BYTES == sizeof(Fq12) && plan::LINE_BYTES == sizeof(LineCoeff) &&
                  plan::RES_WORDS == rns::RES_WORDS && plan::N_LINES == N_LINE_COEFFS && plan::NBLK == NBLK,
              "pairing_plan.h sizes");
static_assert(plan::need(1, 1) == Arena::need(1, 1) && plan::need(257, 3) == Arena::need(257, 3),
              "pairing_plan.h rounds as Arena::take does");

// ---- lines of the pairs, multiplied two and two ------------------------------
// column of pair (g, k) in d_g2 / d_coeffs (pairing_kernels.h: map_s)
__device__ __forceinline__ size_t pair_column(size_t g, size_t k, size_t n, size_t map_s) {
  return map_s ? (k / map_s) * 2 * map_s + (g == 0 ? map_s : 0) + k % map_s : g * n + k;
}

__global__ void k_set_one(Fq12* __restrict__ v, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = Fq12::one();
}

// Products kept in program order: sched_barrier stops the scheduler from
// interleaving independent Montgomery products, which multiplies the live
// limbs past the register file (hundreds of spilled VGPRs otherwise).
__device__ __forceinline__ Fq smul(const Fq& a, const Fq& b) {
  const Fq r = mul(a, b);
  __builtin_amdgcn_sched_barrier(0);
  return r;
}
__device__ __forceinline__ Fq2 smul(const Fq2& a, const Fq2& b) {
  const Fq v0 = smul(a.c0, b.c0);
  const Fq v1 = smul(a.c1, b.c1);
  const Fq t = smul(add(a.c0, a.c1), add(b.c0, b.c1));
  return {sub(v0, mul5(v1)), sub(sub(t, v0), v1)};
}
__device__ __forceinline__ Fq2 smul_fq(const Fq2& a, const Fq& b) { return {smul(a.c0, b), smul(a.c1, b)}; }

// Sparse line value c0' + c3' w + c4' v w of one pair at its G1 point
// (ark ell(): c0 py, c1 px, c2), or the G1 point's lambda = ZZ ZZZ scaling of
// all three when P is XYZZ (a factor the final exponentiation removes).
// Returns false when the G1 point is at infinity (the pair contributes 1).
__device__ __forceinline__ bool line_at(const LineCoeff* __restrict__ coeffs, size_t col, const uint32_t* g1, size_t p,
                                        bool xyzz, Fq2& c0, Fq2& c3, Fq2& c4) {
  Fq px, py, lam;
  if (xyzz) {
    const Xyzz<Fq> P = load_xyzz(reinterpret_cast<const Xyzz<Fq>*>(g1), p);
    if (is_inf(P)) return false;
    px = smul(P.X, P.ZZZ);
    py = smul(P.Y, P.ZZ);
    lam = smul(P.ZZ, P.ZZZ);
  } else {
    const G1A P = load_affine<Fq>(g1, p);
    if (is_inf(P)) return false;
    px = P.x;
    py = P.y;
  }
  const LineCoeff c = coeffs[col];
  c0 = smul_fq(c.c0, py);
  c3 = smul_fq(c.c1, px);
  c4 = xyzz ? smul_fq(c.c2, lam) : c.c2;
  return true;
}

// Pair maps: pair (g, k) of a multi-pairing -> (G1 index, G2 column).
// Standard: column pair_column(g, k), G1 = the same index (affine), or the
// half-rotated XYZZ index within blocks of rot_L (MIPP's t_l / t_r pairs).
struct PairMapStd {
  size_t n, map_s, rot_L;
  __device__ void at(size_t g, size_t k, size_t& p, size_t& q) const {
    q = pair_column(g, k, n, map_s);
    p = rot_L ? (q / rot_L) * rot_L + ((q % rot_L) + rot_L / 2) % rot_L : q;
  }
};

// Pair products of the lines: out[(g 69 + idx) nout + c] = line idx of pair
// (g, 2c) times that of pair (g, 2c + 1) (the lone line when n is odd), one
// lane per product.  Two sparse line values A = a0 + (a3 + a4 v) w and B
// multiply to
//   (a0 b0 + u a4 b4, a3 b3, a3 b4 + a4 b3) + (a0 b3 + a3 b0, a0 b4 + a4 b0, 0) w
// -- six Fq2 products with Karatsuba cross terms -- stored as a dense Fq12:
// half as many values for the tree that follows, and none of its dense x
// dense products at the widest level (its workgroups are latency-bound
// stage chains; this is throughput work).
template <class Map>
__global__ void __launch_bounds__(64, 1) k_line_pair(const LineCoeff* __restrict__ coeffs, size_t ncol,
                                                     const uint32_t* __restrict__ g1, int xyzz,
                                                     const uint32_t* __restrict__ g2, size_t groups, size_t n,
                                                     Map map, size_t nout, Fq12* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= groups * N_LINE_COEFFS * nout) return;
  const size_t c = t % nout, gi = t / nout, idx = gi % N_LINE_COEFFS, g = gi / N_LINE_COEFFS;
  Fq2 a0, a3, a4, b0, b3, b4;
  bool ha = false, hb = false;
  size_t p, q;
  map.at(g, 2 * c, p, q);
  if (!is_inf(load_affine<Fq2>(g2, q))) ha = line_at(coeffs, idx * ncol + q, g1, p, xyzz != 0, a0, a3, a4);
  if (2 * c + 1 < n) {
    map.at(g, 2 * c + 1, p, q);
    if (!is_inf(load_affine<Fq2>(g2, q))) hb = line_at(coeffs, idx * ncol + q, g1, p, xyzz != 0, b0, b3, b4);
  }
  Fq12* o = out + t;
  if (ha && hb) {
    const Fq2 m33 = smul(a3, b3);
    o->c0.c1 = m33;
    const Fq2 m00 = smul(a0, b0);
    o->c1.c0 = sub(sub(smul(add(a0, a3), add(b0, b3)), m00), m33);
    const Fq2 m44 = smul(a4, b4);
    o->c0.c2 = sub(sub(smul(add(a3, a4), add(b3, b4)), m33), m44);
    o->c0.c0 = add(m00, mul_by_u(m44));
    o->c1.c1 = sub(sub(smul(add(a0, a4), add(b0, b4)), m00), m44);
    o->c1.c2 = Fq2::zero();
  } else if (ha || hb) {
    *o = ha ? Fq12{{a0, Fq2::zero(), Fq2::zero()}, {a3, a4, Fq2::zero()}}
            : Fq12{{b0, Fq2::zero(), Fq2::zero()}, {b3, b4, Fq2::zero()}};
  } else {
    *o = Fq12::one();
  }
}

// line index of the doubling at bit b (62..0); its addition line follows it
__device__ __forceinline__ int dbl_idx(int b) {
  int idx = 0;
  for (int c = X_BITS - 2; c > b; c--) idx += 1 + (int)((params::BLS_X >> c) & 1);
  return idx;
}

// ---- tree products, block multipliers and the Horner chain ------------------
// tree products on the RNS engine: out[g][j] = prod in[g][j*CH .. j*CH+CH),
// two outputs per workgroup, the result in RNS form.  From field.h Fq12
// (RES_IN false) the first factor is loaded with K_LOAD[CH] and the others
// raw (no reduction), so a chunk costs CH - 1 stages; a short tail chunk is
// padded with ones so both halves run the same stage sequence.
template <bool RES_IN, int CH>
__global__ void __launch_bounds__(64 * RC_WAVES, 2) k_chunk_prod_rns(const void* __restrict__ in, size_t groups,
                                                                  size_t n, size_t nout, uint32_t* __restrict__ out) {
  __shared__ uint32_t s_slots[(rns::N_CONSTS + 12 * (CH + 1)) * rns::SLOT];
  __shared__ uint32_t s_xch[RC_WAVES * rns::XCH];
  __shared__ uint32_t s_rows[2 * rns::NB * 32];
  const size_t items = groups * nout, pairs = (items + 1) / 2;
  rns::load_consts((rns::lds_t*)s_slots);
  const rns::LaneL L = rns::load_lane_lds((rns::lds_t*)s_rows);
  const rns::Eng e{(rns::lds_t*)s_slots, (rns::lds_t*)s_xch + rns::wave_id() * rns::XCH, 0};
  const int w = rns::wave_id(), lane = threadIdx.x & 63;
  const int X = rns::N_CONSTS;  // factor i in slots X + 12 i; the product ping-pongs with X + 12 CH
  __syncthreads();
  // persistent: a workgroup walks the output pairs (its setup amortized)
  for (size_t pr = blockIdx.x; pr < pairs; pr += gridDim.x) {
    const size_t o = (lane & 32) ? (2 * pr + 1 < items ? 2 * pr + 1 : 2 * pr) : 2 * pr;
    const size_t k0 = (o % nout) * CH, base = (o / nout) * n;
    // wave w fetches coefficient w of all CH factors at once (one memory
    // latency per chunk, not one per factor)
    uint32_t v[CH];
#pragma unroll
    for (int i = 0; i < CH; i++) {
      const bool valid = k0 + i < n;
      if (RES_IN) {
        const uint32_t* r = static_cast<const uint32_t*>(in);
        v[i] = valid ? r[(base + k0 + i) * rns::RES_WORDS + w * 32 + (lane & 31)]
                     : (w == 0 ? e.slots[e.kon * rns::SLOT + lane] : 0u);
      } else {
        const Fq* f = static_cast<const Fq*>(in) + 12 * (base + k0 + i);
        if (valid) {
          v[i] = rns::residue(L, f[w].v);
        } else {
          uint32_t one[12];
#pragma unroll
          for (int k = 0; k < 12; k++) one[k] = w == 0 ? params::FQ_ONE[k] : 0u;
          v[i] = rns::residue(L, one);
        }
      }
    }
    if (!RES_IN) {  // the first of CH raw factors carries the (M/R)^(CH-1) M correction
      const uint32_t kin = e.slots[(e.kon + rns::K_LOAD[CH]) * rns::SLOT + lane];
      v[0] = rns::mont(e, L, rns::red64((uint64_t)v[0] * kin, L));
    }
#pragma unroll
    for (int i = 0; i < CH; i++) e.slots[(X + 12 * i + w) * rns::SLOT + lane] = v[i];
    __syncthreads();
    int acc = X, tmp = X + 12 * CH;
#pragma unroll
    for (int i = 1; i < CH; i++) {
      rns::stage<rns::OP_F12_MUL>(e, L, acc, X + 12 * i, tmp);
      const int t = acc;
      acc = tmp;
      tmp = t;
    }
    rns::store_res(e, acc, out + 2 * pr * rns::RES_WORDS,
                   out + (2 * pr + 1 < items ? 2 * pr + 1 : 2 * pr) * rns::RES_WORDS, 12);
    __syncthreads();  // the next chunk's factors overwrite these slots
  }
}

// block multipliers on the RNS engine: one workgroup per (block, pair of
// groups) -- both halves of a wave must run the same stage sequence, so the
// pair shares the block (and so its bit pattern).  Input: the per-bit line
// products M (field.h Fq12, or RNS form from k_chunk_prod_rns); MB is left
// in RNS form.
constexpr int MB_MAXV = 12;  // line products one block reads (LB doublings + its additions)

template <bool RES_IN>
__global__ void __launch_bounds__(64 * RC_WAVES) k_miller_blocks_rns(const void* __restrict__ M, size_t groups,
                                                                     uint32_t* __restrict__ MBr) {
  __shared__ uint32_t s_slots[(rns::N_CONSTS + 24 + 12 * MB_MAXV) * rns::SLOT];
  __shared__ uint32_t s_xch[RC_WAVES * rns::XCH];
  const size_t pairs = (groups + 1) / 2;
  const int blk = (int)(blockIdx.x / pairs);
  const size_t g0 = 2 * (blockIdx.x % pairs), g1 = g0 + 1 < groups ? g0 + 1 : g0;
  rns::load_consts((rns::lds_t*)s_slots);
  const rns::Lane L = rns::load_lane();
  const rns::Eng e{(rns::lds_t*)s_slots, (rns::lds_t*)s_xch + rns::wave_id() * rns::XCH, 0};
  const int w = rns::wave_id(), lane = threadIdx.x & 63;
  const size_t g = (lane & 32) ? g1 : g0;
  const int lo = blk * LB, hi = (lo + LB < N_BITS ? lo + LB : N_BITS) - 1;
  const int V = rns::N_CONSTS + 24;  // the block's line products, in reading order
  // every line product of the block fetched at once: line index idx(hi) .. ,
  // in the order the Horner below consumes them
  const int idx_hi = dbl_idx(hi);
  const int nv = dbl_idx(lo) + 1 + (int)((params::BLS_X >> lo) & 1) - idx_hi;
  for (int v = 0; v < nv; v++) {
    const size_t li = g * N_LINE_COEFFS + idx_hi + v;
    uint32_t x;
    if (RES_IN) {
      x = static_cast<const uint32_t*>(M)[li * rns::RES_WORDS + w * 32 + (lane & 31)];
    } else {
      const uint32_t r = rns::residue(L, static_cast<const Fq*>(M)[12 * li + w].v);
      x = rns::mont(e, L, rns::red64((uint64_t)r * e.slots[(e.kon + rns::K_IN) * rns::SLOT + lane], L));
    }
    e.slots[(V + 12 * v + w) * rns::SLOT + lane] = x;
  }
  __syncthreads();
  // two work registers; other(x) is the one not holding x
  const int W0 = rns::N_CONSTS, W1 = rns::N_CONSTS + 12;
  auto other = [&](int x) { return x == W0 ? W1 : W0; };
  int acc = V, v = 1;
  for (int b = hi; b >= lo; b--) {
    if (b != hi) {
      const int t = other(acc);
      rns::stage<rns::OP_F12_SQR>(e, L, acc, 0, t);
      acc = other(t);
      rns::stage<rns::OP_F12_MUL>(e, L, t, V + 12 * v++, acc);
    }
    if ((params::BLS_X >> b) & 1) {
      const int t = other(acc);
      rns::stage<rns::OP_F12_MUL>(e, L, acc, V + 12 * v++, t);
      acc = t;
    }
  }
  rns::store_res(e, acc, MBr + (g0 * NBLK + blk) * rns::RES_WORDS, MBr + (g1 * NBLK + blk) * rns::RES_WORDS, 12);
}

// F = MB_top, F = F^(2^LB) MB_j down the blocks; two groups per workgroup.
// do_final = 0 leaves the Miller product (a rank's partial of a row-sharded
// commit or opening).
__global__ void __launch_bounds__(64 * RC_WAVES) k_chain_final_rns(const uint32_t* __restrict__ MBr, size_t groups,
                                                                   Fq12* __restrict__ out, int do_final) {
  __shared__ uint32_t s_slots[RC_SLOTS * rns::SLOT];
  __shared__ uint32_t s_xch[RC_WAVES * rns::XCH];
  __shared__ Fq sh_n[2];
  const size_t g0 = 2 * (size_t)blockIdx.x, g1 = g0 + 1 < groups ? g0 + 1 : g0;
  rns::load_consts((rns::lds_t*)s_slots);
  const rns::Lane L = rns::load_lane();
  const rns::Eng e{(rns::lds_t*)s_slots, (rns::lds_t*)s_xch + rns::wave_id() * rns::XCH, 0};
  __syncthreads();
  int acc = rns::N_CONSTS, in_r = acc + 12, tmp = acc + 24;
  const uint32_t* m0 = MBr + g0 * NBLK * rns::RES_WORDS;
  const uint32_t* m1 = MBr + g1 * NBLK * rns::RES_WORDS;
  rns::load_res(e, m0 + (NBLK - 1) * rns::RES_WORDS, m1 + (NBLK - 1) * rns::RES_WORDS, acc, 12);
  for (int blk = NBLK - 2; blk >= 0; blk--) {
    for (int i = 0; i < LB; i++) {
      rns::stage<rns::OP_F12_SQR>(e, L, acc, 0, tmp);
      const int t = acc;
      acc = tmp;
      tmp = t;
    }
    rns::load_res(e, m0 + blk * rns::RES_WORDS, m1 + blk * rns::RES_WORDS, in_r, 12);
    rns::stage<rns::OP_F12_MUL>(e, L, acc, in_r, tmp);
    const int t = acc;
    acc = tmp;
    tmp = t;
  }
  int r = acc;
  if (do_final) r = rc_final_exp(e, L, acc, rns::N_CONSTS + 36, rns::N_CONSTS + 36 + 120, sh_n);
  rns::store(e, L, r, reinterpret_cast<Fq*>(out + g0), reinterpret_cast<Fq*>(out + g1), 12);
}

// tree products of the lines, block multipliers, Horner chain (+ final exp).
// lines: n Fq12 per (group, line).  Takes from `ar` one buffer per tree level
// and the block multipliers: plan::from_lines_bytes(groups, n).
static hipError_t pairing_from_lines(Arena& ar, hipStream_t s, Fq12* lines, size_t groups, size_t n, Fq12* d_out,
                                     bool final_exp) {
  const size_t G = groups * N_LINE_COEFFS;
  // tree levels in RNS form (the first from the field.h line products)
  const void* cur = lines;
  bool res = false;
  for (plan::Tree t = plan::line_tree(n); t.more(); t.step()) {
    const size_t nout = t.nout();
    uint32_t* nxt = ar.take<uint32_t>(plan::level_words(groups, nout));
    const unsigned wg = rns_grid((G * nout + 1) / 2);
    if (res)
      k_chunk_prod_rns<true, TREE_CHUNK><<<wg, 64 * RC_WAVES, 0, s>>>(cur, G, t.n, nout, nxt);
    else
      k_chunk_prod_rns<false, TREE_CHUNK><<<wg, 64 * RC_WAVES, 0, s>>>(cur, G, t.n, nout, nxt);
    TPST_TRY(hipGetLastError());
    cur = nxt;
    res = true;
  }
  uint32_t* MBr = ar.take<uint32_t>(plan::mbr_words(groups));
  const unsigned pairs = (unsigned)((groups + 1) / 2);
  if (res)
    k_miller_blocks_rns<true><<<pairs * NBLK, 64 * RC_WAVES, 0, s>>>(cur, groups, MBr);
  else
    k_miller_blocks_rns<false><<<pairs * NBLK, 64 * RC_WAVES, 0, s>>>(cur, groups, MBr);
  TPST_TRY(hipGetLastError());
  // (one instantiation: a second one -- e.g. an s_setprio variant -- made
  // rc_final_exp an out-of-line call with its lane tables behind a
  // reference, 0.5 -> 2.2 ms per chain)
  k_chain_final_rns<<<pairs, 64 * RC_WAVES, 0, s>>>(MBr, groups, d_out, final_exp ? 1 : 0);
  return hipGetLastError();
}

// takes: the lines, then pairing_from_lines (multi_pairing_scratch)
hipError_t multi_pairing_prepared(Arena& ar, hipStream_t s, const uint32_t* d_g1, const uint32_t* d_g2,
                                  const LineCoeff* d_coeffs, size_t groups, size_t n, Fq12* d_out, bool final_exp,
                                  size_t map_s, size_t rot_L) {
  if (!groups) return hipSuccess;
  const size_t G = groups * N_LINE_COEFFS;
  Fq12* lines = ar.take<Fq12>(plan::lines_count(groups, n));
  const size_t nout = plan::pair_products(n);
  if (n) {
    k_line_pair<PairMapStd><<<grid_for(G * nout, 64), 64, 0, s>>>(d_coeffs, groups * n, d_g1, rot_L ? 1 : 0, d_g2,
                                                                 groups, n, PairMapStd{n, map_s, rot_L}, nout, lines);
  } else {
    k_set_one<<<grid_for(G, 64), 64, 0, s>>>(lines, G);
  }
  TPST_TRY(hipGetLastError());
  return pairing_from_lines(ar, s, lines, groups, nout, d_out, final_exp);
}

// takes: the coefficients, the residue lines of the preparation, then
// multi_pairing_prepared (multi_pairing_reserve)
hipError_t multi_pairing(Arena& ar, hipStream_t s, const uint32_t* d_g1, const uint32_t* d_g2, size_t groups,
                         size_t n, Fq12* d_out) {
  const size_t np = groups * n;
  ar.reset();
  TPST_TRY(ar.reserve(multi_pairing_reserve(groups, n)));
  LineCoeff* coeffs = ar.take<LineCoeff>(np * N_LINE_COEFFS);
  uint32_t* prep = ar.take<uint32_t>(plan::prepare_words(np));
  TPST_TRY(g2_prepare_batch(s, d_g2, np, coeffs, prep));
  return multi_pairing_prepared(ar, s, d_g1, d_g2, coeffs, groups, n, d_out);
}

// ---- MIPP look-ahead (pst_open.hip tpst_poly_open) -------------------------
// The 8 pairing products of round-r vectors (a, h; len, s = len/2, s' = s/2)
// whose combination with round r's challenge gives round r+1's cross terms:
//   group  0 A0 (i, i+s')   1 A3 (i+s, i+s+s')   2 A1 (i, i+s+s')   3 A2 (i+s, i+s')
//          4 B0 (i+s', i)   5 B3 (i+s+s', i+s)   6 B1 (i+s', i+s)   7 B2 (i+s+s', i)
// (G1 index, G2 index) for i < s'.  E > 1: h is not prepared but an earlier
// round's h_prev is (row length E len), h_q = sum_j f_j h_prev[q + j len];
// each pair (p, q) becomes the E pairs (X[p + j len], h_prev[q + j len]) with
// X = the E fold sets f_j a (XYZZ).
__constant__ uint32_t LA_P[8] = {0, 2, 0, 2, 1, 3, 1, 3};  // G1 offset in units of s'
__constant__ uint32_t LA_Q[8] = {1, 3, 3, 1, 0, 2, 2, 0};  // G2 offset in units of s'

struct PairMapLA {
  size_t sp, len;
  __device__ void at(size_t g, size_t k, size_t& p, size_t& q) const {
    const size_t i = k % sp, j = k / sp;
    p = LA_P[g] * sp + i + j * len;
    q = LA_Q[g] * sp + i + j * len;
  }
};

// takes: the lines (one entry per pair), then pairing_from_lines
// (mipp_lookahead_scratch)
hipError_t mipp_lookahead(Arena& ar, hipStream_t s, const LineCoeff* d_coeffs, size_t ncol, const uint32_t* d_g2,
                          const uint32_t* d_g1, bool xyzz, size_t len, int E, Fq12* d_out8, bool final_exp) {
  const size_t sp = len / 4;
  if (!sp || E < 1 || E > 8 || (E & (E - 1)) || ncol < (size_t)E * len) return hipErrorInvalidValue;
  const size_t n = sp * (size_t)E;
  Fq12* lines = ar.take<Fq12>(plan::lines_count(8, n));
  const size_t G = 8 * N_LINE_COEFFS, nout = plan::pair_products(n);
  k_line_pair<PairMapLA><<<grid_for(G * nout, 64), 64, 0, s>>>(d_coeffs, ncol, d_g1, xyzz ? 1 : 0, d_g2, 8, n,
                                                              PairMapLA{sp, len}, nout, lines);
  TPST_TRY(hipGetLastError());
  return pairing_from_lines(ar, s, lines, 8, nout, d_out8, final_exp);
}

// ---- gathered Miller partials -> final exponentiation (row-sharded opening)
// out[g] = FE(prod_{w < W} parts[w G + g]): the ranks' unreduced Miller
// products of group g (look-ahead products, round 0's t_l / t_r) multiplied
// and final-exponentiated on the RNS engine, two groups per workgroup (the
// halves of every wave) -- W - 1 products + the chain of k_chain_final_rns
__global__ void __launch_bounds__(64 * RC_WAVES) k_prod_final_rns(const Fq12* __restrict__ parts, size_t W,
                                                                  size_t G, Fq12* __restrict__ out) {
  __shared__ uint32_t s_slots[RC_SLOTS * rns::SLOT];
  __shared__ uint32_t s_xch[RC_WAVES * rns::XCH];
  __shared__ Fq sh_n[2];
  const size_t g0 = 2 * (size_t)blockIdx.x, g1 = g0 + 1 < G ? g0 + 1 : g0;
  rns::load_consts((rns::lds_t*)s_slots);
  const rns::Lane L = rns::load_lane();
  const rns::Eng e{(rns::lds_t*)s_slots, (rns::lds_t*)s_xch + rns::wave_id() * rns::XCH, 0};
  __syncthreads();
  int acc = rns::N_CONSTS, in_r = acc + 12, tmp = acc + 24;
  rns::load(e, L, reinterpret_cast<const Fq*>(parts + g0), reinterpret_cast<const Fq*>(parts + g1), acc, 12);
  for (size_t w = 1; w < W; w++) {
    rns::load(e, L, reinterpret_cast<const Fq*>(parts + w * G + g0), reinterpret_cast<const Fq*>(parts + w * G + g1),
              in_r, 12);
    rns::stage<rns::OP_F12_MUL>(e, L, acc, in_r, tmp);
    const int t = acc;
    acc = tmp;
    tmp = t;
  }
  const int r = rc_final_exp(e, L, acc, rns::N_CONSTS + 36, rns::N_CONSTS + 36 + 120, sh_n);
  rns::store(e, L, r, reinterpret_cast<Fq*>(out + g0), reinterpret_cast<Fq*>(out + g1), 12);
}

hipError_t gt_prod_final(hipStream_t s, const Fq12* d_parts, size_t W, size_t G, Fq12* d_out) {
  if (!G) return hipSuccess;
  if (!W) return hipErrorInvalidValue;
  k_prod_final_rns<<<(unsigned)((G + 1) / 2), 64 * RC_WAVES, 0, s>>>(d_parts, W, G, d_out);
  return hipGetLastError();
}

__global__ void k_fq12_from_mont(const Fq12* __restrict__ in, uint32_t* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * 12) return;
  const Fq* c = reinterpret_cast<const Fq*>(in);
  store_f<Fq>(out + 12 * i, from_mont(c[i]));
}

hipError_t fq12_from_mont(hipStream_t s, const Fq12* d_in, uint32_t* d_out, size_t n) {
  if (!n) return hipSuccess;
  k_fq12_from_mont<<<grid_for(n * 12, 64), 64, 0, s>>>(d_in, d_out, n);
  return hipGetLastError();
}

}  // namespace tpst
