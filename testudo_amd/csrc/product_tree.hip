// SPARK grand products on gfx950: the memory-checking argument of
// product_tree.rs -- ProductCircuit, DotProductCircuit and
// ProductCircuitEvalProofBatched::{prove, verify} (product_tree.rs:255-476),
// driven by SumcheckInstanceProof::prove_cubic_batched (sumcheck.rs:220-385) --
// over PoseidonTranscript<Fr>.  The core of ProductLayerProof::prove
// (sparse_mlpoly.rs:1053-1236).
//
//   layers        every layer of every circuit lives in one device arena as
//                 Montgomery Fr, allocated before the first round.  A layer of
//                 an instance is ONE buffer: its left is the first half, its
//                 right the second; layer k + 1 [i] = layer k [i] * layer k
//                 [i + half], one elementwise launch per layer over all P
//                 instances.  The last step (one entry per instance) is
//                 ProductCircuit::evaluate.
//   batched round one launch, blockIdx.y = instance (P product instances, then at
//                 layer 0 the D dot-product instances with their own weight
//                 table): bind the previous challenge fused with this round's
//                 sums at t = 0, 2, 3, per-block partial triples; one block then
//                 sums them per instance and applies the layer's coefficients,
//                 so 3 Fr come back per round.  Exact field sums, no atomics:
//                 the value does not depend on the grid.
//   the shared eq eq(rand) is read by all P product instances.  Every instance
//                 reads the UNBOUND pair and binds it in registers; only
//                 instance 0 stores, into the other buffer of a ping-pong pair,
//                 so no block reads what another writes.  A, B (and a
//                 dot-product instance's weight) are bound in place: a lane
//                 writes only the indices it alone reads (i and i + h/2).
//   transcript    on the host between launches: per round one 96-byte copy
//                 down, 4 absorbs, 1 squeeze, 32 bytes up.
//
// The verifier is pure host Fr (fr_sponge.h): no context, no device.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/tpst.h"
#include "ctx.h"
#include "device_util.h"
#include "fr_sponge.h"
#include "product_tree.h"
#include "pst_kernels.h"
#include "r1cs_state.h"

using namespace tpst;

namespace {

constexpr int PT_BS = 256;  // 4 waves of 64
#ifndef TPST_PT_MAX_BLOCKS
#define TPST_PT_MAX_BLOCKS 256  // A/B builds: TPST_EXTRA_FLAGS=-DTPST_PT_MAX_BLOCKS=n
#endif
// blocks per instance of a round (grid-stride beyond): bounds the partials
constexpr unsigned PT_MAX_BLOCKS = TPST_PT_MAX_BLOCKS;
constexpr size_t PT_MAX_INSTANCES = TPST_PRODCIRCUIT_MAX_INSTANCES;

__device__ __forceinline__ Fr ld_fr(const uint32_t* p) {
  const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
  Fr r;
  r.v[0] = a.x, r.v[1] = a.y, r.v[2] = a.z, r.v[3] = a.w;
  r.v[4] = b.x, r.v[5] = b.y, r.v[6] = b.z, r.v[7] = b.w;
  return r;
}
__device__ __forceinline__ void st_fr(uint32_t* p, const Fr& v) {
  uint4* o = reinterpret_cast<uint4*>(p);
  o[0] = make_uint4(v.v[0], v.v[1], v.v[2], v.v[3]);
  o[1] = make_uint4(v.v[4], v.v[5], v.v[6], v.v[7]);
}

// sum over the 64 lanes of a wave, valid in lane 0
__device__ __forceinline__ Fr wave_sum(Fr a) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    Fr b;
#pragma unroll
    for (int k = 0; k < 8; k++) b.v[k] = __shfl_down(a.v[k], off, 64);
    a = add(a, b);
  }
  return a;
}

// sums of three values over a block of PT_BS threads, valid in thread 0
__device__ __forceinline__ void block_sum3(Fr (&a)[3], Fr (*sh)[PT_BS / 64]) {
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const Fr w = wave_sum(a[k]);
    if ((threadIdx.x & 63) == 0) sh[k][threadIdx.x >> 6] = w;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
      Fr t = sh[k][0];
      for (int w = 1; w < PT_BS / 64; w++) t = add(t, sh[k][w]);
      a[k] = t;
    }
  }
}

// ------------------------------------------------------------ kernels ----
// ProductCircuit::compute_layer (product_tree.rs:19-34) for all instances:
// cur = P buffers of 2 half entries, next = P buffers of half (half = 2^lg_half):
// next[p][i] = cur[p][i] * cur[p][i + half]; total = P half
__global__ void __launch_bounds__(PT_BS) k_pt_layer(const uint32_t* __restrict__ cur, int lg_half, size_t total,
                                                    uint32_t* __restrict__ next) {
  const size_t g = (size_t)blockIdx.x * PT_BS + threadIdx.x;
  if (g >= total) return;
  const size_t half = (size_t)1 << lg_half, p = g >> lg_half, i = g & (half - 1);
  const uint32_t* c = cur + 8 * ((p << (lg_half + 1)) + i);
  st_fr(next + 8 * g, mul(ld_fr(c), ld_fr(c + 8 * half)));
}

// DotProductCircuit::evaluate (product_tree.rs:87-91), blockIdx.y = circuit:
// partial[d][block] = (sum over the block's i of l r w, 0, 0)
__global__ void __launch_bounds__(PT_BS) k_pt_dotp(const uint32_t* __restrict__ l, const uint32_t* __restrict__ r,
                                                   const uint32_t* __restrict__ w, size_t n,
                                                   uint32_t* __restrict__ partial) {
  __shared__ Fr sh[3][PT_BS / 64];
  const size_t base = 8 * n * blockIdx.y;
  Fr a[3] = {Fr::zero(), Fr::zero(), Fr::zero()};
  for (size_t i = (size_t)blockIdx.x * PT_BS + threadIdx.x; i < n; i += (size_t)gridDim.x * PT_BS)
    a[0] = add(a[0], mul(mul(ld_fr(l + base + 8 * i), ld_fr(r + base + 8 * i)), ld_fr(w + base + 8 * i)));
  block_sum3(a, sh);
  if (threadIdx.x == 0)
    for (int k = 0; k < 3; k++) st_fr(partial + 8 * (3 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x) + k), a[k]);
}

// the tables of a layer's batched sum-check
struct PtTabs {
  uint32_t* lay;           // P buffers of 2 n: left | right
  uint32_t *dl, *dr, *dw;  // D tables of n each (layer 0 with dot products)
  size_t n;                // a table's length before the first round
  unsigned P;
};

// One round of prove_cubic_batched (sumcheck.rs:248-358) for every instance.
// r != nullptr: the tables have length 2 h; bind the previous challenge
// (X'[i] = X[i] + r (X[i + h] - X[i]), bound_poly_var_top) -- A, B and a
// dot-product instance's weight in place, the shared eq from eq_in into eq_out
// by instance 0 alone.  r == nullptr (the first round): the tables have length
// h.  Then the sums over i < h / 2 at t = 0, 2, 3 of A B C (h >= 2).
__global__ void __launch_bounds__(PT_BS) k_pt_round(PtTabs t, const uint32_t* eq_in, uint32_t* eq_out, size_t h,
                                                    const uint32_t* __restrict__ r, uint32_t* __restrict__ partial) {
  __shared__ Fr sh[3][PT_BS / 64];
  const unsigned y = blockIdx.y;
  const bool prod = y < t.P;
  const size_t d = prod ? 0 : y - t.P;
  uint32_t* A = prod ? t.lay + 16 * t.n * y : t.dl + 8 * t.n * d;
  uint32_t* B = prod ? A + 8 * t.n : t.dr + 8 * t.n * d;
  const uint32_t* Ci = prod ? eq_in : t.dw + 8 * t.n * d;
  uint32_t* Co = prod ? (y == 0 ? eq_out : nullptr) : t.dw + 8 * t.n * d;
  const size_t half = h >> 1;
  const bool bind = r != nullptr;
  const Fr rr = bind ? ld_fr(r) : Fr::zero();
  Fr s[3] = {Fr::zero(), Fr::zero(), Fr::zero()};
  for (size_t i = (size_t)blockIdx.x * PT_BS + threadIdx.x; i < half; i += (size_t)gridDim.x * PT_BS) {
    Fr lo[3], hi[3];
    if (bind) {
      {
        const Fr a0 = ld_fr(A + 8 * i), b0 = ld_fr(A + 8 * (i + h));
        const Fr a1 = ld_fr(A + 8 * (i + half)), b1 = ld_fr(A + 8 * (i + half + h));
        lo[0] = add(a0, mul(rr, sub(b0, a0)));
        hi[0] = add(a1, mul(rr, sub(b1, a1)));
        st_fr(A + 8 * i, lo[0]);
        st_fr(A + 8 * (i + half), hi[0]);
      }
      {
        const Fr a0 = ld_fr(B + 8 * i), b0 = ld_fr(B + 8 * (i + h));
        const Fr a1 = ld_fr(B + 8 * (i + half)), b1 = ld_fr(B + 8 * (i + half + h));
        lo[1] = add(a0, mul(rr, sub(b0, a0)));
        hi[1] = add(a1, mul(rr, sub(b1, a1)));
        st_fr(B + 8 * i, lo[1]);
        st_fr(B + 8 * (i + half), hi[1]);
      }
      {
        const Fr a0 = ld_fr(Ci + 8 * i), b0 = ld_fr(Ci + 8 * (i + h));
        const Fr a1 = ld_fr(Ci + 8 * (i + half)), b1 = ld_fr(Ci + 8 * (i + half + h));
        lo[2] = add(a0, mul(rr, sub(b0, a0)));
        hi[2] = add(a1, mul(rr, sub(b1, a1)));
        if (Co) {
          st_fr(Co + 8 * i, lo[2]);
          st_fr(Co + 8 * (i + half), hi[2]);
        }
      }
    } else {
      lo[0] = ld_fr(A + 8 * i), hi[0] = ld_fr(A + 8 * (i + half));
      lo[1] = ld_fr(B + 8 * i), hi[1] = ld_fr(B + 8 * (i + half));
      lo[2] = ld_fr(Ci + 8 * i), hi[2] = ld_fr(Ci + 8 * (i + half));
    }
    s[0] = add(s[0], mul(mul(lo[0], lo[1]), lo[2]));
    Fr p[3], q[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const Fr df = sub(hi[k], lo[k]);
      p[k] = add(hi[k], df);  // 2 hi - lo
      q[k] = add(p[k], df);   // 3 hi - 2 lo
    }
    s[1] = add(s[1], mul(mul(p[0], p[1]), p[2]));
    s[2] = add(s[2], mul(mul(q[0], q[1]), q[2]));
  }
  block_sum3(s, sh);
  if (threadIdx.x == 0)
    for (int k = 0; k < 3; k++) st_fr(partial + 8 * (3 * ((size_t)y * gridDim.x + blockIdx.x) + k), s[k]);
}

// one block: out[k] = sum_y coeff[y] sum_b partial[y][b][k] (canonical); coeff
// == nullptr: out[3 y + k] = sum_b partial[y][b][k], the plain per-instance sums
__global__ void __launch_bounds__(PT_BS) k_pt_reduce(const uint32_t* __restrict__ partial, unsigned nblk, unsigned ni,
                                                     const uint32_t* __restrict__ coeff, uint32_t* __restrict__ out) {
  __shared__ Fr sh[3][PT_BS / 64];
  Fr acc[3] = {Fr::zero(), Fr::zero(), Fr::zero()};
  for (unsigned y = 0; y < ni; y++) {
    Fr t[3] = {Fr::zero(), Fr::zero(), Fr::zero()};
    for (unsigned b = threadIdx.x; b < nblk; b += PT_BS)
#pragma unroll
      for (int k = 0; k < 3; k++) t[k] = add(t[k], ld_fr(partial + 8 * (3 * ((size_t)y * nblk + b) + k)));
    if (coeff) {
      if (threadIdx.x < nblk) {
        const Fr c = ld_fr(coeff + 8 * y);
#pragma unroll
        for (int k = 0; k < 3; k++) acc[k] = add(acc[k], mul(c, t[k]));
      }
    } else {
      block_sum3(t, sh);
      if (threadIdx.x == 0)
        for (int k = 0; k < 3; k++) st_fr(out + 8 * (3 * (size_t)y + k), from_mont(t[k]));
      __syncthreads();  // sh is reused by the next instance
    }
  }
  if (!coeff) return;
  block_sum3(acc, sh);
  if (threadIdx.x == 0)
    for (int k = 0; k < 3; k++) st_fr(out + 8 * k, from_mont(acc[k]));
}

// X[0], or with bind X[0] + r (X[1] - X[0]); canonical
__device__ __forceinline__ Fr final_claim(const uint32_t* X, bool bind, const Fr& rr) {
  const Fr a = ld_fr(X);
  return from_mont(bind ? add(a, mul(rr, sub(ld_fr(X + 8), a))) : a);
}

// the end of a layer's sum-check: bind the last challenge (tables of length 2;
// r == nullptr for a layer without rounds, tables of length 1) and gather the
// final claims, canonical: out = left[ni] | right[ni] | weight[ni - P]
__global__ void k_pt_finals(PtTabs t, unsigned ni, const uint32_t* __restrict__ r, uint32_t* __restrict__ out) {
  const unsigned y = blockIdx.x * blockDim.x + threadIdx.x;
  if (y >= ni) return;
  const bool prod = y < t.P;
  const size_t d = prod ? 0 : y - t.P;
  const uint32_t* A = prod ? t.lay + 16 * t.n * y : t.dl + 8 * t.n * d;
  const uint32_t* B = prod ? A + 8 * t.n : t.dr + 8 * t.n * d;
  const bool bind = r != nullptr;
  const Fr rr = bind ? ld_fr(r) : Fr::zero();
  st_fr(out + 8 * (size_t)y, final_claim(A, bind, rr));
  st_fr(out + 8 * ((size_t)ni + y), final_claim(B, bind, rr));
  if (!prod) st_fr(out + 8 * (2 * (size_t)ni + d), final_claim(t.dw + 8 * t.n * d, bind, rr));
}

// -------------------------------------------------------- proof layout ----
// the flat proof (include/tpst.h): offsets in Fr
struct Layout {
  size_t polys, left, right, dotp, total;
  Layout(int ell, size_t P, size_t D) {
    polys = 0;
    left = 4 * ((size_t)ell * (ell - 1) / 2);
    right = left + (size_t)ell * P;
    dotp = right + (size_t)ell * P;
    total = dotp + 3 * D;
  }
  static size_t poly_off(int layer) { return 4 * ((size_t)layer * (layer - 1) / 2); }  // layer proof i: i rounds
};

bool dims_ok(int ell, size_t P, size_t D) {
  return ell >= 1 && ell <= 30 && P >= 1 && (D & 1) == 0 && P <= PT_MAX_INSTANCES && D <= PT_MAX_INSTANCES - P;
}

}  // namespace

// ------------------------------------------------------------- prover ----
// ProductCircuitEvalProofBatched::prove (product_tree.rs:255-377) over device
// inputs (canonical Fr), in two steps (product_tree.h): build allocates the
// arena, builds every layer and returns the claims; rounds runs the layer
// proofs.  The caller holds the context lock.
namespace {
// pinned staging: sums down | challenge up | layer block up | finals and claims down
struct Pins {
  uint64_t (*hs)[4];
  Fr* rpin;
  Fr* laypin;
  uint64_t (*finpin)[4];
};
int pins_for(tpst_ctx* ctx, int ell, size_t P, size_t D, Pins& pn) {
  const size_t NI = P + D;
  const size_t pin_lay = 256, pin_fin = pin_lay + 32 * ((size_t)ell + NI), pin_end = pin_fin + 32 * (2 * NI + D + P + 3 * D);
  if (int rc = ensure_pinned(ctx, pin_end)) return rc;
  char* const pin = (char*)ctx->pinned;
  pn.hs = reinterpret_cast<uint64_t(*)[4]>(pin);
  pn.rpin = reinterpret_cast<Fr*>(pin + 128);
  pn.laypin = reinterpret_cast<Fr*>(pin + pin_lay);
  pn.finpin = reinterpret_cast<uint64_t(*)[4]>(pin + pin_fin);
  return TPST_OK;
}
}  // namespace

int tpst::ProdCircuitProver::build(tpst_ctx* ctx, int ell_, size_t P_, const uint32_t* d_polys, size_t D_,
                                   const uint32_t* d_left, const uint32_t* d_right, const uint32_t* d_weight,
                                   uint64_t* claims_prod, uint64_t* claims_dotp) {
  ell = ell_, P = P_, D = D_;
  hipStream_t s = ctx->stream;
  const size_t N = (size_t)1 << ell, nh = N >> 1, NI = P + D;
  // ---- the arena, in Fr: every layer (layer k: P buffers of 2^(ell - k), k =
  // ell the products themselves), the dot-product tables, the eq ping-pong
  // pair and its scratch, partials, and the small per-round / per-layer slots
  loff.assign(ell + 2, 0);
  size_t off = 0;
  for (int k = 0; k <= ell; k++) {
    loff[k] = off;
    off += P * (N >> k);
  }
  o_dot = off;
  off += 3 * D * nh;
  o_eq = off;
  off += 2 * nh;
  o_eqs = off;
  off += eq_table_scratch(ell - 1);
  o_part = off;
  off += 3 * NI * PT_MAX_BLOCKS;
  o_sums = off;  // 3: the round's combined sums; 3 D: the dot products' evaluations
  off += 3 + 3 * D;
  o_r = off;  // the round's challenge
  off += 1;
  o_lay = off;  // rand | coeffs of the layer
  off += (size_t)ell + NI;
  o_fin = off;  // left | right | weight final claims
  off += 2 * NI + D;
  TPST_HIP(ctx, arena.alloc(off * 32));
  uint32_t* const base = arena.u();
  const auto at = [&](size_t o) { return base + 8 * o; };
  Pins pn;
  if (int rc = pins_for(ctx, ell, P, D, pn)) return rc;
  uint64_t(*const finpin)[4] = pn.finpin;

  Profiler& pf = ctx->prof;
  // ---- layers: Montgomery copies of the inputs, then one pass per layer
  pf.begin(ST_PRODTREE_BUILD, s);
  TPST_HIP(ctx, fr_to_mont(s, d_polys, at(loff[0]), P * N));
  if (D) {
    TPST_HIP(ctx, fr_to_mont(s, d_left, at(o_dot), D * nh));
    TPST_HIP(ctx, fr_to_mont(s, d_right, at(o_dot + D * nh), D * nh));
    TPST_HIP(ctx, fr_to_mont(s, d_weight, at(o_dot + 2 * D * nh), D * nh));
  }
  for (int k = 0; k < ell; k++) {
    const size_t total = P * (N >> (k + 1));
    k_pt_layer<<<grid_for(total, PT_BS), PT_BS, 0, s>>>(at(loff[k]), ell - k - 1, total, at(loff[k + 1]));
    TPST_HIP(ctx, hipGetLastError());
  }
  if (D) {
    const unsigned nb = std::min<unsigned>(grid_for(nh, PT_BS), PT_MAX_BLOCKS);
    k_pt_dotp<<<dim3(nb, (unsigned)D), PT_BS, 0, s>>>(at(o_dot), at(o_dot + D * nh), at(o_dot + 2 * D * nh), nh,
                                                     at(o_part));
    TPST_HIP(ctx, hipGetLastError());
    k_pt_reduce<<<1, PT_BS, 0, s>>>(at(o_part), nb, (unsigned)D, nullptr, at(o_sums + 3));
    TPST_HIP(ctx, hipGetLastError());
  }
  pf.end(ST_PRODTREE_BUILD, s);
  // the claims: ProductCircuit::evaluate of every circuit, DotProductCircuit::evaluate
  uint64_t(*clpin)[4] = finpin + (2 * NI + D);
  TPST_HIP(ctx, fr_from_mont(s, at(loff[ell]), at(o_fin), P));
  TPST_HIP(ctx, hipMemcpyAsync(clpin, at(o_fin), P * 32, hipMemcpyDeviceToHost, s));
  if (D) TPST_HIP(ctx, hipMemcpyAsync(clpin + P, at(o_sums + 3), 3 * D * 32, hipMemcpyDeviceToHost, s));
  TPST_HIP(ctx, hipStreamSynchronize(s));
  claims.resize(P);
  cdot.resize(D);
  for (size_t p = 0; p < P; p++) {
    memcpy(claims_prod + 4 * p, clpin[p], 32);
    claims[p] = fr_canon(clpin[p]);
  }
  for (size_t d = 0; d < D; d++) {
    memcpy(claims_dotp + 4 * d, clpin[P + 3 * d], 32);
    cdot[d] = fr_canon(clpin[P + 3 * d]);
  }
  return TPST_OK;
}

int tpst::ProdCircuitProver::rounds(tpst_ctx* ctx, tpst_transcript_fr* tr, uint64_t* proof, uint64_t* rand_out) {
  hipStream_t s = ctx->stream;
  FrSponge sp;
  if (!sp.load(tr)) return fail(ctx, TPST_E_ARG, "bad transcript state");
  const Layout lay(ell, P, D);
  const size_t nh = (size_t)1 << (ell - 1);
  uint32_t* const base = arena.u();
  const auto at = [&](size_t o) { return base + 8 * o; };
  Pins pn;
  if (int rc = pins_for(ctx, ell, P, D, pn)) return rc;
  uint64_t(*const hs)[4] = pn.hs;
  Fr* const rpin = pn.rpin;
  Fr* const laypin = pn.laypin;
  uint64_t(*const finpin)[4] = pn.finpin;
  Profiler& pf = ctx->prof;

  // ---- layer proofs, from the top (product_tree.rs:270-368): layer proof i
  // runs over circuit layer ell - 1 - i, whose sides have 2^i entries
  pf.begin(ST_PRODTREE_ROUNDS, s);
  std::vector<Fr> rand, coeffs, rs;
  for (int i = 0; i < ell; i++) {
    const int layer_id = ell - 1 - i;
    const size_t n = (size_t)1 << i;
    const bool dot = layer_id == 0 && D;
    if (dot) claims.insert(claims.end(), cdot.begin(), cdot.end());
    const unsigned ni = (unsigned)claims.size();
    coeffs.resize(ni);
    Fr e = Fr::zero();
    for (unsigned k = 0; k < ni; k++) coeffs[k] = sp.squeeze1();  // challenge_scalar_vec
    for (unsigned k = 0; k < ni; k++) e = add(e, mul(claims[k], coeffs[k]));
    // rand | coeffs up in one copy, then eq(rand) (poly_C_par)
    for (int j = 0; j < i; j++) laypin[j] = rand[j];
    for (unsigned k = 0; k < ni; k++) laypin[i + k] = coeffs[k];
    TPST_HIP(ctx, hipMemcpyAsync(at(o_lay), laypin, ((size_t)i + ni) * 32, hipMemcpyHostToDevice, s));
    uint32_t* eq_cur = at(o_eq);
    uint32_t* eq_alt = at(o_eq + nh);
    TPST_HIP(ctx, eq_table(s, at(o_lay), i, at(o_eqs), eq_cur));
    const PtTabs tabs = {at(loff[layer_id]), at(o_dot), at(o_dot + D * nh), at(o_dot + 2 * D * nh), n, (unsigned)P};
    rs.resize(i);
    for (int j = 0; j < i; j++) {
      const size_t h = n >> j;  // the tables' length after binding the previous challenge
      const unsigned nb = std::min<unsigned>(grid_for(h / 2, PT_BS), PT_MAX_BLOCKS);
      const int st = layer_id == 0 && j < 2 ? (j ? ST_PRODTREE_ROUND1 : ST_PRODTREE_ROUND0) : -1;
      if (st >= 0) pf.begin(st, s);
      k_pt_round<<<dim3(nb, ni), PT_BS, 0, s>>>(tabs, eq_cur, eq_alt, h, j ? at(o_r) : nullptr, at(o_part));
      TPST_HIP(ctx, hipGetLastError());
      if (j) std::swap(eq_cur, eq_alt);
      k_pt_reduce<<<1, PT_BS, 0, s>>>(at(o_part), nb, ni, at(o_lay + i), at(o_sums));
      TPST_HIP(ctx, hipGetLastError());
      if (st >= 0) pf.end(st, s);
      TPST_HIP(ctx, hipMemcpyAsync(hs, at(o_sums), 96, hipMemcpyDeviceToHost, s));
      TPST_HIP(ctx, hipStreamSynchronize(s));
      // evaluations at 0, 1 (= e - eval(0)), 2, 3 (sumcheck.rs:320-330)
      Fr ev[4] = {fr_canon(hs[0]), Fr::zero(), fr_canon(hs[1]), fr_canon(hs[2])};
      ev[1] = sub(e, ev[0]);
      Fr cs[4];
      from_evals(ev, 4, cs);
      uint64_t* out = proof + 4 * (lay.polys + Layout::poly_off(i) + 4 * (size_t)j);
      for (int c = 0; c < 4; c++) {
        fr_out(cs[c], out + 4 * c);
        sp.absorb(&cs[c], 1);  // write_to_transcript: one absorb per coefficient
      }
      rs[j] = sp.squeeze1();
      e = uni_eval(cs, 4, rs[j]);
      *rpin = rs[j];
      TPST_HIP(ctx, hipMemcpyAsync(at(o_r), rpin, 32, hipMemcpyHostToDevice, s));
    }
    k_pt_finals<<<grid_for(ni, 64), 64, 0, s>>>(tabs, ni, i ? at(o_r) : nullptr, at(o_fin));
    TPST_HIP(ctx, hipGetLastError());
    const size_t nfin = 2 * (size_t)ni + (dot ? D : 0);
    TPST_HIP(ctx, hipMemcpyAsync(finpin, at(o_fin), nfin * 32, hipMemcpyDeviceToHost, s));
    TPST_HIP(ctx, hipStreamSynchronize(s));
    std::vector<Fr> cl(P), cr(P);
    for (size_t p = 0; p < P; p++) {
      memcpy(proof + 4 * (lay.left + (size_t)i * P + p), finpin[p], 32);
      memcpy(proof + 4 * (lay.right + (size_t)i * P + p), finpin[ni + p], 32);
      cl[p] = fr_canon(finpin[p]);
      cr[p] = fr_canon(finpin[ni + p]);
      sp.absorb(&cl[p], 1);
      sp.absorb(&cr[p], 1);
    }
    if (dot)
      for (size_t d = 0; d < D; d++) {
        const uint64_t* v[3] = {finpin[P + d], finpin[ni + P + d], finpin[2 * (size_t)ni + d]};
        for (int k = 0; k < 3; k++) {
          memcpy(proof + 4 * (lay.dotp + k * D + d), v[k], 32);
          const Fr f = fr_canon(v[k]);
          sp.absorb(&f, 1);
        }
      }
    const Fr r_layer = sp.squeeze1();
    claims.resize(P);
    for (size_t p = 0; p < P; p++) claims[p] = add(cl[p], mul(r_layer, sub(cr[p], cl[p])));
    rand.assign(1, r_layer);
    rand.insert(rand.end(), rs.begin(), rs.end());
  }
  pf.end(ST_PRODTREE_ROUNDS, s);
  for (int j = 0; j < ell; j++) fr_out(rand[j], rand_out + 4 * j);
  sp.store(tr);
  return TPST_OK;
}

namespace {

int prove_locked(tpst_ctx* ctx, int ell, size_t P, const uint32_t* d_polys, size_t D, const uint32_t* d_left,
                 const uint32_t* d_right, const uint32_t* d_weight, tpst_transcript_fr* tr, uint64_t* proof,
                 uint64_t* claims_prod, uint64_t* claims_dotp, uint64_t* rand_out) {
  FrSponge sp;
  if (!sp.load(tr)) return fail(ctx, TPST_E_ARG, "bad transcript state");
  ProdCircuitProver pv;
  if (int rc = pv.build(ctx, ell, P, d_polys, D, d_left, d_right, d_weight, claims_prod, claims_dotp)) return rc;
  return pv.rounds(ctx, tr, proof, rand_out);
}

int prove_args(tpst_ctx* ctx, int ell, size_t P, const void* polys, size_t D, const void* l, const void* r,
               const void* w, const void* tr, const void* proof, const void* claims_prod, const void* claims_dotp,
               const void* rand) {
  if (!ctx || !polys || !tr || !proof || !claims_prod || !rand || (D && (!l || !r || !w || !claims_dotp)))
    return fail(ctx, TPST_E_ARG, "null argument");
  if (!dims_ok(ell, P, D)) return fail(ctx, TPST_E_ARG, "prodcircuit: ell (1..30), P (>= 1) or D (even) out of range");
  return TPST_OK;
}

}  // namespace

extern "C" size_t tpst_prodcircuit_proof_len(int ell, size_t P, size_t D) {
  return dims_ok(ell, P, D) ? Layout(ell, P, D).total : 0;
}

extern "C" int tpst_prodcircuit_prove_dev(tpst_ctx* ctx, int ell, size_t P, const void* d_polys, size_t D,
                                          const void* d_left, const void* d_right, const void* d_weight,
                                          tpst_transcript_fr* tr, uint64_t* proof, uint64_t* claims_prod,
                                          uint64_t* claims_dotp, uint64_t* rand) {
  if (int rc = prove_args(ctx, ell, P, d_polys, D, d_left, d_right, d_weight, tr, proof, claims_prod, claims_dotp, rand))
    return rc;
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  return prove_locked(ctx, ell, P, (const uint32_t*)d_polys, D, (const uint32_t*)d_left, (const uint32_t*)d_right,
                      (const uint32_t*)d_weight, tr, proof, claims_prod, claims_dotp, rand);
}

extern "C" int tpst_prodcircuit_prove(tpst_ctx* ctx, int ell, size_t P, const uint64_t* polys, size_t D,
                                      const uint64_t* left, const uint64_t* right, const uint64_t* weight,
                                      tpst_transcript_fr* tr, uint64_t* proof, uint64_t* claims_prod,
                                      uint64_t* claims_dotp, uint64_t* rand) {
  if (int rc = prove_args(ctx, ell, P, polys, D, left, right, weight, tr, proof, claims_prod, claims_dotp, rand))
    return rc;
  const size_t N = (size_t)1 << ell, nh = N >> 1;
  const uint64_t* src[4] = {polys, left, right, weight};
  const size_t cnt[4] = {P * N, D * nh, D * nh, D * nh};
  for (int k = 0; k < 4; k++)
    for (size_t i = 0; i < cnt[k]; i++)
      if (!fr_ok(src[k] + 4 * i)) return fail(ctx, TPST_E_ARG, "prodcircuit: input value >= r");
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  DevBuf up;
  TPST_HIP(ctx, up.alloc((cnt[0] + 3 * cnt[1]) * 32));
  uint32_t* d[4];
  size_t o = 0;
  for (int k = 0; k < 4; k++) {
    d[k] = up.u() + 8 * o;
    if (cnt[k]) TPST_HIP(ctx, hipMemcpyAsync(d[k], src[k], cnt[k] * 32, hipMemcpyHostToDevice, ctx->stream));
    o += cnt[k];
  }
  return prove_locked(ctx, ell, P, d[0], D, d[1], d[2], d[3], tr, proof, claims_prod, claims_dotp, rand);
}

// ProductCircuitEvalProofBatched::verify (product_tree.rs:379-476) with
// SumcheckInstanceProof::verify (sumcheck.rs:29-63): host only
extern "C" int tpst_prodcircuit_verify(int ell, size_t P, size_t D, const uint64_t* claims_prod,
                                       const uint64_t* claims_dotp, const uint64_t* proof, tpst_transcript_fr* tr,
                                       uint64_t* claims_out, uint64_t* claims_dotp_out, uint64_t* rand_out) {
  if (!claims_prod || !proof || !tr || !claims_out || !rand_out || (D && (!claims_dotp || !claims_dotp_out)))
    return TPST_E_ARG;
  if (!dims_ok(ell, P, D)) return TPST_E_ARG;
  FrSponge sp;
  if (!sp.load(tr)) return TPST_E_ARG;
  const Layout lay(ell, P, D);
  // element checks before the transcript absorbs anything
  for (size_t k = 0; k < lay.total; k++)
    if (!fr_ok(proof + 4 * k)) return TPST_E_VERIFY;
  for (size_t k = 0; k < P; k++)
    if (!fr_ok(claims_prod + 4 * k)) return TPST_E_VERIFY;
  for (size_t k = 0; k < D; k++)
    if (!fr_ok(claims_dotp + 4 * k)) return TPST_E_VERIFY;
  const auto F = [&](size_t k) { return fr_canon(proof + 4 * k); };
  const Fr one = Fr::one();
  std::vector<Fr> claims(P), coeffs, rand, rs, cl(P), cr(P);
  for (size_t p = 0; p < P; p++) claims[p] = fr_canon(claims_prod + 4 * p);
  for (int i = 0; i < ell; i++) {  // layer proof i has i rounds
    const bool last = i == ell - 1;
    if (last)
      for (size_t d = 0; d < D; d++) claims.push_back(fr_canon(claims_dotp + 4 * d));
    const size_t ni = claims.size();
    coeffs.resize(ni);
    Fr e = Fr::zero();
    for (size_t k = 0; k < ni; k++) coeffs[k] = sp.squeeze1();
    for (size_t k = 0; k < ni; k++) e = add(e, mul(claims[k], coeffs[k]));
    rs.resize(i);
    for (int j = 0; j < i; j++) {  // SumcheckInstanceProof::verify
      Fr cs[4];
      Fr at01 = Fr::zero();  // G(0) + G(1) = 2 c_0 + c_1 + c_2 + c_3
      for (int c = 0; c < 4; c++) {
        cs[c] = F(lay.polys + Layout::poly_off(i) + 4 * (size_t)j + c);
        at01 = add(at01, cs[c]);
      }
      if (!eq(add(at01, cs[0]), e)) return TPST_E_VERIFY;
      for (int c = 0; c < 4; c++) sp.absorb(&cs[c], 1);  // write_to_transcript
      rs[j] = sp.squeeze1();
      e = uni_eval(cs, 4, rs[j]);
    }
    for (size_t p = 0; p < P; p++) {
      cl[p] = F(lay.left + (size_t)i * P + p);
      cr[p] = F(lay.right + (size_t)i * P + p);
      sp.absorb(&cl[p], 1);
      sp.absorb(&cr[p], 1);
    }
    Fr eqv = one;  // eq(rand, rand_prod), product_tree.rs:419-421
    for (int j = 0; j < i; j++)
      eqv = mul(eqv, add(mul(rand[j], rs[j]), mul(sub(one, rand[j]), sub(one, rs[j]))));
    Fr expected = Fr::zero();
    for (size_t p = 0; p < P; p++) expected = add(expected, mul(coeffs[p], mul(mul(cl[p], cr[p]), eqv)));
    if (last)
      for (size_t d = 0; d < D; d++) {
        const Fr l = F(lay.dotp + d), r = F(lay.dotp + D + d), w = F(lay.dotp + 2 * D + d);
        sp.absorb(&l, 1);
        sp.absorb(&r, 1);
        sp.absorb(&w, 1);
        expected = add(expected, mul(mul(mul(coeffs[P + d], l), r), w));
      }
    if (!eq(expected, e)) return TPST_E_VERIFY;
    const Fr r_layer = sp.squeeze1();
    claims.resize(P);
    for (size_t p = 0; p < P; p++) claims[p] = add(cl[p], mul(r_layer, sub(cr[p], cl[p])));
    if (last)
      for (size_t d = 0; d < D / 2; d++)
        for (int k = 0; k < 3; k++) {
          const Fr a = F(lay.dotp + k * D + 2 * d), b = F(lay.dotp + k * D + 2 * d + 1);
          fr_out(add(a, mul(r_layer, sub(b, a))), claims_dotp_out + 4 * (3 * d + k));
        }
    rand.assign(1, r_layer);
    rand.insert(rand.end(), rs.begin(), rs.end());
  }
  for (size_t p = 0; p < P; p++) fr_out(claims[p], claims_out + 4 * p);
  for (int j = 0; j < ell; j++) fr_out(rand[j], rand_out + 4 * j);
  sp.store(tr);
  return TPST_OK;
}
