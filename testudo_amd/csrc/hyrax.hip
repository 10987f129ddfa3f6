// Hyrax evaluation proofs on gfx950: PolyEvalProof::{prove, verify,
// verify_plain} (dense_mlpoly.rs:473-575) over DotProductProofLog
// (nizk/mod.rs:32-180) and BulletReductionProof (nizk/bullet.rs), and the
// PoseidonTranscript<Fr> they run over (poseidon_transcript.rs).
//
//   bound            DensePolynomial::bound (dense_mlpoly.rs:379-387): LZ[i] =
//                    sum_j L[j] Z[j R + i], a column sum read coalesced across i;
//                    j is tiled over blocks, exact partial sums, a second pass
//                    adds them (no atomics: the value does not depend on the grid)
//   bullet rounds    the generators are never folded.  Round k keeps the fold
//                    weights w_k (w_{k+1}[2t] = w_k[t] u^-1, w_{k+1}[2t+1] =
//                    w_k[t] u), so G^(k)[i] = sum_t w_k[t] G[t n_k + i], and its
//                    L_k, R_k are ONE K1 launch (msm.h msm_batch) of two rows of
//                    n scalars over the generator set's resident window tables.
//                    Cx shares the first launch (three rows); g_hat is one more
//                    row with s = w_final.  c_L Q + blind_L H, the transcript,
//                    u^-1, blind_fin, z1, z2 and the point conversions are host
//                    work between launches.
//   verify           the s vector (bullet.rs:205-215) from a kernel, G_hat one
//                    K1 row, a_hat = fr_dot(a, s); the few-point combination and
//                    the final equation on the host.
#include <cstring>
#include <vector>

#include "../../include/tpst.h"
#include "ctx.h"
#include "device_util.h"
#include "fr_sponge.h"
#include "gens_state.h"
#include "point_codec.h"
#include "pst_kernels.h"
#include "pst_state.h"

using namespace tpst;

namespace {

constexpr int HB_BS = 256;  // bound: columns i per block
constexpr int HB_TJ = 64;   // bound: rows j per block (the partial-sum tile)

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

// ------------------------------------------------------------ kernels ----
// partial[jb][i] = sum_{j in tile jb} L[j] Z[j R + i].  L is Montgomery and Z
// canonical, so each Montgomery product is the canonical value of L[j] Z[.]:
// the partials (and their sum) are canonical.
__global__ void __launch_bounds__(HB_BS) k_bound_partial(const uint32_t* __restrict__ Z, const uint32_t* __restrict__ L,
                                                         size_t Lsize, size_t R, uint32_t* __restrict__ partial) {
  __shared__ Fr shL[HB_TJ];
  const size_t i = (size_t)blockIdx.x * HB_BS + threadIdx.x;
  const size_t j0 = (size_t)blockIdx.y * HB_TJ;
  const int nj = (int)(Lsize - j0 < (size_t)HB_TJ ? Lsize - j0 : (size_t)HB_TJ);
  if ((int)threadIdx.x < nj) shL[threadIdx.x] = ld_fr(L + 8 * (j0 + threadIdx.x));
  __syncthreads();
  if (i >= R) return;
  Fr acc = Fr::zero();
#pragma unroll 4
  for (int j = 0; j < nj; j++) acc = add(acc, mul(shL[j], ld_fr(Z + 8 * ((j0 + j) * R + i))));
  st_fr(partial + 8 * ((size_t)blockIdx.y * R + i), acc);
}

// x[i] = Montgomery(sum_jb partial[jb][i])
__global__ void __launch_bounds__(HB_BS) k_bound_sum(const uint32_t* __restrict__ partial, unsigned njb, size_t R,
                                                     uint32_t* __restrict__ x) {
  const size_t i = (size_t)blockIdx.x * HB_BS + threadIdx.x;
  if (i >= R) return;
  Fr acc = Fr::zero();
  for (unsigned b = 0; b < njb; b++) acc = add(acc, ld_fr(partial + 8 * ((size_t)b * R + i)));
  st_fr(x + 8 * i, to_mont(acc));
}

// both cross inner products of a round in one pass (bullet.rs:82-83):
// out[0] = <a_L, b_R>, out[1] = <a_R, b_L>, canonical; one block
__global__ void __launch_bounds__(256) k_cross(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                               size_t half, uint32_t* __restrict__ out) {
  __shared__ Fr sh[2][256];
  Fr cl = Fr::zero(), cr = Fr::zero();
  for (size_t i = threadIdx.x; i < half; i += 256) {
    cl = add(cl, mul(ld_fr(a + 8 * i), ld_fr(b + 8 * (half + i))));
    cr = add(cr, mul(ld_fr(a + 8 * (half + i)), ld_fr(b + 8 * i)));
  }
  sh[0][threadIdx.x] = cl;
  sh[1][threadIdx.x] = cr;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
      sh[0][threadIdx.x] = add(sh[0][threadIdx.x], sh[0][threadIdx.x + h]);
      sh[1][threadIdx.x] = add(sh[1][threadIdx.x], sh[1][threadIdx.x + h]);
    }
    __syncthreads();
  }
  if (threadIdx.x < 2) st_fr(out + 8 * threadIdx.x, from_mont(sh[threadIdx.x][0]));
}

struct FrPair {
  Fr u, ui;
};

// One round's end and the next one's scalars.  With fold != 0 the vectors of
// length 2 nk are folded by (u, u^-1) (bullet.rs:126-130) into a2 / b2 and the
// weights advance into w2 (2^(lgn - lgnk) entries); with fold == 0 (the first
// call) a' = a, b' = b, w' = w.  Then, over the n fixed generators
// (column j = t nk + p, t = j / nk, p = j % nk, h2 = nk / 2):
//   nk > 1:  rowL[j] = p >= h2 ? a'[p - h2] w'[t] : 0     L = <a'_L, G'_R>
//            rowR[j] = p <  h2 ? a'[p + h2] w'[t] : 0     R = <a'_R, G'_L>
//   nk == 1: rowL[j] = w'[j]                               g_hat
// all canonical.  row0 != nullptr (the first call): row0[j] = a[j], the
// scalars of Cx.
__global__ void __launch_bounds__(256) k_fold_rows(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                   const uint32_t* __restrict__ w, uint32_t* __restrict__ a2,
                                                   uint32_t* __restrict__ b2, uint32_t* __restrict__ w2, size_t n,
                                                   int lgnk, int fold, FrPair c, uint32_t* __restrict__ row0,
                                                   uint32_t* __restrict__ rowL, uint32_t* __restrict__ rowR) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const size_t nk = (size_t)1 << lgnk, t = j >> lgnk, p = j & (nk - 1);
  Fr wt;
  if (fold) {
    wt = mul(ld_fr(w + 8 * (t >> 1)), (t & 1) ? c.u : c.ui);
    if (p == 0) st_fr(w2 + 8 * t, wt);
    if (j < nk) {
      st_fr(a2 + 8 * j, add(mul(ld_fr(a + 8 * j), c.u), mul(ld_fr(a + 8 * (nk + j)), c.ui)));
      st_fr(b2 + 8 * j, add(mul(ld_fr(b + 8 * j), c.ui), mul(ld_fr(b + 8 * (nk + j)), c.u)));
    }
  } else {
    wt = ld_fr(w + 8 * t);
  }
  if (row0) st_fr(row0 + 8 * j, from_mont(ld_fr(a + 8 * j)));
  if (nk == 1) {
    st_fr(rowL + 8 * j, from_mont(wt));
    return;
  }
  const size_t h2 = nk >> 1, q = p ^ h2;
  const Fr aq = fold ? add(mul(ld_fr(a + 8 * q), c.u), mul(ld_fr(a + 8 * (nk + q)), c.ui)) : ld_fr(a + 8 * q);
  const Fr v = from_mont(mul(aq, wt));
  st_fr(rowL + 8 * j, p >= h2 ? v : Fr::zero());
  st_fr(rowR + 8 * j, p < h2 ? v : Fr::zero());
}

// verification_scalars' s (bullet.rs:205-215): s[i] = allinv prod_{bit j of i}
// usq[lg - 1 - j]; Montgomery (for a_hat) and canonical (the K1 row of G_hat)
__global__ void __launch_bounds__(256) k_verif_s(const uint32_t* __restrict__ usq, Fr allinv, int lg, size_t n,
                                                 uint32_t* __restrict__ s_mont, uint32_t* __restrict__ s_can) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fr v = allinv;
  for (int j = 0; j < lg; j++)
    if ((i >> j) & 1) v = mul(v, ld_fr(usq + 8 * (lg - 1 - j)));
  st_fr(s_mont + 8 * i, v);
  st_fr(s_can + 8 * i, from_mont(v));
}

// -------------------------------------------------------- host helpers ----
using host::HFq;
typedef Xyzz<HFq> HX;
typedef Affine<HFq> HA;

inline HX h_mul(const HA& P, const Fr& k_mont) {
  const Fr c = from_mont(k_mont);
  return scalar_mul(P, c.v, 253);
}
inline HX h_mul(const HX& P, const Fr& k_mont) {
  const Fr c = from_mont(k_mont);
  return scalar_mul_xyzz(P, c.v, 253);
}
inline HX h_dev(const Xyzz<Fq>& d) {  // a device XYZZ point (the same bits)
  HX x;
  static_assert(sizeof(HX) == sizeof(Xyzz<Fq>), "host and device XYZZ layouts differ");
  memcpy(&x, &d, sizeof x);
  return x;
}
inline void h_put(const HX& x, uint64_t* out) { host::aff_put(to_affine(x), out); }

inline int log2_pow2(size_t n) {  // -1 unless a power of two
  if (!n || (n & (n - 1))) return -1;
  int l = 0;
  while (((size_t)1 << l) < n) l++;
  return l;
}

// append_point (poseidon_transcript.rs:77-86): the Compress::Yes bytes as Vec<u8>
bool absorb_point(FrSponge& sp, const uint64_t* p) {
  uint8_t b[48];
  if (tpst_ser_g1(p, b) != TPST_OK) return false;
  sp.absorb_bytes(b, 48);
  return true;
}
inline void absorb_fr(FrSponge& sp, const Fr& m) { sp.absorb(&m, 1); }

int check_gens(tpst_ctx* ctx, const tpst_gens* g, const uint64_t* Q) {
  if (g->ctx != ctx) return fail(ctx, TPST_E_ARG, "generator set belongs to another context");
  if (!g->has_h) return fail(ctx, TPST_E_STATE, "generator set has no blinding base h");
  const int lg = log2_pow2(g->n);
  if (lg < 0 || lg > TPST_HYRAX_MAX_ROUNDS) return fail(ctx, TPST_E_ARG, "gens->n must be a power of two <= 2^16");
  for (int k = 0; k < 2; k++)
    if (!fq_ok(Q + 6 * k)) return fail(ctx, TPST_E_ARG, "Q coordinate >= p");
  return TPST_OK;
}

// the blinding base h of a generator set, back on the host
int fetch_h(tpst_ctx* ctx, const tpst_gens* g, HA& H) {
  Affine<Fq> hm;
  TPST_HIP(ctx, hipMemcpyAsync(&hm, g->d_h, 96, hipMemcpyDeviceToHost, ctx->stream));
  TPST_HIP(ctx, hipStreamSynchronize(ctx->stream));
  H = {HFq::from(hm.x), HFq::from(hm.y)};
  return TPST_OK;
}

// ------------------------------------------------------------- prover ----
// DotProductProofLog::prove (nizk/mod.rs:45-125) over device vectors: d_x and
// d_a are n Montgomery Fr, a_can the canonical a for the transcript.  The
// caller holds the context lock.
int dotprod_prove_locked(tpst_ctx* ctx, const tpst_gens* g, const uint64_t* Qc, const uint32_t* d_x, const Fr& blind_x,
                         const uint32_t* d_a, const uint64_t* a_can, const Fr& y, const Fr& blind_y,
                         const uint64_t* rnd, tpst_transcript_fr* tr, tpst_dotprod_proof* proof, uint64_t* Cx_out,
                         uint64_t* Cy_out) {
  hipStream_t s = ctx->stream;
  const size_t n = g->n;
  const int lg = log2_pow2(n);
  FrSponge sp;
  if (!sp.load(tr)) return fail(ctx, TPST_E_ARG, "bad transcript state");
  for (int k = 0; k < 3 + 4 * lg; k++)
    if (!fr_ok(rnd + 4 * k)) return fail(ctx, TPST_E_ARG, "rnd value >= r");
  const Fr d = fr_canon(rnd), r_delta = fr_canon(rnd + 4), r_beta = fr_canon(rnd + 8);
  const HA Q = host::aff_in<HFq>(Qc);
  HA H;
  if (int rc = fetch_h(ctx, g, H)) return rc;

  // every buffer before the first round
  DevBuf av[2], bv[2], wv[2], rows, dc, dpts, dfin;
  for (int k = 0; k < 2; k++) {
    TPST_HIP(ctx, av[k].alloc(n * 32));
    TPST_HIP(ctx, bv[k].alloc(n * 32));
    TPST_HIP(ctx, wv[k].alloc(n * 32));
  }
  TPST_HIP(ctx, rows.alloc(3 * n * 32));
  TPST_HIP(ctx, dc.alloc(64));
  TPST_HIP(ctx, dpts.alloc(3 * sizeof(Xyzz<Fq>)));
  TPST_HIP(ctx, dfin.alloc(64));
  TPST_HIP(ctx, hipMemcpyAsync(av[0].p, d_x, n * 32, hipMemcpyDeviceToDevice, s));
  TPST_HIP(ctx, hipMemcpyAsync(bv[0].p, d_a, n * 32, hipMemcpyDeviceToDevice, s));
  const Fr one = Fr::one();
  TPST_HIP(ctx, hipMemcpyAsync(wv[0].p, &one, 32, hipMemcpyHostToDevice, s));
  uint32_t* row0 = rows.u();
  uint32_t* rowL = rows.u() + 8 * n;
  uint32_t* rowR = rows.u() + 16 * n;
  const unsigned grid = grid_for(n, 256);
  Profiler& pf = ctx->prof;
  pf.begin(ST_HYRAX_ROUNDS, s);

  // Cx's scalars and round 0's rows (or g_hat's when n == 1): one K1 launch
  FrPair uu = {one, one};
  k_fold_rows<<<grid, 256, 0, s>>>(av[0].u(), bv[0].u(), wv[0].u(), nullptr, nullptr, nullptr, n, lg, 0, uu, row0, rowL,
                                   rowR);
  TPST_HIP(ctx, hipGetLastError());
  const size_t first_rows = lg ? 3 : 2;
  Xyzz<Fq> hp[3];
  uint64_t hc[8];
  if (lg) k_cross<<<1, 256, 0, s>>>(av[0].u(), bv[0].u(), n / 2, dc.u());
  TPST_HIP(ctx, hipGetLastError());
  TPST_HIP(ctx, msm_batch(ctx->arena, s, g->tables, row0, first_rows, n, 1, (Xyzz<Fq>*)dpts.p));
  TPST_HIP(ctx, hipMemcpyAsync(hp, dpts.p, first_rows * sizeof(Xyzz<Fq>), hipMemcpyDeviceToHost, s));
  if (lg) TPST_HIP(ctx, hipMemcpyAsync(hc, dc.p, 64, hipMemcpyDeviceToHost, s));
  TPST_HIP(ctx, hipStreamSynchronize(s));

  uint64_t Cx[12], Cy[12];
  h_put(add(h_dev(hp[0]), h_mul(H, blind_x)), Cx);    // commit_slice(x, blind_x), mod.rs:75
  h_put(add(h_mul(Q, y), h_mul(H, blind_y)), Cy);     // commit_scalar(y, blind_y), mod.rs:78
  if (!absorb_point(sp, Cx) || !absorb_point(sp, Cy)) return fail(ctx, TPST_E_HIP, "non-canonical commitment");
  for (size_t i = 0; i < n; i++) absorb_fr(sp, fr_canon(a_can + 4 * i));  // append_scalar_vector, mod.rs:80

  memset(proof, 0, sizeof *proof);
  proof->rounds = lg;
  Fr blind_fin = add(blind_x, blind_y);  // blind_Gamma, mod.rs:82
  int cur = 0;
  HX g_hat = h_dev(hp[1]);  // n == 1: the row after Cx's is g_hat's
  for (int k = 0; k < lg; k++) {
    const int lgnk = lg - k;  // the round's vectors have 2^lgnk entries
    if (k) {
      k_cross<<<1, 256, 0, s>>>(av[cur].u(), bv[cur].u(), (size_t)1 << (lgnk - 1), dc.u());
      TPST_HIP(ctx, hipGetLastError());
      TPST_HIP(ctx, msm_batch(ctx->arena, s, g->tables, rowL, 2, n, 1, (Xyzz<Fq>*)dpts.p + 1));
      TPST_HIP(ctx, hipMemcpyAsync(hp + 1, (Xyzz<Fq>*)dpts.p + 1, 2 * sizeof(Xyzz<Fq>), hipMemcpyDeviceToHost, s));
      TPST_HIP(ctx, hipMemcpyAsync(hc, dc.p, 64, hipMemcpyDeviceToHost, s));
      TPST_HIP(ctx, hipStreamSynchronize(s));
    }
    const Fr cL = fr_canon(hc), cR = fr_canon(hc + 4);
    const Fr bL = fr_canon(rnd + 4 * (3 + 2 * k)), bR = fr_canon(rnd + 4 * (4 + 2 * k));
    h_put(add(add(h_dev(hp[1]), h_mul(Q, cL)), h_mul(H, bL)), proof->L[k]);  // bullet.rs:93-102
    h_put(add(add(h_dev(hp[2]), h_mul(Q, cR)), h_mul(H, bR)), proof->R[k]);  // bullet.rs:109-118
    if (!absorb_point(sp, proof->L[k]) || !absorb_point(sp, proof->R[k]))
      return fail(ctx, TPST_E_HIP, "non-canonical round point");
    const Fr u = sp.squeeze1();
    if (is_zero(u)) return fail(ctx, TPST_E_STATE, "zero challenge (bullet.rs:124 unwrap)");
    const Fr ui = inv(u);
    blind_fin = add(blind_fin, add(mul(mul(u, u), bL), mul(mul(ui, ui), bR)));  // bullet.rs:132
    FrPair c = {u, ui};
    k_fold_rows<<<grid, 256, 0, s>>>(av[cur].u(), bv[cur].u(), wv[cur].u(), av[cur ^ 1].u(), bv[cur ^ 1].u(),
                                     wv[cur ^ 1].u(), n, lgnk - 1, 1, c, nullptr, rowL, rowR);
    TPST_HIP(ctx, hipGetLastError());
    cur ^= 1;
  }
  if (lg) {  // g_hat = MSM(G, w_final): one more K1 row
    Xyzz<Fq> gh;
    TPST_HIP(ctx, msm_batch(ctx->arena, s, g->tables, rowL, 1, n, 1, (Xyzz<Fq>*)dpts.p));
    TPST_HIP(ctx, hipMemcpyAsync(&gh, dpts.p, sizeof gh, hipMemcpyDeviceToHost, s));
    TPST_HIP(ctx, hipStreamSynchronize(s));
    g_hat = h_dev(gh);
  }
  Fr fin[2];
  TPST_HIP(ctx, hipMemcpyAsync(&fin[0], av[cur].p, 32, hipMemcpyDeviceToHost, s));
  TPST_HIP(ctx, hipMemcpyAsync(&fin[1], bv[cur].p, 32, hipMemcpyDeviceToHost, s));
  pf.end(ST_HYRAX_ROUNDS, s);
  TPST_HIP(ctx, hipStreamSynchronize(s));
  const Fr x_hat = fin[0], a_hat = fin[1];
  const Fr y_hat = mul(x_hat, a_hat);                                   // mod.rs:94
  h_put(add(h_mul(g_hat, d), h_mul(H, r_delta)), proof->delta);         // mod.rs:96-103
  h_put(add(h_mul(Q, d), h_mul(H, r_beta)), proof->beta);               // mod.rs:106
  if (!absorb_point(sp, proof->delta) || !absorb_point(sp, proof->beta))
    return fail(ctx, TPST_E_HIP, "non-canonical delta / beta");
  const Fr c = sp.squeeze1();
  fr_out(add(d, mul(c, y_hat)), proof->z1);                                           // mod.rs:111
  fr_out(add(mul(a_hat, add(mul(c, blind_fin), r_beta)), r_delta), proof->z2);        // mod.rs:112
  sp.store(tr);
  if (Cx_out) memcpy(Cx_out, Cx, 96);
  if (Cy_out) memcpy(Cy_out, Cy, 96);
  return TPST_OK;
}

// ----------------------------------------------------------- verifier ----
bool proof_elements_ok(const tpst_dotprod_proof* pr, int lg) {
  if (pr->rounds != lg) return false;
  if (!fr_ok(pr->z1) || !fr_ok(pr->z2)) return false;
  if (!point_valid<Fq>(pr->delta) || !point_valid<Fq>(pr->beta)) return false;
  for (int k = 0; k < lg; k++)
    if (!point_valid<Fq>(pr->L[k]) || !point_valid<Fq>(pr->R[k])) return false;
  return true;
}

// DotProductProofLog::verify (nizk/mod.rs:127-179); a_can = n canonical Fr.
// Cx, Cy and the proof's elements are already validated.  Lock held.
int dotprod_verify_locked(tpst_ctx* ctx, const tpst_gens* g, const uint64_t* Qc, const uint64_t* a_can,
                          const uint64_t* Cx, const uint64_t* Cy, tpst_transcript_fr* tr,
                          const tpst_dotprod_proof* pr) {
  hipStream_t s = ctx->stream;
  const size_t n = g->n;
  const int lg = log2_pow2(n);
  FrSponge sp;
  if (!sp.load(tr)) return fail(ctx, TPST_E_ARG, "bad transcript state");
  const HA Q = host::aff_in<HFq>(Qc);
  HA H;
  if (int rc = fetch_h(ctx, g, H)) return rc;
  DevBuf da, dam, dusq, dsm, dsc, dpt, dah;
  TPST_HIP(ctx, da.alloc(n * 32));
  TPST_HIP(ctx, dam.alloc(n * 32));
  TPST_HIP(ctx, dusq.alloc((lg ? lg : 1) * 32));
  TPST_HIP(ctx, dsm.alloc(n * 32));
  TPST_HIP(ctx, dsc.alloc(n * 32));
  TPST_HIP(ctx, dpt.alloc(sizeof(Xyzz<Fq>)));
  TPST_HIP(ctx, dah.alloc(32));
  TPST_HIP(ctx, hipMemcpyAsync(da.p, a_can, n * 32, hipMemcpyHostToDevice, s));
  TPST_HIP(ctx, fr_to_mont(s, da.u(), dam.u(), n));

  if (!absorb_point(sp, Cx) || !absorb_point(sp, Cy)) return fail(ctx, TPST_E_VERIFY, "non-canonical commitment");
  for (size_t i = 0; i < n; i++) absorb_fr(sp, fr_canon(a_can + 4 * i));
  // verification_scalars (bullet.rs:157-218)
  std::vector<Fr> u(lg), ui(lg), usq(lg ? lg : 1), uisq(lg);
  Fr all = Fr::one();
  for (int k = 0; k < lg; k++) {
    if (!absorb_point(sp, pr->L[k]) || !absorb_point(sp, pr->R[k]))
      return fail(ctx, TPST_E_VERIFY, "non-canonical round point");
    u[k] = sp.squeeze1();
    if (is_zero(u[k])) return fail(ctx, TPST_E_VERIFY, "zero challenge");
    all = mul(all, u[k]);
  }
  // the batch inverse of the challenges: one inversion, then a backward sweep
  Fr allinv = inv(all), run = allinv;
  {
    std::vector<Fr> pre(lg + 1, Fr::one());
    for (int k = 0; k < lg; k++) pre[k + 1] = mul(pre[k], u[k]);
    for (int k = lg - 1; k >= 0; k--) {
      ui[k] = mul(run, pre[k]);
      run = mul(run, u[k]);
    }
  }
  for (int k = 0; k < lg; k++) {
    usq[k] = mul(u[k], u[k]);
    uisq[k] = mul(ui[k], ui[k]);
  }
  TPST_HIP(ctx, hipMemcpyAsync(dusq.p, usq.data(), (lg ? lg : 1) * 32, hipMemcpyHostToDevice, s));
  k_verif_s<<<grid_for(n, 256), 256, 0, s>>>(dusq.u(), allinv, lg, n, dsm.u(), dsc.u());
  TPST_HIP(ctx, hipGetLastError());
  TPST_HIP(ctx, msm_batch(ctx->arena, s, g->tables, dsc.u(), 1, n, 1, (Xyzz<Fq>*)dpt.p));  // G_hat, bullet.rs:237
  TPST_HIP(ctx, fr_dot(s, dam.u(), dsm.u(), n, dah.u()));                                  // a_hat, bullet.rs:238
  Xyzz<Fq> gh;
  Fr a_hat;
  TPST_HIP(ctx, hipMemcpyAsync(&gh, dpt.p, sizeof gh, hipMemcpyDeviceToHost, s));
  TPST_HIP(ctx, hipMemcpyAsync(&a_hat, dah.p, 32, hipMemcpyDeviceToHost, s));
  // Gamma_hat = sum u_k^2 L_k + u_k^-2 R_k + Gamma (bullet.rs:240-257), while the device works
  HX Gam = add_affine(to_xyzz(host::aff_in<HFq>(Cx)), host::aff_in<HFq>(Cy));  // mod.rs:148
  for (int k = 0; k < lg; k++) {
    Gam = add(Gam, h_mul(host::aff_in<HFq>(pr->L[k]), usq[k]));
    Gam = add(Gam, h_mul(host::aff_in<HFq>(pr->R[k]), uisq[k]));
  }
  TPST_HIP(ctx, hipStreamSynchronize(s));
  if (!absorb_point(sp, pr->delta) || !absorb_point(sp, pr->beta))
    return fail(ctx, TPST_E_VERIFY, "non-canonical delta / beta");
  const Fr c = sp.squeeze1();
  sp.store(tr);
  const HA beta = host::aff_in<HFq>(pr->beta), delta = host::aff_in<HFq>(pr->delta);
  const Fr z1 = fr_canon(pr->z1), z2 = fr_canon(pr->z2);
  // (Gamma_hat c + beta) a_hat + delta == (g_hat + Q a_hat) z1 + h z2   (mod.rs:169-170)
  const HX lhs = add_affine(h_mul(add_affine(h_mul(Gam, c), beta), a_hat), delta);
  const HX rhs = add(h_mul(add(h_dev(gh), h_mul(Q, a_hat)), z1), h_mul(H, z2));
  if (!eq(lhs, rhs)) return fail(ctx, TPST_E_VERIFY, "dot-product proof: lhs != rhs");
  return TPST_OK;
}

// ------------------------------------------------- evaluation proofs ----
struct EvalTabs {
  DevBuf dr, Lt, Rt, partial, x;
  int lv = 0, rv = 0;
  size_t Ls = 0, Rs = 0;
};

// L, R (compute_factored_evals, dense_mlpoly.rs:256-264) by the chi-table
// kernel on the two halves of r, then LZ = bound(L) into t.x (Montgomery)
int eval_bound_locked(tpst_ctx* ctx, const uint32_t* d_Z, int ell, const uint64_t* r, EvalTabs& t) {
  hipStream_t s = ctx->stream;
  t.lv = ell / 2;
  t.rv = ell - t.lv;
  t.Ls = (size_t)1 << t.lv;
  t.Rs = (size_t)1 << t.rv;
  std::vector<Fr> rm(ell);
  for (int j = 0; j < ell; j++) rm[j] = fr_canon(r + 4 * j);
  const unsigned njb = grid_for(t.Ls, HB_TJ);
  TPST_HIP(ctx, t.dr.alloc((size_t)ell * 32));
  TPST_HIP(ctx, t.Lt.alloc(t.Ls * 32));
  TPST_HIP(ctx, t.Rt.alloc(t.Rs * 32));
  TPST_HIP(ctx, t.partial.alloc((size_t)njb * t.Rs * 32));
  TPST_HIP(ctx, t.x.alloc(t.Rs * 32));
  TPST_HIP(ctx, hipMemcpyAsync(t.dr.p, rm.data(), (size_t)ell * 32, hipMemcpyHostToDevice, s));
  Profiler& pf = ctx->prof;
  pf.begin(ST_HYRAX_EQ, s);
  TPST_HIP(ctx, chi_table(s, t.dr.u(), t.lv, t.Lt.u()));
  TPST_HIP(ctx, chi_table(s, t.dr.u() + 8 * t.lv, t.rv, t.Rt.u()));
  pf.end(ST_HYRAX_EQ, s);
  pf.begin(ST_HYRAX_BOUND, s);
  k_bound_partial<<<dim3(grid_for(t.Rs, HB_BS), njb), HB_BS, 0, s>>>(d_Z, t.Lt.u(), t.Ls, t.Rs, t.partial.u());
  k_bound_sum<<<grid_for(t.Rs, HB_BS), HB_BS, 0, s>>>(t.partial.u(), njb, t.Rs, t.x.u());
  pf.end(ST_HYRAX_BOUND, s);
  TPST_HIP(ctx, hipGetLastError());
  return TPST_OK;
}

int eval_args(tpst_ctx* ctx, const tpst_gens* g, const uint64_t* Q, int ell, const uint64_t* r) {
  if (ell < 1 || ell > 32) return fail(ctx, TPST_E_ARG, "ell out of range (1..32)");
  if (int rc = check_gens(ctx, g, Q)) return rc;
  if (g->n != (size_t)1 << (ell - ell / 2)) return fail(ctx, TPST_E_ARG, "gens->n != 2^(ell - ell/2)");
  for (int j = 0; j < ell; j++)
    if (!fr_ok(r + 4 * j)) return fail(ctx, TPST_E_ARG, "r_j >= r");
  return TPST_OK;
}

// PolyEvalProof::prove (dense_mlpoly.rs:482-534); d_Z canonical on the device
int eval_prove_locked(tpst_ctx* ctx, const tpst_gens* g, const uint64_t* Q, const uint32_t* d_Z, int ell,
                      const uint64_t* blinds, const uint64_t* r, const uint64_t* Zr, const uint64_t* blind_Zr,
                      const uint64_t* rnd, tpst_transcript_fr* tr, tpst_dotprod_proof* proof, uint64_t* C_Zr) {
  hipStream_t s = ctx->stream;
  EvalTabs t;
  if (int rc = eval_bound_locked(ctx, d_Z, ell, r, t)) return rc;
  // LZ_blind = <blinds, L> (dense_mlpoly.rs:520)
  Fr lz_blind = Fr::zero();
  DevBuf db, dbm, dv, dac;
  if (blinds) {
    TPST_HIP(ctx, db.alloc(t.Ls * 32));
    TPST_HIP(ctx, dbm.alloc(t.Ls * 32));
    TPST_HIP(ctx, dv.alloc(32));
    TPST_HIP(ctx, hipMemcpyAsync(db.p, blinds, t.Ls * 32, hipMemcpyHostToDevice, s));
    TPST_HIP(ctx, fr_to_mont(s, db.u(), dbm.u(), t.Ls));
    TPST_HIP(ctx, fr_dot(s, dbm.u(), t.Lt.u(), t.Ls, dv.u()));
    TPST_HIP(ctx, hipMemcpyAsync(&lz_blind, dv.p, 32, hipMemcpyDeviceToHost, s));
  }
  // R, canonical, for the transcript (append_scalar_vector)
  std::vector<uint64_t> a_can(t.Rs * 4);
  TPST_HIP(ctx, dac.alloc(t.Rs * 32));
  TPST_HIP(ctx, fr_from_mont(s, t.Rt.u(), dac.u(), t.Rs));
  TPST_HIP(ctx, hipMemcpyAsync(a_can.data(), dac.p, t.Rs * 32, hipMemcpyDeviceToHost, s));
  TPST_HIP(ctx, hipStreamSynchronize(s));
  const Fr zero = Fr::zero();
  return dotprod_prove_locked(ctx, g, Q, t.x.u(), lz_blind, t.Rt.u(), a_can.data(), fr_canon(Zr),
                              blind_Zr ? fr_canon(blind_Zr) : zero, rnd, tr, proof, nullptr, C_Zr);
}

}  // namespace

// ================================================== Fr transcript (host) ==
extern "C" void tpst_transcript_fr_init(tpst_transcript_fr* t) {
  if (t) memset(t, 0, sizeof *t);
}

extern "C" int tpst_transcript_fr_append_scalar(tpst_transcript_fr* t, const uint64_t* fr) {
  return tpst_transcript_fr_append_scalars(t, fr, 1);
}

// append_scalar_vector (poseidon_transcript.rs:88-96): one absorb per scalar
extern "C" int tpst_transcript_fr_append_scalars(tpst_transcript_fr* t, const uint64_t* fr, size_t n) {
  if (!t || (n && !fr)) return TPST_E_ARG;
  for (size_t i = 0; i < n; i++)
    if (!fr_ok(fr + 4 * i)) return TPST_E_ARG;
  FrSponge sp;
  if (!sp.load(t)) return TPST_E_ARG;
  for (size_t i = 0; i < n; i++) absorb_fr(sp, fr_canon(fr + 4 * i));
  sp.store(t);
  return TPST_OK;
}

extern "C" int tpst_transcript_fr_append_point(tpst_transcript_fr* t, const uint64_t* g1) {
  if (!t || !g1) return TPST_E_ARG;
  FrSponge sp;
  if (!sp.load(t) || !absorb_point(sp, g1)) return TPST_E_ARG;
  sp.store(t);
  return TPST_OK;
}

extern "C" int tpst_transcript_fr_append_bytes(tpst_transcript_fr* t, const uint8_t* b, size_t n) {
  if (!t || (n && !b)) return TPST_E_ARG;
  FrSponge sp;
  if (!sp.load(t)) return TPST_E_ARG;
  sp.absorb_bytes(b, n);
  sp.store(t);
  return TPST_OK;
}

extern "C" int tpst_transcript_fr_challenge(tpst_transcript_fr* t, uint64_t* out_fr) {
  if (!t || !out_fr) return TPST_E_ARG;
  FrSponge sp;
  if (!sp.load(t)) return TPST_E_ARG;
  fr_out(sp.squeeze1(), out_fr);
  sp.store(t);
  return TPST_OK;
}

// ====================================================== dot-product proof ==
extern "C" int tpst_dotprod_prove(tpst_ctx* ctx, const tpst_gens* g, const uint64_t* Q, const uint64_t* x,
                                  const uint64_t* blind_x, const uint64_t* a, const uint64_t* y,
                                  const uint64_t* blind_y, const uint64_t* rnd, tpst_transcript_fr* tr,
                                  tpst_dotprod_proof* proof, uint64_t* Cx, uint64_t* Cy) {
  if (!ctx || !g || !Q || !x || !blind_x || !a || !y || !blind_y || !rnd || !tr || !proof || !Cx || !Cy)
    return fail(ctx, TPST_E_ARG, "null argument");
  if (int rc = check_gens(ctx, g, Q)) return rc;
  const size_t n = g->n;
  for (size_t i = 0; i < n; i++)
    if (!fr_ok(x + 4 * i) || !fr_ok(a + 4 * i)) return fail(ctx, TPST_E_ARG, "vector entry >= r");
  if (!fr_ok(blind_x) || !fr_ok(y) || !fr_ok(blind_y)) return fail(ctx, TPST_E_ARG, "scalar >= r");
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DevBuf up, dx, da;
  TPST_HIP(ctx, up.alloc(2 * n * 32));
  TPST_HIP(ctx, dx.alloc(n * 32));
  TPST_HIP(ctx, da.alloc(n * 32));
  TPST_HIP(ctx, hipMemcpyAsync(up.p, x, n * 32, hipMemcpyHostToDevice, s));
  TPST_HIP(ctx, hipMemcpyAsync(up.u() + 8 * n, a, n * 32, hipMemcpyHostToDevice, s));
  TPST_HIP(ctx, fr_to_mont(s, up.u(), dx.u(), n));
  TPST_HIP(ctx, fr_to_mont(s, up.u() + 8 * n, da.u(), n));
  return dotprod_prove_locked(ctx, g, Q, dx.u(), fr_canon(blind_x), da.u(), a, fr_canon(y), fr_canon(blind_y), rnd, tr,
                              proof, Cx, Cy);
}

extern "C" int tpst_dotprod_verify(tpst_ctx* ctx, const tpst_gens* g, const uint64_t* Q, const uint64_t* a,
                                   const uint64_t* Cx, const uint64_t* Cy, tpst_transcript_fr* tr,
                                   const tpst_dotprod_proof* proof) {
  if (!ctx || !g || !Q || !a || !Cx || !Cy || !tr || !proof) return fail(ctx, TPST_E_ARG, "null argument");
  if (int rc = check_gens(ctx, g, Q)) return rc;
  for (size_t i = 0; i < g->n; i++)
    if (!fr_ok(a + 4 * i)) return fail(ctx, TPST_E_ARG, "vector entry >= r");
  // element checks before the transcript absorbs anything
  if (!proof_elements_ok(proof, log2_pow2(g->n)) || !point_valid<Fq>(Cx) || !point_valid<Fq>(Cy))
    return fail(ctx, TPST_E_VERIFY, "malformed proof element or commitment");
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  return dotprod_verify_locked(ctx, g, Q, a, Cx, Cy, tr, proof);
}

// ======================================================= evaluation proof ==
extern "C" int tpst_hyrax_eval_prove_dev(tpst_ctx* ctx, const tpst_gens* g, const uint64_t* Q, const void* d_Z, int ell,
                                         const uint64_t* blinds, const uint64_t* r, const uint64_t* Zr,
                                         const uint64_t* blind_Zr, const uint64_t* rnd, tpst_transcript_fr* tr,
                                         tpst_dotprod_proof* proof, uint64_t* C_Zr) {
  if (!ctx || !g || !Q || !d_Z || !r || !Zr || !rnd || !tr || !proof || !C_Zr)
    return fail(ctx, TPST_E_ARG, "null argument");
  if (int rc = eval_args(ctx, g, Q, ell, r)) return rc;
  if (!fr_ok(Zr) || (blind_Zr && !fr_ok(blind_Zr))) return fail(ctx, TPST_E_ARG, "scalar >= r");
  if (blinds)
    for (size_t i = 0; i < (size_t)1 << (ell / 2); i++)
      if (!fr_ok(blinds + 4 * i)) return fail(ctx, TPST_E_ARG, "blind >= r");
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  return eval_prove_locked(ctx, g, Q, (const uint32_t*)d_Z, ell, blinds, r, Zr, blind_Zr, rnd, tr, proof, C_Zr);
}

extern "C" int tpst_hyrax_eval_prove(tpst_ctx* ctx, const tpst_gens* g, const uint64_t* Q, const uint64_t* Z, int ell,
                                     const uint64_t* blinds, const uint64_t* r, const uint64_t* Zr,
                                     const uint64_t* blind_Zr, const uint64_t* rnd, tpst_transcript_fr* tr,
                                     tpst_dotprod_proof* proof, uint64_t* C_Zr) {
  if (!ctx || !g || !Q || !Z || !r || !Zr || !rnd || !tr || !proof || !C_Zr)
    return fail(ctx, TPST_E_ARG, "null argument");
  if (int rc = eval_args(ctx, g, Q, ell, r)) return rc;
  if (!fr_ok(Zr) || (blind_Zr && !fr_ok(blind_Zr))) return fail(ctx, TPST_E_ARG, "scalar >= r");
  const size_t N = (size_t)1 << ell;
  for (size_t i = 0; i < N; i++)
    if (!fr_ok(Z + 4 * i)) return fail(ctx, TPST_E_ARG, "evaluation >= r");
  if (blinds)
    for (size_t i = 0; i < (size_t)1 << (ell / 2); i++)
      if (!fr_ok(blinds + 4 * i)) return fail(ctx, TPST_E_ARG, "blind >= r");
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  DevBuf dZ;
  TPST_HIP(ctx, dZ.alloc(N * 32));
  TPST_HIP(ctx, hipMemcpyAsync(dZ.p, Z, N * 32, hipMemcpyHostToDevice, ctx->stream));
  return eval_prove_locked(ctx, g, Q, dZ.u(), ell, blinds, r, Zr, blind_Zr, rnd, tr, proof, C_Zr);
}

// PolyEvalProof::verify (dense_mlpoly.rs:536-560)
extern "C" int tpst_hyrax_eval_verify(tpst_ctx* ctx, const tpst_gens* g, const uint64_t* Q, int ell, const uint64_t* r,
                                      const uint64_t* C_Zr, const uint64_t* comm, tpst_transcript_fr* tr,
                                      const tpst_dotprod_proof* proof) {
  if (!ctx || !g || !Q || !r || !C_Zr || !comm || !tr || !proof) return fail(ctx, TPST_E_ARG, "null argument");
  if (int rc = eval_args(ctx, g, Q, ell, r)) return rc;
  const int lv = ell / 2, rv = ell - lv;
  const size_t Ls = (size_t)1 << lv, Rs = (size_t)1 << rv;
  // element checks before the transcript absorbs anything
  bool ok = proof_elements_ok(proof, rv) && point_valid<Fq>(C_Zr);
  if (ok)  // the host loop below POINT_CHECK_DEVICE_MIN rows, the device check from there
    if (int rc = g1_rows_valid(ctx, comm, Ls, &ok)) return rc;
  if (!ok) return fail(ctx, TPST_E_VERIFY, "malformed proof element or commitment");
  // L, R by the eq-table kernel; C_LZ = MSM(comm, L) by the variable-base MSM
  // (library calls: each takes the context lock itself)
  std::vector<uint64_t> Lc(Ls * 4), Rc(Rs * 4);
  uint64_t C_LZ[12];
  if (int rc = tpst_eq_evals(ctx, r, lv, Lc.data())) return rc;
  if (int rc = tpst_eq_evals(ctx, r + 4 * lv, rv, Rc.data())) return rc;
  if (int rc = tpst_g1_msm(ctx, comm, Ls, Lc.data(), Ls, C_LZ)) return rc;
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  return dotprod_verify_locked(ctx, g, Q, Rc.data(), C_LZ, C_Zr, tr, proof);
}

// PolyEvalProof::verify_plain (dense_mlpoly.rs:562-574): C_Zr = Zr Q (zero blind)
extern "C" int tpst_hyrax_eval_verify_plain(tpst_ctx* ctx, const tpst_gens* g, const uint64_t* Q, int ell,
                                            const uint64_t* r, const uint64_t* Zr, const uint64_t* comm,
                                            tpst_transcript_fr* tr, const tpst_dotprod_proof* proof) {
  if (!ctx || !g || !Q || !r || !Zr || !comm || !tr || !proof) return fail(ctx, TPST_E_ARG, "null argument");
  if (!fr_ok(Zr)) return fail(ctx, TPST_E_ARG, "Zr >= r");
  for (int k = 0; k < 2; k++)
    if (!fq_ok(Q + 6 * k)) return fail(ctx, TPST_E_ARG, "Q coordinate >= p");
  uint64_t C_Zr[12];
  h_put(h_mul(host::aff_in<HFq>(Q), fr_canon(Zr)), C_Zr);
  return tpst_hyrax_eval_verify(ctx, g, Q, ell, r, C_Zr, comm, tr, proof);
}

// DensePolynomial::evaluate (dense_mlpoly.rs:408-414): <bound(L), R>
extern "C" int tpst_dense_evaluate(tpst_ctx* ctx, const uint64_t* Z, int ell, const uint64_t* r, uint64_t* out_fr) {
  if (!ctx || !Z || !r || !out_fr) return fail(ctx, TPST_E_ARG, "null argument");
  if (ell < 1 || ell > 32) return fail(ctx, TPST_E_ARG, "ell out of range (1..32)");
  const size_t N = (size_t)1 << ell;
  for (int j = 0; j < ell; j++)
    if (!fr_ok(r + 4 * j)) return fail(ctx, TPST_E_ARG, "r_j >= r");
  for (size_t i = 0; i < N; i++)
    if (!fr_ok(Z + 4 * i)) return fail(ctx, TPST_E_ARG, "evaluation >= r");
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DevBuf dZ, dv;
  TPST_HIP(ctx, dZ.alloc(N * 32));
  TPST_HIP(ctx, dv.alloc(32));
  TPST_HIP(ctx, hipMemcpyAsync(dZ.p, Z, N * 32, hipMemcpyHostToDevice, s));
  EvalTabs t;
  if (int rc = eval_bound_locked(ctx, dZ.u(), ell, r, t)) return rc;
  TPST_HIP(ctx, fr_dot(s, t.x.u(), t.Rt.u(), t.Rs, dv.u()));
  Fr v;
  TPST_HIP(ctx, hipMemcpyAsync(&v, dv.p, 32, hipMemcpyDeviceToHost, s));
  TPST_HIP(ctx, hipStreamSynchronize(s));
  fr_out(v, out_fr);
  return TPST_OK;
}
