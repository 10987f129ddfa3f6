// SPARK sparse-polynomial evaluation proofs on gfx950: R1CSEvalProof =
// SparseMatPolyEvalProof::{prove, verify} (r1csinstance.rs:336-386,
// sparse_mlpoly.rs:1441-1569), the opening of the computational commitment of
// tpst_r1cs_commit.  The assembly of the Hyrax openings (hyrax.hip) and the
// batched product circuits (product_tree.hip) around three data-parallel
// stages of its own:
//
//   k_deref       row_ops_val[m][i] = mem_rx[row_addr[m][i]] and the same for
//                 the columns (AddrTimestamps::deref): 6 N gathers from the two
//                 eq tables, written straight into comb_derefs (8 N canonical
//                 Fr, the last 2 N zero = DensePolynomial::merge's padding).
//   k_hash_ops /  Layers::build_hash_layer (sparse_mlpoly.rs:542-615) in the
//   k_hash_mem    layout the product prover reads (P x 2^ell contiguous).
//                 Addresses and timestamps are the decommitment's u32 arrays.
//                 A Montgomery product of one Montgomery and one canonical
//                 operand is their canonical product, so with r_hash and
//                 r_hash^2 in Montgomery form the canonical inputs give
//                 canonical outputs at 2 products per op: read = r_hash^2 ts +
//                 r_hash val + addr - gamma, write = read + r_hash^2.
//   k_seg_eval    the 21 + 2 evaluations of HashLayerProof::prove as segmented
//                 dot products against one shared eq table per group:
//                 blockIdx.y = segment, lanes stride over it, one exact partial
//                 per block, one block per segment sums them.  No atomics: the
//                 value does not depend on the grid.
//
// The transcript (PoseidonTranscript<Fr>), the n-to-1 reductions and the whole
// verifier but its three Hyrax openings are host work.
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/tpst.h"
#include "ctx.h"
#include "device_util.h"
#include "fr_sponge.h"
#include "point_codec.h"
#include "product_tree.h"
#include "pst_kernels.h"
#include "r1cs_state.h"
#include "sparse_eval_state.h"

using namespace tpst;

namespace {

constexpr int SE_BS = 256;                // 4 waves of 64
constexpr unsigned SE_MAX_BLOCKS = 256;   // blocks per segment of k_seg_eval (grid-stride beyond)
constexpr int BATCH = 3;                  // (A, B, C)
constexpr int N_SEG_OPS = 15, N_SEG_DEREFS = 6, N_SEG_MEM = 2;
constexpr int N_SEG = N_SEG_OPS + N_SEG_DEREFS + N_SEG_MEM;

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
__device__ __forceinline__ Fr fr_u32(uint32_t x) {  // the canonical small integer
  Fr r = Fr::zero();
  r.v[0] = x;
  return r;
}

// comb_derefs[side 3 N + j] = eq_side[addr_side[j]] (canonical), j < 3 N
__global__ void __launch_bounds__(SE_BS) k_deref(const uint32_t* __restrict__ addr_row,
                                                 const uint32_t* __restrict__ addr_col,
                                                 const uint32_t* __restrict__ eq_rx,
                                                 const uint32_t* __restrict__ eq_ry, size_t n3, size_t cells,
                                                 uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * SE_BS + threadIdx.x;
  if (i >= 2 * n3) return;
  const bool col = i >= n3;
  const size_t j = col ? i - n3 : i;
  const uint32_t a = (col ? addr_col : addr_row)[j];
  const Fr v = a < cells ? from_mont(ld_fr((col ? eq_ry : eq_rx) + 8 * (size_t)a)) : Fr::zero();
  st_fr(out + 8 * i, v);
}

// ch = r_hash (Montgomery) | r_hash^2 (Montgomery) | r_hash^2 (canonical) | gamma (canonical)
// out: row read (3 N) | row write | col read | col write, canonical
__global__ void __launch_bounds__(SE_BS) k_hash_ops(const uint32_t* __restrict__ addr_row,
                                                    const uint32_t* __restrict__ addr_col,
                                                    const uint32_t* __restrict__ rts_row,
                                                    const uint32_t* __restrict__ rts_col,
                                                    const uint32_t* __restrict__ derefs,
                                                    const uint32_t* __restrict__ ch, size_t n3,
                                                    uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * SE_BS + threadIdx.x;
  if (i >= n3) return;
  const Fr h = ld_fr(ch), h2 = ld_fr(ch + 8), h2c = ld_fr(ch + 16), gamma = ld_fr(ch + 24);
#pragma unroll
  for (int side = 0; side < 2; side++) {
    const uint32_t a = (side ? addr_col : addr_row)[i], ts = (side ? rts_col : rts_row)[i];
    const Fr val = ld_fr(derefs + 8 * ((size_t)side * n3 + i));
    const Fr read = sub(add(add(mul(h2, fr_u32(ts)), mul(h, val)), fr_u32(a)), gamma);
    st_fr(out + 8 * ((size_t)(2 * side) * n3 + i), read);
    st_fr(out + 8 * ((size_t)(2 * side + 1) * n3 + i), add(read, h2c));
  }
}

// ch = r_hash (canonical) | r_hash^2 (Montgomery) | gamma (canonical); eq tables Montgomery
// out: row init (cells) | row audit | col init | col audit, canonical
__global__ void __launch_bounds__(SE_BS) k_hash_mem(const uint32_t* __restrict__ eq_rx,
                                                    const uint32_t* __restrict__ eq_ry,
                                                    const uint32_t* __restrict__ audit_row,
                                                    const uint32_t* __restrict__ audit_col,
                                                    const uint32_t* __restrict__ ch, size_t cells,
                                                    uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * SE_BS + threadIdx.x;
  if (i >= cells) return;
  const Fr hc = ld_fr(ch), h2 = ld_fr(ch + 8), gamma = ld_fr(ch + 16);
#pragma unroll
  for (int side = 0; side < 2; side++) {
    const Fr e = ld_fr((side ? eq_ry : eq_rx) + 8 * i);
    const Fr init = sub(add(mul(hc, e), fr_u32((uint32_t)i)), gamma);
    st_fr(out + 8 * ((size_t)(2 * side) * cells + i), init);
    st_fr(out + 8 * ((size_t)(2 * side + 1) * cells + i),
          add(init, mul(h2, fr_u32((side ? audit_col : audit_row)[i]))));
  }
}

// sum over a block of SE_BS threads, valid in thread 0
__device__ __forceinline__ Fr block_sum(Fr a, Fr* sh) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    Fr b;
#pragma unroll
    for (int k = 0; k < 8; k++) b.v[k] = __shfl_down(a.v[k], off, 64);
    a = add(a, b);
  }
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
  __syncthreads();
  Fr t = sh[0];
  if (threadIdx.x == 0)
    for (int k = 1; k < SE_BS / 64; k++) t = add(t, sh[k]);
  return t;
}

// segment y < n0: base0 + y n, else base1 + (y - n0) n (canonical Fr); eq
// Montgomery: partial[y][block] = sum eq[i] seg[i], canonical
__global__ void __launch_bounds__(SE_BS) k_seg_eval(const uint32_t* __restrict__ base0, unsigned n0,
                                                    const uint32_t* __restrict__ base1,
                                                    const uint32_t* __restrict__ eq, size_t n,
                                                    uint32_t* __restrict__ partial) {
  __shared__ Fr sh[SE_BS / 64];
  const unsigned y = blockIdx.y;
  const uint32_t* __restrict__ seg = y < n0 ? base0 + 8 * (size_t)y * n : base1 + 8 * (size_t)(y - n0) * n;
  const size_t stride = (size_t)gridDim.x * SE_BS;
  Fr acc = Fr::zero();
  for (size_t i = (size_t)blockIdx.x * SE_BS + threadIdx.x; i < n; i += stride)
    acc = add(acc, mul(ld_fr(eq + 8 * i), ld_fr(seg + 8 * i)));
  const Fr t = block_sum(acc, sh);
  if (threadIdx.x == 0) st_fr(partial + 8 * ((size_t)y * gridDim.x + blockIdx.x), t);
}

// one block per segment: out[y] = sum of its nblk partials
__global__ void __launch_bounds__(SE_BS) k_seg_sum(const uint32_t* __restrict__ partial, unsigned nblk,
                                                   uint32_t* __restrict__ out) {
  __shared__ Fr sh[SE_BS / 64];
  Fr a = Fr::zero();
  for (unsigned b = threadIdx.x; b < nblk; b += SE_BS) a = add(a, ld_fr(partial + 8 * ((size_t)blockIdx.x * nblk + b)));
  const Fr t = block_sum(a, sh);
  if (threadIdx.x == 0) st_fr(out + 8 * (size_t)blockIdx.x, t);
}

// ------------------------------------------------------------ dimensions --
size_t next_pow2(size_t n) {
  size_t p = 1;
  while (p < n) p <<= 1;
  return p;
}

struct Dims {
  size_t N = 0, cells = 0;
  int vx = 0, vy = 0, vmax = 0, logN = 0;
  int ell[3] = {0, 0, 0};  // ops, mem, derefs
  size_t rows(int k) const { return (size_t)1 << (ell[k] / 2); }
  size_t cols(int k) const { return (size_t)1 << (ell[k] - ell[k] / 2); }
  int lg_cols(int k) const { return ell[k] - ell[k] / 2; }
};

// SparseMatPolyCommitmentGens::setup's sizes (sparse_mlpoly.rs:296-323), batch 3
bool dims_of(size_t num_cons, size_t num_vars, size_t nz, Dims& d) {
  if (!num_cons || !num_vars || !nz || nz > ((size_t)1 << 28)) return false;
  d.vx = log2_exact(num_cons);
  d.vy = log2_exact(2 * num_vars);
  if (d.vx < 0 || d.vy < 1 || d.vx > 30 || d.vy > 30) return false;
  d.vmax = std::max(d.vx, d.vy);
  d.N = next_pow2(nz);
  d.logN = log2_exact(d.N);
  if (d.logN < 1 || d.vmax < 1) return false;  // a product circuit has at least two inputs
  d.cells = (size_t)1 << d.vmax;
  d.ell[0] = d.logN + 4;  // (3 * 5).next_power_of_two() = 16
  d.ell[1] = d.vmax + 1;
  d.ell[2] = d.logN + 3;  // (3 * 2).next_power_of_two() = 8
  return d.lg_cols(0) <= TPST_HYRAX_MAX_ROUNDS && d.lg_cols(1) <= TPST_HYRAX_MAX_ROUNDS;
}

Dims dims_of(const tpst_r1cs_gens* g) {
  Dims d;
  dims_of(g->num_cons, g->num_vars, g->N, d);
  return d;
}

// --------------------------------------------------------- host helpers --
// the caller's transcript, worked on as a copy: stored back only on success
struct Tr {
  tpst_transcript_fr t;
  FrSponge sp;
  bool load() { return sp.load(&t); }
  void sync() { sp.store(&t); }    // before a library call that takes &t
  void resync() { sp.load(&t); }   // after it
  void scalar(const uint64_t* c) {
    const Fr f = fr_canon(c);
    sp.absorb(&f, 1);
  }
  void scalars(const uint64_t* c, size_t n) {
    for (size_t i = 0; i < n; i++) scalar(c + 4 * i);
  }
  bool point(const uint64_t* p) {
    uint8_t b[48];
    if (tpst_ser_g1(p, b) != TPST_OK) return false;
    sp.absorb_bytes(b, 48);
    return true;
  }
  Fr challenge() { return sp.squeeze1(); }
};

// the n-to-1 reduction of sparse_mlpoly.rs:107-121 / 778-789: append the n
// evaluations (canonical, n a power of two), draw log2(n) challenges, bind
// from the last (bound_poly_var_bot) -> challenges and the joint claim
Fr n_to_1(Tr& tr, const uint64_t* evals, size_t n, std::vector<Fr>& ch) {
  tr.scalars(evals, n);
  const int lg = log2_exact(n);
  ch.resize(lg);
  for (int k = 0; k < lg; k++) ch[k] = tr.challenge();
  std::vector<Fr> Z(n);
  for (size_t i = 0; i < n; i++) Z[i] = fr_canon(evals + 4 * i);
  for (int k = lg - 1; k >= 0; k--) {
    n >>= 1;
    for (size_t i = 0; i < n; i++) Z[i] = add(Z[2 * i], mul(sub(Z[2 * i + 1], Z[2 * i]), ch[k]));
  }
  return Z[0];
}

// SparseMatPolyEvalProof::equalize (sparse_mlpoly.rs:1452-1471): leading zeros
void equalize(const Dims& d, const uint64_t* rx, const uint64_t* ry, std::vector<Fr>& rxe, std::vector<Fr>& rye) {
  rxe.assign(d.vmax, Fr::zero());
  rye.assign(d.vmax, Fr::zero());
  for (int j = 0; j < d.vx; j++) rxe[d.vmax - d.vx + j] = fr_canon(rx + 4 * j);
  for (int j = 0; j < d.vy; j++) rye[d.vmax - d.vy + j] = fr_canon(ry + 4 * j);
}

bool frs_ok(const uint64_t* p, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!fr_ok(p + 4 * i)) return false;
  return true;
}

int check_handles(tpst_ctx* ctx, const tpst_r1cs_decomm* dc, const tpst_r1cs_gens* gn) {
  if (gn->owner != ctx) return fail(ctx, TPST_E_ARG, "generators belong to another context");
  if (dc) {
    if (dc->owner != ctx) return fail(ctx, TPST_E_ARG, "decommitment belongs to another context");
    if (dc->num_cons != gn->num_cons || dc->num_vars != gn->num_vars || dc->N != gn->N || dc->cells != gn->cells)
      return fail(ctx, TPST_E_ARG, "generators of another shape");
  }
  return TPST_OK;
}

// ---------------------------------------------------------- the stages ----
// every device buffer of the prover, allocated before the first launch
struct Bufs {
  DevBuf pt, eqx, eqy, eqs, derefs, hops, hmem, ch, seq, part, segout, comm;
};

int alloc_bufs(tpst_ctx* ctx, const Dims& d, Bufs& b) {
  const size_t big = std::max(d.N, d.cells);
  const int lgbig = std::max(d.logN, d.vmax);
  TPST_HIP(ctx, b.pt.alloc((size_t)2 * lgbig * 32 + 32));
  TPST_HIP(ctx, b.eqx.alloc(d.cells * 32));
  TPST_HIP(ctx, b.eqy.alloc(d.cells * 32));
  TPST_HIP(ctx, b.eqs.alloc((eq_table_scratch(lgbig) + 1) * 32));
  TPST_HIP(ctx, b.derefs.alloc(8 * d.N * 32));
  TPST_HIP(ctx, b.hops.alloc(12 * d.N * 32));
  TPST_HIP(ctx, b.hmem.alloc(4 * d.cells * 32));
  TPST_HIP(ctx, b.ch.alloc(8 * 32));
  TPST_HIP(ctx, b.seq.alloc(big * 32));
  TPST_HIP(ctx, b.part.alloc((size_t)N_SEG * SE_MAX_BLOCKS * 32));
  TPST_HIP(ctx, b.segout.alloc(N_SEG * 32));
  TPST_HIP(ctx, b.comm.alloc(d.rows(2) * 96));
  return TPST_OK;
}

// a. the eq tables of the equalized point, b. the dereference.  Lock held.
int stage_deref(tpst_ctx* ctx, const tpst_r1cs_decomm* dc, const Dims& d, const std::vector<Fr>& rxe,
                const std::vector<Fr>& rye, Bufs& b) {
  hipStream_t s = ctx->stream;
  std::vector<Fr> up(rxe);
  up.insert(up.end(), rye.begin(), rye.end());
  TPST_HIP(ctx, hipMemcpyAsync(b.pt.p, up.data(), up.size() * 32, hipMemcpyHostToDevice, s));
  TPST_HIP(ctx, hipStreamSynchronize(s));  // `up` is pageable and leaves scope
  TPST_HIP(ctx, eq_table(s, b.pt.u(), d.vmax, b.eqs.u(), b.eqx.u()));
  TPST_HIP(ctx, eq_table(s, b.pt.u() + 8 * (size_t)d.vmax, d.vmax, b.eqs.u(), b.eqy.u()));
  TPST_HIP(ctx, hipMemsetAsync(b.derefs.u() + 8 * 6 * d.N, 0, 2 * d.N * 32, s));
  Profiler& pf = ctx->prof;
  pf.begin(ST_SPARSE_DEREF, s);
  k_deref<<<grid_for(6 * d.N, SE_BS), SE_BS, 0, s>>>(dc->addr[0].u(), dc->addr[1].u(), b.eqx.u(), b.eqy.u(), 3 * d.N,
                                                     d.cells, b.derefs.u());
  pf.end(ST_SPARSE_DEREF, s);
  TPST_HIP(ctx, hipGetLastError());
  return TPST_OK;
}

// c. the hash layer at r_mem_check = (r_hash, gamma), Montgomery.  Lock held.
int stage_hash(tpst_ctx* ctx, const tpst_r1cs_decomm* dc, const Dims& d, const Fr& r_hash, const Fr& gamma, Bufs& b) {
  hipStream_t s = ctx->stream;
  const Fr h2 = mul(r_hash, r_hash);
  // ops: h (M) | h^2 (M) | h^2 (c) | gamma (c);  mem: h (c) | h^2 (M) | gamma (c)
  const Fr up[7] = {r_hash, h2, from_mont(h2), from_mont(gamma), from_mont(r_hash), h2, from_mont(gamma)};
  TPST_HIP(ctx, hipMemcpyAsync(b.ch.p, up, sizeof up, hipMemcpyHostToDevice, s));
  TPST_HIP(ctx, hipStreamSynchronize(s));
  Profiler& pf = ctx->prof;
  pf.begin(ST_SPARSE_HASH_OPS, s);
  k_hash_ops<<<grid_for(3 * d.N, SE_BS), SE_BS, 0, s>>>(dc->addr[0].u(), dc->addr[1].u(), dc->rts[0].u(),
                                                        dc->rts[1].u(), b.derefs.u(), b.ch.u(), 3 * d.N, b.hops.u());
  pf.end(ST_SPARSE_HASH_OPS, s);
  TPST_HIP(ctx, hipGetLastError());
  pf.begin(ST_SPARSE_HASH_MEM, s);
  k_hash_mem<<<grid_for(d.cells, SE_BS), SE_BS, 0, s>>>(b.eqx.u(), b.eqy.u(), dc->audit[0].u(), dc->audit[1].u(),
                                                        b.ch.u() + 8 * 4, d.cells, b.hmem.u());
  pf.end(ST_SPARSE_HASH_MEM, s);
  TPST_HIP(ctx, hipGetLastError());
  return TPST_OK;
}

// e. the 15 + 6 evaluations at rand_ops and the 2 at rand_mem (Montgomery
// points) -> out: N_SEG canonical Fr (ops segments, derefs segments, mem
// halves).  Lock held.
int stage_seg_eval(tpst_ctx* ctx, const tpst_r1cs_decomm* dc, const Dims& d, const std::vector<Fr>& rand_ops,
                   const std::vector<Fr>& rand_mem, Bufs& b, uint64_t* out) {
  hipStream_t s = ctx->stream;
  std::vector<Fr> up(rand_ops);
  up.insert(up.end(), rand_mem.begin(), rand_mem.end());
  TPST_HIP(ctx, hipMemcpyAsync(b.pt.p, up.data(), up.size() * 32, hipMemcpyHostToDevice, s));
  TPST_HIP(ctx, hipStreamSynchronize(s));
  Profiler& pf = ctx->prof;
  const unsigned nb_ops = std::min<unsigned>(grid_for(d.N, SE_BS), SE_MAX_BLOCKS);
  const unsigned nb_mem = std::min<unsigned>(grid_for(d.cells, SE_BS), SE_MAX_BLOCKS);
  constexpr int NO = N_SEG_OPS + N_SEG_DEREFS;
  TPST_HIP(ctx, eq_table(s, b.pt.u(), d.logN, b.eqs.u(), b.seq.u()));
  pf.begin(ST_SPARSE_SEG_EVAL, s);
  k_seg_eval<<<dim3(nb_ops, NO), SE_BS, 0, s>>>(dc->ops.u(), N_SEG_OPS, b.derefs.u(), b.seq.u(), d.N, b.part.u());
  k_seg_sum<<<NO, SE_BS, 0, s>>>(b.part.u(), nb_ops, b.segout.u());
  pf.end(ST_SPARSE_SEG_EVAL, s);
  TPST_HIP(ctx, hipGetLastError());
  TPST_HIP(ctx, eq_table(s, b.pt.u() + 8 * (size_t)d.logN, d.vmax, b.eqs.u(), b.seq.u()));
  uint32_t* const part_mem = b.part.u() + 8 * (size_t)NO * SE_MAX_BLOCKS;
  pf.begin(ST_SPARSE_SEG_EVAL, s);
  k_seg_eval<<<dim3(nb_mem, N_SEG_MEM), SE_BS, 0, s>>>(dc->mem.u(), N_SEG_MEM, dc->mem.u(), b.seq.u(), d.cells, part_mem);
  k_seg_sum<<<N_SEG_MEM, SE_BS, 0, s>>>(part_mem, nb_mem, b.segout.u() + 8 * NO);
  pf.end(ST_SPARSE_SEG_EVAL, s);
  TPST_HIP(ctx, hipGetLastError());
  TPST_HIP(ctx, hipMemcpyAsync(out, b.segout.p, N_SEG * 32, hipMemcpyDeviceToHost, s));
  TPST_HIP(ctx, hipStreamSynchronize(s));
  return TPST_OK;
}

bool dotprod_elements_ok(const tpst_dotprod_proof* pr, int lg) {
  if (pr->rounds != lg) return false;
  if (!fr_ok(pr->z1) || !fr_ok(pr->z2)) return false;
  if (!point_valid<Fq>(pr->delta) || !point_valid<Fq>(pr->beta)) return false;
  for (int k = 0; k < lg; k++)
    if (!point_valid<Fq>(pr->L[k]) || !point_valid<Fq>(pr->R[k])) return false;
  return true;
}

// ok = ok && every row commitment is valid: g1_rows_valid (point_codec.h) runs the host loop below
// POINT_CHECK_DEVICE_MIN rows and the device check from there
int points_ok(tpst_ctx* ctx, const uint64_t* p, size_t n, bool& ok) {
  if (!ok) return TPST_OK;
  return g1_rows_valid(ctx, p, n, &ok);
}

// hash(addr, val, ts) - gamma (sparse_mlpoly.rs:559), Montgomery
Fr hash_at(const Fr& h, const Fr& h2, const Fr& gamma, const Fr& addr, const Fr& val, const Fr& ts) {
  return sub(add(add(mul(h2, ts), mul(val, h)), addr), gamma);
}

}  // namespace

// ============================================================ generators ==
extern "C" int tpst_r1cs_gens_setup(tpst_ctx* ctx, const uint8_t* label, size_t label_len, size_t num_cons,
                                    size_t num_vars, size_t num_inputs, size_t num_nz_entries, tpst_r1cs_gens** out) {
  if (!ctx || !out || (label_len && !label)) return fail(ctx, TPST_E_ARG, "null argument");
  Dims d;
  if (num_inputs >= num_vars || !dims_of(num_cons, num_vars, num_nz_entries, d))
    return fail(ctx, TPST_E_ARG, "r1cs gens: dimensions must be powers of two, num_inputs < num_vars, >= 2 entries");
  std::unique_ptr<tpst_r1cs_gens> g(new tpst_r1cs_gens);
  g->owner = ctx;
  g->num_cons = num_cons, g->num_vars = num_vars, g->num_inputs = num_inputs, g->N = d.N, g->cells = d.cells;
  for (int k = 0; k < 3; k++) {
    g->ell[k] = d.ell[k];
    const size_t Rn = d.cols(k);
    std::vector<uint64_t> G((Rn + 1) * 12), h(12);
    if (int rc = tpst_gens_new(ctx, Rn + 1, label, label_len, G.data(), h.data(), nullptr)) return rc;
    if (int rc = tpst_gens_load(ctx, G.data(), Rn, h.data(), &g->g[k])) return rc;
    memcpy(g->Q[k], G.data() + 12 * Rn, 96);
  }
  *out = g.release();
  return TPST_OK;
}

extern "C" void tpst_r1cs_gens_free(tpst_r1cs_gens* g) { delete g; }
extern "C" void tpst_r1cs_decomm_free(tpst_r1cs_decomm* d) { delete d; }

extern "C" int tpst_r1cs_eval_proof_sizes(size_t num_cons, size_t num_vars, size_t num_nz_entries,
                                          tpst_r1cs_eval_sizes* out) {
  Dims d;
  if (!out || !dims_of(num_cons, num_vars, num_nz_entries, d)) return TPST_E_ARG;
  out->num_ops = d.N;
  out->num_mem_cells = d.cells;
  out->ell_ops = d.ell[0], out->ell_mem = d.ell[1], out->ell_derefs = d.ell[2];
  out->log_ops = d.logN, out->log_cells = d.vmax;
  out->ops_rows = d.rows(0), out->mem_rows = d.rows(1), out->derefs_rows = d.rows(2);
  out->prod_ops_len = tpst_prodcircuit_proof_len(d.logN, 4 * BATCH, 2 * BATCH);
  out->prod_mem_len = tpst_prodcircuit_proof_len(d.vmax, 4, 0);
  const int order[3] = {2, 0, 1};  // proving order: derefs, ops, mem
  for (int k = 0; k < 3; k++) out->rnd_len[k] = 3 + 4 * (size_t)d.lg_cols(order[k]);
  return TPST_OK;
}

// R1CSInstance::commit keeping the decommitment (r1csinstance.rs:313-333)
extern "C" int tpst_r1cs_commit_decomm(tpst_ctx* ctx, tpst_r1cs* R, const tpst_r1cs_gens* gn, uint64_t* comm_ops,
                                       size_t* ops_rows, uint64_t* comm_mem, size_t* mem_rows,
                                       tpst_r1cs_decomm** out) {
  if (!ctx || !R || !gn || !ops_rows || !mem_rows) return fail(ctx, TPST_E_ARG, "null argument");
  if (R->owner != ctx) return fail(ctx, TPST_E_ARG, "instance belongs to another context");
  if (int rc = check_handles(ctx, nullptr, gn)) return rc;
  size_t maxnz = 1;
  for (int m = 0; m < 3; m++) maxnz = std::max(maxnz, R->nnz[m]);
  if (R->num_cons != gn->num_cons || R->num_vars != gn->num_vars || R->num_inputs != gn->num_inputs ||
      next_pow2(maxnz) != gn->N)
    return fail(ctx, TPST_E_ARG, "generators of another shape");
  const Dims d = dims_of(gn);
  *ops_rows = d.rows(0);
  *mem_rows = d.rows(1);
  if (!comm_ops || !comm_mem) return TPST_OK;  // size query
  if (!out) return fail(ctx, TPST_E_ARG, "null argument");
  std::unique_ptr<tpst_r1cs_decomm> dc(new tpst_r1cs_decomm);
  if (int rc = r1cs_dense_rep(ctx, R, *dc)) return rc;
  const DevBuf* src[2] = {&dc->ops, &dc->mem};
  uint64_t* dst[2] = {comm_ops, comm_mem};
  for (int k = 0; k < 2; k++) {
    DevBuf dout;
    TPST_HIP(ctx, dout.alloc(d.rows(k) * 96));
    if (int rc = tpst_g1_msm_batch_dev(ctx, gn->g[k], src[k]->p, d.rows(k), d.cols(k), d.cols(k), 1, dout.p)) return rc;
    TPST_HIP(ctx, hipMemcpyAsync(dst[k], dout.p, d.rows(k) * 96, hipMemcpyDeviceToHost, ctx->stream));
    TPST_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  *out = dc.release();
  return TPST_OK;
}

// ================================================================ prover ==
// SparseMatPolyEvalProof::prove (sparse_mlpoly.rs:1473-1532)
extern "C" int tpst_r1cs_eval_prove(tpst_ctx* ctx, const tpst_r1cs_decomm* dc, const tpst_r1cs_gens* gn,
                                    const uint64_t* rx, const uint64_t* ry, const uint64_t* evals,
                                    const uint64_t* rnd_derefs, const uint64_t* rnd_ops, const uint64_t* rnd_mem,
                                    tpst_transcript_fr* tr_io, tpst_r1cs_eval_proof* proof, uint64_t* comm_derefs,
                                    uint64_t* prod_ops, uint64_t* prod_mem) {
  if (!ctx || !dc || !gn || !rx || !ry || !evals || !rnd_derefs || !rnd_ops || !rnd_mem || !tr_io || !proof ||
      !comm_derefs || !prod_ops || !prod_mem)
    return fail(ctx, TPST_E_ARG, "null argument");
  if (int rc = check_handles(ctx, dc, gn)) return rc;
  const Dims d = dims_of(gn);
  if (!frs_ok(rx, d.vx) || !frs_ok(ry, d.vy) || !frs_ok(evals, BATCH)) return fail(ctx, TPST_E_ARG, "value >= r");
  const uint64_t* rnd[3] = {rnd_derefs, rnd_ops, rnd_mem};
  const int order[3] = {2, 0, 1};  // proving order: derefs, ops, mem
  for (int k = 0; k < 3; k++)
    if (!frs_ok(rnd[k], 3 + 4 * (size_t)d.lg_cols(order[k]))) return fail(ctx, TPST_E_ARG, "draw >= r");
  Tr tr;
  tr.t = *tr_io;
  if (!tr.load()) return fail(ctx, TPST_E_ARG, "bad transcript state");
  const size_t N = d.N;
  std::vector<Fr> rxe, rye;
  equalize(d, rx, ry, rxe, rye);
  Bufs b;
  ProdCircuitProver pv_ops, pv_mem;
  tpst_r1cs_eval_proof pf;
  memset(&pf, 0, sizeof pf);
  const size_t Ld = d.rows(2), Rd = d.cols(2);
  std::vector<uint64_t> cd(Ld * 12), flat_ops(4 * tpst_prodcircuit_proof_len(d.logN, 12, 6)),
      flat_mem(4 * tpst_prodcircuit_proof_len(d.vmax, 4, 0));
  // ---- a, b: eq tables, dereference; Derefs::commit (the MSM takes the lock itself)
  {
    std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
    TPST_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = alloc_bufs(ctx, d, b)) return rc;
    if (int rc = stage_deref(ctx, dc, d, rxe, rye, b)) return rc;
  }
  if (int rc = tpst_g1_msm_batch_dev(ctx, gn->g[2], b.derefs.p, Ld, Rd, Rd, 1, b.comm.p)) return rc;
  std::vector<Fr> rand_ops, rand_mem;
  uint64_t seg[N_SEG][4];
  {
    std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
    TPST_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    TPST_HIP(ctx, hipMemcpyAsync(cd.data(), b.comm.p, Ld * 96, hipMemcpyDeviceToHost, s));
    TPST_HIP(ctx, hipStreamSynchronize(s));
    for (size_t i = 0; i < Ld; i++)
      if (!tr.point(cd.data() + 12 * i)) return fail(ctx, TPST_E_HIP, "derefs commitment is not a canonical point");
    const Fr r_hash = tr.challenge(), gamma = tr.challenge();  // r_mem_check
    // ---- c: hash layer; d: both circuit builds, the claims, then both proofs
    if (int rc = stage_hash(ctx, dc, d, r_hash, gamma, b)) return rc;
    uint64_t cp_ops[12][4], cdot[6][4], cp_mem[4][4];
    if (int rc = pv_ops.build(ctx, d.logN, 12, b.hops.u(), 6, b.derefs.u(), b.derefs.u() + 8 * 3 * N,
                              dc->ops.u() + 8 * 12 * N, &cp_ops[0][0], &cdot[0][0]))
      return rc;
    if (int rc = pv_mem.build(ctx, d.vmax, 4, b.hmem.u(), 0, nullptr, nullptr, nullptr, &cp_mem[0][0], nullptr)) return rc;
    for (int side = 0; side < 2; side++) {  // eval_row, eval_col = (init, read, write, audit)
      uint64_t(*e)[4] = side ? pf.prod_col : pf.prod_row;
      memcpy(e[0], cp_mem[2 * side], 32);
      memcpy(e[1], cp_ops[6 * side], 6 * 32);
      memcpy(e[7], cp_mem[2 * side + 1], 32);
      Fr ws = fr_canon(e[0]), rs = fr_canon(e[7]);
      for (int m = 0; m < BATCH; m++) {
        rs = mul(rs, fr_canon(e[1 + m]));
        ws = mul(ws, fr_canon(e[4 + m]));
      }
      if (!eq(ws, rs))
        return fail(ctx, TPST_E_ARG, side ? "eval prove: init * writes != reads * audit over the columns"
                                          : "eval prove: init * writes != reads * audit over the rows");
      tr.scalars(e[0], 8);
    }
    for (int m = 0; m < BATCH; m++) {
      memcpy(pf.prod_val[0][m], cdot[2 * m], 32);
      memcpy(pf.prod_val[1][m], cdot[2 * m + 1], 32);
      tr.scalar(cdot[2 * m]);
      tr.scalar(cdot[2 * m + 1]);
      if (!eq(add(fr_canon(cdot[2 * m]), fr_canon(cdot[2 * m + 1])), fr_canon(evals + 4 * m)))
        return fail(ctx, TPST_E_ARG, "eval prove: evals is not (A, B, C)(rx, ry)");
    }
    std::vector<uint64_t> ro(4 * (size_t)d.logN), rm(4 * (size_t)d.vmax);
    tr.sync();
    if (int rc = pv_ops.rounds(ctx, &tr.t, flat_ops.data(), ro.data())) return rc;
    if (int rc = pv_mem.rounds(ctx, &tr.t, flat_mem.data(), rm.data())) return rc;
    tr.resync();
    rand_ops.resize(d.logN);
    rand_mem.resize(d.vmax);
    for (int j = 0; j < d.logN; j++) rand_ops[j] = fr_canon(ro.data() + 4 * j);
    for (int j = 0; j < d.vmax; j++) rand_mem[j] = fr_canon(rm.data() + 4 * j);
    // ---- e: HashLayerProof::prove's evaluations
    if (int rc = stage_seg_eval(ctx, dc, d, rand_ops, rand_mem, b, &seg[0][0])) return rc;
  }
  uint64_t(*O)[4] = seg, (*D)[4] = seg + N_SEG_OPS, (*M)[4] = seg + N_SEG_OPS + N_SEG_DEREFS;
  memcpy(pf.hash_derefs, D, 6 * 32);
  memcpy(pf.hash_row, O[0], 6 * 32);
  memcpy(pf.hash_row[6], M[0], 32);
  memcpy(pf.hash_col, O[6], 6 * 32);
  memcpy(pf.hash_col[6], M[1], 32);
  memcpy(pf.hash_val, O[12], 3 * 32);
  // the three openings: n-to-1, append the joint claim, PolyEvalProof::prove
  struct Open {
    const uint64_t* evals;
    size_t n_evals, n_pad;
    const std::vector<Fr>* rand;
    const void* d_Z;
    int k;
    tpst_dotprod_proof* out;
  } opens[3] = {{D[0], 6, 8, &rand_ops, b.derefs.p, 2, &pf.proof_derefs},
                {O[0], 15, 16, &rand_ops, dc->ops.p, 0, &pf.proof_ops},
                {M[0], 2, 2, &rand_mem, dc->mem.p, 1, &pf.proof_mem}};
  for (int k = 0; k < 3; k++) {
    const Open& o = opens[k];
    std::vector<uint64_t> ev(4 * o.n_pad, 0);
    memcpy(ev.data(), o.evals, o.n_evals * 32);
    std::vector<Fr> ch;
    const Fr claim = n_to_1(tr, ev.data(), o.n_pad, ch);
    ch.insert(ch.end(), o.rand->begin(), o.rand->end());
    std::vector<uint64_t> rj(4 * ch.size());
    for (size_t j = 0; j < ch.size(); j++) fr_out(ch[j], rj.data() + 4 * j);
    uint64_t claim_c[4], C_Zr[12];
    fr_out(claim, claim_c);
    tr.scalar(claim_c);
    tr.sync();
    if (int rc = tpst_hyrax_eval_prove_dev(ctx, gn->g[o.k], gn->Q[o.k], o.d_Z, d.ell[o.k], nullptr, rj.data(), claim_c,
                                           nullptr, rnd[k], &tr.t, o.out, C_Zr))
      return rc;
    tr.resync();
  }
  tr.sync();
  *proof = pf;
  memcpy(comm_derefs, cd.data(), Ld * 96);
  memcpy(prod_ops, flat_ops.data(), flat_ops.size() * 8);
  memcpy(prod_mem, flat_mem.data(), flat_mem.size() * 8);
  *tr_io = tr.t;
  return TPST_OK;
}

// the stages alone (tests, tools): any output may be NULL.  derefs: 8 N Fr;
// hash_ops: 12 N (row read | row write | col read | col write, 3 N each);
// hash_mem: 4 cells (row init | row audit | col init | col audit); seg: the 15
// + 6 evaluations at rand_ops (log2 N Fr) and the 2 at rand_mem (log2 cells).
extern "C" int tpst_r1cs_eval_stages(tpst_ctx* ctx, const tpst_r1cs_decomm* dc, const uint64_t* rx,
                                     const uint64_t* ry, const uint64_t* r_mem_check, const uint64_t* rand_ops,
                                     const uint64_t* rand_mem, uint64_t* derefs, uint64_t* hash_ops,
                                     uint64_t* hash_mem, uint64_t* seg) {
  if (!ctx || !dc || !rx || !ry) return fail(ctx, TPST_E_ARG, "null argument");
  if (dc->owner != ctx) return fail(ctx, TPST_E_ARG, "decommitment belongs to another context");
  if ((hash_ops || hash_mem) && !r_mem_check) return fail(ctx, TPST_E_ARG, "null argument");
  if (seg && (!rand_ops || !rand_mem)) return fail(ctx, TPST_E_ARG, "null argument");
  Dims d;
  if (!dims_of(dc->num_cons, dc->num_vars, dc->N, d)) return fail(ctx, TPST_E_ARG, "bad dimensions");
  if (!frs_ok(rx, d.vx) || !frs_ok(ry, d.vy) || (r_mem_check && !frs_ok(r_mem_check, 2)) ||
      (seg && (!frs_ok(rand_ops, d.logN) || !frs_ok(rand_mem, d.vmax))))
    return fail(ctx, TPST_E_ARG, "value >= r");
  std::vector<Fr> rxe, rye;
  equalize(d, rx, ry, rxe, rye);
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  Bufs b;
  if (int rc = alloc_bufs(ctx, d, b)) return rc;
  if (int rc = stage_deref(ctx, dc, d, rxe, rye, b)) return rc;
  if (derefs) TPST_HIP(ctx, hipMemcpyAsync(derefs, b.derefs.p, 8 * d.N * 32, hipMemcpyDeviceToHost, s));
  if (hash_ops || hash_mem) {
    if (int rc = stage_hash(ctx, dc, d, fr_canon(r_mem_check), fr_canon(r_mem_check + 4), b)) return rc;
    if (hash_ops) TPST_HIP(ctx, hipMemcpyAsync(hash_ops, b.hops.p, 12 * d.N * 32, hipMemcpyDeviceToHost, s));
    if (hash_mem) TPST_HIP(ctx, hipMemcpyAsync(hash_mem, b.hmem.p, 4 * d.cells * 32, hipMemcpyDeviceToHost, s));
  }
  TPST_HIP(ctx, hipStreamSynchronize(s));
  if (seg) {
    std::vector<Fr> ro(d.logN), rm(d.vmax);
    for (int j = 0; j < d.logN; j++) ro[j] = fr_canon(rand_ops + 4 * j);
    for (int j = 0; j < d.vmax; j++) rm[j] = fr_canon(rand_mem + 4 * j);
    if (int rc = stage_seg_eval(ctx, dc, d, ro, rm, b, seg)) return rc;
  }
  return TPST_OK;
}

// ============================================================== verifier ==
// SparseMatPolyEvalProof::verify -> PolyEvalNetworkProof::verify ->
// ProductLayerProof::verify + HashLayerProof::verify (sparse_mlpoly.rs:
// 1534-1568, 1377-1438, 1238-1334, 896-1040)
extern "C" int tpst_r1cs_eval_verify(tpst_ctx* ctx, const uint64_t* comm_ops, const uint64_t* comm_mem,
                                     size_t num_ops, size_t num_mem_cells, const tpst_r1cs_gens* gn,
                                     const uint64_t* rx, const uint64_t* ry, const uint64_t* evals,
                                     tpst_transcript_fr* tr_io, const tpst_r1cs_eval_proof* pf,
                                     const uint64_t* comm_derefs, const uint64_t* prod_ops,
                                     const uint64_t* prod_mem) {
  if (!ctx || !comm_ops || !comm_mem || !gn || !rx || !ry || !evals || !tr_io || !pf || !comm_derefs || !prod_ops ||
      !prod_mem)
    return fail(ctx, TPST_E_ARG, "null argument");
  if (int rc = check_handles(ctx, nullptr, gn)) return rc;
  if (num_ops != gn->N || num_mem_cells != gn->cells)
    return fail(ctx, TPST_E_ARG, "commitment dimensions do not match the generators");
  const Dims d = dims_of(gn);
  Tr tr;
  tr.t = *tr_io;
  if (!tr.load()) return fail(ctx, TPST_E_ARG, "bad transcript state");
  const size_t len_ops = tpst_prodcircuit_proof_len(d.logN, 12, 6), len_mem = tpst_prodcircuit_proof_len(d.vmax, 4, 0);
  // ---- every element before the transcript absorbs anything
  const size_t n_fixed = offsetof(tpst_r1cs_eval_proof, proof_derefs) / 32;
  bool ok = frs_ok(rx, d.vx) && frs_ok(ry, d.vy) && frs_ok(evals, BATCH) &&
            frs_ok(reinterpret_cast<const uint64_t*>(pf), n_fixed) && frs_ok(prod_ops, len_ops) &&
            frs_ok(prod_mem, len_mem);
  ok = ok && dotprod_elements_ok(&pf->proof_derefs, d.lg_cols(2)) && dotprod_elements_ok(&pf->proof_ops, d.lg_cols(0)) &&
       dotprod_elements_ok(&pf->proof_mem, d.lg_cols(1));
  if (int rc = points_ok(ctx, comm_derefs, d.rows(2), ok)) return rc;
  if (int rc = points_ok(ctx, comm_ops, d.rows(0), ok)) return rc;
  if (int rc = points_ok(ctx, comm_mem, d.rows(1), ok)) return rc;
  if (!ok) return fail(ctx, TPST_E_VERIFY, "malformed proof element, commitment or argument");
  const auto bad = [&](const char* what) { return fail(ctx, TPST_E_VERIFY, what); };
  for (size_t i = 0; i < d.rows(2); i++) tr.point(comm_derefs + 12 * i);
  const Fr r_hash = tr.challenge(), gamma = tr.challenge();
  // ---- ProductLayerProof::verify
  for (int side = 0; side < 2; side++) {
    const uint64_t(*e)[4] = side ? pf->prod_col : pf->prod_row;
    Fr ws = fr_canon(e[0]), rs = fr_canon(e[7]);
    for (int m = 0; m < BATCH; m++) {
      rs = mul(rs, fr_canon(e[1 + m]));
      ws = mul(ws, fr_canon(e[4 + m]));
    }
    if (!eq(ws, rs)) return bad("subset check");
    tr.scalars(e[0], 8);
  }
  uint64_t claims_dotp[6][4], claims_prod[12][4], claims_mem_in[4][4];
  for (int m = 0; m < BATCH; m++) {
    const uint64_t *l = pf->prod_val[0][m], *r = pf->prod_val[1][m];
    if (!eq(add(fr_canon(l), fr_canon(r)), fr_canon(evals + 4 * m))) return bad("left + right != eval");
    tr.scalar(l);
    tr.scalar(r);
    memcpy(claims_dotp[2 * m], l, 32);
    memcpy(claims_dotp[2 * m + 1], r, 32);
  }
  memcpy(claims_prod[0], pf->prod_row[1], 6 * 32);
  memcpy(claims_prod[6], pf->prod_col[1], 6 * 32);
  memcpy(claims_mem_in[0], pf->prod_row[0], 32);
  memcpy(claims_mem_in[1], pf->prod_row[7], 32);
  memcpy(claims_mem_in[2], pf->prod_col[0], 32);
  memcpy(claims_mem_in[3], pf->prod_col[7], 32);
  uint64_t c_ops[12][4], c_dot[9][4], c_mem[4][4];
  std::vector<uint64_t> ro(4 * (size_t)d.logN), rm(4 * (size_t)d.vmax);
  tr.sync();
  if (int rc = tpst_prodcircuit_verify(d.logN, 12, 6, &claims_prod[0][0], &claims_dotp[0][0], prod_ops, &tr.t,
                                       &c_ops[0][0], &c_dot[0][0], ro.data()))
    return rc == TPST_E_VERIFY ? bad("ops product proof") : fail(ctx, rc, "ops product proof");
  if (int rc = tpst_prodcircuit_verify(d.vmax, 4, 0, &claims_mem_in[0][0], nullptr, prod_mem, &tr.t, &c_mem[0][0],
                                       nullptr, rm.data()))
    return rc == TPST_E_VERIFY ? bad("mem product proof") : fail(ctx, rc, "mem product proof");
  tr.resync();
  std::vector<Fr> rand_ops(d.logN), rand_mem(d.vmax);
  for (int j = 0; j < d.logN; j++) rand_ops[j] = fr_canon(ro.data() + 4 * j);
  for (int j = 0; j < d.vmax; j++) rand_mem[j] = fr_canon(rm.data() + 4 * j);
  // ---- HashLayerProof::verify: the three openings
  uint64_t ev_ops[16][4] = {};
  memcpy(ev_ops[0], pf->hash_row[0], 6 * 32);
  memcpy(ev_ops[6], pf->hash_col[0], 6 * 32);
  memcpy(ev_ops[12], pf->hash_val[0], 3 * 32);
  uint64_t ev_derefs[8][4] = {};
  memcpy(ev_derefs[0], pf->hash_derefs, 6 * 32);
  uint64_t ev_mem[2][4];
  memcpy(ev_mem[0], pf->hash_row[6], 32);
  memcpy(ev_mem[1], pf->hash_col[6], 32);
  struct Open {
    const uint64_t* evals;
    size_t n;
    const std::vector<Fr>* rand;
    const uint64_t* comm;
    int k;
    const tpst_dotprod_proof* pr;
  } opens[3] = {{&ev_derefs[0][0], 8, &rand_ops, comm_derefs, 2, &pf->proof_derefs},
                {&ev_ops[0][0], 16, &rand_ops, comm_ops, 0, &pf->proof_ops},
                {&ev_mem[0][0], 2, &rand_mem, comm_mem, 1, &pf->proof_mem}};
  for (int k = 0; k < 3; k++) {
    const Open& o = opens[k];
    std::vector<Fr> ch;
    const Fr claim = n_to_1(tr, o.evals, o.n, ch);
    ch.insert(ch.end(), o.rand->begin(), o.rand->end());
    std::vector<uint64_t> rj(4 * ch.size());
    for (size_t j = 0; j < ch.size(); j++) fr_out(ch[j], rj.data() + 4 * j);
    uint64_t claim_c[4];
    fr_out(claim, claim_c);
    tr.scalar(claim_c);
    tr.sync();
    if (int rc = tpst_hyrax_eval_verify_plain(ctx, gn->g[o.k], gn->Q[o.k], d.ell[o.k], rj.data(), claim_c, o.comm, &tr.t,
                                              o.pr))
      return rc;
    tr.resync();
    if (k == 0)  // the claims of the evaluation sum-check (sparse_mlpoly.rs:938-949)
      for (int m = 0; m < BATCH; m++)
        if (memcmp(c_dot[3 * m], pf->hash_derefs[0][m], 32) || memcmp(c_dot[3 * m + 1], pf->hash_derefs[1][m], 32) ||
            memcmp(c_dot[3 * m + 2], pf->hash_val[m], 32))
          return bad("dot-product claims");
  }
  // ---- verify_helper (sparse_mlpoly.rs:839-894), rows then columns
  std::vector<Fr> rxe, rye;
  equalize(d, rx, ry, rxe, rye);
  const Fr one = Fr::one(), h2 = mul(r_hash, r_hash);
  Fr ident = Fr::zero(), pw = one;  // IdentityPolynomial::evaluate: sum 2^(len - i - 1) r[i]
  for (int i = d.vmax - 1; i >= 0; i--) {
    ident = add(ident, mul(pw, rand_mem[i]));
    pw = add(pw, pw);
  }
  for (int side = 0; side < 2; side++) {
    const std::vector<Fr>& r = side ? rye : rxe;
    Fr eqv = one;  // EqPolynomial::evaluate
    for (int j = 0; j < d.vmax; j++) eqv = mul(eqv, add(mul(r[j], rand_mem[j]), mul(sub(one, r[j]), sub(one, rand_mem[j]))));
    const uint64_t(*hv)[4] = side ? pf->hash_col : pf->hash_row;
    if (!eq(hash_at(r_hash, h2, gamma, ident, eqv, Fr::zero()), fr_canon(c_mem[2 * side]))) return bad("init claim");
    for (int m = 0; m < BATCH; m++) {
      const Fr addr = fr_canon(hv[m]), ts = fr_canon(hv[3 + m]), val = fr_canon(pf->hash_derefs[side][m]);
      if (!eq(hash_at(r_hash, h2, gamma, addr, val, ts), fr_canon(c_ops[6 * side + m]))) return bad("read claim");
      if (!eq(hash_at(r_hash, h2, gamma, addr, val, add(ts, one)), fr_canon(c_ops[6 * side + 3 + m])))
        return bad("write claim");
    }
    if (!eq(hash_at(r_hash, h2, gamma, ident, eqv, fr_canon(hv[6])), fr_canon(c_mem[2 * side + 1])))
      return bad("audit claim");
  }
  tr.sync();
  *tr_io = tr.t;
  return TPST_OK;
}
