// State and small host helpers shared by the sqrt-PST translation units:
// pst_api.hip (SRS, Polynomial handle, commit, verifier, MultilinearPC),
// pst_open.hip (the opening) and the R1CS / Groth16 callers (r1cs.hip,
// groth16.hip).  Internal: nothing here is part of include/tpst.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <vector>

#include "../../include/tpst.h"
#include "ctx.h"
#include "field.h"
#include "host_curve.h"
#include "msm.h"

namespace tpst {

// ------------------------------------------------------ host Fr / Fq ------
inline Fr fr_canon(const uint64_t* c) {  // canonical -> Montgomery
  Fr a;
  memcpy(a.v, c, 32);
  return to_mont(a);
}
inline void fr_out(const Fr& a, uint64_t* c) {
  Fr r = from_mont(a);
  memcpy(c, r.v, 32);
}

// ---- proof-element validation (the reference's elements are typed arkworks
// values, validated when deserialized; here they arrive as raw limbs) ----
inline bool limbs_lt(const uint64_t* a, const uint32_t* mod32, int n64) {
  for (int i = n64 - 1; i >= 0; i--) {
    const uint64_t mi = (uint64_t)mod32[2 * i] | ((uint64_t)mod32[2 * i + 1] << 32);
    if (a[i] != mi) return a[i] < mi;
  }
  return false;
}
inline bool fq_ok(const uint64_t* a) { return limbs_lt(a, params::FQ_P, 6); }
inline bool fr_ok(const uint64_t* a) { return limbs_lt(a, params::FR_P, 4); }
inline bool gt_ok(const uint64_t* f) {  // the 12 Fq coefficients of a GT value
  for (int k = 0; k < 12; k++)
    if (!fq_ok(f + 6 * k)) return false;
  return true;
}

// y > -y on canonical limbs  <=>  2y > p
inline bool y_is_negative(const uint64_t* y) {
  // compare y with p - y
  uint64_t ny[6];
  unsigned __int128 br = 0;
  const uint32_t* p32 = params::FQ_P;
  for (int i = 0; i < 6; i++) {
    const uint64_t pi = (uint64_t)p32[2 * i] | ((uint64_t)p32[2 * i + 1] << 32);
    unsigned __int128 d = (unsigned __int128)pi - y[i] - (uint64_t)br;
    ny[i] = (uint64_t)d;
    br = (d >> 64) & 1;
  }
  for (int i = 5; i >= 0; i--)
    if (y[i] != ny[i]) return y[i] > ny[i];
  return false;
}

inline void g1_bytes(const uint64_t* p, uint8_t* b) {  // ark serialize Compress::No
  bool inf = true;
  for (int i = 0; i < 12; i++) inf &= p[i] == 0;
  memcpy(b, p, 96);
  if (inf)
    b[95] |= 0x40;
  else if (y_is_negative(p + 6))
    b[95] |= 0x80;
}

// device XYZZ points (field.h Montgomery limbs, the same bits as host::HFq)
// -> canonical affine on the host: the open's few-point outputs (a round's
// u_l / u_r, U, final_a, final_h) need one inversion each, ~15 us here
// against a ~0.1 ms single-point kernel on the round's critical stream
template <class F>
inline void xyzz_to_canonical_host(const uint8_t* raw, size_t n, uint64_t* out) {
  using H = typename host::HostOf<F>::T;
  constexpr size_t PT = sizeof(Xyzz<F>), NQ = host::HostOf<F>::NQ;
  static_assert(sizeof(Xyzz<H>) == PT, "host and device XYZZ layouts differ");
  for (size_t i = 0; i < n; i++) {
    Xyzz<H> x;
    memcpy(&x, raw + i * PT, PT);
    host::aff_put(to_affine(x), out + i * 12 * NQ);
  }
}

// base-x digits of a canonical Fr e (e < r < x^4): e = sum_j out[j] x^j, for
// the GT exponentiations by Frobenius splitting (pairing_wave.hip k_gt_pow_wave)
inline void base_x_digits(const uint64_t* e, uint64_t* out) {
  uint64_t q[4] = {e[0], e[1], e[2], e[3]};
  for (int t = 0; t < 4; t++) {
    unsigned __int128 rem = 0;
    for (int l = 3; l >= 0; l--) {
      const unsigned __int128 cur = (rem << 64) | q[l];
      q[l] = (uint64_t)(cur / params::BLS_X);
      rem = cur % params::BLS_X;
    }
    out[t] = (uint64_t)rem;
  }
}

// ---------------------------------------------------------------- state ----
struct DevBuf {  // owning device allocation
  void* p = nullptr;
  size_t bytes = 0;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(size_t b) {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = b;
    return b ? hipMalloc(&p, b) : hipSuccess;
  }
  uint32_t* u() const { return (uint32_t*)p; }
  // grow-only: keep the buffer when it is large enough
  hipError_t grow(size_t b) { return (p && bytes >= b) ? hipSuccess : alloc(b); }
};

// the opening's device buffers, kept across openings (grow-only): ~40
// hipMalloc / hipFree pairs per call cost the host ~0.4 ms
struct OpenBufs {
  DevBuf up, A, P, Y, chiC, ScA, ScB, ScC, ScD[2], xa, xb, xd, xh, xp, xl[2], LAo[2], Hb[3], Lb[3], gts, canA, canC,
      canD, pstA, pstB, Wall, Wiall, SqT[2], SqG[2], SqM, chis_own, tLoc, A1x, A1, tA1, Hbl[3], Lbl[3];
};

struct SrsState {
  int nv = 0;
  DevBuf g, h;                    // affine Montgomery
  std::vector<std::unique_ptr<DevBuf>> pg, ph, pg_pair, ph_pair;
  DevBuf gmask, hmask;
  BatchTables tables;             // K1 tables over powers_of_g[0]
  DevBuf hprep[2];                // G2Prepared of powers_of_h[odd], odd = 0/1
  DevBuf prep_scratch;            // residue lines of the RNS G2 preparation (g2_prepare_scratch)
  // fixed-base tables (fbt.h), built on first open
  DevBuf t_pg0;                   // powers_of_g[0]            (U = commit(q))
  DevBuf t_h[2];                  // powers_of_h[odd]           (MIPP h folds)
  DevBuf t_pgp, t_php;            // concatenated pg_pair / ph_pair levels (PST level proofs)
  DevBuf seg;                     // u32 level offsets into the concatenation
  std::vector<size_t> lvl_off;
  bool fbt_ready = false, t_h_ready[2] = {false, false};
  DevBuf t_A;                     // per-opening table over the row commitments
  size_t t_A_n = 0;
  // a rank's share of the SRS side for the row-sharded opening (every W-th
  // point of powers_of_h[odd] from `rank`, its prepared lines and table)
  struct Local {
    int W = 0, rank = -1;
    DevBuf H0, L0, tH;
  } local[2];
  // t_A prebuilt by tpst_poly_commit (beside its IPP) for exactly these
  // canonical row commitments; consumed by the next opening of them
  std::vector<uint64_t> t_A_key;
  std::vector<uint64_t> flat;     // canonical export
  OpenBufs ob;                    // the opening's device buffers (grow-only)
  ~SrsState() { batch_tables_free(tables); }
};

}  // namespace tpst

struct tpst_poly {
  tpst_ctx* ctx;
  int n, m_col, m_row, odd;
  tpst::DevBuf Zown;
  const uint32_t* d_Z = nullptr;  // canonical Fr
  // column slice (multi-GPU shard): only columns [col0,
  // col0 + ncols) of the strided view are resident, as an N x ncols block;
  // ncols == 0 means the whole polynomial
  size_t col0 = 0, ncols = 0;
  tpst::DevBuf q, chis;           // Montgomery
  bool has_q = false;
  // opening-only handle (row-sharded commit): q combined from
  // the ranks' shares, no evaluations resident; optionally c_u combined too
  bool q_only = false;
  bool has_u = false;
  uint64_t U[12] = {};
};

namespace tpst {

// ------------------------------------------- pst_api.hip, for the opening ---
SrsState* srs_of(tpst_ctx* ctx);  // the context's loaded SRS, or nullptr
int poly_dims(int n, int& m_col, int& m_row, int& odd);
int poly_get_q(tpst_ctx* ctx, tpst_poly* p, const uint64_t* point);
int poly_need_q_source(tpst_ctx* ctx, const tpst_poly* p);
int chi_b_table(tpst_ctx* ctx, int m_col, int m_row, const uint64_t* point, DevBuf& chis);
int ensure_pinned(tpst_ctx* ctx, size_t bytes);
int prep_scratch_for(tpst_ctx* ctx, SrsState* st, size_t n);
int srs_fbt(tpst_ctx* ctx, SrsState* st, int odd);

// ------------------------------------ pst_open.hip, for commit / verify / MLPC
// streams of the opening (created once per context) and a pool of events
int open_streams(tpst_ctx* ctx, size_t n_events, size_t pinned_bytes, bool comm = false);
// one PST open (k XYZZ level proofs) on the context stream with its own
// scratch; F = Fq, Fq2
template <class F>
int pst_open_fbt(tpst_ctx* ctx, SrsState* st, const uint32_t* table, int off, const uint32_t* d_evals, int k,
                 const uint32_t* d_pt, Xyzz<F>* d_out);

// ---------------------------------- pst_api.hip, for r1cs.hip / groth16.hip
int srs_nv(tpst_ctx* ctx);  // the number of variables of the loaded SRS, or -1
// the device copy of a whole polynomial's evaluations (canonical Fr, original
// order), or nullptr for a column shard
inline const uint32_t* poly_evals(const tpst_poly* p) { return p && !p->ncols ? p->d_Z : nullptr; }
// Valid::check of a canonical affine point, as the PST verifier runs it:
// canonical coordinates, on the curve, in the r-torsion subgroup (host_curve.h)
template <class F>
inline bool point_valid(const uint64_t* p) {
  return host::point_in_subgroup<F>(p);
}
// canonical coordinates and on the curve (infinity = all-zero is on it), no
// subgroup test: what the lincomb entry points ask of their points, as tpst_g1_msm
template <class F>
inline bool point_on_curve(const uint64_t* p) {
  using H = typename host::HostOf<F>::T;
  constexpr int NQ = host::HostOf<F>::NQ;
  bool all0 = true;
  for (int k = 0; k < 2 * NQ; k++) {
    if (!fq_ok(p + 6 * k)) return false;
    for (int i = 0; i < 6; i++) all0 = all0 && !p[6 * k + i];
  }
  if (all0) return true;
  const Affine<H> a = host::aff_in<H>(p);
  return eq(sqr(a.y), add(mul(sqr(a.x), a.x), CurveB<H>::b()));
}

}  // namespace tpst
