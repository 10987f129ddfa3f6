// sqrt-PST protocol layer of libtpst (include/tpst.h): SRS (MultilinearPC
// keys), the Polynomial handle and its commit (sqrt_pst.rs:14-265), the
// verifier (mipp.rs:182-320), the MultilinearPC calls and the Poseidon
// transcript (poseidon_transcript.rs).  The opening (Polynomial::open with
// the MIPP prover) is pst_open.hip; the state both share is pst_state.h.
//
// Everything heavy runs on the device (K1 row MSMs, K2 MSMs, K3 G2 MSMs, K4
// pairings, MIPP folds, Fr kernels); the host keeps the Fiat-Shamir
// transcript, which is inherently sequential and only absorbs a few KB per
// round.
#include <cstring>
#include <memory>
#include <vector>
#include <cstdio>
#include <cstdlib>

#include "../../include/tpst.h"
#include "ctx.h"
#include "fbt.h"
#include "host_curve.h"
#include "device_util.h"
#include "pst_kernels.h"
#include "trace.h"
#include "poseidon_host.h"
#include "pst_state.h"

using namespace tpst;

// =================================================================== host ==
namespace {

// host Fr helpers
Fr fr_inv(const Fr& a) { return inv(a); }

bool all_zero(const uint64_t* a, int n) {
  for (int i = 0; i < n; i++)
    if (a[i]) return false;
  return true;
}

}  // namespace

// ================================================================ state ==
static std::unique_ptr<SrsState>& srs_slot(tpst_ctx* ctx) {
  static std::mutex mu;
  static std::vector<std::pair<tpst_ctx*, std::unique_ptr<SrsState>>> slots;
  std::lock_guard<std::mutex> lk(mu);
  for (auto& s : slots)
    if (s.first == ctx) return s.second;
  slots.emplace_back(ctx, nullptr);
  return slots.back().second;
}

void tpst_release_pst_state(tpst_ctx* ctx) { srs_slot(ctx).reset(); }

extern "C" size_t tpst_srs_flat_len(int nv) {
  size_t n = 12 + 24;
  for (int i = 0; i < nv; i++) n += ((size_t)1 << (nv - i)) * 36;
  return n + (size_t)nv * 36;
}

// upload the flat canonical SRS and build every derived device table
static int srs_install(tpst_ctx* ctx, int nv, const uint64_t* flat) {
  auto st = std::make_unique<SrsState>();
  st->nv = nv;
  st->flat.assign(flat, flat + tpst_srs_flat_len(nv));
  hipStream_t s = ctx->stream;
  DevBuf stage;
  TPST_HIP(ctx, stage.alloc(st->flat.size() * 8));
  TPST_HIP(ctx, hipMemcpyAsync(stage.p, flat, st->flat.size() * 8, hipMemcpyHostToDevice, s));
  const uint32_t* src = stage.u();
  auto take = [&](DevBuf& dst, size_t npts, int words) -> hipError_t {
    hipError_t e = dst.alloc(npts * words * 4);
    if (e != hipSuccess) return e;
    e = words == 24 ? points_to_mont<Fq>(s, src, dst.u(), npts) : points_to_mont<Fq2>(s, src, dst.u(), npts);
    src += npts * words;
    return e;
  };
  TPST_HIP(ctx, take(st->g, 1, 24));
  TPST_HIP(ctx, take(st->h, 1, 48));
  for (int i = 0; i < nv; i++) {
    const size_t m = (size_t)1 << (nv - i);
    st->pg.emplace_back(new DevBuf());
    st->ph.emplace_back(new DevBuf());
    TPST_HIP(ctx, take(*st->pg.back(), m, 24));
    TPST_HIP(ctx, take(*st->ph.back(), m, 48));
    st->pg_pair.emplace_back(new DevBuf());
    st->ph_pair.emplace_back(new DevBuf());
    TPST_HIP(ctx, st->pg_pair.back()->alloc(m / 2 * 96));
    TPST_HIP(ctx, st->ph_pair.back()->alloc(m / 2 * 192));
    TPST_HIP(ctx, pair_sum<Fq>(s, st->pg.back()->u(), m / 2, st->pg_pair.back()->u()));
    TPST_HIP(ctx, pair_sum<Fq2>(s, st->ph.back()->u(), m / 2, st->ph_pair.back()->u()));
  }
  TPST_HIP(ctx, take(st->gmask, nv, 24));
  TPST_HIP(ctx, take(st->hmask, nv, 48));
  const size_t N = (size_t)1 << nv;
  TPST_HIP(ctx, batch_tables_build(s, st->pg[0]->u(), N, batch_window_bits(N), st->tables));
  TPST_HIP(ctx, st->prep_scratch.alloc(g2_prepare_scratch((size_t)1 << nv)));  // released below
  for (int odd = 0; odd < 2 && odd < nv; odd++) {
    const size_t m = (size_t)1 << (nv - odd);
    TPST_HIP(ctx, st->hprep[odd].alloc(m * N_LINE_COEFFS * sizeof(LineCoeff)));
    TPST_HIP(ctx, g2_prepare_batch(s, st->ph[odd]->u(), m, (LineCoeff*)st->hprep[odd].p, st->prep_scratch.u()));
  }
  // fixed-base tables of the opening (a function of the key only, like the
  // cached G2Prepared above): built here so that no open pays for them
  for (int odd = 0; odd < 2 && odd < nv; odd++) {
    int rc = srs_fbt(ctx, st.get(), odd);
    if (rc) return rc;
  }
  TPST_HIP(ctx, hipStreamSynchronize(s));
  TPST_HIP(ctx, st->prep_scratch.alloc(0));
  srs_slot(ctx) = std::move(st);
  return TPST_OK;
}

SrsState* tpst::srs_of(tpst_ctx* ctx) { return srs_slot(ctx).get(); }

// (r1cs.hip) the number of variables of the loaded SRS, or -1
int tpst::srs_nv(tpst_ctx* ctx) {
  SrsState* st = srs_of(ctx);
  return st ? st->nv : -1;
}

// scratch of the RNS G2 preparation (g2_prepare_scratch(n) bytes: residue
// lines, ~53 KB per point) sized for the largest batch prepared since the
// SRS was installed -- the install's 2^nv batch is released right after it
// (217 MB at nv = 12); callers size it before enqueueing any stream work
int tpst::prep_scratch_for(tpst_ctx* ctx, SrsState* st, size_t n) {
  const size_t b = g2_prepare_scratch(n);
  if (st->prep_scratch.p && st->prep_scratch.bytes >= b) return TPST_OK;
  TPST_HIP(ctx, st->prep_scratch.alloc(b));  // hipFree of a smaller one waits for its users
  return TPST_OK;
}

// SplitMix64 Fr stream (same definition as the bench / oracle generators)
static uint64_t splitmix(uint64_t seed, uint64_t i) {
  uint64_t z = seed + (i + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

extern "C" uint64_t tpst_fr_stream(uint64_t seed, size_t n, uint64_t start, uint64_t* out) {
  const uint32_t* r = params::FR_P;
  uint64_t k = start;
  size_t got = 0;
  while (got < n) {
    uint64_t v[4];
    for (int j = 0; j < 4; j++) v[j] = splitmix(seed, 4 * k + j);
    v[3] &= (1ull << 61) - 1;
    k++;
    bool lt = false;
    for (int i = 3; i >= 0; i--) {
      const uint64_t ri = (uint64_t)r[2 * i] | ((uint64_t)r[2 * i + 1] << 32);
      if (v[i] != ri) {
        lt = v[i] < ri;
        break;
      }
    }
    if (lt) {
      memcpy(out + 4 * got, v, 32);
      got++;
    }
  }
  return k;
}

// MultilinearPC::setup semantics from a seeded trapdoor: g = k_g G1, h = k_h G2,
// powers_of_g[i][x] = g^{eq(t[i..], x)} (LSB-first), g_mask[i] = g^{t_i}
extern "C" int tpst_srs_setup(tpst_ctx* ctx, int nv, uint64_t seed) {
  if (!ctx || nv <= 0 || nv > 28) return fail(ctx, TPST_E_ARG, "bad nv");
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  std::vector<uint64_t> vals(4 * (nv + 2));
  tpst_fr_stream(seed, nv + 2, 0, vals.data());
  std::vector<Fr> t(nv);
  for (int i = 0; i < nv; i++) t[i] = fr_canon(&vals[4 * (2 + i)]);
  // all scalars: [k_g], [k_h] handled by generator muls; then eq tables and t
  std::vector<uint64_t> sc;  // canonical: for i: eq(t[i..]) ; then t
  for (int i = 0; i < nv; i++) {
    std::vector<Fr> tab(1, Fr::one());
    for (int j = i; j < nv; j++) {
      const size_t m = tab.size();
      tab.resize(2 * m);
      for (size_t x = 0; x < m; x++) {
        const Fr v = tab[x];
        tab[x] = mul(v, sub(Fr::one(), t[j]));
        tab[x + m] = mul(v, t[j]);
      }
    }
    for (auto& v : tab) {
      uint64_t c[4];
      fr_out(v, c);
      sc.insert(sc.end(), c, c + 4);
    }
  }
  for (int i = 0; i < nv; i++) sc.insert(sc.end(), &vals[4 * (2 + i)], &vals[4 * (2 + i)] + 4);
  const size_t ns = sc.size() / 4;
  hipStream_t s = ctx->stream;
  DevBuf d_sc, d_gh_sc, d_g, d_h, d_og, d_oh;
  TPST_HIP(ctx, d_sc.alloc(ns * 32));
  TPST_HIP(ctx, d_gh_sc.alloc(64));
  TPST_HIP(ctx, d_g.alloc(96));
  TPST_HIP(ctx, d_h.alloc(192));
  TPST_HIP(ctx, d_og.alloc(ns * 96));
  TPST_HIP(ctx, d_oh.alloc(ns * 192));
  TPST_HIP(ctx, hipMemcpyAsync(d_sc.p, sc.data(), ns * 32, hipMemcpyHostToDevice, s));
  TPST_HIP(ctx, hipMemcpyAsync(d_gh_sc.p, vals.data(), 64, hipMemcpyHostToDevice, s));
  // g, h from the standard generators
  {
    const uint32_t* gs = params::G1_GEN_X;
    std::vector<uint32_t> gen1(24), gen2(48);
    memcpy(gen1.data(), params::G1_GEN_X, 48);
    memcpy(gen1.data() + 12, params::G1_GEN_Y, 48);
    memcpy(gen2.data(), params::G2_GEN_X, 96);
    memcpy(gen2.data() + 24, params::G2_GEN_Y, 96);
    (void)gs;
    DevBuf dg1, dg2;
    TPST_HIP(ctx, dg1.alloc(96));
    TPST_HIP(ctx, dg2.alloc(192));
    TPST_HIP(ctx, hipMemcpyAsync(dg1.p, gen1.data(), 96, hipMemcpyHostToDevice, s));
    TPST_HIP(ctx, hipMemcpyAsync(dg2.p, gen2.data(), 192, hipMemcpyHostToDevice, s));
    TPST_HIP(ctx, fixed_base_mul<Fq>(s, dg1.u(), d_gh_sc.u(), 1, d_g.u()));
    TPST_HIP(ctx, fixed_base_mul<Fq2>(s, dg2.u(), d_gh_sc.u() + 8, 1, d_h.u()));
    TPST_HIP(ctx, fixed_base_mul<Fq>(s, d_g.u(), d_sc.u(), ns, d_og.u()));
    TPST_HIP(ctx, fixed_base_mul<Fq2>(s, d_h.u(), d_sc.u(), ns, d_oh.u()));
    TPST_HIP(ctx, affine_from_mont<Fq>(s, d_g.u(), d_g.u(), 1));
    TPST_HIP(ctx, affine_from_mont<Fq2>(s, d_h.u(), d_h.u(), 1));
    TPST_HIP(ctx, affine_from_mont<Fq>(s, d_og.u(), d_og.u(), ns));
    TPST_HIP(ctx, affine_from_mont<Fq2>(s, d_oh.u(), d_oh.u(), ns));
    TPST_HIP(ctx, hipStreamSynchronize(s));
  }
  std::vector<uint64_t> og(ns * 12), oh(ns * 24), flat(tpst_srs_flat_len(nv));
  TPST_HIP(ctx, hipMemcpy(og.data(), d_og.p, ns * 96, hipMemcpyDeviceToHost));
  TPST_HIP(ctx, hipMemcpy(oh.data(), d_oh.p, ns * 192, hipMemcpyDeviceToHost));
  TPST_HIP(ctx, hipMemcpy(flat.data(), d_g.p, 96, hipMemcpyDeviceToHost));
  TPST_HIP(ctx, hipMemcpy(flat.data() + 12, d_h.p, 192, hipMemcpyDeviceToHost));
  uint64_t* o = flat.data() + 36;
  size_t off = 0;
  for (int i = 0; i < nv; i++) {
    const size_t m = (size_t)1 << (nv - i);
    memcpy(o, &og[12 * off], m * 96);
    o += 12 * m;
    memcpy(o, &oh[24 * off], m * 192);
    o += 24 * m;
    off += m;
  }
  memcpy(o, &og[12 * off], nv * 96);
  o += 12 * nv;
  memcpy(o, &oh[24 * off], nv * 192);
  return srs_install(ctx, nv, flat.data());
}

extern "C" int tpst_srs_load(tpst_ctx* ctx, int nv, const uint64_t* flat) {
  if (!ctx || !flat || nv <= 0 || nv > 28) return fail(ctx, TPST_E_ARG, "bad argument");
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  return srs_install(ctx, nv, flat);
}

extern "C" int tpst_srs_export(tpst_ctx* ctx, uint64_t* flat) {
  if (!ctx || !flat) return fail(ctx, TPST_E_ARG, "null argument");
  SrsState* st = srs_of(ctx);
  if (!st) return fail(ctx, TPST_E_STATE, "no SRS loaded");
  memcpy(flat, st->flat.data(), st->flat.size() * 8);
  return TPST_OK;
}

// Valid::check of an affine point (what Validate::Yes deserialisation runs):
// canonical coordinates, on the curve, in the r-torsion subgroup.  Host only.
extern "C" int tpst_g1_check(const uint64_t* p) { return p && point_valid<Fq>(p) ? TPST_OK : TPST_E_VERIFY; }
extern "C" int tpst_g2_check(const uint64_t* p) { return p && point_valid<Fq2>(p) ? TPST_OK : TPST_E_VERIFY; }

// ============================================================ transcript ==
extern "C" void tpst_transcript_init(tpst_transcript* t) {
  if (!t) return;
  memset(t, 0, sizeof *t);
}

extern "C" int tpst_transcript_append_g1(tpst_transcript* t, const uint64_t* p) {
  if (!t || !p) return TPST_E_ARG;
  Sponge sp;
  sp.load(t);
  uint8_t b[96];
  g1_bytes(p, b);
  sp.absorb_bytes(b, 96);
  sp.store(t);
  return TPST_OK;
}

extern "C" int tpst_transcript_append_gt(tpst_transcript* t, const uint64_t* gt) {
  if (!t || !gt) return TPST_E_ARG;
  Sponge sp;
  sp.load(t);
  sp.absorb_bytes((const uint8_t*)gt, 576);
  sp.store(t);
  return TPST_OK;
}

// append_bytes (poseidon_transcript.rs:67-69): Absorb of a Vec<u8> (u64 length
// prefix, 47-byte chunks); `append` of any CanonicalSerialize value is this
// over its Compress::No bytes (poseidon_transcript.rs:22-28)
extern "C" int tpst_transcript_append_bytes(tpst_transcript* t, const uint8_t* b, size_t n) {
  if (!t || (n && !b)) return TPST_E_ARG;
  Sponge sp;
  sp.load(t);
  sp.absorb_bytes(b, n);
  sp.store(t);
  return TPST_OK;
}

// append_scalar (poseidon_transcript.rs:83-85): Absorb of an Fr into the Fq
// sponge = one Fq element with the same integer value (r < p)
extern "C" int tpst_transcript_append_fr(tpst_transcript* t, const uint64_t* fr) {
  if (!t || !fr || !fr_ok(fr)) return TPST_E_ARG;
  Sponge sp;
  sp.load(t);
  const uint64_t l[6] = {fr[0], fr[1], fr[2], fr[3], 0, 0};
  sp.absorb(std::vector<Fq>{fq_canon(l)});
  sp.store(t);
  return TPST_OK;
}

// new_from_state2 (poseidon_transcript.rs:55-60): a fresh sponge, then
// append(Fr) = absorb of its 32-byte uncompressed serialisation
extern "C" int tpst_transcript_reset_fr(tpst_transcript* t, const uint64_t* fr) {
  if (!t || !fr || !fr_ok(fr)) return TPST_E_ARG;
  memset(t, 0, sizeof *t);
  Sponge sp;
  sp.load(t);
  sp.absorb_bytes((const uint8_t*)fr, 32);
  sp.store(t);
  return TPST_OK;
}

extern "C" int tpst_transcript_challenge(tpst_transcript* t, uint64_t* out) {
  if (!t || !out) return TPST_E_ARG;
  Sponge sp;
  sp.load(t);
  sp.challenge(out);
  sp.store(t);
  return TPST_OK;
}

// ================================================================ poly ===
int tpst::poly_dims(int n, int& m_col, int& m_row, int& odd) {
  if (n < 2 || n > 40) return -1;
  m_col = n / 2;
  m_row = n - m_col;
  odd = n % 2;
  return 0;
}

extern "C" int tpst_poly_from_evaluations(tpst_ctx* ctx, const uint64_t* Z, int n, tpst_poly** out) {
  if (!ctx || !Z || !out) return fail(ctx, TPST_E_ARG, "null argument");
  auto p = std::make_unique<tpst_poly>();
  if (poly_dims(n, p->m_col, p->m_row, p->odd)) return fail(ctx, TPST_E_ARG, "bad num_vars");
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  p->ctx = ctx;
  p->n = n;
  TPST_HIP(ctx, p->Zown.alloc(((size_t)1 << n) * 32));
  TPST_HIP(ctx, hipMemcpy(p->Zown.p, Z, ((size_t)1 << n) * 32, hipMemcpyHostToDevice));
  p->d_Z = p->Zown.u();
  *out = p.release();
  return TPST_OK;
}

// rank-local upload of the columns [c0, c1) of the strided view: for every
// j < 2^m_row the run Z[j 2^m_col + c0 .. j 2^m_col + c1) -- one 2D copy, no
// host transpose, (c1 - c0) / 2^m_col of the bytes
extern "C" int tpst_poly_from_evaluations_cols(tpst_ctx* ctx, const uint64_t* Z, int n, size_t c0, size_t c1,
                                               tpst_poly** out) {
  if (!ctx || !Z || !out) return fail(ctx, TPST_E_ARG, "null argument");
  auto p = std::make_unique<tpst_poly>();
  if (poly_dims(n, p->m_col, p->m_row, p->odd)) return fail(ctx, TPST_E_ARG, "bad num_vars");
  const size_t C = (size_t)1 << p->m_col, N = (size_t)1 << p->m_row;
  if (c0 >= c1 || c1 > C) return fail(ctx, TPST_E_ARG, "bad column range");
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  p->ctx = ctx;
  p->n = n;
  p->col0 = c0;
  p->ncols = c1 - c0;
  TPST_HIP(ctx, p->Zown.alloc(N * p->ncols * 32));
  TPST_HIP(ctx, hipMemcpy2DAsync(p->Zown.p, p->ncols * 32, Z + 4 * c0, C * 32, p->ncols * 32, N,
                                 hipMemcpyHostToDevice, ctx->stream));
  TPST_HIP(ctx, hipStreamSynchronize(ctx->stream));
  p->d_Z = p->Zown.u();
  *out = p.release();
  return TPST_OK;
}

// base pointer and column stride of rows [r0, r1) in the resident block
static int poly_rows_view(tpst_ctx* ctx, const tpst_poly* p, size_t r0, size_t r1, const uint32_t** base,
                          size_t* cs) {
  const size_t C = (size_t)1 << p->m_col;
  if (!p->ncols) {
    if (r1 > C) return fail(ctx, TPST_E_ARG, "row range out of bounds");
    *base = p->d_Z + 8 * r0;
    *cs = C;
    return TPST_OK;
  }
  if (r0 < p->col0 || r1 > p->col0 + p->ncols) return fail(ctx, TPST_E_ARG, "rows outside the resident column slice");
  *base = p->d_Z + 8 * (r0 - p->col0);
  *cs = p->ncols;
  return TPST_OK;
}

static int poly_need_full(tpst_ctx* ctx, const tpst_poly* p) {
  if (p->q_only) return fail(ctx, TPST_E_STATE, "operation needs the evaluations (this handle holds q only)");
  return p->ncols ? fail(ctx, TPST_E_STATE, "operation needs the whole polynomial (this handle holds a column slice)")
                  : TPST_OK;
}

// eval / open need q and chi(b): a whole polynomial computes them, an
// opening-only handle carries them
int tpst::poly_need_q_source(tpst_ctx* ctx, const tpst_poly* p) {
  return p->q_only ? TPST_OK : poly_need_full(ctx, p);
}

extern "C" int tpst_poly_from_evaluations_dev(tpst_ctx* ctx, const void* d_Z, int n, tpst_poly** out) {
  if (!ctx || !d_Z || !out) return fail(ctx, TPST_E_ARG, "null argument");
  auto p = std::make_unique<tpst_poly>();
  if (poly_dims(n, p->m_col, p->m_row, p->odd)) return fail(ctx, TPST_E_ARG, "bad num_vars");
  p->ctx = ctx;
  p->n = n;
  p->d_Z = (const uint32_t*)d_Z;
  *out = p.release();
  return TPST_OK;
}

extern "C" void tpst_poly_free(tpst_poly* p) { delete p; }

// get_q (sqrt_pst.rs:81-101): chis over b = point[m_row..], q = Z^T chis
int tpst::poly_get_q(tpst_ctx* ctx, tpst_poly* p, const uint64_t* point) {
  TraceRange tr("build_q");
  hipStream_t s = ctx->stream;
  ctx->prof.begin(ST_BUILD_Q, s);
  DevBuf b;
  TPST_HIP(ctx, b.alloc((size_t)(p->m_col ? p->m_col : 1) * 32));
  if (p->m_col) {
    TPST_HIP(ctx, hipMemcpyAsync(b.p, point + 4 * p->m_row, p->m_col * 32, hipMemcpyHostToDevice, s));
    TPST_HIP(ctx, fr_to_mont(s, b.u(), b.u(), p->m_col));
  }
  TPST_HIP(ctx, p->chis.alloc(((size_t)1 << p->m_col) * 32));
  TPST_HIP(ctx, p->q.alloc(((size_t)1 << p->m_row) * 32));
  TPST_HIP(ctx, chi_table(s, b.u(), p->m_col, p->chis.u()));
  TPST_HIP(ctx, get_q(s, p->d_Z, p->m_col, p->m_row, p->chis.u(), p->q.u()));
  ctx->prof.end(ST_BUILD_Q, s);
  TPST_HIP(ctx, hipStreamSynchronize(s));
  p->has_q = true;
  return TPST_OK;
}

extern "C" int tpst_poly_eval(tpst_ctx* ctx, tpst_poly* p, const uint64_t* point, uint64_t* out_v) {
  if (!ctx || !p || !point || !out_v) return fail(ctx, TPST_E_ARG, "null argument");
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  if (int rc = poly_need_q_source(ctx, p)) return rc;
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  if (!p->has_q) {
    int rc = poly_get_q(ctx, p, point);
    if (rc) return rc;
  }
  hipStream_t s = ctx->stream;
  DevBuf a, ca, v;
  TPST_HIP(ctx, a.alloc(p->m_row * 32));
  TPST_HIP(ctx, ca.alloc(((size_t)1 << p->m_row) * 32));
  TPST_HIP(ctx, v.alloc(32));
  TPST_HIP(ctx, hipMemcpyAsync(a.p, point, p->m_row * 32, hipMemcpyHostToDevice, s));
  TPST_HIP(ctx, fr_to_mont(s, a.u(), a.u(), p->m_row));
  TPST_HIP(ctx, chi_table(s, a.u(), p->m_row, ca.u()));
  TPST_HIP(ctx, fr_dot(s, p->q.u(), ca.u(), (size_t)1 << p->m_row, v.u()));
  TPST_HIP(ctx, fr_from_mont(s, v.u(), v.u(), 1));
  TPST_HIP(ctx, hipMemcpyAsync(out_v, v.p, 32, hipMemcpyDeviceToHost, s));
  TPST_HIP(ctx, hipStreamSynchronize(s));
  return TPST_OK;
}

// commit (sqrt_pst.rs:117-149): K1 row MSMs + IPP T = prod e(C_i, h_i)

// the context's pinned host staging (grow-only; the opening's per-round
// transfers, the commit's outputs)
int tpst::ensure_pinned(tpst_ctx* ctx, size_t bytes) {
  if (ctx->pinned_cap >= bytes) return TPST_OK;
  if (ctx->pinned) TPST_HIP(ctx, hipHostFree(ctx->pinned));
  ctx->pinned = nullptr;
  ctx->pinned_cap = 0;
  TPST_HIP(ctx, hipHostMalloc(&ctx->pinned, bytes, hipHostMallocDefault));
  ctx->pinned_cap = bytes;
  return TPST_OK;
}

// prebuild (tpst_poly_commit): also build the opening's fold table over the
// row commitments on a side stream while the IPP runs (TPST_COMMIT_TABLE=0 /
// 1 forces it off / on)
static int poly_commit_dev(tpst_ctx* ctx, tpst_poly* p, uint32_t* d_comms_mont, Fq12* d_T, bool prebuild = false) {
  SrsState* st = srs_of(ctx);
  if (!st) return fail(ctx, TPST_E_STATE, "no SRS loaded");
  if (st->nv != p->m_row) return fail(ctx, TPST_E_ARG, "SRS num_vars != ceil(n/2)");
  hipStream_t s = ctx->stream;
  const size_t C = (size_t)1 << p->m_col;
  ctx->arena2.reset();
  TPST_HIP(ctx, ctx->arena2.reserve(Arena::need(C, sizeof(Xyzz<Fq>)) + 256));
  Xyzz<Fq>* rows = ctx->arena2.take<Xyzz<Fq>>(C);
  Profiler& pf = ctx->prof;
  pf.begin(ST_SQRT_COMMIT, s);
  {
    TraceRange tr("comm_list");  // sqrt_pst.rs:119-126
    pf.begin(ST_COMM_LIST, s);
    TPST_HIP(ctx, msm_batch(ctx->arena, s, st->tables, p->d_Z, C, 1, C, rows));
    TPST_HIP(ctx, xyzz_to_affine_mont<Fq>(s, rows, d_comms_mont, C));
    pf.end(ST_COMM_LIST, s);
  }
  if (prebuild) {  // the opening's GLV fold table over comm_list, beside the IPP
    if (int rc = open_streams(ctx, 8, 0)) return rc;
    if (st->t_A_n < C) {
      TPST_HIP(ctx, st->t_A.alloc(fbt_words<Fq>(C) * 4));
      st->t_A_n = C;
    }
    st->t_A_key.clear();
    hipEvent_t* ev = ctx->events.data();
    TPST_HIP(ctx, hipEventRecord(ev[0], s));
    TPST_HIP(ctx, hipStreamWaitEvent(ctx->side[1], ev[0], 0));
    TPST_HIP(ctx, fbt_build<Fq>(ctx->arena_side[1], ctx->side[1], d_comms_mont, C, st->t_A.u(), true));
    TPST_HIP(ctx, hipEventRecord(ev[1], ctx->side[1]));
  }
  {
    TraceRange tr("ipp");  // sqrt_pst.rs:131-144
    pf.begin(ST_IPP, s);
    const LineCoeff* hp = (const LineCoeff*)st->hprep[p->odd].p;
    ctx->arena.reset();
    TPST_HIP(ctx, ctx->arena.reserve(multi_pairing_scratch(1, C)));
    TPST_HIP(ctx, multi_pairing_prepared(ctx->arena, s, d_comms_mont, st->ph[p->odd]->u(), hp, 1, C, d_T));
    pf.end(ST_IPP, s);
  }
  if (prebuild) TPST_HIP(ctx, hipStreamWaitEvent(s, ctx->events[1], 0));
  pf.end(ST_SQRT_COMMIT, s);
  return TPST_OK;
}

extern "C" int tpst_poly_commit(tpst_ctx* ctx, tpst_poly* p, uint64_t* comms, uint64_t* T) {
  if (!ctx || !p || !comms || !T) return fail(ctx, TPST_E_ARG, "null argument");
  TraceRange tr("sqrt_commit");
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  if (int rc = poly_need_full(ctx, p)) return rc;
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  const size_t C = (size_t)1 << p->m_col;
  ctx->io.reset();  // (grow-only: no per-call hipMalloc / hipFree)
  TPST_HIP(ctx, ctx->io.reserve(Arena::need(C * 24, 4) + Arena::need(1, sizeof(Fq12)) +
                                Arena::need(C * 24 + 144, 4) + 512));
  uint32_t* cm = ctx->io.take<uint32_t>(C * 24);
  Fq12* tt = ctx->io.take<Fq12>(1);
  uint32_t* out = ctx->io.take<uint32_t>(C * 24 + 144);
  // the table build runs beside the IPP (2^20: commit + open 21.7 -> 21.2
  // ms); at C = 4096 it outlasts the IPP by ~2 ms but leaves the opening's
  // first round free of it.  TPST_COMMIT_TABLE=0: the opening builds it
  static const int table_env = [] {
    const char* e = getenv("TPST_COMMIT_TABLE");
    return e ? atoi(e) : -1;
  }();
  const bool prebuild = table_env != 0;
  int rc = poly_commit_dev(ctx, p, cm, tt, prebuild);
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  TPST_HIP(ctx, affine_from_mont<Fq>(s, cm, out, C));
  TPST_HIP(ctx, fq12_from_mont(s, tt, out + 24 * C, 1));
  // one asynchronous copy into pinned staging (not two pageable ones)
  if (int rc2 = ensure_pinned(ctx, C * 96 + 576)) return rc2;
  TPST_HIP(ctx, hipMemcpyAsync(ctx->pinned, out, C * 96 + 576, hipMemcpyDeviceToHost, s));
  TPST_HIP(ctx, hipStreamSynchronize(s));
  memcpy(comms, ctx->pinned, C * 96);
  memcpy(T, (const uint8_t*)ctx->pinned + C * 96, 576);
  if (prebuild) srs_of(ctx)->t_A_key.assign(comms, comms + 12 * C);
  return TPST_OK;
}

// device-resident commit: d_comms canonical affine (C*96 B), d_T canonical GT
extern "C" int tpst_poly_commit_dev(tpst_ctx* ctx, tpst_poly* p, void* d_comms, void* d_T) {
  if (!ctx || !p || !d_comms || !d_T) return fail(ctx, TPST_E_ARG, "null argument");
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  if (int rc = poly_need_full(ctx, p)) return rc;
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  const size_t C = (size_t)1 << p->m_col;
  ctx->io.reset();
  TPST_HIP(ctx, ctx->io.reserve(Arena::need(C * 24, 4) + Arena::need(1, sizeof(Fq12)) + 512));
  uint32_t* cm = ctx->io.take<uint32_t>(C * 24);
  Fq12* tt = ctx->io.take<Fq12>(1);
  int rc = poly_commit_dev(ctx, p, cm, tt);
  if (rc) return rc;
  TPST_HIP(ctx, affine_from_mont<Fq>(ctx->stream, cm, (uint32_t*)d_comms, C));
  TPST_HIP(ctx, fq12_from_mont(ctx->stream, tt, (uint32_t*)d_T, 1));
  return TPST_OK;
}

// row-sharded commit: rows [r0, r1) of the strided view,
// i.e. this rank's block of columns of Z.  comms: (r1-r0) canonical affine G1.
extern "C" int tpst_poly_commit_rows(tpst_ctx* ctx, tpst_poly* p, size_t r0, size_t r1, uint64_t* comms) {
  if (!ctx || !p || !comms || r1 < r0) return fail(ctx, TPST_E_ARG, "bad argument");
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  SrsState* st = srs_of(ctx);
  if (!st) return fail(ctx, TPST_E_STATE, "no SRS loaded");
  if (st->nv != p->m_row) return fail(ctx, TPST_E_ARG, "SRS num_vars != ceil(n/2)");
  const uint32_t* zb;
  size_t cs;
  if (int rc = poly_rows_view(ctx, p, r0, r1, &zb, &cs)) return rc;
  const size_t R = r1 - r0;
  if (R == 0) return TPST_OK;
  hipStream_t s = ctx->stream;
  DevBuf rows, out;
  TPST_HIP(ctx, rows.alloc(R * sizeof(Xyzz<Fq>)));
  TPST_HIP(ctx, out.alloc(R * 96));
  TPST_HIP(ctx, msm_batch(ctx->arena, s, st->tables, zb, R, 1, cs, (Xyzz<Fq>*)rows.p));
  TPST_HIP(ctx, xyzz_to_affine_canonical<Fq>(s, (Xyzz<Fq>*)rows.p, out.u(), R));
  TPST_HIP(ctx, hipMemcpyAsync(comms, out.p, R * 96, hipMemcpyDeviceToHost, s));
  TPST_HIP(ctx, hipStreamSynchronize(s));
  return TPST_OK;
}

// IPP of a full commitment list: T = prod_i e(comms[i], powers_of_h[odd][i])
// (sqrt_pst.rs:128-143), for a list gathered from the ranks
extern "C" int tpst_poly_ipp(tpst_ctx* ctx, int n, const uint64_t* comms, uint64_t* T) {
  if (!ctx || !comms || !T) return fail(ctx, TPST_E_ARG, "null argument");
  int m_col, m_row, odd;
  if (poly_dims(n, m_col, m_row, odd)) return fail(ctx, TPST_E_ARG, "bad num_vars");
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  SrsState* st = srs_of(ctx);
  if (!st) return fail(ctx, TPST_E_STATE, "no SRS loaded");
  if (st->nv != m_row) return fail(ctx, TPST_E_ARG, "SRS num_vars != ceil(n/2)");
  const size_t C = (size_t)1 << m_col;
  hipStream_t s = ctx->stream;
  DevBuf up, cm, tt, out;
  TPST_HIP(ctx, up.alloc(C * 96));
  TPST_HIP(ctx, cm.alloc(C * 96));
  TPST_HIP(ctx, tt.alloc(sizeof(Fq12)));
  TPST_HIP(ctx, out.alloc(576));
  TPST_HIP(ctx, hipMemcpyAsync(up.p, comms, C * 96, hipMemcpyHostToDevice, s));
  TPST_HIP(ctx, points_to_mont<Fq>(s, up.u(), cm.u(), C));
  ctx->arena.reset();
  TPST_HIP(ctx, ctx->arena.reserve(multi_pairing_scratch(1, C)));
  TPST_HIP(ctx, multi_pairing_prepared(ctx->arena, s, cm.u(), st->ph[odd]->u(), (const LineCoeff*)st->hprep[odd].p, 1,
                                       C, (Fq12*)tt.p));
  TPST_HIP(ctx, fq12_from_mont(s, (Fq12*)tt.p, out.u(), 1));
  TPST_HIP(ctx, hipMemcpyAsync(T, out.p, 576, hipMemcpyDeviceToHost, s));
  TPST_HIP(ctx, hipStreamSynchronize(s));
  return TPST_OK;
}

// Row-sharded commit with the IPP split across ranks: the
// MSMs of rows [r0, r1) AND the Miller-loop product of their pairs
// prod_{r0 <= i < r1} ml(C_i, h_i) before final exponentiation (canonical
// Fq12, 72 u64).  Rank 0 finishes T = FE(prod over ranks) with
// tpst_gt_final_exp_product, so no rank runs more than its share of Miller loops.
static int commit_rows_partial(tpst_ctx* ctx, tpst_poly* p, size_t r0, size_t r1, uint64_t* comms, uint64_t* miller,
                               void* d_out) {
  if (!ctx || !p || ((!comms || !miller) && !d_out) || r1 < r0) return fail(ctx, TPST_E_ARG, "bad argument");
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  SrsState* st = srs_of(ctx);
  if (!st) return fail(ctx, TPST_E_STATE, "no SRS loaded");
  if (st->nv != p->m_row) return fail(ctx, TPST_E_ARG, "SRS num_vars != ceil(n/2)");
  const uint32_t* zb;
  size_t cs;
  if (int rc = poly_rows_view(ctx, p, r0, r1, &zb, &cs)) return rc;
  const size_t R = r1 - r0;
  hipStream_t s = ctx->stream;
  if (R == 0) {  // empty share: comms untouched, partial = 1
    uint64_t one[72] = {1};
    if (d_out) {
      TPST_HIP(ctx, hipMemcpyAsync(d_out, one, 576, hipMemcpyHostToDevice, s));
      TPST_HIP(ctx, hipStreamSynchronize(s));
    } else {
      memcpy(miller, one, 576);
    }
    return TPST_OK;
  }
  if (int rc = prep_scratch_for(ctx, st, R)) return rc;
  DevBuf rows, cm, out, hsub, tt;
  TPST_HIP(ctx, rows.alloc(R * sizeof(Xyzz<Fq>)));
  TPST_HIP(ctx, cm.alloc(R * 96));
  TPST_HIP(ctx, out.alloc(R * 96 + 576));
  TPST_HIP(ctx, tt.alloc(sizeof(Fq12)));
  TPST_HIP(ctx, msm_batch(ctx->arena, s, st->tables, zb, R, 1, cs, (Xyzz<Fq>*)rows.p));
  TPST_HIP(ctx, xyzz_to_affine_mont<Fq>(s, (Xyzz<Fq>*)rows.p, cm.u(), R));
  // this rank's h_i and their prepared lines: the coefficient-major cache has
  // row length C, so the R-pair slice is re-prepared (R G2 points, one launch)
  const uint32_t* h = st->ph[p->odd]->u() + 48 * r0;
  const size_t need = Arena::need(R * N_LINE_COEFFS, sizeof(LineCoeff)) + multi_pairing_scratch(1, R) + 4096;
  ctx->arena.reset();
  TPST_HIP(ctx, ctx->arena.reserve(need));
  LineCoeff* lc = ctx->arena.take<LineCoeff>(R * N_LINE_COEFFS);
  TPST_HIP(ctx, g2_prepare_batch(s, h, R, lc, st->prep_scratch.u()));
  TPST_HIP(ctx, multi_pairing_prepared(ctx->arena, s, cm.u(), h, lc, 1, R, (Fq12*)tt.p, false));
  TPST_HIP(ctx, affine_from_mont<Fq>(s, cm.u(), out.u(), R));
  TPST_HIP(ctx, fq12_from_mont(s, (Fq12*)tt.p, out.u() + 24 * R, 1));
  if (d_out) {  // [comms | partial] straight into the caller's (all-gather) buffer
    TPST_HIP(ctx, hipMemcpyAsync(d_out, out.p, R * 96 + 576, hipMemcpyDeviceToDevice, s));
  } else {
    TPST_HIP(ctx, hipMemcpyAsync(comms, out.p, R * 96, hipMemcpyDeviceToHost, s));
    TPST_HIP(ctx, hipMemcpyAsync(miller, out.u() + 24 * R, 576, hipMemcpyDeviceToHost, s));
  }
  TPST_HIP(ctx, hipStreamSynchronize(s));
  return TPST_OK;
}

extern "C" int tpst_poly_commit_rows_partial(tpst_ctx* ctx, tpst_poly* p, size_t r0, size_t r1, uint64_t* comms,
                                             uint64_t* miller) {
  return commit_rows_partial(ctx, p, r0, r1, comms, miller, nullptr);
}

extern "C" int tpst_poly_commit_rows_partial_dev(tpst_ctx* ctx, tpst_poly* p, size_t r0, size_t r1, void* d_out) {
  return commit_rows_partial(ctx, p, r0, r1, nullptr, nullptr, d_out);
}

// T = FE(prod_k partials[k]) for k Miller-loop partials (canonical Fq12 each;
// host, or device with a byte stride between consecutive partials)
static int final_exp_product(tpst_ctx* ctx, const uint64_t* partials, const void* d_partials, size_t stride,
                             size_t k, uint64_t* T) {
  if (!ctx || (!partials && !d_partials && k) || !T) return fail(ctx, TPST_E_ARG, "null argument");
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DevBuf up, out;
  const size_t kk = k ? k : 1;
  TPST_HIP(ctx, up.alloc(kk * sizeof(Fq12)));
  TPST_HIP(ctx, out.alloc(sizeof(Fq12) + 576));
  if (k) {
    if (d_partials)
      TPST_HIP(ctx, hipMemcpy2DAsync(up.p, 576, d_partials, stride, 576, k, hipMemcpyDeviceToDevice, s));
    else
      TPST_HIP(ctx, hipMemcpyAsync(up.p, partials, k * 576, hipMemcpyHostToDevice, s));
    TPST_HIP(ctx, points_to_mont<Fq>(s, up.u(), up.u(), 6 * k));  // 12 Fq = 6 "points"
  }
  ctx->arena.reset();
  TPST_HIP(ctx, ctx->arena.reserve(gt_product_scratch(1, k)));
  TPST_HIP(ctx, gt_product_final(ctx->arena, s, (const Fq12*)up.p, 1, k, (Fq12*)out.p));
  TPST_HIP(ctx, fq12_from_mont(s, (Fq12*)out.p, out.u() + sizeof(Fq12) / 4, 1));
  TPST_HIP(ctx, hipMemcpyAsync(T, out.u() + sizeof(Fq12) / 4, 576, hipMemcpyDeviceToHost, s));
  TPST_HIP(ctx, hipStreamSynchronize(s));
  return TPST_OK;
}

extern "C" int tpst_gt_final_exp_product(tpst_ctx* ctx, const uint64_t* partials, size_t k, uint64_t* T) {
  return final_exp_product(ctx, partials, nullptr, 0, k, T);
}

extern "C" int tpst_gt_final_exp_product_dev(tpst_ctx* ctx, const void* d_partials, size_t stride_bytes, size_t k,
                                             uint64_t* T) {
  if (stride_bytes < 576) return fail(ctx, TPST_E_ARG, "stride below one Fq12");
  return final_exp_product(ctx, nullptr, d_partials, stride_bytes, k, T);
}

// ------------------------------------------------ row-sharded opening -----
// rank g holds rows [r0, r1) of the strided view (a
// column-slice handle), so it computes its share of get_q's mat-vec
//   zq_g[j] = sum_{r0 <= i < r1} Z_i[j] chi_i(b)            (sqrt_pst.rs:92-95)
// and of c_u = MSM(comm_list, chi(b))                      (sqrt_pst.rs:198);
// the shares are gathered as bytes (RCCL has no mod-r or elliptic-curve
// reduction) and summed on rank 0, which then opens from q alone.
int tpst::chi_b_table(tpst_ctx* ctx, int m_col, int m_row, const uint64_t* point, DevBuf& chis) {
  hipStream_t s = ctx->stream;
  DevBuf b;
  TPST_HIP(ctx, b.alloc((size_t)(m_col ? m_col : 1) * 32));
  if (m_col) {
    TPST_HIP(ctx, hipMemcpyAsync(b.p, point + 4 * m_row, m_col * 32, hipMemcpyHostToDevice, s));
    TPST_HIP(ctx, fr_to_mont(s, b.u(), b.u(), m_col));
  }
  TPST_HIP(ctx, chis.alloc(((size_t)1 << m_col) * 32));
  TPST_HIP(ctx, chi_table(s, b.u(), m_col, chis.u()));
  return hipStreamSynchronize(s) == hipSuccess ? TPST_OK : fail(ctx, TPST_E_HIP, "chi table");
}

static int poly_q_partial(tpst_ctx* ctx, tpst_poly* p, const uint64_t* point, size_t r0, size_t r1, void* d_out,
                          uint64_t* h_out) {
  if (!ctx || !p || !point || (!d_out && !h_out) || r1 < r0) return fail(ctx, TPST_E_ARG, "bad argument");
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  if (p->q_only) return fail(ctx, TPST_E_STATE, "opening-only handle holds no evaluations");
  for (int i = 0; i < p->n; i++)
    if (!fr_ok(point + 4 * i)) return fail(ctx, TPST_E_ARG, "point coordinate >= r");
  const uint32_t* zb;
  size_t cs;
  if (int rc = poly_rows_view(ctx, p, r0, r1, &zb, &cs)) return rc;
  DevBuf chis, tmp;
  if (int rc = chi_b_table(ctx, p->m_col, p->m_row, point, chis)) return rc;
  hipStream_t s = ctx->stream;
  const size_t N = (size_t)1 << p->m_row;
  uint32_t* dst = (uint32_t*)d_out;
  if (!dst) {
    TPST_HIP(ctx, tmp.alloc(N * 32));
    dst = tmp.u();
  }
  if (r1 > r0) {
    TPST_HIP(ctx, get_q_rows(s, zb, cs, r1 - r0, p->m_row, chis.u() + 8 * r0, dst));
  } else {
    TPST_HIP(ctx, hipMemsetAsync(dst, 0, N * 32, s));
  }
  if (h_out) TPST_HIP(ctx, hipMemcpyAsync(h_out, dst, N * 32, hipMemcpyDeviceToHost, s));
  TPST_HIP(ctx, hipStreamSynchronize(s));
  return TPST_OK;
}

extern "C" int tpst_poly_get_q_partial(tpst_ctx* ctx, tpst_poly* p, const uint64_t* point, size_t r0, size_t r1,
                                       uint64_t* zq) {
  return poly_q_partial(ctx, p, point, r0, r1, nullptr, zq);
}

extern "C" int tpst_poly_get_q_partial_dev(tpst_ctx* ctx, tpst_poly* p, const uint64_t* point, size_t r0, size_t r1,
                                           void* d_zq) {
  return poly_q_partial(ctx, p, point, r0, r1, d_zq, nullptr);
}

extern "C" int tpst_fr_sum_dev(tpst_ctx* ctx, const void* d_parts, size_t k, size_t n, void* d_out) {
  if (!ctx || (n && (!d_parts || !d_out))) return fail(ctx, TPST_E_ARG, "null argument");
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  TPST_HIP(ctx, fr_sum_parts(ctx->stream, (const uint32_t*)d_parts, k, n, (uint32_t*)d_out));
  TPST_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return TPST_OK;
}

// c_u's share: sum_{r0 <= i < r1} chi_i(b) C_i over this rank's row commitments
extern "C" int tpst_poly_cu_partial(tpst_ctx* ctx, int n, const uint64_t* point, size_t r0, size_t r1,
                                    const uint64_t* comms, uint64_t* out) {
  if (!ctx || !point || (!comms && r1 > r0) || !out || r1 < r0) return fail(ctx, TPST_E_ARG, "bad argument");
  int m_col, m_row, odd;
  if (poly_dims(n, m_col, m_row, odd)) return fail(ctx, TPST_E_ARG, "bad num_vars");
  if (r1 > ((size_t)1 << m_col)) return fail(ctx, TPST_E_ARG, "row range out of bounds");
  for (int i = 0; i < n; i++)
    if (!fr_ok(point + 4 * i)) return fail(ctx, TPST_E_ARG, "point coordinate >= r");
  std::vector<uint64_t> sc((r1 - r0) * 4 + 4);
  {
    std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
    TPST_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf chis;
    if (int rc = chi_b_table(ctx, m_col, m_row, point, chis)) return rc;
    if (r1 > r0) {
      TPST_HIP(ctx, fr_from_mont(ctx->stream, chis.u() + 8 * r0, chis.u() + 8 * r0, r1 - r0));
      TPST_HIP(ctx, hipMemcpyAsync(sc.data(), chis.u() + 8 * r0, (r1 - r0) * 32, hipMemcpyDeviceToHost, ctx->stream));
      TPST_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
  }
  if (r1 == r0) {
    memset(out, 0, 96);
    return TPST_OK;
  }
  return tpst_g1_msm(ctx, comms, r1 - r0, sc.data(), r1 - r0, out);
}

// opening-only Polynomial from the combined q (2^m_row canonical Fr, device)
// and, optionally, the combined c_u (canonical affine; NULL = the opening
// computes U = MSM(comm_list, chi(b)) itself)
extern "C" int tpst_poly_from_q_dev(tpst_ctx* ctx, int n, const uint64_t* point, const void* d_zq,
                                    const uint64_t* U, tpst_poly** out) {
  if (!ctx || !point || !d_zq || !out) return fail(ctx, TPST_E_ARG, "null argument");
  auto p = std::make_unique<tpst_poly>();
  if (poly_dims(n, p->m_col, p->m_row, p->odd)) return fail(ctx, TPST_E_ARG, "bad num_vars");
  for (int i = 0; i < n; i++)
    if (!fr_ok(point + 4 * i)) return fail(ctx, TPST_E_ARG, "point coordinate >= r");
  if (U && !point_valid<Fq>(U)) return fail(ctx, TPST_E_ARG, "c_u is not a valid G1 point");
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  p->ctx = ctx;
  p->n = n;
  p->q_only = true;
  if (int rc = chi_b_table(ctx, p->m_col, p->m_row, point, p->chis)) return rc;
  const size_t N = (size_t)1 << p->m_row;
  TPST_HIP(ctx, p->q.alloc(N * 32));
  TPST_HIP(ctx, fr_to_mont(ctx->stream, (const uint32_t*)d_zq, p->q.u(), N));
  TPST_HIP(ctx, hipStreamSynchronize(ctx->stream));
  p->has_q = true;
  if (U) {
    memcpy(p->U, U, 96);
    p->has_u = true;
  }
  *out = p.release();
  return TPST_OK;
}

// tabulate the SRS (fbt.h) for opening polynomials of parity `odd` (at SRS
// install; the open path re-checks and is a no-op then)
int tpst::srs_fbt(tpst_ctx* ctx, SrsState* st, int odd) {
  hipStream_t s = ctx->stream;
  const int nv = st->nv;
  if (!st->fbt_ready) {
    const size_t N = (size_t)1 << nv;
    TPST_HIP(ctx, st->t_pg0.alloc(fbt_words<Fq>(N) * 4));
    TPST_HIP(ctx, fbt_build<Fq>(ctx->arena, s, st->pg[0]->u(), N, st->t_pg0.u()));
    st->lvl_off.assign(nv + 1, 0);
    for (int i = 0; i < nv; i++) st->lvl_off[i + 1] = st->lvl_off[i] + ((size_t)1 << (nv - i - 1));
    const size_t tot = st->lvl_off[nv];
    TPST_HIP(ctx, st->t_pgp.alloc(fbt_words<Fq>(tot) * 4));
    TPST_HIP(ctx, st->t_php.alloc(fbt_words<Fq2>(tot) * 4));
    for (int i = 0; i < nv; i++) {
      const size_t m = (size_t)1 << (nv - i - 1);
      TPST_HIP(ctx, fbt_build<Fq>(ctx->arena, s, st->pg_pair[i]->u(), m, st->t_pgp.u() + fbt_words<Fq>(st->lvl_off[i])));
      TPST_HIP(ctx,
               fbt_build<Fq2>(ctx->arena, s, st->ph_pair[i]->u(), m, st->t_php.u() + fbt_words<Fq2>(st->lvl_off[i])));
    }
    std::vector<uint32_t> off32(st->lvl_off.begin(), st->lvl_off.end());
    TPST_HIP(ctx, st->seg.alloc(off32.size() * 4));
    TPST_HIP(ctx, hipMemcpyAsync(st->seg.p, off32.data(), off32.size() * 4, hipMemcpyHostToDevice, s));
    TPST_HIP(ctx, hipStreamSynchronize(s));
    st->fbt_ready = true;
  }
  if (!st->t_h_ready[odd]) {
    const size_t C = (size_t)1 << (nv - odd);
    TPST_HIP(ctx, st->t_h[odd].alloc(fbt_words<Fq2>(C) * 4));
    TPST_HIP(ctx, fbt_build<Fq2>(ctx->arena, s, st->ph[odd]->u(), C, st->t_h[odd].u()));
    TPST_HIP(ctx, hipStreamSynchronize(s));
    st->t_h_ready[odd] = true;
  }
  return TPST_OK;
}

// -------------------------------------------------------------- verify ---
// The verifier is a handful of short serial chains (two-term scalar
// combinations, subgroup checks) plus three pairing products and the GT
// exponentiations: the chains run on host threads (host_curve.h, ~30 ns per
// Fq product against ~1.6 us on a lone GPU lane), the pairing products in ONE
// device launch (groups padded with infinity pairs), the GT powers on a side
// stream (pairing_wave.hip k_gt_pow_wave).
static bool gt_is_one(const uint64_t* gt) {
  if (gt[0] != 1) return false;
  for (int i = 1; i < 72; i++)
    if (gt[i]) return false;
  return true;
}

static void push(std::vector<uint64_t>& v, const uint64_t* p, size_t n) { v.insert(v.end(), p, p + n); }

// pairs of one pairing-product check (canonical affine G1 12 u64, G2 24 u64)
struct PairSet {
  std::vector<uint64_t> g1, g2;
  size_t n() const { return g1.size() / 12; }
};

// prod_{pairs in group g} e(P, Q) for every group, one multi-pairing launch
// (groups padded to a common length with infinity pairs, which contribute 1)
static int pairing_groups(tpst_ctx* ctx, const std::vector<const PairSet*>& sets, std::vector<uint64_t>& gts) {
  const size_t G = sets.size();
  size_t n = 1;
  for (const PairSet* p : sets) n = std::max(n, p->n());
  std::vector<uint64_t> g1(G * n * 12, 0), g2(G * n * 24, 0);
  for (size_t g = 0; g < G; g++) {
    std::copy(sets[g]->g1.begin(), sets[g]->g1.end(), g1.begin() + g * n * 12);
    std::copy(sets[g]->g2.begin(), sets[g]->g2.end(), g2.begin() + g * n * 24);
  }
  hipStream_t s = ctx->stream;
  DevBuf a, b, f, o;
  TPST_HIP(ctx, a.alloc(G * n * 96));
  TPST_HIP(ctx, b.alloc(G * n * 192));
  TPST_HIP(ctx, f.alloc(G * sizeof(Fq12)));
  TPST_HIP(ctx, o.alloc(G * 576));
  TPST_HIP(ctx, hipMemcpyAsync(a.p, g1.data(), G * n * 96, hipMemcpyHostToDevice, s));
  TPST_HIP(ctx, hipMemcpyAsync(b.p, g2.data(), G * n * 192, hipMemcpyHostToDevice, s));
  TPST_HIP(ctx, points_to_mont<Fq>(s, a.u(), a.u(), G * n));
  TPST_HIP(ctx, points_to_mont<Fq2>(s, b.u(), b.u(), G * n));
  TPST_HIP(ctx, multi_pairing(ctx->arena, s, a.u(), b.u(), G, n, (Fq12*)f.p));
  TPST_HIP(ctx, fq12_from_mont(s, (Fq12*)f.p, o.u(), G));
  gts.assign(G * 72, 0);
  TPST_HIP(ctx, hipMemcpyAsync(gts.data(), o.p, G * 576, hipMemcpyDeviceToHost, s));
  TPST_HIP(ctx, hipStreamSynchronize(s));
  return TPST_OK;
}

// MultilinearPC::check (circuit_verifier.rs:245-314): for k points pt (LSB-first,
// canonical Fr) and k G2 proofs,
//   e(C - g^v, h) * prod_i e(g^{pt_i} - g_mask[nv - k + i], pi_i) == 1.
// A polynomial of k < ck.nv variables lives on SRS level ck.nv - k, i.e. on
// the trapdoor coordinates t[ck.nv - k ..], hence the mask offset (the same
// offset check_2 applies to h_mask, circuit_verifier.rs:214); the reference
// only checks full-level polynomials (sqrt_pst.rs:261), where it is 0.
static void mlpc_check_pairs(const SrsState* st, int k, const uint64_t* comm, const uint64_t* pt, const uint64_t* v,
                             const uint64_t* proofs, PairSet& ps) {
  const uint64_t* flat = st->flat.data();
  const uint64_t* g = flat;
  const uint64_t* h = flat + 12;
  const uint64_t* gmask = flat + tpst_srs_flat_len(st->nv) - 36 * st->nv;
  uint64_t negv[4];
  fr_out(sub(Fr::zero(), fr_canon(v)), negv);
  ps.g1.assign((size_t)(k + 1) * 12, 0);
  ps.g2.clear();
  push(ps.g2, h, 24);
  for (int i = 0; i < k; i++) push(ps.g2, proofs + 24 * i, 24);
  host::parallel_for((size_t)k + 1, [&](size_t i) {
    if (i == 0)
      host::mul_add<Fq>(g, negv, comm, 1, &ps.g1[0]);  // C - g^v
    else
      host::mul_add<Fq>(g, pt + 4 * (i - 1), gmask + 12 * (st->nv - k + i - 1), -1, &ps.g1[12 * i]);
  });
}

// check_2 (circuit_verifier.rs:175-243; mipp.rs:307): G2 commitment C_h, k G1
// proofs,  e(g, C_h - h^v) * prod_i e(pi_i, h^{pt_i} - h_mask[nv - k + i]) == 1
static void mlpc_check2_pairs(const SrsState* st, int k, const uint64_t* comm_h, const uint64_t* pt,
                              const uint64_t* v, const uint64_t* proofs, PairSet& ps) {
  const uint64_t* flat = st->flat.data();
  const uint64_t* g = flat;
  const uint64_t* h = flat + 12;
  const uint64_t* hmask = flat + tpst_srs_flat_len(st->nv) - 24 * st->nv;
  uint64_t negv[4];
  fr_out(sub(Fr::zero(), fr_canon(v)), negv);
  ps.g1.clear();
  push(ps.g1, g, 12);
  for (int i = 0; i < k; i++) push(ps.g1, proofs + 12 * i, 12);
  ps.g2.assign((size_t)(k + 1) * 24, 0);
  host::parallel_for((size_t)k + 1, [&](size_t i) {
    if (i == 0)
      host::mul_add<Fq2>(h, negv, comm_h, 1, &ps.g2[0]);  // C_h - h^v
    else
      host::mul_add<Fq2>(h, pt + 4 * (i - 1), hmask + 24 * (st->nv - k + i - 1), -1, &ps.g2[24 * i]);
  });
}

static int mlpc_check_impl(tpst_ctx* ctx, SrsState* st, int k, const uint64_t* comm, const uint64_t* pt,
                           const uint64_t* v, const uint64_t* proofs) {
  PairSet ps;
  mlpc_check_pairs(st, k, comm, pt, v, proofs, ps);
  std::vector<uint64_t> gt;
  if (int rc = pairing_groups(ctx, {&ps}, gt)) return rc;
  return gt_is_one(gt.data()) ? TPST_OK : TPST_E_VERIFY;
}

static int mlpc_check2_impl(tpst_ctx* ctx, SrsState* st, int k, const uint64_t* comm_h, const uint64_t* pt,
                            const uint64_t* v, const uint64_t* proofs) {
  PairSet ps;
  mlpc_check2_pairs(st, k, comm_h, pt, v, proofs, ps);
  std::vector<uint64_t> gt;
  if (int rc = pairing_groups(ctx, {&ps}, gt)) return rc;
  return gt_is_one(gt.data()) ? TPST_OK : TPST_E_VERIFY;
}

// ------------------------------------------------- MultilinearPC calls ---
// Single-call forms of the ark-poly-commit fork's MultilinearPC<E> used by the
// reference: commit (sqrt_pst.rs:124), commit_g2
// (mipp.rs:133), open (sqrt_pst.rs:225), open_g1 (mipp.rs:144), check
// (sqrt_pst.rs:261), check_2 (mipp.rs:307).  A polynomial of nv variables uses
// SRS level ck.nv - nv (the variable-CRS offset); points are LSB-first as
// MultilinearPC takes them; values canonical.
static int mlpc_args(tpst_ctx* ctx, SrsState* st, int nv) {
  if (!st) return fail(ctx, TPST_E_STATE, "no SRS loaded");
  if (nv < 0 || nv > st->nv) return fail(ctx, TPST_E_ARG, "num_vars > SRS num_vars");
  return TPST_OK;
}

template <class F>
static int mlpc_commit_impl(tpst_ctx* ctx, const uint64_t* evals, int nv, uint64_t* out) {
  if (!ctx || !evals || !out) return fail(ctx, TPST_E_ARG, "null argument");
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  SrsState* st = srs_of(ctx);
  int rc = mlpc_args(ctx, st, nv);
  if (rc) return rc;
  const size_t n = (size_t)1 << nv;
  const int lvl = st->nv - nv;
  constexpr size_t PW = 2 * Words<F>::n;
  const uint32_t* bases;
  if (lvl < st->nv) {
    bases = (sizeof(F) == sizeof(Fq) ? st->pg[lvl] : st->ph[lvl])->u();
  } else {  // nv = 0: the level of one base is g (h), the constant polynomial
    bases = (sizeof(F) == sizeof(Fq) ? st->g : st->h).u();
  }
  hipStream_t s = ctx->stream;
  DevBuf sc, r, o;
  TPST_HIP(ctx, sc.alloc(n * 32));
  TPST_HIP(ctx, r.alloc(sizeof(Xyzz<F>)));
  TPST_HIP(ctx, o.alloc(PW * 4));
  TPST_HIP(ctx, hipMemcpyAsync(sc.p, evals, n * 32, hipMemcpyHostToDevice, s));
  TPST_HIP(ctx, msm_var<F>(ctx->arena, s, bases, sc.u(), n, (Xyzz<F>*)r.p));
  TPST_HIP(ctx, xyzz_to_affine_canonical<F>(s, (Xyzz<F>*)r.p, o.u(), 1));
  TPST_HIP(ctx, hipMemcpyAsync(out, o.p, PW * 4, hipMemcpyDeviceToHost, s));
  TPST_HIP(ctx, hipStreamSynchronize(s));
  return TPST_OK;
}

extern "C" int tpst_mlpc_commit(tpst_ctx* ctx, const uint64_t* evals, int nv, uint64_t* g_product) {
  return mlpc_commit_impl<Fq>(ctx, evals, nv, g_product);
}

extern "C" int tpst_mlpc_commit_g2(tpst_ctx* ctx, const uint64_t* evals, int nv, uint64_t* h_product) {
  return mlpc_commit_impl<Fq2>(ctx, evals, nv, h_product);
}

template <class F>
static int mlpc_open_impl(tpst_ctx* ctx, const uint64_t* evals, int nv, const uint64_t* point, uint64_t* proofs) {
  if (!ctx || !evals || !point || !proofs) return fail(ctx, TPST_E_ARG, "null argument");
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  SrsState* st = srs_of(ctx);
  int rc = mlpc_args(ctx, st, nv);
  if (rc) return rc;
  if (nv == 0) return TPST_OK;  // no quotients
  for (int i = 0; i < nv; i++)
    if (!fr_ok(point + 4 * i)) return fail(ctx, TPST_E_ARG, "point coordinate >= r");
  const size_t n = (size_t)1 << nv;
  constexpr size_t PW = 2 * Words<F>::n;
  hipStream_t s = ctx->stream;
  DevBuf ev, pt, r, o;
  TPST_HIP(ctx, ev.alloc(n * 32));
  TPST_HIP(ctx, pt.alloc(nv * 32));
  TPST_HIP(ctx, r.alloc(nv * sizeof(Xyzz<F>)));
  TPST_HIP(ctx, o.alloc(nv * PW * 4));
  TPST_HIP(ctx, hipMemcpyAsync(ev.p, evals, n * 32, hipMemcpyHostToDevice, s));
  TPST_HIP(ctx, hipMemcpyAsync(pt.p, point, nv * 32, hipMemcpyHostToDevice, s));
  TPST_HIP(ctx, fr_to_mont(s, ev.u(), ev.u(), n));
  TPST_HIP(ctx, fr_to_mont(s, pt.u(), pt.u(), nv));
  const uint32_t* table = sizeof(F) == sizeof(Fq) ? st->t_pgp.u() : st->t_php.u();
  rc = pst_open_fbt<F>(ctx, st, table, st->nv - nv, ev.u(), nv, pt.u(), (Xyzz<F>*)r.p);
  if (rc) return rc;
  TPST_HIP(ctx, xyzz_to_affine_canonical<F>(s, (Xyzz<F>*)r.p, o.u(), nv));
  TPST_HIP(ctx, hipMemcpyAsync(proofs, o.p, nv * PW * 4, hipMemcpyDeviceToHost, s));
  TPST_HIP(ctx, hipStreamSynchronize(s));
  return TPST_OK;
}

extern "C" int tpst_mlpc_open(tpst_ctx* ctx, const uint64_t* evals, int nv, const uint64_t* point,
                              uint64_t* proofs) {
  return mlpc_open_impl<Fq2>(ctx, evals, nv, point, proofs);
}

extern "C" int tpst_mlpc_open_g1(tpst_ctx* ctx, const uint64_t* evals, int nv, const uint64_t* point,
                                 uint64_t* proofs) {
  return mlpc_open_impl<Fq>(ctx, evals, nv, point, proofs);
}

extern "C" int tpst_mlpc_check(tpst_ctx* ctx, int nv, const uint64_t* comm, const uint64_t* point,
                               const uint64_t* value, const uint64_t* proofs) {
  if (!ctx || !comm || !point || !value || (nv && !proofs)) return fail(ctx, TPST_E_ARG, "null argument");
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  SrsState* st = srs_of(ctx);
  int rc = mlpc_args(ctx, st, nv);
  if (rc) return rc;
  if (!fr_ok(value) || !point_valid<Fq>(comm)) return fail(ctx, TPST_E_VERIFY, "malformed input");
  for (int i = 0; i < nv; i++)
    if (!fr_ok(point + 4 * i) || !point_valid<Fq2>(proofs + 24 * i)) return fail(ctx, TPST_E_VERIFY, "malformed input");
  return mlpc_check_impl(ctx, st, nv, comm, point, value, proofs);
}

extern "C" int tpst_mlpc_check_2(tpst_ctx* ctx, int nv, const uint64_t* comm_h, const uint64_t* point,
                                 const uint64_t* value, const uint64_t* proofs) {
  if (!ctx || !comm_h || !point || !value || (nv && !proofs)) return fail(ctx, TPST_E_ARG, "null argument");
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  SrsState* st = srs_of(ctx);
  int rc = mlpc_args(ctx, st, nv);
  if (rc) return rc;
  if (!fr_ok(value) || !point_valid<Fq2>(comm_h)) return fail(ctx, TPST_E_VERIFY, "malformed input");
  for (int i = 0; i < nv; i++)
    if (!fr_ok(point + 4 * i) || !point_valid<Fq>(proofs + 12 * i)) return fail(ctx, TPST_E_VERIFY, "malformed input");
  return mlpc_check2_impl(ctx, st, nv, comm_h, point, value, proofs);
}

// Every proof element is validated before the transcript absorbs it (a
// non-canonical encoding of a point would otherwise change the Fiat-Shamir
// challenges without changing the point): Fq limbs < p, points on the curve
// and in the r-torsion (host threads), GT coefficients < p (GT membership of
// comms_t is tested on the device with its exponentiation), scalars < r.
static bool proof_valid(const tpst_open_proof* pr, int n, const uint64_t* point, const uint64_t* v,
                        const uint64_t* T) {
  for (int i = 0; i < n; i++)
    if (!fr_ok(point + 4 * i)) return false;
  if (!fr_ok(v) || !gt_ok(T)) return false;
  for (int i = 0; i < pr->m_col; i++)
    if (!gt_ok(pr->comms_t[i][0]) || !gt_ok(pr->comms_t[i][1])) return false;
  std::vector<const uint64_t*> g1 = {pr->U, pr->final_a}, g2 = {pr->final_h};
  for (int i = 0; i < pr->m_col; i++) {
    g1.push_back(pr->comms_u[i][0]);
    g1.push_back(pr->comms_u[i][1]);
    g1.push_back(pr->pst_proof_h[i]);
  }
  for (int i = 0; i < pr->m_row; i++) g2.push_back(pr->pst_proof[i]);
  std::atomic<bool> ok(true);
  host::parallel_for(g1.size() + g2.size(), [&](size_t t) {
    if (!ok.load(std::memory_order_relaxed)) return;
    const bool good = t < g2.size() ? point_valid<Fq2>(g2[t]) : point_valid<Fq>(g1[t - g2.size()]);
    if (!good) ok.store(false);
  });
  return ok.load();
}

// Polynomial::verify (sqrt_pst.rs:232-264) with MippProof::verify (mipp.rs:182-320)
extern "C" int tpst_pst_verify(tpst_ctx* ctx, tpst_transcript* tr, int n, const uint64_t* point, const uint64_t* v,
                               const uint64_t* T, const tpst_open_proof* proof) {
  if (!ctx || !tr || !point || !v || !T || !proof) return fail(ctx, TPST_E_ARG, "null argument");
  int m_col, m_row, odd;
  if (poly_dims(n, m_col, m_row, odd)) return fail(ctx, TPST_E_ARG, "bad num_vars");
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  SrsState* st = srs_of(ctx);
  if (!st) return fail(ctx, TPST_E_STATE, "no SRS loaded");
  if (st->nv != m_row || proof->m_col != m_col || proof->m_row != m_row) return fail(ctx, TPST_E_ARG, "size mismatch");
  if (!proof_valid(proof, n, point, v, T)) return fail(ctx, TPST_E_VERIFY, "malformed proof element (non-canonical, off-curve or outside the subgroup)");
  const int m = m_col;
  Sponge sp;
  sp.load(tr);
  uint8_t b[96];
  g1_bytes(proof->U, b);
  sp.absorb_bytes(b, 96);
  std::vector<Fr> xs(m), xs_inv(m);
  Fr final_y = Fr::one();
  for (int i = 0; i < m; i++) {  // mipp.rs:207-227
    g1_bytes(proof->comms_u[i][0], b);
    sp.absorb_bytes(b, 96);
    g1_bytes(proof->comms_u[i][1], b);
    sp.absorb_bytes(b, 96);
    sp.absorb_bytes((const uint8_t*)proof->comms_t[i][0], 576);
    sp.absorb_bytes((const uint8_t*)proof->comms_t[i][1], 576);
    uint64_t cc[4];
    sp.challenge(cc);
    xs_inv[i] = fr_canon(cc);
    xs[i] = fr_inv(xs_inv[i]);
    const Fr bi = fr_canon(point + 4 * (m_row + i));
    final_y = mul(final_y, sub(add(Fr::one(), mul(xs_inv[i], bi)), bi));
  }
  std::vector<Fr> rs(m);
  for (int i = 0; i < m; i++) {
    uint64_t cc[4];
    sp.challenge(cc);
    rs[i] = fr_canon(cc);
  }
  Fr vh = Fr::one();
  for (int i = 0; i < m; i++) vh = mul(vh, sub(add(Fr::one(), mul(rs[i], xs_inv[m - i - 1])), rs[i]));
  auto canon4 = [](const Fr& x) {
    std::vector<uint64_t> c(4);
    fr_out(x, c.data());
    return c;
  };
  // T check, device side first (side stream): t_l^{c_inv}, t_r^{c} for every
  // round after a GT membership test of each (mipp.rs:263-283)
  const size_t k = 2 * (size_t)m;
  if (int rc = open_streams(ctx, 8, k * (sizeof(Fq12) + 4))) return rc;
  hipStream_t s2 = ctx->side[0];
  DevBuf db, de, dout, dok;
  // the powers and flags come back into the context's pinned staging (a true
  // async copy); every return path below drains s2 first (the guard is
  // destroyed before the device buffers the copies read)
  Fq12* pw = reinterpret_cast<Fq12*>(ctx->pinned);
  uint32_t* okv = reinterpret_cast<uint32_t*>(pw + k);
  struct Drain {
    hipStream_t s;
    ~Drain() { (void)hipStreamSynchronize(s); }
  } drain{s2};
  if (k) {
    std::vector<uint32_t> bases;
    std::vector<uint64_t> dg(4 * k);
    for (int i = 0; i < m; i++) {
      for (int j = 0; j < 2; j++) {
        Fq12 f;
        Fq* c = reinterpret_cast<Fq*>(&f);
        for (int q = 0; q < 12; q++) c[q] = fq_canon(proof->comms_t[i][j] + 6 * q);
        const uint32_t* fw = reinterpret_cast<const uint32_t*>(&f);
        bases.insert(bases.end(), fw, fw + sizeof(Fq12) / 4);
        uint64_t e4[4];  // base-x digits of the exponent (e < r < x^4)
        fr_out(j == 0 ? xs_inv[i] : xs[i], e4);
        base_x_digits(e4, &dg[4 * (2 * i + j)]);
      }
    }
    TPST_HIP(ctx, db.alloc(k * sizeof(Fq12)));
    TPST_HIP(ctx, de.alloc(k * 32));
    TPST_HIP(ctx, dout.alloc(k * sizeof(Fq12)));
    TPST_HIP(ctx, dok.alloc(k * 4));
    TPST_HIP(ctx, hipMemcpyAsync(db.p, bases.data(), k * sizeof(Fq12), hipMemcpyHostToDevice, s2));
    TPST_HIP(ctx, hipMemcpyAsync(de.p, dg.data(), k * 32, hipMemcpyHostToDevice, s2));
    TPST_HIP(ctx, gt_pow_wave(s2, (const Fq12*)db.p, (const uint64_t*)de.p, k, (Fq12*)dout.p, dok.u()));
    TPST_HIP(ctx, hipMemcpyAsync(pw, dout.p, k * sizeof(Fq12), hipMemcpyDeviceToHost, s2));
    TPST_HIP(ctx, hipMemcpyAsync(okv, dok.p, k * 4, hipMemcpyDeviceToHost, s2));
  }
  // host threads meanwhile: the U check's terms and the check / check_2 pairs
  // U check: uc = U + sum(c_inv u_l + c u_r) == final_y * final_a (mipp.rs:239-251)
  std::vector<Xyzz<host::HFq>> terms(2 * (size_t)m + 1);
  std::vector<std::vector<uint64_t>> tsc(2 * (size_t)m + 1);
  for (int i = 0; i < m; i++) {
    tsc[2 * i] = canon4(xs_inv[i]);
    tsc[2 * i + 1] = canon4(xs[i]);
  }
  tsc[2 * m] = canon4(sub(Fr::zero(), final_y));
  PairSet chk2, chk;
  {
    std::vector<uint64_t> rsc(4 * (size_t)m);
    for (int i = 0; i < m; i++) fr_out(rs[i], &rsc[4 * i]);
    uint64_t vhc[4];
    fr_out(vh, vhc);
    std::vector<uint64_t> arev(4 * (size_t)m_row);
    for (int i = 0; i < m_row; i++) memcpy(&arev[4 * i], point + 4 * (m_row - 1 - i), 32);
    host::parallel_for(terms.size(), [&](size_t t) {
      const uint64_t* P = t == 2 * (size_t)m ? proof->final_a : proof->comms_u[t / 2][t % 2];
      terms[t] = scalar_mul(host::aff_in<host::HFq>(P), reinterpret_cast<const uint32_t*>(tsc[t].data()), 253);
    });
    mlpc_check2_pairs(st, m, proof->final_h, rsc.data(), vhc, &proof->pst_proof_h[0][0], chk2);  // mipp.rs:307
    mlpc_check_pairs(st, m_row, proof->U, arev.data(), v, &proof->pst_proof[0][0], chk);         // sqrt_pst.rs:261
  }
  Xyzz<host::HFq> uc = to_xyzz(host::aff_in<host::HFq>(proof->U));
  for (auto& t : terms) uc = add(uc, t);
  if (!is_inf(uc)) return TPST_E_VERIFY;
  // the three pairing products in one launch: e(final_a, final_h), check_2, check
  PairSet fin;
  push(fin.g1, proof->final_a, 12);
  push(fin.g2, proof->final_h, 24);
  std::vector<uint64_t> gts;
  if (int rc = pairing_groups(ctx, {&fin, &chk2, &chk}, gts)) return rc;
  TPST_HIP(ctx, hipStreamSynchronize(s2));
  for (size_t i = 0; i < k; i++)
    if (!okv[i]) return fail(ctx, TPST_E_VERIFY, "comms_t element outside GT");
  // T * prod t_l^{c_inv} t_r^{c} == e(final_a, final_h)
  Fq12 acc;
  {
    Fq* c = reinterpret_cast<Fq*>(&acc);
    for (int q = 0; q < 12; q++) c[q] = fq_canon(T + 6 * q);
  }
  for (size_t i = 0; i < k; i++) acc = mul(acc, pw[i]);
  {
    const Fq* c = reinterpret_cast<const Fq*>(&acc);
    for (int q = 0; q < 12; q++) {
      uint64_t lim[6];
      fq_out(c[q], lim);
      if (memcmp(lim, gts.data() + 6 * q, 48) != 0) return TPST_E_VERIFY;
    }
  }
  if (!gt_is_one(gts.data() + 72) || !gt_is_one(gts.data() + 144)) return TPST_E_VERIFY;
  sp.store(tr);
  return TPST_OK;
}
