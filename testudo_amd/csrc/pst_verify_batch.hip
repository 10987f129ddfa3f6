// tpst_pst_verify_batch (include/tpst.h): B sqrt-PST openings against one
// SRS, checked by one combined equation.
//
// tpst_pst_verify (pst_api.hip) checks, per opening,
//   (A) T prod_l t_l^{1/x_l} t_r^{x_l} = e(final_a, final_h)              (mipp.rs:263-283)
//   (B) e(g, final_h - v_h h) prod_{i<m_col} e(pi^h_i, r_i h - hmask_i) = 1   (check_2, mipp.rs:307)
//   (C) e(U - v g, h) prod_{i<m_row} e(a_i g - gmask_i, pi_i) = 1             (check, sqrt_pst.rs:261)
//   (D) U + sum_l (u_l / x_l + x_l u_r) - final_y final_a = O             (mipp.rs:239-251)
// with three final exponentiations, ~3 m_col + m_row + 3 host scalar
// multiplications and a stream synchronisation.  All four are equations in
// groups of prime order r, so for multipliers rho_T, rho_2, rho_1, rho_U
// drawn after the proofs are fixed, the B openings hold (up to 2^-128) iff
//   prod_j [ e(rho_T final_a, final_h) (B_j)^{rho_2} (C_j)^{rho_1} ] = prod_j (T_j prod t_l^{..} t_r^{..})^{rho_T}
//   sum_j rho_U (D_j) = O.
// The left side is ONE multi-pairing with one final exponentiation over
// B (3 + m_col + m_row) pairs, every scaled point of which comes out of
// k_lincomb2 (lincomb.hip); the right side one gt_pow_wave launch over
// B (2 m_col + 1) bases (which also tests their GT membership) and a host
// product; the second line one msm_var over B (2 m_col + 2) points.
//
// Pair order (block-wise, so that every lincomb launch writes a contiguous
// range of the pairing's inputs; V = the items that go into the check):
//   G1: [rho_2 pi^h_{j,i}] [rho_T final_a_j] [rho_1 (U_j - v_j g), (rho_1 a_i) g - rho_1 gmask_i] [g]
//   G2: [r_{j,i} h - hmask_i] [final_h_j]    [h, pi_{j,i}]                                        [rho_2 (final_h_j - v_h,j h)]
//
// On failure the per-item verdicts come from bisection over the same check
// (the subset's points are rebuilt: the failure path only).
#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/tpst.h"
#include "ctx.h"
#include "device_util.h"
#include "host_curve.h"
#include "lincomb.h"
#include "point_codec.h"
#include "poseidon_host.h"
#include "pst_kernels.h"
#include "pst_state.h"

using namespace tpst;

namespace {

// (x, -y) of a canonical affine point (NQ Fq coefficients per coordinate); infinity stays all-zero
template <int NQ>
void neg_point(const uint64_t* p, uint64_t* o) {
  memcpy(o, p, 48 * NQ);
  for (int q = 0; q < NQ; q++) {
    const uint64_t* y = p + 6 * (NQ + q);
    uint64_t* d = o + 6 * (NQ + q);
    bool zero = true;
    for (int i = 0; i < 6; i++) zero = zero && !y[i];
    unsigned __int128 br = 0;
    for (int i = 0; i < 6; i++) {
      const uint64_t pi = (uint64_t)params::FQ_P[2 * i] | ((uint64_t)params::FQ_P[2 * i + 1] << 32);
      const unsigned __int128 t = (unsigned __int128)pi - y[i] - (uint64_t)br;
      d[i] = zero ? 0 : (uint64_t)t;
      br = (t >> 64) & 1;
    }
  }
}

Fq12 gt_mont(const uint64_t* c72) {  // canonical GT -> Montgomery Fq12
  Fq12 f;
  Fq* c = reinterpret_cast<Fq*>(&f);
  for (int q = 0; q < 12; q++) c[q] = fq_canon(c72 + 6 * q);
  return f;
}

void push(std::vector<uint64_t>& v, const uint64_t* p, size_t n) { v.insert(v.end(), p, p + n); }
void push_fr(std::vector<uint64_t>& v, const Fr& x) {
  uint64_t c[4];
  fr_out(x, c);
  v.insert(v.end(), c, c + 4);
}

// what the transcript replay of one item yields (tpst_pst_verify, pst_api.hip)
struct Replay {
  Sponge sp;  // the item's end state, stored to its tr once it is accepted
  std::vector<Fr> xs, xs_inv, rs;
  Fr final_y, vh;
  Fr rT, r2, r1, rU;  // the item's multipliers
  Fq12 R;             // (T prod t_l^{1/x} t_r^{x})^{rho_T}, from the GT powers
};

void replay(const tpst_verify_item& it, int m, int m_row, Replay& o) {
  const tpst_open_proof* pr = it.proof;
  o.sp.load(it.tr);
  uint8_t b[96];
  g1_bytes(pr->U, b);
  o.sp.absorb_bytes(b, 96);
  o.xs.resize(m);
  o.xs_inv.resize(m);
  o.rs.resize(m);
  o.final_y = Fr::one();
  for (int i = 0; i < m; i++) {  // mipp.rs:207-227
    g1_bytes(pr->comms_u[i][0], b);
    o.sp.absorb_bytes(b, 96);
    g1_bytes(pr->comms_u[i][1], b);
    o.sp.absorb_bytes(b, 96);
    o.sp.absorb_bytes((const uint8_t*)pr->comms_t[i][0], 576);
    o.sp.absorb_bytes((const uint8_t*)pr->comms_t[i][1], 576);
    uint64_t cc[4];
    o.sp.challenge(cc);
    o.xs_inv[i] = fr_canon(cc);
    o.xs[i] = inv(o.xs_inv[i]);
    const Fr bi = fr_canon(it.point + 4 * (m_row + i));
    o.final_y = mul(o.final_y, sub(add(Fr::one(), mul(o.xs_inv[i], bi)), bi));
  }
  for (int i = 0; i < m; i++) {
    uint64_t cc[4];
    o.sp.challenge(cc);
    o.rs[i] = fr_canon(cc);
  }
  o.vh = Fr::one();
  for (int i = 0; i < m; i++) o.vh = mul(o.vh, sub(add(Fr::one(), mul(o.rs[i], o.xs_inv[m - i - 1])), o.rs[i]));
}

// device buffers of one call, carved from ctx->io before the first launch
struct Bufs {
  uint32_t *g1in, *g2in, *sc, *pg1, *pg2, *fo;
  Xyzz<Fq>*x1, *usum;
  Xyzz<Fq2>* x2;
  Fq12 *f, *gb, *gout;
  uint64_t* ge;
  uint32_t* gok;
};

struct Batch {
  tpst_ctx* ctx;
  SrsState* st;
  const tpst_verify_item* items;
  int m, m_row;
  std::vector<Replay> rp;
  std::vector<uint64_t> ng, nh, ngmask, nhmask;  // -g, -h, -gmask_i, -hmask_i (canonical)
  Bufs d;
  uint8_t* pin;  // pinned: [GT powers | flags | pairing value 576 B | U sum 192 B]
  size_t K;      // GT bases of the call
};

// offset of the pairing value in the pinned staging, behind K GT powers and their flags
size_t pin_gt_off(size_t K) { return (K * (sizeof(Fq12) + 4) + 63) & ~(size_t)63; }

// the combined check over the items S, device side: everything is queued on the context stream, nothing waits
int enqueue_check(Batch& b, const std::vector<size_t>& S) {
  tpst_ctx* ctx = b.ctx;
  const int m = b.m, mr = b.m_row;
  const size_t Bv = S.size();
  const size_t n1s = Bv * (m + 1), n1l = Bv * (1 + mr), n2 = Bv * (m + 1), nu = Bv * (2 * m + 2);
  const size_t NP = Bv * (3 + m + mr);
  const uint64_t* flat = b.st->flat.data();
  const uint64_t *g = flat, *h = flat + 12;
  // ---- host: the points and scalars of the three lincomb launches, the U check and the direct pairs
  std::vector<uint64_t> g1, g2, sc, dir1, dir2;
  g1.reserve((n1s + 2 * n1l + nu) * 12);
  g2.reserve(2 * n2 * 24);
  sc.reserve((n1s + 2 * n1l + 2 * n2 + nu) * 4);
  // G1 short, one scalar of 128 bits: [rho_2 pi^h_{j,i}] then [rho_T final_a_j]
  for (size_t j : S)
    for (int i = 0; i < m; i++) {
      push(g1, b.items[j].proof->pst_proof_h[i], 12);
      push_fr(sc, b.rp[j].r2);
    }
  for (size_t j : S) {
    push(g1, b.items[j].proof->final_a, 12);
    push_fr(sc, b.rp[j].rT);
  }
  // G1 long: rho_1 U + (rho_1 v)(-g); (rho_1 a_i) g + rho_1 (-gmask_i), a_i the reversed point (pst_api.hip:1293)
  for (size_t j : S) {
    push(g1, b.items[j].proof->U, 12);
    push_fr(sc, b.rp[j].r1);
    for (int i = 0; i < mr; i++) {
      push(g1, g, 12);
      push_fr(sc, mul(b.rp[j].r1, fr_canon(b.items[j].point + 4 * (mr - 1 - i))));
    }
  }
  for (size_t j : S) {
    push(g1, b.ng.data(), 12);
    push_fr(sc, mul(b.rp[j].r1, fr_canon(b.items[j].v)));
    for (int i = 0; i < mr; i++) {
      push(g1, &b.ngmask[12 * i], 12);
      push_fr(sc, b.rp[j].r1);
    }
  }
  // G2: r_{j,i} h + 1 (-hmask_{nv - m + i}) then rho_2 final_h + (rho_2 v_h)(-h)
  const uint64_t one4[4] = {1, 0, 0, 0};
  for (size_t j : S)
    for (int i = 0; i < m; i++) {
      push(g2, h, 24);
      push_fr(sc, b.rp[j].rs[i]);
    }
  for (size_t j : S) {
    push(g2, b.items[j].proof->final_h, 24);
    push_fr(sc, b.rp[j].r2);
  }
  for (size_t j : S)
    for (int i = 0; i < m; i++) {
      push(g2, &b.nhmask[24 * (b.st->nv - m + i)], 24);
      push(sc, one4, 4);
    }
  for (size_t j : S) {
    push(g2, b.nh.data(), 24);
    push_fr(sc, mul(b.rp[j].r2, b.rp[j].vh));
  }
  // U check: rho_U U, (rho_U / x) u_l, (rho_U x) u_r, (-rho_U final_y) final_a
  for (size_t j : S) {
    const tpst_open_proof* pr = b.items[j].proof;
    const Replay& r = b.rp[j];
    push(g1, pr->U, 12);
    push_fr(sc, r.rU);
    for (int i = 0; i < m; i++) {
      push(g1, pr->comms_u[i][0], 12);
      push_fr(sc, mul(r.rU, r.xs_inv[i]));
      push(g1, pr->comms_u[i][1], 12);
      push_fr(sc, mul(r.rU, r.xs[i]));
    }
    push(g1, pr->final_a, 12);
    push_fr(sc, sub(Fr::zero(), mul(r.rU, r.final_y)));
  }
  // pairs that take a proof or SRS point as it is: G1 [g] x Bv; G2 [final_h_j] [h, pi_{j,i}]
  for (size_t j = 0; j < Bv; j++) push(dir1, g, 12);
  for (size_t j : S) push(dir2, b.items[j].proof->final_h, 24);
  for (size_t j : S) {
    push(dir2, h, 24);
    for (int i = 0; i < mr; i++) push(dir2, b.items[j].proof->pst_proof[i], 24);
  }
  // ---- device
  hipStream_t s = ctx->stream;
  const Bufs& d = b.d;
  uint32_t* pg1_dir = d.pg1 + (n1s + n1l) * 24;
  uint32_t* pg2_dir = d.pg2 + (size_t)Bv * m * 48;
  uint32_t* pg2_c = d.pg2 + (NP - Bv) * 48;
  TPST_HIP(ctx, hipMemcpyAsync(d.g1in, g1.data(), g1.size() * 8, hipMemcpyHostToDevice, s));
  TPST_HIP(ctx, hipMemcpyAsync(d.g2in, g2.data(), g2.size() * 8, hipMemcpyHostToDevice, s));
  TPST_HIP(ctx, hipMemcpyAsync(d.sc, sc.data(), sc.size() * 8, hipMemcpyHostToDevice, s));
  TPST_HIP(ctx, hipMemcpyAsync(pg1_dir, dir1.data(), dir1.size() * 8, hipMemcpyHostToDevice, s));
  TPST_HIP(ctx, hipMemcpyAsync(pg2_dir, dir2.data(), dir2.size() * 8, hipMemcpyHostToDevice, s));
  TPST_HIP(ctx, points_to_mont<Fq>(s, d.g1in, d.g1in, n1s + 2 * n1l + nu));
  TPST_HIP(ctx, points_to_mont<Fq2>(s, d.g2in, d.g2in, 2 * n2));
  TPST_HIP(ctx, points_to_mont<Fq>(s, pg1_dir, pg1_dir, Bv));
  TPST_HIP(ctx, points_to_mont<Fq2>(s, pg2_dir, pg2_dir, Bv * (2 + mr)));
  const uint32_t* sc_short = d.sc;
  const uint32_t* sc_ls = sc_short + n1s * 8;
  const uint32_t* sc_lt = sc_ls + n1l * 8;
  const uint32_t* sc_2s = sc_lt + n1l * 8;
  const uint32_t* sc_2t = sc_2s + n2 * 8;
  const uint32_t* sc_u = sc_2t + n2 * 8;
  const uint32_t* p_short = d.g1in;
  const uint32_t* p_lp = p_short + n1s * 24;
  const uint32_t* p_lq = p_lp + n1l * 24;
  const uint32_t* p_u = p_lq + n1l * 24;
  // the U check first: msm_var sizes its own scratch (ctx->arena)
  TPST_HIP(ctx, msm_var<Fq>(ctx->arena, s, p_u, sc_u, nu, d.usum));
  ctx->prof.begin(ST_LINCOMB, s);
  TPST_HIP(ctx, lincomb2<Fq>(s, p_short, sc_short, nullptr, nullptr, n1s, 128, d.x1));
  TPST_HIP(ctx, lincomb2<Fq>(s, p_lp, sc_ls, p_lq, sc_lt, n1l, 253, d.x1 + n1s));
  TPST_HIP(ctx, lincomb2<Fq2>(s, d.g2in, sc_2s, d.g2in + n2 * 48, sc_2t, n2, 253, d.x2));
  ctx->prof.end(ST_LINCOMB, s);
  TPST_HIP(ctx, xyzz_to_affine_mont<Fq>(s, d.x1, d.pg1, n1s + n1l));
  TPST_HIP(ctx, xyzz_to_affine_mont<Fq2>(s, d.x2, d.pg2, (size_t)Bv * m));
  TPST_HIP(ctx, xyzz_to_affine_mont<Fq2>(s, d.x2 + (size_t)Bv * m, pg2_c, Bv));
  ctx->prof.begin(ST_VERIFY_BATCH_PAIRING, s);
  TPST_HIP(ctx, multi_pairing(ctx->arena2, s, d.pg1, d.pg2, 1, NP, d.f));
  ctx->prof.end(ST_VERIFY_BATCH_PAIRING, s);
  TPST_HIP(ctx, fq12_from_mont(s, d.f, d.fo, 1));
  uint8_t* pin_gt = b.pin + pin_gt_off(b.K);
  TPST_HIP(ctx, hipMemcpyAsync(pin_gt, d.fo, 576, hipMemcpyDeviceToHost, s));
  TPST_HIP(ctx, hipMemcpyAsync(pin_gt + 576, d.usum, sizeof(Xyzz<Fq>), hipMemcpyDeviceToHost, s));
  return TPST_OK;
}

// ... and its verdict: *pass = the pairing value equals prod_j R_j and the U sum is infinity
int finish_check(Batch& b, const std::vector<size_t>& S, bool* pass) {
  tpst_ctx* ctx = b.ctx;
  const uint8_t* pin_gt = b.pin + pin_gt_off(b.K);
  Fq12 R = Fq12::one();
  for (size_t j : S) R = mul(R, b.rp[j].R);
  TPST_HIP(ctx, hipStreamSynchronize(ctx->stream));
  bool ok = true;
  const uint64_t* zz = reinterpret_cast<const uint64_t*>(pin_gt + 576) + 12;  // ZZ of the U sum
  for (int i = 0; i < 6; i++) ok = ok && zz[i] == 0;
  const Fq* c = reinterpret_cast<const Fq*>(&R);
  for (int q = 0; q < 12 && ok; q++) {
    uint64_t lim[6];
    fq_out(c[q], lim);
    ok = memcmp(lim, pin_gt + 48 * q, 48) == 0;
  }
  *pass = ok;
  return TPST_OK;
}

int run_check(Batch& b, const std::vector<size_t>& S, bool* pass) {
  if (int rc = enqueue_check(b, S)) return rc;
  return finish_check(b, S, pass);
}

// verdicts of the items S by bisection; known_bad: the check over S is known to fail
int solve(Batch& b, const std::vector<size_t>& S, bool known_bad, std::vector<uint8_t>& good) {
  if (S.empty()) return TPST_OK;
  if (!known_bad) {
    bool pass = false;
    if (int rc = run_check(b, S, &pass)) return rc;
    if (pass) {
      for (size_t j : S) good[j] = 1;
      return TPST_OK;
    }
  }
  if (S.size() == 1) return TPST_OK;  // good[S[0]] stays 0
  const std::vector<size_t> L(S.begin(), S.begin() + S.size() / 2), Rt(S.begin() + S.size() / 2, S.end());
  bool lp = false;
  if (int rc = run_check(b, L, &lp)) return rc;
  if (lp) {
    for (size_t j : L) good[j] = 1;
    return solve(b, Rt, true, good);  // the failure is in the other half
  }
  if (int rc = solve(b, L, true, good)) return rc;
  return solve(b, Rt, false, good);
}

}  // namespace

extern "C" int tpst_pst_verify_batch(tpst_ctx* ctx, int n, const tpst_verify_item* items, size_t B,
                                     const uint64_t* rho, uint8_t* ok) {
  if (!ctx) return TPST_E_ARG;
  if (B == 0) return TPST_OK;
  if (!items || !rho) return fail(ctx, TPST_E_ARG, "null argument");
  for (size_t j = 0; j < B; j++)
    if (!items[j].point || !items[j].v || !items[j].T || !items[j].proof || !items[j].tr)
      return fail(ctx, TPST_E_ARG, "null argument in item " + std::to_string(j));
  int m, m_row, odd;
  if (poly_dims(n, m, m_row, odd)) return fail(ctx, TPST_E_ARG, "bad num_vars");
  if (B > ((size_t)1 << 20)) return fail(ctx, TPST_E_ARG, "more than 2^20 items: split the batch");
  for (size_t k = 0; k < 4 * B; k++)
    if (!rho[2 * k] && !rho[2 * k + 1]) return fail(ctx, TPST_E_ARG, "zero multiplier");
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  SrsState* st = srs_of(ctx);
  if (!st) return fail(ctx, TPST_E_STATE, "no SRS loaded");
  if (st->nv != m_row) return fail(ctx, TPST_E_ARG, "size mismatch");
  for (size_t j = 0; j < B; j++)
    if (items[j].proof->m_col != m || items[j].proof->m_row != m_row)
      return fail(ctx, TPST_E_ARG, "size mismatch in item " + std::to_string(j));

  // ---- every device buffer of the call, before the first launch (grow-only arenas: nothing is freed between
  // launches; msm_var sizes ctx->arena itself, before its own first launch)
  const size_t c1 = 2 + 3 * (size_t)m, c2 = 1 + (size_t)m_row;  // G1 / G2 points of one proof
  const size_t n1s = B * (m + 1), n1l = B * (1 + m_row), n2 = B * (m + 1), nu = B * (2 * m + 2);
  const size_t NP = B * (3 + m + m_row), K = B * (2 * (size_t)m + 1);
  const size_t main_need = Arena::need((n1s + 2 * n1l + nu) * 24, 4) + Arena::need(2 * n2 * 48, 4) +
                           Arena::need((n1s + 2 * n1l + 2 * n2 + nu) * 8, 4) + Arena::need(NP * 24, 4) +
                           Arena::need(NP * 48, 4) + Arena::need(144, 4) + Arena::need(n1s + n1l, sizeof(Xyzz<Fq>)) +
                           Arena::need(1, sizeof(Xyzz<Fq>)) + Arena::need(n2, sizeof(Xyzz<Fq2>)) +
                           Arena::need(1, sizeof(Fq12)) + 2 * Arena::need(K, sizeof(Fq12)) + Arena::need(K * 4, 8) +
                           Arena::need(K, 4) + 4096;
  const size_t check_need = std::max(Arena::need(B * c1 * 24, 4), Arena::need(B * c2 * 48, 4)) + Arena::need(B * c1, 1);
  TPST_HIP(ctx, ctx->io.reserve(std::max(main_need, check_need)));
  TPST_HIP(ctx, ctx->arena2.reserve(multi_pairing_reserve(1, NP)));
  if (int rc = open_streams(ctx, 8, pin_gt_off(K) + 576 + sizeof(Xyzz<Fq>))) return rc;

  // ---- validation, before any sponge absorbs anything (pst_api.hip proof_valid)
  std::vector<uint8_t> valid(B, 1);
  host::parallel_for(B, [&](size_t j) {
    const tpst_verify_item& it = items[j];
    bool good = fr_ok(it.v) && gt_ok(it.T);
    for (int i = 0; i < n; i++) good = good && fr_ok(it.point + 4 * i);
    for (int i = 0; i < m; i++) good = good && gt_ok(it.proof->comms_t[i][0]) && gt_ok(it.proof->comms_t[i][1]);
    valid[j] = good;
  });
  {
    std::vector<const uint64_t*> p1, p2;
    p1.reserve(B * c1);
    p2.reserve(B * c2);
    for (size_t j = 0; j < B; j++) {
      const tpst_open_proof* pr = items[j].proof;
      p1.push_back(pr->U);
      p1.push_back(pr->final_a);
      for (int i = 0; i < m; i++) {
        p1.push_back(pr->comms_u[i][0]);
        p1.push_back(pr->comms_u[i][1]);
        p1.push_back(pr->pst_proof_h[i]);
      }
      p2.push_back(pr->final_h);
      for (int i = 0; i < m_row; i++) p2.push_back(pr->pst_proof[i]);
    }
    std::vector<uint8_t> s1(p1.size(), 0), s2(p2.size(), 0);
    if (p1.size() >= POINT_CHECK_DEVICE_MIN) {
      std::vector<uint64_t> flat1(p1.size() * 12);
      for (size_t t = 0; t < p1.size(); t++) memcpy(&flat1[12 * t], p1[t], 96);
      if (int rc = point_status_batch_locked<Fq>(ctx, flat1.data(), p1.size(), s1.data())) return rc;
    } else {
      host::parallel_for(p1.size(), [&](size_t t) { s1[t] = !point_valid<Fq>(p1[t]); });
    }
    if (p2.size() >= POINT_CHECK_DEVICE_MIN) {
      std::vector<uint64_t> flat2(p2.size() * 24);
      for (size_t t = 0; t < p2.size(); t++) memcpy(&flat2[24 * t], p2[t], 192);
      if (int rc = point_status_batch_locked<Fq2>(ctx, flat2.data(), p2.size(), s2.data())) return rc;
    } else {
      host::parallel_for(p2.size(), [&](size_t t) { s2[t] = !point_valid<Fq2>(p2[t]); });
    }
    for (size_t t = 0; t < p1.size(); t++)
      if (s1[t]) valid[t / c1] = 0;
    for (size_t t = 0; t < p2.size(); t++)
      if (s2[t]) valid[t / c2] = 0;
  }

  Batch b;
  b.ctx = ctx;
  b.st = st;
  b.items = items;
  b.m = m;
  b.m_row = m_row;
  b.K = K;
  b.pin = reinterpret_cast<uint8_t*>(ctx->pinned);
  b.rp.resize(B);
  std::vector<size_t> V;
  for (size_t j = 0; j < B; j++)
    if (valid[j]) V.push_back(j);

  // ---- transcript replay on host threads (local sponges: no tr changes yet)
  host::parallel_for(V.size(), [&](size_t t) {
    const size_t j = V[t];
    Replay& r = b.rp[j];
    replay(items[j], m, m_row, r);
    const uint64_t* q = rho + 8 * j;
    const uint64_t a[4][4] = {{q[0], q[1], 0, 0}, {q[2], q[3], 0, 0}, {q[4], q[5], 0, 0}, {q[6], q[7], 0, 0}};
    r.rT = fr_canon(a[0]);
    r.r2 = fr_canon(a[1]);
    r.r1 = fr_canon(a[2]);
    r.rU = fr_canon(a[3]);
  });

  // ---- carve the buffers
  ctx->io.reset();
  Bufs& d = b.d;
  d.g1in = ctx->io.take<uint32_t>((n1s + 2 * n1l + nu) * 24);
  d.g2in = ctx->io.take<uint32_t>(2 * n2 * 48);
  d.sc = ctx->io.take<uint32_t>((n1s + 2 * n1l + 2 * n2 + nu) * 8);
  d.pg1 = ctx->io.take<uint32_t>(NP * 24);
  d.pg2 = ctx->io.take<uint32_t>(NP * 48);
  d.fo = ctx->io.take<uint32_t>(144);
  d.x1 = ctx->io.take<Xyzz<Fq>>(n1s + n1l);
  d.usum = ctx->io.take<Xyzz<Fq>>(1);
  d.x2 = ctx->io.take<Xyzz<Fq2>>(n2);
  d.f = ctx->io.take<Fq12>(1);
  d.gb = ctx->io.take<Fq12>(K);
  d.gout = ctx->io.take<Fq12>(K);
  d.ge = ctx->io.take<uint64_t>(K * 4);
  d.gok = ctx->io.take<uint32_t>(K);

  // every return below drains the side stream first: its copies write the pinned staging
  hipStream_t s2 = ctx->side[0];
  struct Drain {
    hipStream_t s;
    ~Drain() { (void)hipStreamSynchronize(s); }
  } drain{s2};

  // ---- GT side (side stream): T^{rho_T}, t_l^{rho_T / x}, t_r^{rho_T x} of every item in one launch
  const size_t kb = 2 * (size_t)m + 1, Kv = V.size() * kb;
  Fq12* pw = reinterpret_cast<Fq12*>(b.pin);
  uint32_t* okv = reinterpret_cast<uint32_t*>(pw + K);
  if (Kv) {
    std::vector<Fq12> bases(Kv);
    std::vector<uint64_t> dg(4 * Kv);
    host::parallel_for(V.size(), [&](size_t t) {
      const size_t j = V[t];
      const Replay& r = b.rp[j];
      for (size_t k = 0; k < kb; k++) {
        const int i = k ? (int)(k - 1) / 2 : 0;
        bases[t * kb + k] = gt_mont(k ? items[j].proof->comms_t[i][(k - 1) % 2] : items[j].T);
        const Fr e = !k ? r.rT : (k - 1) % 2 ? mul(r.rT, r.xs[i]) : mul(r.rT, r.xs_inv[i]);
        uint64_t e4[4];
        fr_out(e, e4);
        base_x_digits(e4, &dg[4 * (t * kb + k)]);
      }
    });
    TPST_HIP(ctx, hipMemcpyAsync(d.gb, bases.data(), Kv * sizeof(Fq12), hipMemcpyHostToDevice, s2));
    TPST_HIP(ctx, hipMemcpyAsync(d.ge, dg.data(), Kv * 32, hipMemcpyHostToDevice, s2));
    ctx->prof.begin(ST_VERIFY_BATCH_GT_POW, s2);
    TPST_HIP(ctx, gt_pow_wave(s2, d.gb, d.ge, Kv, d.gout, d.gok));
    ctx->prof.end(ST_VERIFY_BATCH_GT_POW, s2);
    TPST_HIP(ctx, hipMemcpyAsync(pw, d.gout, Kv * sizeof(Fq12), hipMemcpyDeviceToHost, s2));
    TPST_HIP(ctx, hipMemcpyAsync(okv, d.gok, Kv * 4, hipMemcpyDeviceToHost, s2));
  }
  {
    const uint64_t* flat = st->flat.data();
    b.ng.resize(12);
    b.nh.resize(24);
    b.ngmask.resize(12 * (size_t)st->nv);
    b.nhmask.resize(24 * (size_t)st->nv);
    neg_point<1>(flat, b.ng.data());
    neg_point<2>(flat + 12, b.nh.data());
    const uint64_t* gmask = flat + tpst_srs_flat_len(st->nv) - 36 * st->nv;
    const uint64_t* hmask = flat + tpst_srs_flat_len(st->nv) - 24 * st->nv;
    for (int i = 0; i < st->nv; i++) {
      neg_point<1>(gmask + 12 * i, &b.ngmask[12 * i]);
      neg_point<2>(hmask + 24 * i, &b.nhmask[24 * i]);
    }
  }
  // the combined check of every validated item runs beside the GT powers (their membership flags are not
  // known yet: an item outside GT is rare and costs one more check below)
  if (!V.empty())
    if (int rc = enqueue_check(b, V)) return rc;
  TPST_HIP(ctx, hipStreamSynchronize(s2));
  // per-item R_j; an item with T or a comms_t entry outside GT is invalid
  std::vector<size_t> S;
  {
    std::vector<uint8_t> in_gt(V.size(), 1);
    host::parallel_for(V.size(), [&](size_t t) {
      Fq12 acc = Fq12::one();
      for (size_t k = 0; k < kb; k++) {
        if (!okv[t * kb + k]) in_gt[t] = 0;
        acc = mul(acc, pw[t * kb + k]);
      }
      b.rp[V[t]].R = acc;
    });
    for (size_t t = 0; t < V.size(); t++) {
      if (in_gt[t])
        S.push_back(V[t]);
      else
        valid[V[t]] = 0;
    }
  }

  // ---- the verdict
  std::vector<uint8_t> good(B, 0);
  bool pass = S.empty();
  if (S.size() == V.size()) {
    if (!V.empty())
      if (int rc = finish_check(b, V, &pass)) return rc;
  } else {  // the queued check holds an item outside GT: let it drain, check the others
    TPST_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (!S.empty())
      if (int rc = run_check(b, S, &pass)) return rc;
  }
  if (pass) {
    for (size_t j : S) good[j] = 1;
  } else if (!ok) {
    return fail(ctx, TPST_E_VERIFY, "batch verification failed");  // no verdicts asked for: every tr is left as it was
  } else {
    if (int rc = solve(b, S, true, good)) return rc;
  }
  bool all = true;
  for (size_t j = 0; j < B; j++) {
    if (good[j]) b.rp[j].sp.store(items[j].tr);
    if (ok) ok[j] = good[j];
    all = all && good[j];
  }
  return all ? TPST_OK : fail(ctx, TPST_E_VERIFY, "batch verification failed");
}
