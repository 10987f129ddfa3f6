// The sqrt-PST opening of libtpst (include/tpst.h): tpst_poly_open and its
// row-sharded form tpst_poly_open_sharded -- Polynomial::open
// (sqrt_pst.rs:168-230) with MippProof::prove (mipp.rs:31-153) -- as named
// stages of one `Opening` (below), plus the stream-ordered PST open they and
// the MultilinearPC calls share.  The SRS, the Polynomial handle, the commit
// and the verifier live in pst_api.hip; the shared state in pst_state.h.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

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

// --------------------------------------------------------------- open ----
// The opening is latency-bound (transcript rounds of small MSMs and pairings),
// so every MSM of it runs on fixed-base lookup tables (fbt.h): the SRS sides
// are tabulated once per SRS, the row commitments once per opening, and each
// MIPP round's folds / cross terms are grouped MSMs over the ORIGINAL bases
// with scalars that are products of the challenges so far.
namespace {

// PST open of 2^k evals (Montgomery) at k Montgomery
// scalars d_pt over the pair levels off..off+k-1: the k quotient scalar
// vectors first (cheap Fr recurrence), then ONE grouped table MSM with a
// group per level.  Writes k XYZZ points.  Stream-ordered on `s` with the
// caller's scratch (pst_open_scratch_words u32), so it can run beside the MIPP.
size_t pst_open_scratch_words(const SrsState* st, int k) {
  return ((size_t)2 << k) * 8 + st->lvl_off[st->nv] * 8;
}

template <class F>
hipError_t pst_open_fbt_s(hipStream_t s, Arena& ar, const SrsState* st, const uint32_t* table, int off,
                          const uint32_t* d_evals, int k, const uint32_t* d_pt, Xyzz<F>* d_out, uint32_t* scratch) {
  const size_t full = (size_t)1 << k;
  uint32_t* cur = scratch;
  uint32_t* nxt = scratch + full * 8;
  uint32_t* sc = scratch + 2 * full * 8;
  hipError_t e = hipMemcpyAsync(cur, d_evals, full * 32, hipMemcpyDeviceToDevice, s);
  if (e != hipSuccess) return e;
  for (int i = 0; i < k; i++) {
    const size_t half = (size_t)1 << (k - i - 1);
    e = pst_step(s, cur, half, d_pt + 8 * i, sc + 8 * st->lvl_off[off + i], nxt);
    if (e != hipSuccess) return e;
    std::swap(cur, nxt);
  }
  FbGroups g;
  g.groups = k;
  g.members = (size_t)1 << (k - 1);
  g.d_seg = st->seg.u() + off;
  return fbt_msm<F>(ar, s, table, sc, g, d_out);
}

}  // namespace

namespace tpst {

template <class F>
int pst_open_fbt(tpst_ctx* ctx, SrsState* st, const uint32_t* table, int off, const uint32_t* d_evals, int k,
                 const uint32_t* d_pt, Xyzz<F>* d_out) {
  DevBuf scratch;
  TPST_HIP(ctx, scratch.alloc(pst_open_scratch_words(st, k) * 4));
  TPST_HIP(ctx, pst_open_fbt_s<F>(ctx->stream, ctx->arena, st, table, off, d_evals, k, d_pt, d_out, scratch.u()));
  return TPST_OK;
}
template int pst_open_fbt<Fq>(tpst_ctx*, SrsState*, const uint32_t*, int, const uint32_t*, int, const uint32_t*,
                              Xyzz<Fq>*);
template int pst_open_fbt<Fq2>(tpst_ctx*, SrsState*, const uint32_t*, int, const uint32_t*, int, const uint32_t*,
                               Xyzz<Fq2>*);

// ---------------------------------------------------------------- open ----
// Streams of the opening (created once per context) and a pool of events.
int open_streams(tpst_ctx* ctx, size_t n_events, size_t pinned_bytes, bool comm) {
  int least = 0, greatest = 0;
  TPST_HIP(ctx, hipDeviceGetStreamPriorityRange(&least, &greatest));
  // side streams at the least priority (the look-ahead streams at the
  // greatest won an open-only sweep, 14.2 -> 13.8 ms, but lost in the commit +
  // open bench: 2^20 open 12.3 -> 13.9 ms; profiles/r04/late/prio6_bench*.json)
  for (int i = 0; i < 3; i++)
    if (!ctx->side[i]) TPST_HIP(ctx, hipStreamCreateWithPriority(&ctx->side[i], hipStreamNonBlocking, least));
  // the row-sharded opening's collectives, in one issue order on every rank
  if (comm && !ctx->comm) TPST_HIP(ctx, hipStreamCreateWithPriority(&ctx->comm, hipStreamNonBlocking, greatest));
  // the per-round h preparation of the opening (its own hardware queue: on
  // stream A it delayed the next round's t; 2^20 open 13.0 -> 11.4 ms; at
  // the least priority 11.05 -> 11.30 ms, profiles/r06/ab/ab_open_c_prio.txt)
  if (!ctx->side_c) TPST_HIP(ctx, hipStreamCreateWithPriority(&ctx->side_c, hipStreamNonBlocking, greatest));
  while (ctx->events.size() < n_events) {
    hipEvent_t e;
    TPST_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    ctx->events.push_back(e);
  }
  return ensure_pinned(ctx, pinned_bytes);
}

}  // namespace tpst

// Polynomial::open (sqrt_pst.rs:168-230) with MippProof::prove (mipp.rs:31-153).
//
// Critical path = the transcript: each MIPP round's challenge needs that
// round's comms_u and comms_t, and the next round's folds need the challenge.
// Per round r (len = C >> r, s = len / 2, s' = s / 2) the work is spread
// over 4 streams (one hardware queue each; A at the highest priority):
//   A (critical): t^(r) = (t_l, t_r).  Round 0 pairs the row commitments
//     directly.  From round 1 on, t^(r) comes out of the LOOK-AHEAD of round
//     r-1 (stream D): with a' = a_L + c a_R, h' = h_L + c^-1 h_R (mipp.rs:101-
//     120) bilinearity splits round r's cross products into eight pairing
//     products of round r-1's vectors that do not involve c = c_{r-1},
//       t_l = A0 A3 A1^(c^-1) A2^c,  t_r = B0 B3 B1^(c^-1) B2^c
//     (pairing.hip mipp_lookahead, pairing_mipp.hip the combination), so once c is known the critical path is
//     four GT exponentiations (base-x Frobenius splitting, ~0.7 ms) and two
//     products instead of fold + Miller loops + final exponentiations
//     (~3.3 ms); comms_t -> host.
//   D: the look-ahead of round r for round r+1: a^(r) and c'a^(r) as ONE
//     grouped table MSM over the original row commitments (scalar sets W,
//     c'W: a^(r)_i = sum_t W_t a_{i+t len}, c' = the previous challenge
//     inverse), then the 8 products against the PREVIOUS round's prepared h:
//       e(a_i, h^(r)_k) = e(a_i, h^(r-1)_k) e(c' a_i, h^(r-1)_{k+len})
//     -> Miller loops + 8 final exponentiations, overlapping round r's own
//     transcript work.
//   B: y fold (compress_field, mipp.rs:124-136) and the cross MSMs u_l, u_r
//     (mipp.rs:66-75) -> canonical -> host; in round 0 first U =
//     MSM(comm_list, chi(b)) (sqrt_pst.rs:198) and after it the PST proof of
//     q (sqrt_pst.rs:218-225), which needs nothing from the MIPP.
//   C: in round 0 the fold table over comm_list (fbt.h); then h^(r) =
//     sum_t Wi_t h_{i + t len} (table MSM over powers_of_h) -> affine ->
//     G2Prepared, consumed by the look-ahead of round r+1.
// The host waits only for the round's comms (pinned staging), absorbs them
// (mipp.rs:97-101) and squeezes the challenge; no stream is drained mid-open.
//
// Row-sharded form (sh != nullptr, tpst_poly_open_sharded):
// rank g of W owns the rows i = g mod W of comm_list, h and y.  While
// len >= 4W every fold group (a^(r)_i = sum_t W_t a_{i + t len}) lies on one
// rank (i + t len = i mod W), and so does every look-ahead pair (positions
// i + j s' share i's residue), so each rank runs the round on its own rows
// with every size divided by W: its own table over its C / W commitments,
// the look-ahead's folds and pairings over len / W positions, the h folds and
// preparations of its positions, and the cross MSMs as partial sums over its
// rows.  ONE all-gather per product combines them on every rank: the cross
// partials summed (XYZZ), the Miller partials multiplied before the single
// final exponentiation (gt_prod_final); every rank then combines t^(r) and
// replays the transcript itself (no broadcast).  At the first round with
// len < 4W the ranks gather the folded a^(r1) (len = 2W points) to rank 0,
// which tabulates it and finishes the remaining rounds with the a-side
// rebased on it (a^(r)_i = sum_{t < 2^(r - r1)} W_r[t] a^(r1)_{i + t len}:
// the first weights of the same W_r) and the epilogue alone.  The exchange is
// the caller's (tpst_exchange: RCCL, gloo, ...), ordered on a dedicated comm
// stream so that every rank issues the same collectives in the same order.
//
// Source layout: Opening::run() is the table of contents -- check, plan,
// reserve, local_srs_side, prologue, table_and_U, then per round (round())
// stage_round, hand_over, enqueue_t (A), enqueue_cross (B), enqueue_h_prep
// (C), enqueue_lookahead (D), pst_q, enqueue_rebase, absorb_U, absorb_round,
// and the epilogue.  round() alone fixes the host's issue order across the
// streams, which was measured (see the comments there).
namespace {

// TPST_OPEN_TRACE=1: per-round host timings of tpst_poly_open on stderr
double host_us() {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
bool open_trace() {
  static const bool on = getenv("TPST_OPEN_TRACE") != nullptr;
  return on;
}

struct Shard {
  int W = 1, rank = 0;
  const tpst_exchange* x = nullptr;
  const uint64_t* U = nullptr;  // c_u (canonical affine), every rank
};

size_t xch_align(size_t v) { return (v + 255) & ~(size_t)255; }
size_t xch_slot(size_t bytes, int W) { return xch_align(bytes) + xch_align((size_t)W * bytes); }
// first round whose look-ahead cannot be split over W ranks (len < 4W)
int shard_rounds(int m, int W) {
  int r1 = 0;
  while (r1 < m && (((size_t)1 << m) >> r1) >= (size_t)4 * W) r1++;
  return r1;
}
}  // namespace

extern "C" size_t tpst_open_sharded_arena_bytes(int n, int world) {
  if (n < 1 || n > 2 * TPST_MAX_VARS || world < 1 || (world & (world - 1))) return 0;
  const int m = n / 2, r1 = shard_rounds(m, world);
  if (r1 == 0) return 0;
  constexpr size_t X1 = sizeof(Xyzz<Fq>), T12 = sizeof(Fq12);
  return (size_t)r1 * (xch_slot(2 * X1, world) + xch_slot(8 * T12, world)) + xch_slot(2 * T12, world) +
         xch_slot(2 * X1, world);
}

namespace {

constexpr size_t X1 = sizeof(Xyzz<Fq>), X2 = sizeof(Xyzz<Fq2>);

// host staging layout (byte offsets into the context's pinned buffer; the
// upload part is mirrored in OpenBufs::up): per-round uploads, final upload,
// downloads, comm_list
struct Staging {
  // per round: c_{r-1}, c_{r-1}^-1, f_0..f_7 (Montgomery Fr), base-x digits of
  // (c^-1, c, c^-1, c); the fold weights themselves are formed on the device
  static constexpr size_t UP_ROUND = 10 * 32 + 128;
  // downloads: U, each round's u_l / u_r as raw XYZZ (converted on the host)
  // and t_l / t_r; final_a, final_h raw; pst_proof_h, pst_proof canonical
  static constexpr size_t DN_ROUND = 2 * X1 + 1152;
  size_t up_final = 0;  // c_{m-1}, c_{m-1}^-1, rs (Montgomery Fr), a_rev (canonical Fr)
  size_t a_rev = 0;     // (inside the final upload)
  size_t up_bytes = 0;
  size_t dn_U = 0, dn_round = 0, dn_final = 0, dn_fh = 0, dn_ph = 0, dn_pst = 0, dn_bytes = 0;
  size_t cm = 0;  // comm_list staging (unsharded form)
  size_t up_round(int r) const { return (size_t)r * UP_ROUND; }
  size_t round(int r) const { return dn_round + (size_t)r * DN_ROUND; }
  static Staging make(int m, int k) {
    Staging l;
    l.up_final = (size_t)m * UP_ROUND;
    l.a_rev = l.up_final + (2 + m) * 32;
    l.up_bytes = l.up_final + (2 + m + k) * 32;
    l.dn_U = l.up_bytes;
    l.dn_round = l.dn_U + X1;
    l.dn_final = l.dn_round + (size_t)m * DN_ROUND;
    l.dn_fh = l.dn_final + X1;
    l.dn_ph = l.dn_fh + X2;
    l.dn_pst = l.dn_ph + (size_t)m * 96;
    l.dn_bytes = X1 + (size_t)m * DN_ROUND + X1 + X2 + (size_t)m * 96 + (size_t)k * 192;
    l.cm = l.up_bytes + l.dn_bytes;
    return l;
  }
};

// exchange (sharded form): slots in the caller's arena, one comm stream
struct Exchange {
  tpst_ctx* ctx = nullptr;
  const tpst_exchange* x = nullptr;
  int W = 1;
  hipEvent_t* ev = nullptr;  // two per gather
  size_t off = 0;            // slot cursor
  int n = 0;                 // gathers issued
  struct Slot {
    uint8_t* send;
    uint8_t* recv;
    size_t send_off, recv_off;
  };
  Slot slot(size_t bytes) {
    Slot sl;
    sl.send_off = off;
    sl.recv_off = off + xch_align(bytes);
    off += xch_slot(bytes, W);
    sl.send = (uint8_t*)x->d_arena + sl.send_off;
    sl.recv = (uint8_t*)x->d_arena + sl.recv_off;
    return sl;
  }
  // every rank's `bytes` at its slot's send -> recv (rank-major), ordered
  // after the work queued on `s` so far; `s` then waits for the result
  int gather(hipStream_t s, const Slot& sl, size_t bytes) {
    hipEvent_t e0 = ev[2 * n], e1 = ev[2 * n + 1];
    n++;
    TPST_HIP(ctx, hipEventRecord(e0, s));
    TPST_HIP(ctx, hipStreamWaitEvent(ctx->comm, e0, 0));
    if (x->allgather(x->user, sl.send_off, sl.recv_off, bytes, (void*)ctx->comm))
      return fail(ctx, TPST_E_STATE, "exchange all-gather failed");
    TPST_HIP(ctx, hipEventRecord(e1, ctx->comm));
    TPST_HIP(ctx, hipStreamWaitEvent(s, e1, 0));
    return TPST_OK;
  }
  hipEvent_t spare() const { return ev[2 * n]; }  // past the gathers' events
};

// what the stages of round r share (stage_round fills it)
struct Round {
  int r = 0;
  size_t len = 0, s = 0;     // len = C >> r positions, s = len / 2
  bool loc = false;          // this round on the rank's own rows (sharded form)
  int E = 1;                 // fold sets of the look-ahead: 2^(r - la_src(r))
  uint32_t* dcp = nullptr;   // c' = c_{r-1}^-1 (the y fold)
  uint32_t* dfs = nullptr;   // f_0..f_{E-1}
  const uint64_t* ddig = nullptr;
  uint32_t *dW = nullptr, *dWi = nullptr;  // W_r, Wi_r
  uint8_t* dn = nullptr;     // the round's downloads (pinned)
};

// host time stamps of a round's enqueues (TPST_OPEN_TRACE)
struct RoundTrace {
  double hq = 0, hb = 0, ha = 0, hd = 0, hp = 0;
};

struct Opening {
  tpst_ctx* const ctx;
  SrsState* const st;
  tpst_poly* const p;
  tpst_transcript* const tr;
  const int n;
  const uint64_t* const comms;
  const uint64_t* const point;
  tpst_open_proof* proof;
  const Shard* const sh;
  OpenBufs& b;
  Profiler& pf;
  const bool shd;
  const int W, rho;
  const bool lead;  // produces the proof (and the PST proof of q)

  // ---- plan: dimensions, layout, streams, events
  int m = 0, k = 0, odd = 0;
  size_t C = 0, Cl = 0, Ca0 = 0;  // rows; a rank's rows (i = rho mod W); a-side bases resident: own rows or all
  int r1 = 0;                     // the rounds split across the ranks: [0, r1); rank 0 alone from r1 on
  int rb = -1;                    // the unsharded rebase round (plan()), or -1
  std::unique_ptr<tpst_open_proof> own_proof;
  Sponge sp;
  Staging lay;
  uint8_t* pin = nullptr;
  hipStream_t sA = nullptr, sB = nullptr, sC = nullptr, sCe = nullptr, sLA[2] = {nullptr, nullptr};
  Arena &arA, &arB, &arC;
  Arena* arLA[2];
  hipEvent_t* ev = nullptr;
  Exchange xch;
  // which odd rounds prepare h: for a look-ahead on the rank's own positions
  // (local, sharded rounds) or on every position (global)
  std::vector<char> need_loc, need_glob;
  // the SRS side, and a rank's own positions of it
  const uint32_t *H0 = nullptr, *tH = nullptr, *H0l = nullptr, *tHl = nullptr;
  const LineCoeff *L0 = nullptr, *L0l = nullptr;
  const uint32_t* chis = nullptr;
  const uint64_t* U_given = nullptr;

  // ---- running state of the rounds
  // W_r[t] / Wi_r[t] (device, mipp_weights): products of the challenges
  // (inverses) folded so far, so that a^(r)_i = sum_t W_r[t] a_{i + t len},
  // h^(r)_i = sum_t Wi_r[t] h_{i + t len}
  std::vector<Fr> xs_inv;
  Fr cprev = Fr::one(), cprev_c = Fr::one();
  uint64_t la_digits[16] = {};
  const uint32_t* tA = nullptr;  // the a-side table (rebased at the hand-over)
  size_t Ca = 0;                 // its base count
  hipEvent_t ev_t1 = nullptr;    // the table over a^(r1) / a^(rb) (rank 0 in the sharded form)
  int last_c = -1;               // the last odd round that issued h work "C"

  Opening(tpst_ctx* ctx_, SrsState* st_, tpst_poly* p_, tpst_transcript* tr_, int n_, const uint64_t* comms_,
          const uint64_t* point_, tpst_open_proof* proof_, const Shard* sh_)
      : ctx(ctx_), st(st_), p(p_), tr(tr_), n(n_), comms(comms_), point(point_), proof(proof_), sh(sh_), b(st_->ob),
        pf(ctx_->prof), shd(sh_ != nullptr), W(sh_ ? sh_->W : 1), rho(sh_ ? sh_->rank : 0), lead(rho == 0),
        arA(ctx_->arena), arB(ctx_->arena_side[0]), arC(ctx_->arena2),
        arLA{&ctx_->arena_side[1], &ctx_->arena_side[2]} {}

  // ---- events: a fixed set, six per round, then the exchange's
  enum { EV_PRE, EV_TABLE, EV_U, EV_FINAL_UP, EV_B_DONE, EV_C_DONE, EV_D_DONE, EV_A_DONE, EV_REBASE, EV_FIXED };
  enum { RV_UP, RV_A, RV_B, RV_C, RV_LA, RV_CL, RV_N };
  hipEvent_t ev_round(int r, int which) const { return ev[EV_FIXED + RV_N * r + which]; }
  hipEvent_t ev_up(int r) const { return ev_round(r, RV_UP); }
  hipEvent_t ev_a(int r) const { return ev_round(r, RV_A); }
  hipEvent_t ev_b(int r) const { return ev_round(r, RV_B); }
  hipEvent_t ev_c(int r) const { return ev_round(r, RV_C); }
  hipEvent_t ev_la(int r) const { return ev_round(r, RV_LA); }
  hipEvent_t ev_cl(int r) const { return ev_round(r, RV_CL); }  // the rank's own h positions prepared

  // the prepared h the look-ahead of round r pairs against (see plan())
  // look-ahead 1 pairs h^(1), prepared by C in round 1 (enqueued before D
  // there), with E = 1 instead of h^(0) with E = 2: half the pairs (2^24 open
  // 22.9 -> 22.5 ms, profiles/r06/ab/ab_open_la1.txt)
  static int la_src(int r) { return r == 0 ? 0 : r - 1; }
  uint32_t* dup(size_t byte_off) const { return (uint32_t*)((uint8_t*)b.up.p + byte_off); }

  int run();
  int check();
  int plan();
  int reserve();
  int local_srs_side();
  int prologue();
  int table_and_U();
  int pst_q();
  int round(int r, bool& done);
  int stage_round(int r, Round& q);
  int hand_over(const Round& q, bool& done);
  int tabulate_a1(Arena& ar, hipStream_t s, size_t len, hipEvent_t built);
  int enqueue_t(const Round& q);
  int enqueue_cross(const Round& q);
  int enqueue_h_prep(const Round& q);
  int h_prep(const Round& q, size_t sub, size_t off, size_t nbases, const uint32_t* table, DevBuf& H, DevBuf& L,
             hipEvent_t done);
  int enqueue_lookahead(const Round& q);
  int enqueue_rebase(const Round& q);
  int absorb_U();
  int absorb_round(const Round& q, const RoundTrace& t);
  int epilogue();
};

int Opening::run() {
  if (int rc = check()) return rc;
  TraceRange trace_open("sqrt_open");
  pf.begin(ST_SQRT_OPEN, ctx->stream);
  if (int rc = plan()) return rc;
  if (int rc = reserve()) return rc;
  if (int rc = local_srs_side()) return rc;
  if (int rc = prologue()) return rc;
  pf.begin(ST_MIPP_PROVE, sA);  // mipp.rs:38-149 (sqrt_pst.rs:211-214)
  TraceRange trace_mipp("mipp_prove");
  if (int rc = table_and_U()) return rc;
  for (int r = 0; r < m; r++) {  // mipp.rs:58-120
    bool done = false;           // a rank other than 0 stops at the hand-over
    if (int rc = round(r, done)) return rc;
    if (done) return TPST_OK;
  }
  return epilogue();
}

// arguments against the SRS; q before the reference's open timer
int Opening::check() {
  if (poly_dims(n, m, k, odd)) return fail(ctx, TPST_E_ARG, "bad num_vars");
  if (st->nv != k) return fail(ctx, TPST_E_ARG, "SRS num_vars != ceil(n/2)");
  for (size_t i = 0; i < ((size_t)2 << m); i++)
    if (!fq_ok(comms + 6 * i)) return fail(ctx, TPST_E_ARG, "comm_list coordinate >= p");
  if (lead && !p->has_q) {  // before the reference's open timer (sqrt_pst.rs:177-183)
    int rc = poly_get_q(ctx, p, point);
    if (rc) return rc;
  }
  return TPST_OK;
}

int Opening::plan() {
  {
    int rc = srs_fbt(ctx, st, odd);
    if (rc) return rc;
  }
  C = (size_t)1 << m;  // m >= 1 from here on: poly_dims rejects n < 2
  r1 = shd ? shard_rounds(m, W) : 0;
  Cl = C / W;
  Ca0 = shd ? Cl : C;
  if (!proof) {  // a rank other than 0 fills nothing the caller reads
    own_proof.reset(new tpst_open_proof);
    proof = own_proof.get();
  }
  memset(proof, 0, sizeof *proof);
  proof->m_col = m;
  proof->m_row = k;
  sp.load(tr);
  lay = Staging::make(m, k);
  const size_t n_ev = EV_FIXED + RV_N * (size_t)m + (shd ? 8 * (size_t)m + 8 : 0);
  // unsharded rebase: in round rb = 4, a^(4) (C / 16 points) is tabulated
  // (as the sharded hand-over does) on the otherwise idle comm stream, and the
  // later rounds fold 2^(r - 4) of its points instead of C / len row
  // commitments (2^24 open 24.4 -> 23.0 ms, 2^20 10.4 -> 10.2 ms; rebasing at
  // len 16 / 64 at 2^24 gained less: profiles/r06/ab/ab_open_rebase.txt)
  rb = !shd && m >= 8 ? 4 : -1;
  if (int rc = open_streams(ctx, n_ev, lay.cm + (shd ? 0 : C * 96), shd || rb >= 0)) return rc;
  pin = (uint8_t*)ctx->pinned;
  // five streams: A (critical), B (cross terms), two look-ahead streams for
  // alternating rounds (consecutive look-aheads overlap, each taking longer
  // than a round) and C, the h preparation, at the greatest priority.  h^(r)
  // (G2 fold + G2Prepared lines) is prepared in every round r >= 1 that a
  // look-ahead needs: look-ahead r pairs E = 2^(r - s) fold sets of a^(r)
  // against the prepared h^(s), s = r - 1 (prepared one round earlier: E = 2;
  // in round 1 itself for r = 1: E = 1), s = 0 for r = 0.  Preparing at odd rounds only (s = r - 2 / r - 3, E =
  // 4 / 8) paired two to four times as many pairs; C on stream A delayed the
  // next round's t (2^24 open 26.6 -> 25.5 ms, 2^20 13.0 -> 11.4 ms with both,
  // profiles/r05/i).  The epilogue's final h fold runs on the first look-ahead
  // stream (idle by then), beside final_a (A) and pst_proof_h (B)
  sA = ctx->stream;
  sB = ctx->side[0];
  sC = ctx->side_c;
  sCe = ctx->side[1];
  sLA[0] = ctx->side[1];
  sLA[1] = ctx->side[2];
  ev = ctx->events.data();
  xch.ctx = ctx;
  xch.x = shd ? sh->x : nullptr;
  xch.W = W;
  xch.ev = ev + EV_FIXED + RV_N * m;  // exchange events (sharded form)
  need_loc.assign(m + 1, 0);
  need_glob.assign(m + 1, 0);
  for (int r = 1; r < m; r++) {
    if ((C >> r) < 4 || la_src(r) == 0) continue;
    if (shd && r < r1)
      need_loc[la_src(r)] = 1;
    else if (lead)
      need_glob[la_src(r)] = 1;
  }
  if (shd && (sh->x->arena_bytes < tpst_open_sharded_arena_bytes(n, W) || !sh->x->d_arena || !sh->x->allgather))
    return fail(ctx, TPST_E_ARG, "exchange arena smaller than tpst_open_sharded_arena_bytes");
  return TPST_OK;
}

// device buffers (allocated before any stream runs: no hipFree mid-open)
int Opening::reserve() {
  const size_t Ch = C / 2;
  TPST_HIP(ctx, b.up.grow(lay.up_bytes));
  TPST_HIP(ctx, b.Wall.grow(2 * C * 32));  // round r's 2^r fold weights at offset 2^r - 1
  TPST_HIP(ctx, b.Wiall.grow(2 * C * 32));
  TPST_HIP(ctx, b.A.grow(Ca0 * 96));
  TPST_HIP(ctx, b.P.grow(Ca0 * 96));
  TPST_HIP(ctx, b.Y.grow(C * 32));
  TPST_HIP(ctx, b.chiC.grow(C * 32));
  TPST_HIP(ctx, b.ScA.grow(2 * C * 32));
  TPST_HIP(ctx, b.ScB.grow(C * 32));
  TPST_HIP(ctx, b.ScC.grow(C * 32));
  TPST_HIP(ctx, b.xa.grow(C * sizeof(Xyzz<Fq>)));
  TPST_HIP(ctx, b.xb.grow(2 * sizeof(Xyzz<Fq>)));
  TPST_HIP(ctx, b.xd.grow((k + 1) * sizeof(Xyzz<Fq2>)));
  TPST_HIP(ctx, b.xh.grow(C * sizeof(Xyzz<Fq2>)));
  TPST_HIP(ctx, b.xp.grow(((size_t)m + 1) * sizeof(Xyzz<Fq>)));
  for (int i = 0; i < 3; i++) {  // prepared h^(r) in slot r % 3
    TPST_HIP(ctx, b.Hb[i].grow(Ch * 192));
    TPST_HIP(ctx, b.Lb[i].grow(Ch * N_LINE_COEFFS * sizeof(LineCoeff)));
    if (shd) {
      TPST_HIP(ctx, b.Hbl[i].grow((Ch / W ? Ch / W : 1) * 192));
      TPST_HIP(ctx, b.Lbl[i].grow((Ch / W ? Ch / W : 1) * N_LINE_COEFFS * sizeof(LineCoeff)));
    }
  }
  TPST_HIP(ctx, b.gts.grow(2 * sizeof(Fq12)));
  for (int i = 0; i < 2; i++) {
    TPST_HIP(ctx, b.ScD[i].grow(8 * C * 32));
    TPST_HIP(ctx, b.xl[i].grow(C * sizeof(Xyzz<Fq>)));
    TPST_HIP(ctx, b.LAo[i].grow(8 * sizeof(Fq12)));
    // sized for either engine (RNS form: rns::RES_WORDS u32 per Fq12)
    TPST_HIP(ctx, b.SqT[i].grow(4 * 64 * MIPP_TAB_F12_BYTES));
    TPST_HIP(ctx, b.SqG[i].grow(2 * 10 * MIPP_TAB_F12_BYTES));
  }
  TPST_HIP(ctx, b.SqM.grow(128 * MIPP_TAB_F12_BYTES));
  TPST_HIP(ctx, b.canA.grow(2 * 576));
  TPST_HIP(ctx, b.canC.grow((size_t)(m + 1) * 192));
  TPST_HIP(ctx, b.canD.grow(96 + (size_t)k * 192));
  TPST_HIP(ctx, b.pstA.grow(pst_open_scratch_words(st, m) * 4));
  TPST_HIP(ctx, b.pstB.grow(pst_open_scratch_words(st, k) * 4));
  if (!shd && st->t_A_n < C) {
    TPST_HIP(ctx, st->t_A.alloc(fbt_words<Fq>(C) * 4));
    st->t_A_n = C;
  }
  if (shd) TPST_HIP(ctx, b.tLoc.grow(fbt_words<Fq>(Cl) * 4));
  if (shd || rb >= 0) {
    const size_t len1 = C >> (shd ? r1 : rb);
    TPST_HIP(ctx, b.A1x.grow(len1 * X1));
    TPST_HIP(ctx, b.A1.grow(len1 * 96));
    TPST_HIP(ctx, b.tA1.grow(fbt_words<Fq>(len1) * 4));
  }
  {  // G2 preparation scratch: the prepared h^(r) (global: <= C / 2 points, a rank's: <= C / 2W)
    size_t mx = 0;
    for (int r = 1; r <= m; r++) {
      if (need_glob[r]) mx = std::max(mx, C >> r);
      if (need_loc[r]) mx = std::max(mx, (C >> r) / W);
    }
    if (mx)
      if (int rc = prep_scratch_for(ctx, st, mx)) return rc;
  }
  return TPST_OK;
}

// the SRS side of the pairings and folds, and the a-side table
int Opening::local_srs_side() {
  H0 = st->ph[odd]->u();
  L0 = (const LineCoeff*)st->hprep[odd].p;
  tH = st->t_h[odd].u();
  // a rank's own positions of the SRS side (every W-th of h, its prepared
  // lines and its table), cached per (W, rank, parity)
  H0l = H0;
  tHl = tH;
  L0l = L0;
  if (shd) {
    SrsState::Local& lc = st->local[odd];
    if (lc.W != W || lc.rank != rho) {
      const size_t tb = fbt_words<Fq2>(1) * 4;  // one point's table block
      const size_t lb = sizeof(LineCoeff);
      TPST_HIP(ctx, lc.H0.alloc(Cl * 192));
      TPST_HIP(ctx, lc.L0.alloc(Cl * N_LINE_COEFFS * lb));
      TPST_HIP(ctx, lc.tH.alloc(Cl * tb));
      TPST_HIP(ctx, hipMemcpy2DAsync(lc.H0.p, 192, (const uint8_t*)H0 + 192 * rho, 192 * W, 192, Cl,
                                     hipMemcpyDeviceToDevice, sA));
      // coefficient-major [idx][pair]: row idx * Cl + j of the copy is column
      // W (idx * Cl + j) + rho of the cache (C = W Cl)
      TPST_HIP(ctx, hipMemcpy2DAsync(lc.L0.p, lb, (const uint8_t*)L0 + lb * rho, lb * W, lb, Cl * N_LINE_COEFFS,
                                     hipMemcpyDeviceToDevice, sA));
      TPST_HIP(ctx, hipMemcpy2DAsync(lc.tH.p, tb, (const uint8_t*)tH + tb * rho, tb * W, tb, Cl,
                                     hipMemcpyDeviceToDevice, sA));
      lc.W = W;
      lc.rank = rho;
    }
    H0l = lc.H0.u();
    L0l = (const LineCoeff*)lc.L0.p;
    tHl = lc.tH.u();
  }
  tA = shd ? b.tLoc.u() : st->t_A.u();
  Ca = Ca0;
  return TPST_OK;
}

// prologue (stream A): this rank's comm_list rows -> Montgomery, y = chi(b), canonical chi
int Opening::prologue() {
  {
    uint8_t* a_stage = pin + lay.a_rev;  // a_rev (canonical) -> D
    for (int i = 0; i < k; i++) memcpy(a_stage + 32 * i, point + 4 * (k - 1 - i), 32);
  }
  if (shd) {
    std::vector<uint64_t> own(Cl * 12);
    for (size_t j = 0; j < Cl; j++) memcpy(&own[12 * j], comms + 12 * (W * j + rho), 96);
    TPST_HIP(ctx, hipMemcpyAsync(b.A.p, own.data(), Cl * 96, hipMemcpyHostToDevice, sA));
    TPST_HIP(ctx, hipStreamSynchronize(sA));  // `own` is pageable and local
  } else {
    memcpy(pin + lay.cm, comms, C * 96);  // pinned: an asynchronous copy, not HIP's pageable staging
    TPST_HIP(ctx, hipMemcpyAsync(b.A.p, pin + lay.cm, C * 96, hipMemcpyHostToDevice, sA));
  }
  TPST_HIP(ctx, points_to_mont<Fq>(sA, b.A.u(), b.A.u(), Ca0));
  if (lead) {
    chis = p->chis.u();
  } else {
    if (int rc = chi_b_table(ctx, m, k, point, b.chis_own)) return rc;
    chis = b.chis_own.u();
  }
  TPST_HIP(ctx, hipMemcpyAsync(b.Y.p, chis, C * 32, hipMemcpyDeviceToDevice, sA));
  TPST_HIP(ctx, fr_from_mont(sA, chis, b.chiC.u(), C));
  TPST_HIP(ctx, hipEventRecord(ev[EV_PRE], sA));
  for (hipStream_t s2 : {sB, sLA[0], sLA[1]}) TPST_HIP(ctx, hipStreamWaitEvent(s2, ev[EV_PRE], 0));
  return TPST_OK;
}

int Opening::table_and_U() {
  // ---- look-ahead stream 1 (idle until round 1): the fold table over comm_list
  // (prebuilt by the commit of exactly these row commitments: used once), or
  // over this rank's rows
  if (shd) {
    TPST_HIP(ctx, fbt_build<Fq>(*arLA[1], sLA[1], b.A.u(), Cl, b.tLoc.u(), true));
  } else {
    const bool prebuilt = st->t_A_key.size() == 12 * C && !memcmp(st->t_A_key.data(), comms, C * 96);
    st->t_A_key.clear();
    if (!prebuilt) TPST_HIP(ctx, fbt_build<Fq>(*arLA[1], sLA[1], b.A.u(), C, st->t_A.u(), true));
  }
  TPST_HIP(ctx, hipEventRecord(ev[EV_TABLE], sLA[1]));
  // ---- stream B: U = MSM(comm_list, chi(b)) on that table, or the c_u the
  // ranks combined
  U_given = shd ? sh->U : (p->has_u ? p->U : nullptr);
  if (U_given) {
    TPST_HIP(ctx, hipEventRecord(ev[EV_U], sB));
  } else {
    TPST_HIP(ctx, hipStreamWaitEvent(sB, ev[EV_TABLE], 0));
    TraceRange trace_msm("msm");  // sqrt_pst.rs:188-199
    pf.begin(ST_MSM_U, sB);
    FbGroups gu;
    gu.members = C;
    gu.L = gu.D = C;
    gu.glv = true;
    TPST_HIP(ctx, fbt_msm<Fq>(arB, sB, tA, b.chiC.u(), gu, (Xyzz<Fq>*)b.xd.p));
    pf.end(ST_MSM_U, sB);
    TPST_HIP(ctx, hipMemcpyAsync(pin + lay.dn_U, b.xd.p, X1, hipMemcpyDeviceToHost, sB));
    TPST_HIP(ctx, hipEventRecord(ev[EV_U], sB));
  }
  return TPST_OK;
}

// PST proof of q at a_rev (stream B, after round 0's cross terms)
int Opening::pst_q() {
  TraceRange trace_pst("pst_open");  // sqrt_pst.rs:216-226
  pf.begin(ST_PST_OPEN, sB);
  const size_t a_off = lay.a_rev;
  TPST_HIP(ctx, hipMemcpyAsync(dup(a_off), pin + a_off, (size_t)k * 32, hipMemcpyHostToDevice, sB));
  TPST_HIP(ctx, fr_to_mont(sB, dup(a_off), dup(a_off), k));
  Xyzz<Fq2>* x2 = (Xyzz<Fq2>*)b.xd.p + 1;
  TPST_HIP(ctx, pst_open_fbt_s<Fq2>(sB, arB, st, st->t_php.u(), st->nv - k, p->q.u(), k, dup(a_off), x2, b.pstB.u()));
  TPST_HIP(ctx, xyzz_to_affine_canonical<Fq2>(sB, x2, b.canD.u() + 24, k));
  TPST_HIP(ctx, hipMemcpyAsync(pin + lay.dn_pst, b.canD.u() + 24, (size_t)k * 192, hipMemcpyDeviceToHost, sB));
  pf.end(ST_PST_OPEN, sB);
  return TPST_OK;
}

// One MIPP round: the host's issue order across the streams.
int Opening::round(int r, bool& done) {
  RoundTrace t;
  t.hq = open_trace() ? host_us() : 0.0;
  Round q;
  if (int rc = stage_round(r, q)) return rc;
  if (rb >= 0 && r == rb + 1) {  // the rebase table from here on (B waits for it; D, A do below)
    tA = b.tA1.u();
    Ca = C >> rb;
    TPST_HIP(ctx, hipStreamWaitEvent(sB, ev_t1, 0));
  }
  if (shd && r == r1) {
    if (int rc = hand_over(q, done)) return rc;
    if (done) return TPST_OK;
  }
  // -- A: t_l / t_r of this round, enqueued before B from round 1 on (the
  // combination gates the odd rounds and needs only the upload, while B's
  // table MSM costs the host tens of microseconds to enqueue; 2^20 open
  // 11.40 -> 11.25 ms, 2^24 25.5 -> 24.9 ms, profiles/r06/ab/ab_open_order_prio.txt)
  const bool a_first = r > 0;
  if (a_first)
    if (int rc = enqueue_t(q)) return rc;
  // B goes before the look-ahead: its comms_u gate the transcript, and the
  // look-ahead enqueue below costs the host tens of launches
  if (int rc = enqueue_cross(q)) return rc;
  t.hb = open_trace() ? host_us() : 0.0;
  if (!a_first)
    if (int rc = enqueue_t(q)) return rc;
  t.ha = open_trace() ? host_us() : 0.0;
  const bool c_first = r == 1;  // look-ahead 1 pairs this round's h
  if (c_first)
    if (int rc = enqueue_h_prep(q)) return rc;
  if (q.len >= 4)
    if (int rc = enqueue_lookahead(q)) return rc;
  t.hd = open_trace() ? host_us() : 0.0;
  if (r == 0 && lead)
    if (int rc = pst_q()) return rc;
  t.hp = open_trace() ? host_us() : 0.0;
  if (!c_first)
    if (int rc = enqueue_h_prep(q)) return rc;
  if (r == rb)
    if (int rc = enqueue_rebase(q)) return rc;
  // -- host: transcript (mipp.rs:56, 97-101) and the challenge
  if (r == 0)
    if (int rc = absorb_U()) return rc;
  return absorb_round(q, t);
}

int Opening::stage_round(int r, Round& q) {
  q.r = r;
  q.len = C >> r;
  q.s = q.len / 2;
  const size_t nW = (size_t)1 << r;
  q.loc = shd && r < r1;
  // stage c_{r-1}, c_{r-1}^-1, the look-ahead factors and digits; upload
  // once (stream B, whose previous work -- the round's comms_u -- is
  // already done when the challenge exists: on A the upload queued behind
  // A's wait for the look-ahead), form this round's weights there; A, C, D
  // wait on it
  uint8_t* stg = pin + lay.up_round(r);
  // look-ahead fold factors of h^(r) over h^(s), s = la_src(r): f_j = product
  // of c'_{r-1-b} over the set bits b of j (offset j len of h^(s)'s row)
  q.E = r == 0 ? 1 : 1 << (r - la_src(r));
  Fr f[8];
  f[0] = Fr::one();
  for (int j = 1; j < q.E; j++) {
    const int bit = 31 - __builtin_clz((unsigned)j);
    f[j] = mul(f[j ^ (1 << bit)], xs_inv[r - 1 - bit]);
  }
  memcpy(stg, cprev_c.v, 32);
  memcpy(stg + 32, cprev.v, 32);
  for (int j = 0; j < q.E; j++) memcpy(stg + 64 + 32 * j, f[j].v, 32);
  memcpy(stg + 320, la_digits, 128);
  uint32_t* dup_r = dup(lay.up_round(r));
  q.dcp = dup_r + 8;
  q.dfs = dup_r + 16;
  q.ddig = (const uint64_t*)(dup_r + 80);
  TPST_HIP(ctx, hipMemcpyAsync(dup_r, stg, Staging::UP_ROUND, hipMemcpyHostToDevice, sB));
  TPST_HIP(ctx, mipp_weights(sB, b.Wall.u(), b.Wiall.u(), r, dup_r, q.dcp));
  q.dW = b.Wall.u() + 8 * (nW - 1);
  q.dWi = b.Wiall.u() + 8 * (nW - 1);
  TPST_HIP(ctx, hipEventRecord(ev_up(r), sB));
  // (round 0's A and D work -- the direct t and the first look-ahead --
  // needs no upload: they do not wait behind B's U MSM)
  if (r > 0) TPST_HIP(ctx, hipStreamWaitEvent(sA, ev_up(r), 0));
  q.dn = pin + lay.round(r);
  return TPST_OK;
}

// a^(r1) / a^(rb) in A1x -> affine -> its fold table, `built` recorded after it
int Opening::tabulate_a1(Arena& ar, hipStream_t s, size_t len, hipEvent_t built) {
  TPST_HIP(ctx, xyzz_to_affine_mont<Fq>(s, (const Xyzz<Fq>*)b.A1x.p, b.A1.u(), len));
  TPST_HIP(ctx, fbt_build<Fq>(ar, s, b.A1.u(), len, b.tA1.u(), true));
  ev_t1 = built;
  TPST_HIP(ctx, hipEventRecord(ev_t1, s));
  return TPST_OK;
}

// -- hand-over: a^(r1) (len = 2W positions) folded by the owners of its
// positions, gathered; rank 0 tabulates it and continues alone
int Opening::hand_over(const Round& q, bool& done) {
  const size_t len = q.len, per = len / W;
  TPST_HIP(ctx, hipStreamWaitEvent(sB, ev[EV_TABLE], 0));
  TPST_HIP(ctx, mipp_scalars(sB, q.dW, nullptr, len, 0, Cl, b.ScB.u(), W, rho));
  FbGroups g;
  g.groups = per;
  g.members = C / len;
  g.L = per;
  g.D = 1;
  g.glv = true;
  const Exchange::Slot sl = xch.slot(per * X1);
  TPST_HIP(ctx, fbt_msm<Fq>(arB, sB, tA, b.ScB.u(), g, (Xyzz<Fq>*)sl.send));
  if (int rc = xch.gather(sB, sl, per * X1)) return rc;
  if (!lead) {  // this rank's part is done (its transcript stops here: tpst.h)
    pf.end(ST_MIPP_PROVE, sA);
    pf.end(ST_SQRT_OPEN, sA);
    for (hipStream_t s2 : {sA, sB, sLA[0], sLA[1], sC, ctx->comm}) TPST_HIP(ctx, hipStreamSynchronize(s2));
    sp.store(tr);
    done = true;
    return TPST_OK;
  }
  // recv[w][j] = a^(r1) at position W j + w
  for (int w = 0; w < W; w++)
    TPST_HIP(ctx, hipMemcpy2DAsync((uint8_t*)b.A1x.p + w * X1, W * X1, sl.recv + (size_t)w * per * X1, X1, X1, per,
                                   hipMemcpyDeviceToDevice, sB));
  if (int rc = tabulate_a1(arB, sB, len, xch.spare())) return rc;
  tA = b.tA1.u();
  Ca = len;
  return TPST_OK;
}

// -- A: t_l / t_r of this round (see round() for its place in the order)
int Opening::enqueue_t(const Round& q) {
  const int r = q.r;
  const size_t s = q.s;
  if (r == 0) {  // direct: the rotated comm_list (affine) against h^(0)
    if (q.loc) {  // this rank's pairs (a_i, h_{s+i}), (a_{s+i}, h_i), i = rho mod W
      TPST_HIP(ctx, affine_rot(sA, b.A.u(), b.P.u(), Cl, 24));
      arA.reset();
      TPST_HIP(ctx, arA.reserve(multi_pairing_scratch(2, s / W)));
      const Exchange::Slot sl = xch.slot(2 * sizeof(Fq12));
      TPST_HIP(ctx, multi_pairing_prepared(arA, sA, b.P.u(), H0l, L0l, 2, s / W, (Fq12*)sl.send, false, s / W, 0));
      if (int rc = xch.gather(sA, sl, 2 * sizeof(Fq12))) return rc;
      TPST_HIP(ctx, gt_prod_final(sA, (const Fq12*)sl.recv, W, 2, (Fq12*)b.gts.p));
    } else {
      TPST_HIP(ctx, affine_rot(sA, b.A.u(), b.P.u(), C, 24));
      arA.reset();
      TPST_HIP(ctx, arA.reserve(multi_pairing_scratch(2, s)));
      TPST_HIP(ctx, multi_pairing_prepared(arA, sA, b.P.u(), H0, L0, 2, s, (Fq12*)b.gts.p, true, s, 0));
    }
  } else {  // round r-1's look-ahead products, combined with c_{r-1}
    TPST_HIP(ctx, hipStreamWaitEvent(sA, ev_la(r - 1), 0));
    TPST_HIP(ctx, mipp_combine_tab(sA, (Fq12*)b.SqT[(r - 1) & 1].p, q.ddig, (Fq12*)b.SqG[(r - 1) & 1].p,
                                   (Fq12*)b.SqM.p, (Fq12*)b.gts.p));
  }
  TPST_HIP(ctx, fq12_from_mont(sA, (Fq12*)b.gts.p, b.canA.u(), 2));
  TPST_HIP(ctx, hipMemcpyAsync(q.dn + 2 * X1, b.canA.p, 1152, hipMemcpyDeviceToHost, sA));
  TPST_HIP(ctx, hipEventRecord(ev_a(r), sA));
  return TPST_OK;
}

// -- B: y fold by the previous challenge, cross MSMs u_l / u_r
// (u_l = a[:s]^y[s:], u_r = a[s:]^y[:s], on the comm_list table)
int Opening::enqueue_cross(const Round& q) {
  const int r = q.r;
  const size_t len = q.len, s = q.s;
  TPST_HIP(ctx, hipStreamWaitEvent(sB, ev_up(r), 0));
  if (r > 0) TPST_HIP(ctx, compress_fr(sB, b.Y.u(), len, q.dcp));  // y_l + c' y_r (mipp.rs:124-136)
  {  // (round 0 as two variable-base K2 MSMs over comm_list, skipping the
     // table build, measured slower: 3.4 vs 1.7 ms at 2^20)
    TPST_HIP(ctx, hipStreamWaitEvent(sB, ev[EV_TABLE], 0));
    FbGroups g;
    g.groups = 2;
    g.glv = true;
    if (q.loc) {  // partial sums over this rank's rows, gathered and summed
      TPST_HIP(ctx, mipp_scalars(sB, q.dW, b.Y.u(), len, s, Cl, b.ScB.u(), W, rho));
      g.members = C / len * s / W;
      g.L = len / W;
      g.D = s / W;
      const Exchange::Slot sl = xch.slot(2 * X1);
      TPST_HIP(ctx, fbt_msm<Fq>(arB, sB, tA, b.ScB.u(), g, (Xyzz<Fq>*)sl.send));
      if (int rc = xch.gather(sB, sl, 2 * X1)) return rc;
      TPST_HIP(ctx, xyzz_sum_groups(sB, (const Xyzz<Fq>*)sl.recv, W, 2, (Xyzz<Fq>*)b.xb.p));
    } else {
      TPST_HIP(ctx, mipp_scalars(sB, q.dW, b.Y.u(), len, s, Ca, b.ScB.u()));
      g.members = Ca / len * s;
      g.L = len;
      g.D = s;
      TPST_HIP(ctx, fbt_msm<Fq>(arB, sB, tA, b.ScB.u(), g, (Xyzz<Fq>*)b.xb.p));
    }
  }
  TPST_HIP(ctx, hipMemcpyAsync(q.dn, b.xb.p, 2 * X1, hipMemcpyDeviceToHost, sB));
  TPST_HIP(ctx, hipEventRecord(ev_b(r), sB));
  return TPST_OK;
}

// -- C: h^(r) prepared for the look-ahead of round r+1: at this rank's
// positions (sharded look-aheads) and / or at all
int Opening::enqueue_h_prep(const Round& q) {
  const int r = q.r;
  const bool c_glob = need_glob[r];
  if (need_loc[r] || c_glob) {
    TPST_HIP(ctx, hipStreamWaitEvent(sC, ev_up(r), 0));
    if (r >= 3) TPST_HIP(ctx, hipStreamWaitEvent(sC, ev_la(r - 2), 0));  // last reader of h^(r-3)'s slot
  }
  if (need_loc[r])
    if (int rc = h_prep(q, W, rho, Cl, tHl, b.Hbl[r % 3], b.Lbl[r % 3], ev_cl(r))) return rc;
  if (c_glob)
    if (int rc = h_prep(q, 1, 0, C, tH, b.Hb[r % 3], b.Lb[r % 3], ev_c(r))) return rc;
  return TPST_OK;
}

// h^(r) at the positions off mod sub (nbases = C / sub of h's points, tabulated
// in `table`): fold -> affine H -> G2Prepared L, `done` recorded after it
int Opening::h_prep(const Round& q, size_t sub, size_t off, size_t nbases, const uint32_t* table, DevBuf& H,
                    DevBuf& L, hipEvent_t done) {
  const size_t len = q.len, ln = len / sub;
  TPST_HIP(ctx, mipp_scalars(sC, q.dWi, nullptr, len, 0, nbases, b.ScC.u(), sub, off));
  FbGroups g;
  g.groups = ln;
  g.members = C / len;
  g.L = ln;
  g.D = 1;
  TPST_HIP(ctx, fbt_msm<Fq2>(arC, sC, table, b.ScC.u(), g, (Xyzz<Fq2>*)b.xh.p));
  TPST_HIP(ctx, xyzz_to_affine_mont<Fq2>(sC, (Xyzz<Fq2>*)b.xh.p, H.u(), ln));
  TPST_HIP(ctx, g2_prepare_batch(sC, H.u(), ln, (LineCoeff*)L.p, st->prep_scratch.u()));
  TPST_HIP(ctx, hipEventRecord(done, sC));
  last_c = q.r;
  return TPST_OK;
}

// -- D: look-ahead products of this round's vectors for round r+1
int Opening::enqueue_lookahead(const Round& q) {
  const int r = q.r, E = q.E;
  const size_t len = q.len;
  const bool loc = q.loc;
  hipStream_t sD = sLA[r & 1];
  Arena& arD = *arLA[r & 1];
  if (r > 0) TPST_HIP(ctx, hipStreamWaitEvent(sD, ev_up(r), 0));
  if (ev_t1) TPST_HIP(ctx, hipStreamWaitEvent(sD, ev_t1, 0));
  const size_t ln = loc ? len / W : len;  // positions this rank pairs
  arD.reset();
  TPST_HIP(ctx, arD.reserve(mipp_lookahead_scratch(ln / 4, E) + 4096));
  Exchange::Slot sl{};
  Fq12* la_out = (Fq12*)b.LAo[r & 1].p;
  if (loc) {
    sl = xch.slot(8 * sizeof(Fq12));
    la_out = (Fq12*)sl.send;
  }
  if (r == 0) {  // a^(0) = comm_list (affine), h^(0) prepared
    if (loc)
      TPST_HIP(ctx, mipp_lookahead(arD, sD, L0l, Cl, H0l, b.A.u(), false, ln, 1, la_out, false));
    else
      TPST_HIP(ctx, mipp_lookahead(arD, sD, L0, C, H0, b.A.u(), false, len, 1, la_out));
  } else {
    // E fold sets f_j a^(r): h^(r)_q = sum_j f_j h^(s)[q + j len]
    TPST_HIP(ctx, hipStreamWaitEvent(sD, ev[EV_TABLE], 0));
    uint32_t* sc = b.ScD[r & 1].u();
    FbGroups g;
    g.groups = ln;
    g.L = ln;
    g.D = 1;
    g.sets = (size_t)E;
    g.glv = true;
    if (loc) {
      TPST_HIP(ctx, mipp_scalar_sets(sD, q.dW, q.dfs, E, len, Cl, sc, W, rho));
      g.members = C / len;
      g.set_stride = Cl;
    } else {
      TPST_HIP(ctx, mipp_scalar_sets(sD, q.dW, q.dfs, E, len, Ca, sc));
      g.members = Ca / len;
      g.set_stride = Ca;
    }
    TPST_HIP(ctx, fbt_msm<Fq>(arD, sD, tA, sc, g, (Xyzz<Fq>*)b.xl[r & 1].p));
    // fbt_msm resets arD and takes its own two buffers; its result is in
    // b.xl and the look-ahead follows it on sD, so they are dead by then and
    // the look-ahead takes from the start again: arD holds the larger of the
    // two needs (fbt_msm reserves its own), not their sum
    arD.reset();
    const int src = la_src(r);  // h^(0), or h^(src) prepared by stream C in round src
    const uint32_t* hp = loc ? H0l : H0;
    const LineCoeff* lp = loc ? L0l : L0;
    if (src > 0) {
      TPST_HIP(ctx, hipStreamWaitEvent(sD, loc ? ev_cl(src) : ev_c(src), 0));
      hp = (loc ? b.Hbl : b.Hb)[src % 3].u();
      lp = (const LineCoeff*)(loc ? b.Lbl : b.Lb)[src % 3].p;
    }
    TPST_HIP(ctx, mipp_lookahead(arD, sD, lp, (size_t)E * ln, hp, b.xl[r & 1].u(), true, ln, E, la_out, !loc));
  }
  if (loc) {
    if (int rc = xch.gather(sD, sl, 8 * sizeof(Fq12))) return rc;
    TPST_HIP(ctx, gt_prod_final(sD, (const Fq12*)sl.recv, W, 8, (Fq12*)b.LAo[r & 1].p));
  }
  TPST_HIP(ctx, mipp_sq_tables(sD, (Fq12*)b.LAo[r & 1].p, (Fq12*)b.SqT[r & 1].p, (Fq12*)b.SqG[r & 1].p));
  TPST_HIP(ctx, hipEventRecord(ev_la(r), sD));
  return TPST_OK;
}

// the rebase (see rb in plan()), consumed from round rb + 1 on
int Opening::enqueue_rebase(const Round& q) {
  const size_t len = q.len;
  const hipStream_t sR = ctx->comm;
  TPST_HIP(ctx, hipStreamWaitEvent(sR, ev_up(q.r), 0));
  TPST_HIP(ctx, hipStreamWaitEvent(sR, ev[EV_TABLE], 0));
  TPST_HIP(ctx, mipp_scalars(sR, q.dW, nullptr, len, 0, C, b.ScA.u()));
  FbGroups g;
  g.groups = len;
  g.members = C / len;
  g.L = len;
  g.D = 1;
  g.glv = true;
  TPST_HIP(ctx, fbt_msm<Fq>(ctx->io, sR, tA, b.ScA.u(), g, (Xyzz<Fq>*)b.A1x.p));
  return tabulate_a1(ctx->io, sR, len, ev[EV_REBASE]);
}

// U, before round 0's comms (mipp.rs:56)
int Opening::absorb_U() {
  TPST_HIP(ctx, hipEventSynchronize(ev[EV_U]));
  if (U_given)
    memcpy(proof->U, U_given, 96);
  else
    xyzz_to_canonical_host<Fq>(pin + lay.dn_U, 1, proof->U);
  uint8_t ser[96];
  g1_bytes(proof->U, ser);
  sp.absorb_bytes(ser, 96);
  return TPST_OK;
}

// the round's comms into the transcript (mipp.rs:97-101), the challenge and
// what the next round derives from it
int Opening::absorb_round(const Round& q, const RoundTrace& t) {
  const int r = q.r;
  // comms_u (stream B) is ready well before comms_t (the final
  // exponentiations): absorb it while stream A finishes (mipp.rs:97-100
  // order: u_l, u_r, t_l, t_r)
  const double h0 = host_us();
  TPST_HIP(ctx, hipEventSynchronize(ev_b(r)));
  const double h1 = host_us();
  xyzz_to_canonical_host<Fq>(q.dn, 2, proof->comms_u[r][0]);
  uint8_t ser[96];
  g1_bytes(proof->comms_u[r][0], ser);
  sp.absorb_bytes(ser, 96);
  g1_bytes(proof->comms_u[r][1], ser);
  sp.absorb_bytes(ser, 96);
  const double h2 = host_us();
  TPST_HIP(ctx, hipEventSynchronize(ev_a(r)));
  const double h3 = host_us();
  memcpy(proof->comms_t[r][0], q.dn + 2 * X1, 576);
  memcpy(proof->comms_t[r][1], q.dn + 2 * X1 + 576, 576);
  sp.absorb_bytes((const uint8_t*)proof->comms_t[r][0], 576);
  sp.absorb_bytes((const uint8_t*)proof->comms_t[r][1], 576);
  const double h4 = host_us();
  uint64_t ci_c[4];
  sp.challenge(ci_c);  // mipp.rs:101
  const Fr c_inv = fr_canon(ci_c);
  const double h5 = host_us();
  const Fr c = inv(c_inv);  // mipp.rs:106
  if (open_trace())
    fprintf(stderr,
            "open round %d%s: enqueue %.0f (B %.0f A %.0f D %.0f pst %.0f C %.0f) wait_u %.0f absorb_u %.0f wait_t %.0f "
            "absorb_t %.0f challenge %.0f inv %.0f us\n",
            r, q.loc ? " (sharded)" : "", h0 - t.hq, t.hb - t.hq, t.ha - t.hb, t.hd - t.ha, t.hp - t.hd, h0 - t.hp,
            h1 - h0, h2 - h1, h3 - h2, h4 - h3, h5 - h4, host_us() - h5);
  xs_inv.push_back(c_inv);
  cprev = c_inv;
  cprev_c = c;
  // base-x digits of (c^-1, c, c^-1, c) for the next round's combination
  {
    uint64_t ci[4], cc[4];
    fr_out(c_inv, ci);
    fr_out(c, cc);
    base_x_digits(ci, la_digits);
    base_x_digits(cc, la_digits + 4);
    memcpy(la_digits + 8, la_digits, 64);
  }
  return TPST_OK;
}

// ---- epilogue: final_a (A), final_h (C), pst_proof_h (B); rs need only the
// transcript state after the last round (mipp.rs:138-141)
int Opening::epilogue() {
  // final weights W_m, Wi_m (device); the p_h evaluations of mipp.rs:159-180,
  // prod over the set bits j of t of c^-1_{m-1-j}, are exactly Wi_m[t]
  {
    uint8_t* stg = pin + lay.up_final;
    memcpy(stg, cprev_c.v, 32);
    memcpy(stg + 32, cprev.v, 32);
    for (int i = 0; i < m; i++) {
      uint64_t cc[4];
      sp.challenge(cc);
      const Fr rr = fr_canon(cc);
      memcpy(stg + 32 * (2 + i), rr.v, 32);
    }
  }
  uint32_t* dfin = dup(lay.up_final);
  TPST_HIP(ctx, hipMemcpyAsync(dfin, pin + lay.up_final, (2 + m) * 32, hipMemcpyHostToDevice, sA));
  TPST_HIP(ctx, mipp_weights(sA, b.Wall.u(), b.Wiall.u(), m, dfin, dfin + 8));
  const uint32_t* dWm = b.Wall.u() + 8 * (C - 1);
  const uint32_t* dWim = b.Wiall.u() + 8 * (C - 1);
  TPST_HIP(ctx, hipEventRecord(ev[EV_FINAL_UP], sA));
  TPST_HIP(ctx, hipStreamWaitEvent(sA, ev[EV_TABLE], 0));
  if (ev_t1) TPST_HIP(ctx, hipStreamWaitEvent(sA, ev_t1, 0));
  {  // final_a = a^(m)_0 (one group over the a-side bases: all C, or the gathered a^(r1))
    FbGroups g;
    g.members = Ca;
    TPST_HIP(ctx, mipp_scalars(sA, dWm, nullptr, 1, 0, Ca, b.ScA.u()));
    g.glv = true;
    TPST_HIP(ctx, fbt_msm<Fq>(arA, sA, tA, b.ScA.u(), g, (Xyzz<Fq>*)b.xa.p));
    TPST_HIP(ctx, hipMemcpyAsync(pin + lay.dn_final, b.xa.p, X1, hipMemcpyDeviceToHost, sA));
  }
  TPST_HIP(ctx, hipStreamWaitEvent(sCe, ev[EV_FINAL_UP], 0));
  if (last_c >= 0) TPST_HIP(ctx, hipStreamWaitEvent(sCe, ev_c(last_c), 0));  // xh / ScC / arC reuse
  if (last_c >= 0 && need_loc[last_c]) TPST_HIP(ctx, hipStreamWaitEvent(sCe, ev_cl(last_c), 0));
  {  // final_h = h^(m)_0
    FbGroups g;
    g.members = C;
    TPST_HIP(ctx, mipp_scalars(sCe, dWim, nullptr, 1, 0, C, b.ScC.u()));
    TPST_HIP(ctx, fbt_msm<Fq2>(arC, sCe, tH, b.ScC.u(), g, (Xyzz<Fq2>*)b.xh.p));
    TPST_HIP(ctx, hipMemcpyAsync(pin + lay.dn_fh, b.xh.p, X2, hipMemcpyDeviceToHost, sCe));
    TPST_HIP(ctx, hipEventRecord(ev[EV_C_DONE], sCe));
  }
  // pst_proof_h = open_g1(p_h, rs) (mipp.rs:144)
  TPST_HIP(ctx, hipStreamWaitEvent(sB, ev[EV_FINAL_UP], 0));
  TPST_HIP(ctx, pst_open_fbt_s<Fq>(sB, arB, st, st->t_pgp.u(), st->nv - m, dWim, m, dfin + 16, (Xyzz<Fq>*)b.xp.p,
                                   b.pstA.u()));
  TPST_HIP(ctx, xyzz_to_affine_canonical<Fq>(sB, (Xyzz<Fq>*)b.xp.p, b.canC.u() + 48, m));
  TPST_HIP(ctx, hipMemcpyAsync(pin + lay.dn_ph, b.canC.u() + 48, (size_t)m * 96, hipMemcpyDeviceToHost, sB));
  TPST_HIP(ctx, hipEventRecord(ev[EV_B_DONE], sB));
  if (pf.on) {  // device spans end when every stream of the opening has drained
    TPST_HIP(ctx, hipEventRecord(ev[EV_D_DONE], sLA[0]));
    TPST_HIP(ctx, hipEventRecord(ev[EV_A_DONE], sLA[1]));
    for (int e : {(int)EV_B_DONE, (int)EV_C_DONE, (int)EV_D_DONE, (int)EV_A_DONE})
      TPST_HIP(ctx, hipStreamWaitEvent(sA, ev[e], 0));
    pf.end(ST_MIPP_PROVE, sA);
    pf.end(ST_SQRT_OPEN, sA);
  }
  for (hipStream_t s2 : {sA, sB, sLA[0], sLA[1], sC}) TPST_HIP(ctx, hipStreamSynchronize(s2));
  if (shd || rb >= 0) TPST_HIP(ctx, hipStreamSynchronize(ctx->comm));
  xyzz_to_canonical_host<Fq>(pin + lay.dn_final, 1, proof->final_a);
  xyzz_to_canonical_host<Fq2>(pin + lay.dn_fh, 1, proof->final_h);
  memcpy(proof->pst_proof_h, pin + lay.dn_ph, (size_t)m * 96);
  memcpy(proof->pst_proof, pin + lay.dn_pst, (size_t)k * 192);
  sp.store(tr);
  return TPST_OK;
}

int poly_open(tpst_ctx* ctx, tpst_poly* p, tpst_transcript* tr, int n, const uint64_t* comms, const uint64_t* point,
              tpst_open_proof* proof, const Shard* sh) {
  const bool lead = !sh || sh->rank == 0;  // produces the proof (and the PST proof of q)
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  if (lead)
    if (int rc = poly_need_q_source(ctx, p)) return rc;
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  SrsState* st = srs_of(ctx);
  if (!st) return fail(ctx, TPST_E_STATE, "no SRS loaded");
  Opening o(ctx, st, p, tr, n, comms, point, proof, sh);
  return o.run();
}

}  // namespace

extern "C" int tpst_poly_open(tpst_ctx* ctx, tpst_poly* p, tpst_transcript* tr, const uint64_t* comms,
                              const uint64_t* point, const uint64_t* T, tpst_open_proof* proof) {
  (void)T;  // the reference passes T but the prover does not use it (mipp.rs:38)
  if (!ctx || !p || !tr || !comms || !point || !proof) return fail(ctx, TPST_E_ARG, "null argument");
  return poly_open(ctx, p, tr, p->n, comms, point, proof, nullptr);
}

extern "C" int tpst_poly_open_sharded(tpst_ctx* ctx, tpst_poly* p, tpst_transcript* tr, int n, const uint64_t* comms,
                                      const uint64_t* point, const uint64_t* U, const tpst_exchange* x,
                                      tpst_open_proof* proof) {
  if (!ctx || !tr || !comms || !point || !U || !x) return fail(ctx, TPST_E_ARG, "null argument");
  if (x->world < 1 || (x->world & (x->world - 1)) || x->rank < 0 || x->rank >= x->world)
    return fail(ctx, TPST_E_ARG, "world must be a power of two and 0 <= rank < world");
  if (x->rank == 0 && (!p || !proof)) return fail(ctx, TPST_E_ARG, "rank 0 needs the opening handle and the proof");
  if (p && p->n != n) return fail(ctx, TPST_E_ARG, "handle num_vars != n");
  if (!point_valid<Fq>(U)) return fail(ctx, TPST_E_ARG, "c_u is not a valid G1 point");
  for (int i = 0; i < n; i++)
    if (!fr_ok(point + 4 * i)) return fail(ctx, TPST_E_ARG, "point coordinate >= r");
  const int m = n / 2;
  if (shard_rounds(m, x->world) == 0) {  // too few rows to split: rank 0 opens alone
    if (x->rank != 0) return TPST_OK;
    const bool had = p->has_u;
    uint64_t keep[12];
    memcpy(keep, p->U, 96);
    memcpy(p->U, U, 96);
    p->has_u = true;
    const int rc = poly_open(ctx, p, tr, n, comms, point, proof, nullptr);
    memcpy(p->U, keep, 96);
    p->has_u = had;
    return rc;
  }
  Shard sh;
  sh.W = x->world;
  sh.rank = x->rank;
  sh.x = x;
  sh.U = U;
  return poly_open(ctx, p, tr, n, comms, point, proof, &sh);
}
