// The variable-base MSM driver (msm_var<F>) and the point-format conversions;
// instantiated for G1 in msm.hip and for G2 in msm_g2.hip.
#pragma once
#include <cstdio>
#include <cstring>
#include "msm_sort.h"
#include "msm_acc.h"
#include "msm_reduce.h"

namespace tpst {

template <class F>
__global__ void k_points_to_mont(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Affine<F> a = load_affine<F>(in, i);
  Fq* c = reinterpret_cast<Fq*>(&a);
#pragma unroll
  for (int k = 0; k < (int)(sizeof(Affine<F>) / sizeof(Fq)); k++) c[k] = to_mont(c[k]);
  store_affine(out, i, a);
}

template <class F>
__global__ void k_affine_from_mont(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Affine<F> a = load_affine<F>(in, i);
  Fq* c = reinterpret_cast<Fq*>(&a);
#pragma unroll
  for (int k = 0; k < (int)(sizeof(Affine<F>) / sizeof(Fq)); k++) c[k] = from_mont(c[k]);
  store_affine(out, i, a);
}

template <class F>
__global__ void __launch_bounds__(64, 1) k_xyzz_to_affine_canonical(const Xyzz<F>* __restrict__ in, uint32_t* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Affine<F> a = to_affine(load_xyzz(in, i));
  Fq* c = reinterpret_cast<Fq*>(&a);
#pragma unroll
  for (int k = 0; k < (int)(sizeof(Affine<F>) / sizeof(Fq)); k++) c[k] = from_mont(c[k]);
  store_affine(out, i, a);
}

// the same with one wave per point and the wave-cooperative inverse
// (inv_wave.h): for the few-point conversions on a latency path
template <class F>
__global__ void __launch_bounds__(64) k_xyzz_to_affine_wave(const Xyzz<F>* __restrict__ in, uint32_t* __restrict__ out, size_t n) {
  const size_t i = blockIdx.x;
  if (i >= n) return;
  Affine<F> a = to_affine_w(load_xyzz(in, i));
  Fq* c = reinterpret_cast<Fq*>(&a);
#pragma unroll
  for (int k = 0; k < (int)(sizeof(Affine<F>) / sizeof(Fq)); k++) c[k] = from_mont(c[k]);
  if (threadIdx.x == 0) store_affine(out, i, a);
}

// up to this many points one wave-cooperative inverse per point
// (k_xyzz_to_affine_wave); above it one lone-lane inverse per point
constexpr size_t INV_WAVE_MAX = 4096;

template <class F>
hipError_t points_to_mont(hipStream_t s, const uint32_t* d_in, uint32_t* d_out, size_t n) {
  if (!n) return hipSuccess;
  k_points_to_mont<F><<<grid_for(n, 256), 256, 0, s>>>(d_in, d_out, n);
  return hipGetLastError();
}

template <class F>
hipError_t affine_from_mont(hipStream_t s, const uint32_t* d_in, uint32_t* d_out, size_t n) {
  if (!n) return hipSuccess;
  k_affine_from_mont<F><<<grid_for(n, 256), 256, 0, s>>>(d_in, d_out, n);
  return hipGetLastError();
}

template <class F>
hipError_t xyzz_to_affine_canonical(hipStream_t s, const Xyzz<F>* d_in, uint32_t* d_out, size_t n) {
  if (!n) return hipSuccess;
  if (n <= INV_WAVE_MAX)
    k_xyzz_to_affine_wave<F><<<(unsigned)n, 64, 0, s>>>(d_in, d_out, n);
  else
    k_xyzz_to_affine_canonical<F><<<grid_for(n, 64), 64, 0, s>>>(d_in, d_out, n);
  return hipGetLastError();
}

// the last window group's fixup (on the MSM's tail) runs one quad of lanes
// per bucket in a lone call; the aux-stream groups one lane per bucket at
// s_setprio 2 (priority 0 there measured slower and erratic, 298-310 against
// 311 Mscalar/s: profiles/fixup_order)
constexpr int RED_PRIO = 2;

// window groups of the variable-base MSM (3; sweep of 1-5 in
// profiles/r02/sw2): with more than one, the groups' bucket accumulations run
// top group first on the main stream; each finished group's reduction (the
// two-level one) and doubling chain run on an aux stream under the next
// group's accumulation, so only the last group's reduction and its
// c-doubling Horner remain after the accumulation
static int msm_groups(size_t n, int W) {
  if (n < ((size_t)1 << 17) || W < 4) return 1;
  int g = 3;
  if (g > (Arena::N_AUX_EV - 1) / 2) g = (Arena::N_AUX_EV - 1) / 2;
  return g > W ? W : g;
}

// window boundaries wb[0..NG] of the groups: a short bottom group (~W/8
// windows: its reduction and chain are the tail left after the accumulation)
// and an even split of the rest -- 1,3,4 for the 2^20 G1 MSM, 1.3 % faster
// than 2,3,3 in an interleaved A/B (profiles/r02/sw2)
static void msm_group_bounds(int W, int NG, int* wb) {
  if (NG == 1) {
    wb[0] = 0;
    wb[1] = W;
  } else {
    const int lo = W / 8 > 1 ? W / 8 : 1;
    wb[0] = 0;
    for (int g = 1; g <= NG; g++) wb[g] = lo + (g - 1) * (W - lo) / (NG - 1);
  }
}

// TPST_MSM_TAIL=auto|latency|throughput (read once per process): which tail
// forms the window-grouped G1 MSM takes.  auto (the default): msm_var's
// `throughput` argument, i.e. the caller's regime; the other two force one
// set for every call (A/B, tests).  0 auto, 1 latency, 2 throughput.
static int msm_tail_mode() {
  static const int mode = [] {
    const char* e = getenv("TPST_MSM_TAIL");
    if (e && !strcmp(e, "latency")) return 1;
    if (e && !strcmp(e, "throughput")) return 2;
    return 0;
  }();
  return mode;
}

// TPST_MSM_TAIL_TRACE=1 (diagnostics): one stderr line per window-grouped G1
// MSM naming the tail forms it took
static void msm_tail_trace(bool grouped, bool throughput, size_t n) {
  static const bool on = getenv("TPST_MSM_TAIL_TRACE") != nullptr;
  if (on && grouped) fprintf(stderr, "msm tail %s n=%zu\n", throughput ? "throughput" : "latency", n);
}

template <class F>
hipError_t msm_var(Arena& ar, hipStream_t s, const uint32_t* d_bases, const uint32_t* d_scalars, size_t n,
                   Xyzz<F>* d_out, hipStream_t tail, bool* on_tail, hipStream_t front, bool throughput) {
  if (on_tail) *on_tail = false;
  if (n == 0) {
    Xyzz<F> inf = Xyzz<F>::inf();
    return hipMemcpyAsync(d_out, &inf, sizeof(inf), hipMemcpyHostToDevice, s);
  }
  if (n > MSM_MAX_POINTS) return hipErrorInvalidValue;
  static_assert(2 * MSM_MAX_POINTS - 1 <= VAL_INDEX, "a GLV index must fit below the flags of a sorted value");
  const bool glv = n >= 64;  // phi(x, y) = (beta x, y) on G1, (beta^2 x, y) on G2
  // G1 with GLV: gather records of P and phi(P) (fetch_rec29) instead of phi(P) alone
  constexpr bool g1 = std::is_same<F, Fq>::value;
  const bool rec29 = glv && g1;
  constexpr size_t PW = 2 * Words<F>::n;
  const int c = msm_window_bits(glv ? 2 * n : n);
  const int W = glv ? num_windows_bits(c, 128) : num_windows(c);
  const uint32_t nb = 1u << (c - 1);
  const size_t per_win = (size_t)(glv ? 2 : 1) * n;  // entries of one window (zero digits included)
  const size_t m = per_win * W;
  if (m >= ((size_t)1 << 31)) return hipErrorInvalidValue;
  const size_t nbk = (size_t)W * nb;
  const uint32_t sent = (uint32_t)nbk;  // zero digits; sorts after every bucket key
  SortPlan sp;
  if (!sort_plan(sent, n, m, sp)) return hipErrorInvalidValue;
  const int NG = msm_groups(n, W);
  // Tail forms (G1, window groups).  Latency: what finishes a lone call
  // soonest -- group 0's fixup and group 1's reduction on quads of lanes.
  // Throughput: the call's tail runs under the next call's accumulation, its
  // latency is hidden and its instructions take issue slots from that
  // accumulation -- both run one lane per bucket / segment (the quad forms
  // cost 1.7x / 2x the instructions).  A/Bs of these two and of the members
  // that lost (group 0's reduction two-level, aux priority 0, two groups):
  // profiles/fixup_order.
  const bool tp = g1 && NG > 1 && (msm_tail_mode() == 2 || (msm_tail_mode() == 0 && throughput));
  msm_tail_trace(g1 && NG > 1, tp, n);
  int wb[Arena::N_AUX_EV / 2 + 1];
  msm_group_bounds(W, NG, wb);
  if (NG > 1) TPST_TRY(ar.aux_init());
  // chunk length 2^lg of the short-chunk accumulation.  One group (n < 2^17,
  // at most 2.62 M entries): 32-entry chunks.
  int lg = 5;
  if (NG > 1) {  // per-group launches: keep >= 4 waves per SIMD in each
    static const size_t simds = device_simds();
    // 16-entry chunks: 8 / 32 / 64 measured 4 / 7 / 18 % slower (profiles/r05/g);
    // 8 against 16 again with the chain-start add: profiles/chain_start
    lg = TPST_K2_LG;
    while (lg < 8 && ((m / NG) >> (lg + 1)) >= (size_t)4 * 64 * simds) lg++;
  }
  const size_t nchunk = (m + ((size_t)1 << lg) - 1) >> lg;
  size_t red_need = 0;
  for (int g = 0; g < NG; g++) {
    const size_t gw = (size_t)(wb[g + 1] - wb[g]);
    red_need += reduce_scratch<F>(gw, nb) + (red2_ok(nb) ? reduce2_scratch<F>(gw, nb) : 0);
  }
  size_t need = Arena::need(m, 4) * 4 + Arena::need(nbk, 4) * 2 + Arena::need(nbk, sizeof(Xyzz<F>)) +
                Arena::need(2 * nchunk, sizeof(Xyzz<F>)) + red_need +
                Arena::need(W, sizeof(Xyzz<F>)) + Arena::need(NG, sizeof(Xyzz<F>)) + Arena::need(W + 1, 4) +
                Arena::need(glv && !rec29 ? n * PW : 1, 4) + Arena::need(rec29 ? 2 * n * REC29_WORDS : 1, 4) +
                Arena::need((size_t)sp.ntile * sp.nbins, 4) +
                Arena::need(sp.nbins, 4) + Arena::need(sp.nbins + 1, 4) +
                Arena::need((size_t)NG * (1 + 2 * FIXUP_CLASSES), 4) + Arena::need(g1 ? nbk : 1, 4) +
                Arena::need((size_t)NG * (m / ((size_t)LONG_PARTS << lg) + 1), 4) + 8192;
  ar.reset();
  TPST_TRY(ar.reserve(need));
  uint32_t* keys = ar.take<uint32_t>(m);
  uint32_t* vals = ar.take<uint32_t>(m);
  uint32_t* keys2 = ar.take<uint32_t>(m);
  uint32_t* vals2 = ar.take<uint32_t>(m);
  uint32_t* bstart = ar.take<uint32_t>(nbk);
  uint32_t* bend = ar.take<uint32_t>(nbk);
  Xyzz<F>* buckets = ar.take<Xyzz<F>>(nbk);
  Xyzz<F>* part = ar.take<Xyzz<F>>(2 * nchunk);
  Xyzz<F>* win = ar.take<Xyzz<F>>(W);
  Xyzz<F>* contrib = ar.take<Xyzz<F>>(NG);
  uint32_t* range = ar.take<uint32_t>(W + 1);
  uint32_t* phib = ar.take<uint32_t>(glv && !rec29 ? n * PW : 1);
  uint32_t* rec = rec29 ? ar.take<uint32_t>(2 * n * REC29_WORDS) : nullptr;
  const uint32_t* gb = rec29 ? rec : d_bases;  // what the accumulation gathers
  const uint32_t gnb = rec29 ? 0x7fffffffu : (uint32_t)n;
  uint32_t* tab = ar.take<uint32_t>((size_t)sp.ntile * sp.nbins);
  uint32_t* btot = ar.take<uint32_t>(sp.nbins);
  uint32_t* bin0 = ar.take<uint32_t>(sp.nbins + 1);
  // a listed bucket spans more than LONG_PARTS chunks, so more than
  // LONG_PARTS << lg entries, and buckets are disjoint: at most m / (LONG_PARTS
  // << lg) of them in any group (the list can never overflow)
  const uint32_t lcap = (uint32_t)(m / ((size_t)LONG_PARTS << lg)) + 1;
  // zeroed per call: the long lists' counts, then (G1) the fixup order's
  // class counts and cursors of every group
  const size_t nmeta = (size_t)NG * (1 + 2 * FIXUP_CLASSES);
  uint32_t* lcnt = ar.take<uint32_t>(nmeta);
  uint32_t* fhist = lcnt + NG;
  uint32_t* fcur = fhist + (size_t)NG * FIXUP_CLASSES;
  uint32_t* order = ar.take<uint32_t>(g1 ? nbk : 1);  // group g's listed buckets at order[wb[g] nb ..)
  uint32_t* llist = ar.take<uint32_t>((size_t)NG * lcap);

  Profiler* pf = ar.prof;
  Profiler dummy;
  if (!pf) pf = &dummy;
  const hipStream_t fs = front ? front : s;
  pf->begin(ST_DECOMPOSE, fs);
  TPST_TRY(hipMemsetAsync(lcnt, 0, nmeta * sizeof(uint32_t), fs));
  k_decompose_hist<F><<<sp.ntile, SORT_THREADS, sp.nbins * 4, fs>>>(d_scalars, n, c, W, glv ? 1 : 0, sent, sp.lo,
                                                                  sp.nbins, sp.tile, keys, vals, tab, d_bases, phib,
                                                                  rec);
  TPST_TRY(hipGetLastError());
  pf->end(ST_DECOMPOSE, fs);
  pf->begin(ST_SORT, fs);
  k_sort_colscan<<<grid_for(sp.nbins, 64), 64 * COLSCAN_CH, 0, fs>>>(tab, sp.ntile, sp.nbins, btot);
  TPST_TRY(hipGetLastError());
  k_sort_binscan<<<1, BINSCAN_THREADS, 0, fs>>>(btot, sp.nbins, bin0);
  TPST_TRY(hipGetLastError());
  const int halves = glv ? 2 : 1;
  const uint32_t bpw = nb >> sp.lo;
  // stage of E entries per thread (E = 4, or 2 when the bin cursors are many)
  const auto scat_lds = [&](int E) { return ((size_t)sp.nbins + 2 * (bpw + 1) + 2 * (size_t)E * SORT_THREADS) * 4; };
  const int E = scat_lds(4) <= 60 * 1024 ? 4 : (scat_lds(2) <= 60 * 1024 ? 2 : 0);
  if (sp.lo <= c - 1 && E) {  // bins aligned to windows, stage fits
    if (E == 4)
      k_sort_scatter_win<4><<<sp.ntile, SORT_THREADS, scat_lds(4), fs>>>(keys, vals, n, halves, W, sent, sp.lo,
                                                                       sp.nbins, bpw, sp.tile, tab, bin0, keys2, vals2);
    else
      k_sort_scatter_win<2><<<sp.ntile, SORT_THREADS, scat_lds(2), fs>>>(keys, vals, n, halves, W, sent, sp.lo,
                                                                       sp.nbins, bpw, sp.tile, tab, bin0, keys2, vals2);
  } else {
    k_sort_scatter<<<sp.ntile, SORT_THREADS, sp.nbins * 4, fs>>>(keys, vals, n, (uint32_t)(halves * W), sp.lo,
                                                                sp.nbins, sp.tile, tab, bin0, keys2, vals2);
  }
  TPST_TRY(hipGetLastError());
  // sorted entries back into keys / vals; bucket bounds, empty buckets, range
  k_sort_bin<<<sp.nbins, SORTB_THREADS, (2u << sp.lo) * 4 + SORTB_CAP * 4, fs>>>(
      keys2, vals2, bin0, sp.lo, sent, nb, W, keys, vals, bstart, bend, reinterpret_cast<uint4*>(buckets),
      (uint32_t)(sizeof(Xyzz<F>) / 16), range);
  TPST_TRY(hipGetLastError());
  pf->end(ST_SORT, fs);
  if (fs != s) {  // the accumulation waits for the sort
    TPST_TRY(ar.aux_init());
    TPST_TRY(hipEventRecord(ar.aux_ev[Arena::N_AUX_EV - 1], fs));
    TPST_TRY(hipStreamWaitEvent(s, ar.aux_ev[Arena::N_AUX_EV - 1], 0));
  }
  // groups accumulate on the context stream; the fixup / reduction / chain of
  // group g > 0 run on an aux stream (a separate low-priority accumulation
  // stream measured slower: 4+ streams share the hardware queues)
  hipStream_t bulk = s;
  // the last group's tail: on `tail` when the caller pipelines calls
  const hipStream_t t0 = (tail && NG > 1) ? tail : s;
  if (on_tail) *on_tail = t0 != s;
  pf->begin(ST_BUCKET_ACC, bulk);
  for (int g = NG - 1; g >= 0; g--) {  // top windows first: their chains are the longest
    const int wlo = wb[g], whi = wb[g + 1];
    const size_t gchunks = ((per_win * (size_t)(whi - wlo)) >> lg) + 2;
    if constexpr (std::is_same<F, Fq2>::value) {
      k_bucket_acc_short_pair<<<grid_for(2 * gchunks, 64), 64, 0, bulk>>>(keys, vals, range, wlo, whi, sent,
                                                                          bstart, bend, d_bases, phib, (uint32_t)n,
                                                                          lg, buckets, part);
    } else {
      // the next point staged through LDS (default: 277-279 vs 273 Mscalar/s
      // with the register prefetch, profiles/r05/l); TPST_ACC_LDS=0 selects
      // the register prefetch
      static const bool lds = [] {
        const char* e = getenv("TPST_ACC_LDS");
        return !e || atoi(e) != 0;
      }();
      const unsigned grid = grid_for(gchunks, 64);
      if (lds && rec29)
        k_bucket_acc_short_lds<TPST_K2_MINW, true><<<grid, 64, 0, bulk>>>(keys, vals, range, wlo, whi, sent, bstart, bend, gb,
                                                                nullptr, gnb, lg, buckets, part);
      else if (lds)
        k_bucket_acc_short_lds<2, false><<<grid, 64, 0, bulk>>>(keys, vals, range, wlo, whi, sent, bstart, bend,
                                                                 d_bases, phib, (uint32_t)n, lg, buckets, part);
      else if (rec29)
        k_bucket_acc_short<F, 2, true><<<grid, 64, 0, bulk>>>(keys, vals, range, wlo, whi, sent, bstart, bend, gb,
                                                               nullptr, gnb, lg, buckets, part);
      else
        k_bucket_acc_short<F><<<grid, 64, 0, bulk>>>(keys, vals, range, wlo, whi, sent, bstart, bend, d_bases, phib,
                                                      (uint32_t)n, lg, buckets, part);
    }
    TPST_TRY(hipGetLastError());
    if (g == 0) pf->end(ST_BUCKET_ACC, bulk);
    const size_t b0 = (size_t)wlo * nb, b1 = (size_t)whi * nb;
    hipStream_t a = g ? ar.aux[g % Arena::N_AUX] : t0;
    const LongList ll{lcnt + g, llist + (size_t)g * lcap, lcap};
    uint32_t* const ghist = fhist + g * FIXUP_CLASSES;
    // G1: the group's fixup order and long list (msm_acc.h), on the group's own
    // stream.  With the sort on `front` they wait for the sort alone and run
    // beside the accumulation; otherwise they follow it.  (On `front` itself
    // they cost the pipelined MSM 0.6 %: two more launches in the chain of
    // low-priority sort kernels that the next accumulation waits for;
    // profiles/fixup_order.)
    const auto fixup_order = [&]() -> hipError_t {
      if constexpr (g1) {
        const unsigned grid = grid_for(b1 - b0, ORDER_THREADS);
        k_fixup_hist<<<grid, ORDER_THREADS, 0, a>>>(bstart, bend, (uint32_t)b0, (uint32_t)b1, lg, ghist);
        TPST_TRY(hipGetLastError());
        k_fixup_order<<<grid, ORDER_THREADS, 0, a>>>(bstart, bend, (uint32_t)b0, (uint32_t)b1, lg, ghist,
                                                     fcur + g * FIXUP_CLASSES, order + b0, ll);
        TPST_TRY(hipGetLastError());
      }
      return hipSuccess;
    };
    if (fs != s) {
      TPST_TRY(hipStreamWaitEvent(a, ar.aux_ev[Arena::N_AUX_EV - 1], 0));
      TPST_TRY(fixup_order());
    }
    if (NG > 1) {
      TPST_TRY(hipEventRecord(ar.aux_ev[2 * g], bulk));
      TPST_TRY(hipStreamWaitEvent(a, ar.aux_ev[2 * g], 0));
    }
    if (fs == s) TPST_TRY(fixup_order());
    if constexpr (std::is_same<F, Fq2>::value)
      k_bucket_fixup_short_pair<<<grid_for(2 * (b1 - b0), 64), 64, 0, a>>>(bstart, bend, b0, b1, lg, part, buckets,
                                                                          g ? RED_PRIO : 0, ll);
    else if (g == 0 && !tp)
      k_bucket_fixup_quad<F><<<grid_for(4 * (b1 - b0), 64), 64, 0, a>>>(bstart, bend, order + b0, ghist, lg, part,
                                                                        buckets);
    else
      k_bucket_fixup_short<F><<<grid_for(b1 - b0, 64), 64, 0, a>>>(bstart, bend, order + b0, ghist, lg, part, buckets,
                                                                    g ? RED_PRIO : 0);
    TPST_TRY(hipGetLastError());
    k_bucket_fixup_long<F><<<LONG_GRID, LONG_THREADS, 0, a>>>(bstart, bend, lg, part, buckets, ll);
    TPST_TRY(hipGetLastError());
    if (g == 0) break;
    if (red2_ok(nb))
      // lane form (fewer issue slots) for the groups with slack; the group
      // before the last keeps the quads in a lone call, where its tail ends
      // right after the last group's
      TPST_TRY(reduce_buckets2<F>(ar, a, buckets + b0, (size_t)(whi - wlo), nb, win + wlo, RED_PRIO, g >= 2 || tp));
    else
      TPST_TRY(reduce_buckets<F>(ar, a, buckets + b0, (size_t)(whi - wlo), nb, win + wlo, RED_PRIO));
    k_window_chain<F><<<1, 64, 0, a>>>(win, wlo, whi, c, nullptr, 0, contrib + g);
    TPST_TRY(hipGetLastError());
    TPST_TRY(hipEventRecord(ar.aux_ev[2 * g + 1], a));
  }
  const int w1 = wb[1];  // group 0 = windows [0, w1)
  pf->begin(ST_REDUCE, t0);
  // the last group's reduction is the call's tail: the short-segment form
  // (the two-level one measured slower here: 285-290 vs 295 Mscalar/s, a lone
  // call 5.5 vs 5.1 ms, profiles/r06/ab_g0_red2.jsonl; and again in lane form
  // under the next call's accumulation, 299 vs 311: profiles/fixup_order)
  TPST_TRY(reduce_buckets<F>(ar, t0, buckets, (size_t)w1, nb, win));
  pf->end(ST_REDUCE, t0);
  pf->begin(ST_COMBINE, t0);
  for (int g = 1; g < NG; g++) TPST_TRY(hipStreamWaitEvent(t0, ar.aux_ev[2 * g + 1], 0));
  k_window_chain<F><<<1, 64, 0, t0>>>(win, 0, w1, c, contrib + 1, NG - 1, d_out);
  TPST_TRY(hipGetLastError());
  pf->end(ST_COMBINE, t0);
  return hipSuccess;
}

}  // namespace tpst
