// Bucket accumulation kernels and their fixups (K2 short chunks, K1 long chunks).
#pragma once
#include "msm_common.h"
#include "msm_pieces.h"

namespace tpst {

// K1 window-table record (msm_batch): one affine point already in the
// accumulation field (field29.h radix 2^29, canonical), x (13 words) | y
// (13 words) | 6 pad words = 128 bytes, so a gather is ONE aligned 128-byte
// line (a 96-byte field.h point straddles two lines 3 times in 4) and needs
// no conversion in the accumulation loop.
// rec29_point: the point of a record's first 28 words w, negated when v's
// sign bit is set; fetch_rec29 gathers the record of value v from the table.
__device__ __forceinline__ Affine<Fq29> rec29_point(const uint32_t* w, uint32_t v) {
  Affine<Fq29> p;
#pragma unroll
  for (int i = 0; i < r29::N; i++) {
    p.x.v[i] = w[i];
    p.y.v[i] = w[r29::N + i];
  }
  p.y = cneg(p.y, (v >> 31) != 0);
  return p;
}

__device__ __forceinline__ Affine<Fq29> fetch_rec29(const uint32_t* table, uint32_t v) {
  const uint4* r = reinterpret_cast<const uint4*>(table + (size_t)(v & VAL_INDEX) * REC29_WORDS);
  uint32_t w[28];
#pragma unroll
  for (int i = 0; i < 7; i++) {
    const uint4 q = r[i];
    w[4 * i] = q.x;
    w[4 * i + 1] = q.y;
    w[4 * i + 2] = q.z;
    w[4 * i + 3] = q.w;
  }
  return rec29_point(w, v);
}

// Staging of the next point through LDS (the _lds accumulation kernels): NP
// global_load_lds_dwordx4 land lane i's 16-byte piece j of src at buf[j][i]
// (no VGPR destination; the instruction is wave-wide, so every lane issues
// every load), and stage_read waits for them and reads the lane's 4 NP words
// back with NP ds_read_b128.
template <int NP>
__device__ __forceinline__ void stage_load(uint4 (*buf)[ACC_BLOCK], const uint32_t* src) {
#pragma unroll
  for (int j = 0; j < NP; j++)
    __builtin_amdgcn_global_load_lds((const void*)(src + 4 * j),
                                     (__attribute__((address_space(3))) void*)&buf[j][0], 16, 0, 0);
}
template <int NP>
__device__ __forceinline__ void stage_read(const uint4 (*buf)[ACC_BLOCK], int lane, uint32_t* w) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
  for (int j = 0; j < NP; j++) {
    const uint4 q = buf[j][lane];
    w[4 * j] = q.x;
    w[4 * j + 1] = q.y;
    w[4 * j + 2] = q.z;
    w[4 * j + 3] = q.w;
  }
}

template <class F>
__device__ __forceinline__ Affine<F> fetch_point(const uint32_t* bases, const uint32_t* phib, uint32_t nbase,
                                                uint32_t v) {
  const uint32_t idx = v & VAL_INDEX;
  Affine<F> p = (idx < nbase) ? load_affine<F>(bases, idx) : load_affine<F>(phib, idx - nbase);
  if (v >> 31) p.y = neg(p.y);
  return p;
}

// Chain start: every lane of the accumulation kernels below enters its chunk
// with acc = infinity and step 0 copies the gathered point in, so at step 1
// every live lane's accumulator is infinity (an empty or just-closed bucket)
// or has ZZ = ZZZ = 1 -- for the whole wave, by construction.  That step runs
// add_affine's `unit` form (curve.h), four products shorter, under a scalar
// branch on the step counter.  Later bucket starts inside a chunk are per
// lane and take the full addition.  TPST_CHAIN_UNIT=0 builds the full
// addition at every step (A/B).
#ifndef TPST_CHAIN_UNIT
#define TPST_CHAIN_UNIT 1
#endif
#ifndef TPST_K2_LG  // log2 of the window-grouped path's chunk length (A/B)
#define TPST_K2_LG 4
#endif
#ifndef TPST_CHAIN_UNIT_G2  // the G2 pair kernel (k_bucket_acc_short_pair)
#define TPST_CHAIN_UNIT_G2 TPST_CHAIN_UNIT
#endif

// K1's balanced bucket accumulation over the key-sorted entries: thread t owns
// the chunk of entries [t 2^lg, (t+1) 2^lg).  A bucket lying wholly inside the
// chunk is stored directly.  A bucket crossing chunk boundaries is finished by
// its owner (the chunk holding its first entry): the owner keeps its tail
// piece in registers while every later chunk parks its leading piece in
// part[t]; after the workgroup barrier the owner adds the pieces of the
// following chunks of its workgroup (still in L2) and stores the bucket.  Only
// the bucket crossing the workgroup's last chunk is left to k_bucket_fixup
// (its owner's partial goes to bpart[workgroup]), so the fixup runs one thread
// per workgroup instead of one per bucket.
// `table` is K1's window table of fetch_rec29 records; the next record is
// staged through LDS, as in k_bucket_acc_short_lds: seven
// global_load_lds_dwordx4 per step land lane i's 16-byte pieces at
// stage[buf][j][i] while the current mixed add runs; the loop runs to the
// wave's longest chunk (every lane issues every staging load).
#ifndef TPST_K1_MINW
#define TPST_K1_MINW 2
#endif
template <int MINW>
__global__ void __launch_bounds__(ACC_BLOCK, MINW)
    k_bucket_acc_chunk_lds(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, size_t m_all,
                           const uint32_t* __restrict__ mend, uint32_t sent, const uint32_t* __restrict__ bstart,
                           const uint32_t* __restrict__ bend, const uint32_t* __restrict__ table, int lg,
                           Xyzz<Fq>* __restrict__ buckets, Xyzz<Fq>* __restrict__ part,
                           Xyzz<Fq>* __restrict__ bpart) {
  constexpr int NP = 7;  // the first 112 bytes of a 128-byte record
  constexpr int NBUF = 2;  // double-buffered
  __shared__ uint4 stage[NBUF][NP][ACC_BLOCK];
  using A = AccField<Fq>;
  using C = typename A::T;
  const int lane = threadIdx.x;
  const size_t t = (size_t)blockIdx.x * ACC_BLOCK + lane;
  const size_t c0 = t << lg;
  const size_t m = mend ? (size_t)*mend : m_all;
  if ((((size_t)blockIdx.x * ACC_BLOCK) << lg) >= m) return;  // the whole workgroup (one wave) idle
  const bool active = c0 < m;
  const size_t c1 = active ? ((c0 + ((size_t)1 << lg) < m) ? c0 + ((size_t)1 << lg) : m) : c0;
  // lanes without a record load table[0]
  auto load_next = [&](int buf, uint32_t v, bool want) {
    stage_load<NP>(stage[buf], want ? table + (size_t)REC29_WORDS * (v & 0x7fffffffu) : table);
  };
  auto read_point = [&](int buf, uint32_t v) {
    uint32_t w[4 * NP];
    stage_read<NP>(stage[buf], lane, w);
    return rec29_point(w, v);
  };
  uint32_t tail_key = sent;
  Xyzz<C> acc = Xyzz<C>::inf();
  uint32_t key = active ? keys[c0] : sent;
  uint32_t val = active && key < sent ? vals[c0] : 0u;
  load_next(0, val, key < sent);
  const size_t steps = c1 - c0;
  const size_t maxsteps = (size_t)1 << lg;
  for (size_t s = 0; s < maxsteps; s++) {
    const size_t e = c0 + s;
    const bool live = s < steps;
    uint32_t key_n = sent, val_n = 0;
    if (s + 1 < steps) {
      key_n = keys[e + 1];
      if (key_n < sent) val_n = vals[e + 1];
    }
    const Affine<C> pt = read_point((int)(s & 1), val);
    load_next((int)((s + 1) & 1), val_n, key_n < sent);
    if (live && key < sent) {
      acc = add_affine(acc, pt, TPST_CHAIN_UNIT && s == 1);
      if (key_n != key) {
        if (bend[key] <= c1) {  // the bucket ends in this chunk
          if (bstart[key] >= c0)
            store_pk(buckets, key, acc);
          else
            store_pk(part, t, acc);
          acc = Xyzz<C>::inf();
        } else {  // continues: the chunk's last segment
          tail_key = key;
        }
      }
    }
    key = key_n;
    val = val_n;
    if (__all(s + 1 >= steps ? 1 : 0)) break;  // wave-uniform exit
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no staging load outstanding
  if (tail_key < sent && bstart[tail_key] < c0) {  // spans the whole chunk
    store_pk(part, t, acc);
    tail_key = sent;
  }
  __threadfence_block();
  __syncthreads();
  if (tail_key >= sent) return;
  const size_t t1 = ((size_t)bend[tail_key] - 1) >> lg;  // chunk of the bucket's last entry
  const size_t tb = (size_t)blockIdx.x * ACC_BLOCK + (ACC_BLOCK - 1);
  const size_t stop = t1 < tb ? t1 : tb;
  for (size_t u = t + 1; u <= stop; u++) acc = add(acc, load_pk(part, u));
  if (t1 <= tb)
    store_pk(buckets, tail_key, acc);
  else
    store_pk(bpart, blockIdx.x, acc);
}

// buckets crossing a workgroup boundary: thread B finishes the bucket holding
// workgroup B's last entry when that bucket began in B -- its owner's partial
// plus the leading pieces of the chunks after B up to the bucket's last one
template <class F>
__global__ void __launch_bounds__(64, (sizeof(F) > 48 ? 1 : 2))
    k_bucket_fixup(const uint32_t* __restrict__ keys, size_t m_all, const uint32_t* __restrict__ mend, uint32_t sent,
                   const uint32_t* __restrict__ bstart, const uint32_t* __restrict__ bend, int lg, size_t nblk,
                   const Xyzz<F>* __restrict__ part, const Xyzz<F>* __restrict__ bpart,
                   Xyzz<F>* __restrict__ buckets) {
  using C = typename AccField<F>::T;
  const size_t B = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (B + 1 >= nblk) return;
  const int lb = lg + ACC_BLOCK_LG;
  const size_t e = (B + 1) << lb;  // first entry of workgroup B + 1
  if (e >= (mend ? (size_t)*mend : m_all)) return;
  const uint32_t key = keys[e];
  if (key >= sent || keys[e - 1] != key || ((size_t)bstart[key] >> lb) != B) return;
  const size_t t1 = ((size_t)bend[key] - 1) >> lg;
  Xyzz<C> acc = load_pk(bpart, B);
  for (size_t u = (B + 1) << ACC_BLOCK_LG; u <= t1; u++) acc = add(acc, load_pk(part, u));
  store_pk(buckets, key, acc);
}

// Short-chunk accumulation for the variable-base MSM (32-entry chunks over
// ~64-entry buckets): no in-workgroup owner walk (it costs registers and a
// barrier that the short chunks do not amortise); every piece of a bucket
// that crosses a chunk boundary is parked -- the chunk's trailing piece in
// part[2t + 1], its leading piece in part[2t] -- and k_bucket_fixup_short
// sums them per bucket.  One launch covers the entries of windows [wlo, whi)
// (range[w] = first sorted entry of window w, device-side): chunk indices stay
// global (t = entry >> lg) so a chunk straddling two window groups is split
// between their launches without sharing a part[] slot.  The G1 kernels
// (this one and k_bucket_acc_short_lds) walk by the first / last flags of the
// sorted values and never read bstart / bend; keys only for a bucket stored
// whole.  The G2 pair kernel keeps the walk by keys and bounds.
template <class F, int MINW = (sizeof(F) > 48 ? 1 : 2), bool REC29 = false>
__global__ void __launch_bounds__(64, MINW)
    k_bucket_acc_short(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                       const uint32_t* __restrict__ range, int wlo, int whi, uint32_t sent,
                       const uint32_t* __restrict__ bstart, const uint32_t* __restrict__ bend,
                       const uint32_t* __restrict__ bases, const uint32_t* __restrict__ phib, uint32_t nbase,
                       int lg, Xyzz<F>* __restrict__ buckets, Xyzz<F>* __restrict__ part) {
  const size_t e_lo = range[wlo], e_hi = range[whi];
  const size_t t = (e_lo >> lg) + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t c0 = t << lg;
  if (c0 >= e_hi) return;
  const size_t c1 = (c0 + ((size_t)1 << lg) < e_hi) ? c0 + ((size_t)1 << lg) : e_hi;
  if (c0 < e_lo) c0 = e_lo;
  using A = AccField<F>;
  using C = typename A::T;
  auto fetch = [&](uint32_t v) -> Affine<C> {
    if constexpr (REC29)
      return fetch_rec29(bases, v);
    else
      return A::in(fetch_point<F>(bases, phib, nbase, v));
  };
  // the walk of k_bucket_acc_short_lds below, the next point prefetched into
  // registers: val_n was loaded one step ago, the load issued here is vals[e + 2]
  const size_t steps = c1 - c0;
  if (steps == 0) return;  // an empty window group
  uint32_t key = keys[c0];
  uint32_t val = vals[c0];
  uint32_t val_n = steps > 1 ? vals[c0 + 1] : 0u;
  uint32_t first_val = val;
  Affine<C> pt = fetch(val);
  Xyzz<C> acc = Xyzz<C>::inf();
  for (size_t s = 0; s < steps; s++) {  // s is the same in every lane still in the loop
    const size_t e = c0 + s;
    const uint32_t val_nn = s + 2 < steps ? vals[e + 2] : 0u;
    const uint32_t first_n = run_ends(val, s + 1 == steps) ? val_n : first_val;
    const uint32_t key_n = s + 1 < steps && run_slot(first_n, val_n) == RUN_BUCKET ? keys[e + 1] : 0u;
    Affine<C> pt_n;
    if (s + 1 < steps) pt_n = fetch(val_n);
    acc = add_affine(acc, pt, TPST_CHAIN_UNIT && s == 1);
    if (run_ends(val, s + 1 == steps)) {
      const uint32_t slot = run_slot(first_val, val);
      if (slot == RUN_BUCKET)
        store_pk(buckets, key, acc);
      else
        store_pk(part, 2 * t + slot, acc);
      acc = Xyzz<C>::inf();
    }
    val = val_n;
    val_n = val_nn;
    first_val = first_n;
    key = key_n;
    pt = pt_n;
  }
}

// k_bucket_acc_short<Fq> with the next point staged through LDS instead of
// registers: the wave issues six global_load_lds_dwordx4 for the 64 lanes'
// next points (lane i's 16-byte piece j lands at stage[buf][j][i]; no VGPR
// destination), runs the current mixed add meanwhile, and reads the staged
// point back with six ds_read_b128.  Frees the prefetched point's VGPRs
// (occupancy) and moves the gathers off the register file.  The default for
// G1 (TPST_ACC_LDS=0: k_bucket_acc_short's register prefetch).
#ifndef TPST_K2_MINW
#define TPST_K2_MINW 2  // waves per SIMD the register allocation targets (G1 records)
#endif
template <int MINW, bool REC29>
__global__ void __launch_bounds__(64, MINW)
    k_bucket_acc_short_lds(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                           const uint32_t* __restrict__ range, int wlo, int whi, uint32_t sent,
                           const uint32_t* __restrict__ bstart, const uint32_t* __restrict__ bend,
                           const uint32_t* __restrict__ bases, const uint32_t* __restrict__ phib, uint32_t nbase,
                           int lg, Xyzz<Fq>* __restrict__ buckets, Xyzz<Fq>* __restrict__ part) {
  // double-buffered points, piece-major: 96-byte field.h points or the
  // first 112 bytes of a 128-byte record (REC29)
  constexpr int NP = REC29 ? 7 : 6;
  constexpr int NBUF = 2;
  __shared__ uint4 stage[NBUF][NP][64];
  using A = AccField<Fq>;
  using C = typename A::T;
  const int lane = threadIdx.x;
  const size_t e_lo = range[wlo], e_hi = range[whi];
  const size_t t = (e_lo >> lg) + (size_t)blockIdx.x * blockDim.x + lane;
  size_t c0 = t << lg;
  if ((e_lo >> lg) + (size_t)blockIdx.x * blockDim.x >= e_hi) return;  // wave-uniform: no lane has work
  const bool active = c0 < e_hi;
  const size_t c1 = active ? ((c0 + ((size_t)1 << lg) < e_hi) ? c0 + ((size_t)1 << lg) : e_hi) : c0;
  if (c0 < e_lo) c0 = e_lo;
  // every lane issues every staging load (the instruction is wave-wide);
  // lanes without a point load bases[0]
  auto load_next = [&](int buf, uint32_t v, bool want) {
    const uint32_t idx = v & VAL_INDEX;
    stage_load<NP>(stage[buf], !want  ? bases
                               : REC29 ? bases + (size_t)REC29_WORDS * idx
                                       : ((idx < nbase) ? bases + 24 * (size_t)idx : phib + 24 * (size_t)(idx - nbase)));
  };
  auto read_point = [&](int buf, uint32_t v) {
    uint32_t w[4 * NP];
    stage_read<NP>(stage[buf], lane, w);
    if constexpr (REC29) {
      return rec29_point(w, v);
    } else {
      Affine<Fq> p = {Fq::from_limbs(w), Fq::from_limbs(w + 12)};
      if (v >> 31) p.y = neg(p.y);
      return A::in(p);
    }
  };
  // The walk reads nothing but vals[]: every entry of [c0, c1) is live (zero
  // digits sort past range[W]) and its flags say where its bucket starts and
  // ends (msm_pieces.h run_ends / run_slot).  No load is consumed in the step
  // that issues it: the value two entries ahead is issued after the step's
  // wait for the staged point and first used one step later, behind the next
  // wait, so the mixed add covers its latency and a bucket's end waits for
  // nothing.  Only a bucket lying wholly inside the chunk needs its key: the
  // flags of the entry ahead tell one step early, and the key is loaded then.
  const size_t steps = c1 - c0;  // per lane (0: no chunk, or an empty window group)
  // (the first key unconditionally and ahead of the values: the wait for them
  // covers it, so the compiler carries no pending load into the loop)
  uint32_t key = steps > 0 ? keys[c0] : 0u;
  uint32_t val = steps > 0 ? vals[c0] : 0u;
  uint32_t val_n = steps > 1 ? vals[c0 + 1] : 0u;
  uint32_t first_val = val;  // first entry of the current run
  // Stores count on vmcnt like loads and complete in order with them, so the
  // wait for a staged point would also wait for a run's stores issued just
  // before it (some lane of a wave ends a run in almost every step).  The
  // next point is therefore read back at the end of the step, after the add
  // and before the step's stores: the wait then finds this step's loads, a
  // whole add old, and the stores get the next add to complete (a small part
  // of the measured stall: profiles/acc_loop).
  load_next(0, val, steps > 0);
  Xyzz<C> acc = Xyzz<C>::inf();
  Affine<C> pt = read_point(0, val);
  const size_t maxsteps = (size_t)1 << lg;  // the loop runs to the wave's longest chunk
  for (size_t s = 0; s < maxsteps; s++) {
    const size_t e = c0 + s;
    uint32_t val_nn = s + 2 < steps ? vals[e + 2] : 0u;
    // the run entry e + 1 belongs to; its key when it ends there as a whole bucket
    const uint32_t first_n = run_ends(val, s + 1 == steps) ? val_n : first_val;
    uint32_t key_n = s + 1 < steps && run_slot(first_n, val_n) == RUN_BUCKET ? keys[e + 1] : 0u;
    load_next((int)((s + 1) & 1), val_n, s + 1 < steps);
    if (s < steps) acc = add_affine(acc, pt, TPST_CHAIN_UNIT && s == 1);
    pt = read_point((int)((s + 1) & 1), val_n);
    // the loaded words are complete here: the compiler places its own wait for
    // them at this point and none behind the stores
    asm volatile("" : "+v"(val_nn), "+v"(key_n));
    if (s < steps && run_ends(val, s + 1 == steps)) {
      const uint32_t slot = run_slot(first_val, val);
      if (slot == RUN_BUCKET)
        store_pk(buckets, key, acc);
      else
        store_pk(part, 2 * t + slot, acc);
      acc = Xyzz<C>::inf();
    }
    val = val_n;
    val_n = val_nn;
    first_val = first_n;
    key = key_n;
    if (__all(s + 1 >= steps ? 1 : 0)) break;  // wave-uniform exit
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no staging load outstanding at exit
}

// k_bucket_acc_short over G2 with pair-distributed Fq2 (pair_fq2.h): lanes
// 2t and 2t+1 run chunk t's bucket chain together, each holding one Fq
// coordinate of every Fq2 value; same chunking, parking and bucket stores.
static __device__ __forceinline__ Affine<Fq2P> fetch_point_pair(const uint32_t* bases, const uint32_t* phib, uint32_t nbase,
                                                        uint32_t v) {
  const uint32_t idx = v & VAL_INDEX;
  Affine<Fq2P> p = (idx < nbase) ? load_affine_pair(bases, idx) : load_affine_pair(phib, idx - nbase);
  if (v >> 31) p.y = neg(p.y);
  return p;
}

static __global__ void __launch_bounds__(64, 2)
    k_bucket_acc_short_pair(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                            const uint32_t* __restrict__ range, int wlo, int whi, uint32_t sent,
                            const uint32_t* __restrict__ bstart, const uint32_t* __restrict__ bend,
                            const uint32_t* __restrict__ bases, const uint32_t* __restrict__ phib, uint32_t nbase,
                            int lg, Xyzz<Fq2>* __restrict__ buckets, Xyzz<Fq2>* __restrict__ part) {
  const size_t e_lo = range[wlo], e_hi = range[whi];
  const size_t t = (e_lo >> lg) + (((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 1);
  size_t c0 = t << lg;
  if (c0 >= e_hi) return;  // pair-uniform
  const size_t c1 = (c0 + ((size_t)1 << lg) < e_hi) ? c0 + ((size_t)1 << lg) : e_hi;
  if (c0 < e_lo) c0 = e_lo;
  uint32_t key = keys[c0];
  Affine<Fq2P> pt;
  if (key < sent) pt = fetch_point_pair(bases, phib, nbase, vals[c0]);
  Xyzz<Fq2P> acc = Xyzz<Fq2P>::inf();
  int step = 0;  // the same in every lane still in the loop
  for (size_t e = c0; e < c1; e++, step++) {
    uint32_t key_n = sent;
    Affine<Fq2P> pt_n;
    if (e + 1 < c1) {
      key_n = keys[e + 1];
      if (key_n < sent) pt_n = fetch_point_pair(bases, phib, nbase, vals[e + 1]);
    }
    if (key < sent) {
      acc = add_affine(acc, pt, TPST_CHAIN_UNIT_G2 && step == 1);
      if (key_n != key) {
        const bool starts = bstart[key] >= c0;
        const bool ends = bend[key] <= c1;
        if (starts && ends)
          store_xyzz_pair(buckets, key, acc);
        else
          store_xyzz_pair(part, 2 * t + (starts ? 1 : 0), acc);
        acc = Xyzz<Fq2P>::inf();
      }
    }
    key = key_n;
    pt = pt_n;
  }
}

// The long list (LONG_PARTS, msm_pieces.h): a bucket spanning more than
// LONG_PARTS chunks is summed by k_bucket_fixup_long, one workgroup per bucket
// (strided partial sums, then a tree in LDS).  cap bounds the list: every
// listed bucket covers more than LONG_PARTS whole chunks of its group's
// entries.  G1: k_fixup_order fills it; G2: the pair fixup.
constexpr int LONG_THREADS = 256;
constexpr unsigned LONG_GRID = 32;
struct LongList {
  uint32_t* cnt;
  uint32_t* list;
  uint32_t cap;
  __device__ __forceinline__ void push(uint32_t b) const {
    const uint32_t i = atomicAdd(cnt, 1u);
    if (i < cap) list[i] = b;
  }
};

template <class F>
__global__ void __launch_bounds__(LONG_THREADS) k_bucket_fixup_long(const uint32_t* __restrict__ bstart,
                                                                    const uint32_t* __restrict__ bend, int lg,
                                                                    const Xyzz<F>* __restrict__ part,
                                                                    Xyzz<F>* __restrict__ buckets, LongList ll) {
  using C = typename AccField<F>::T;
  __shared__ Xyzz<C> sh[LONG_THREADS];
  const uint32_t n = *ll.cnt < ll.cap ? *ll.cnt : ll.cap;
  const uint32_t tid = threadIdx.x;
  for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint32_t b = ll.list[i];
    const size_t t0 = (size_t)bstart[b] >> lg, t1 = t0 + fixup_pieces(bstart[b], bend[b], lg);
    Xyzz<C> acc = tid == 0 ? load_pk(part, 2 * t0 + 1) : Xyzz<C>::inf();
    for (size_t t = t0 + 1 + tid; t <= t1; t += LONG_THREADS) acc = add(acc, load_pk(part, 2 * t));
    sh[tid] = acc;
    __syncthreads();
    for (uint32_t h = LONG_THREADS / 2; h > 0; h >>= 1) {
      if (tid < h) sh[tid] = add(sh[tid], sh[tid + h]);
      __syncthreads();
    }
    if (tid == 0) store_pk(buckets, b, sh[0]);
    __syncthreads();
  }
}

// k_bucket_fixup_short over G2 with pair-distributed Fq2: lanes 2b, 2b+1
// finish bucket b0 + b together
static __global__ void __launch_bounds__(64, 2)
    k_bucket_fixup_short_pair(const uint32_t* __restrict__ bstart, const uint32_t* __restrict__ bend, size_t b0,
                              size_t b1, int lg, const Xyzz<Fq2>* __restrict__ part, Xyzz<Fq2>* __restrict__ buckets,
                              int prio, LongList ll) {
  set_wave_prio(prio);
  const size_t b = b0 + (((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 1);
  if (b >= b1) return;
  const uint32_t s = bstart[b], e = bend[b];
  if (e <= s) return;
  const size_t t0 = (size_t)s >> lg, t1 = (size_t)(e - 1) >> lg;
  if (t0 == t1) return;
  if (t1 - t0 > LONG_PARTS) {
    if (!(threadIdx.x & 1)) ll.push((uint32_t)b);
    return;
  }
  Xyzz<Fq2P> acc = load_xyzz_pair(part, 2 * t0 + 1);
  for (size_t t = t0 + 1; t <= t1; t++) acc = add(acc, load_xyzz_pair(part, 2 * t));
  store_xyzz_pair(buckets, b, acc);
}

// G1: the fixup visits a window group's buckets in order of their piece count
// (fixup_pieces), longest class first, so that the lanes of a wave run the
// same number of additions: in bucket order a wave of 64 runs to its longest
// bucket (5.2 additions at the 2^20 shape against a mean of 3.9).  Two small
// kernels per group, a counting sort over the FIXUP_CLASSES classes of its
// buckets [b0, b1): k_fixup_hist counts the classes (LDS histogram per
// workgroup, then hist[class]); k_fixup_order gives every workgroup a run of
// each class (cur[class]) and writes the bucket indices to order[0 ..), class
// FIXUP_CAP first.  Buckets with nothing to fix are left out, those of the
// long list are pushed there.  The order inside a class is whatever the
// atomics give: each bucket's sum is independent.  hist and cur are zero
// before the two run.
constexpr int ORDER_THREADS = 256;

// listed buckets of a group: its classes 1 .. FIXUP_CAP
__device__ __forceinline__ uint32_t fixup_listed(const uint32_t* __restrict__ hist) {
  uint32_t n = 0;
  for (uint32_t k = 1; k < FIXUP_CLASSES; k++) n += hist[k];
  return n;
}

static __global__ void __launch_bounds__(ORDER_THREADS)
    k_fixup_hist(const uint32_t* __restrict__ bstart, const uint32_t* __restrict__ bend, uint32_t b0, uint32_t b1,
                 int lg, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[FIXUP_CLASSES];
  if (threadIdx.x < FIXUP_CLASSES) h[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t b = b0 + blockIdx.x * ORDER_THREADS + threadIdx.x;
  const uint32_t cls = b < b1 ? fixup_class(fixup_pieces(bstart[b], bend[b], lg)) : 0u;
  if (cls != 0 && cls != FIXUP_LONG) atomicAdd(&h[cls], 1u);
  __syncthreads();
  if (threadIdx.x != 0 && threadIdx.x < FIXUP_CLASSES && h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}

static __global__ void __launch_bounds__(ORDER_THREADS)
    k_fixup_order(const uint32_t* __restrict__ bstart, const uint32_t* __restrict__ bend, uint32_t b0, uint32_t b1,
                  int lg, const uint32_t* __restrict__ hist, uint32_t* __restrict__ cur,
                  uint32_t* __restrict__ order, LongList ll) {
  __shared__ uint32_t h[FIXUP_CLASSES], base[FIXUP_CLASSES];
  if (threadIdx.x < FIXUP_CLASSES) h[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t b = b0 + blockIdx.x * ORDER_THREADS + threadIdx.x;
  const uint32_t cls = b < b1 ? fixup_class(fixup_pieces(bstart[b], bend[b], lg)) : 0u;
  uint32_t r = 0;
  if (cls == FIXUP_LONG)
    ll.push(b);
  else if (cls != 0)
    r = atomicAdd(&h[cls], 1u);
  __syncthreads();
  if (threadIdx.x != 0 && threadIdx.x < FIXUP_CLASSES) {
    uint32_t off = 0;  // the longer classes come first
    for (uint32_t k = FIXUP_CAP; k > threadIdx.x; k--) off += hist[k];
    base[threadIdx.x] = off + (h[threadIdx.x] ? atomicAdd(&cur[threadIdx.x], h[threadIdx.x]) : 0u);
  }
  __syncthreads();
  // base + r < the group's listed buckets <= b1 - b0: both kernels class the same bounds
  if (cls != 0 && cls != FIXUP_LONG) order[base[cls] + r] = b;
}

// buckets crossing chunk boundaries: trailing piece of the first chunk plus
// the leading pieces of the following ones.  Lane i finishes bucket order[i]
// of its group's listed buckets (hist: the group's class counts); the grid
// covers the group's buckets, waves past the listed ones exit at once.
template <class F>
__global__ void __launch_bounds__(64, (sizeof(F) > 48 ? 1 : 2))
    k_bucket_fixup_short(const uint32_t* __restrict__ bstart, const uint32_t* __restrict__ bend,
                         const uint32_t* __restrict__ order, const uint32_t* __restrict__ hist, int lg,
                         const Xyzz<F>* __restrict__ part, Xyzz<F>* __restrict__ buckets, int prio) {
  using C = typename AccField<F>::T;
  set_wave_prio(prio);
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= fixup_listed(hist)) return;
  const uint32_t b = order[i];
  const uint32_t s = bstart[b];
  const size_t t0 = (size_t)s >> lg, t1 = t0 + fixup_pieces(s, bend[b], lg);
  Xyzz<C> acc = load_pk(part, 2 * t0 + 1);
  for (size_t t = t0 + 1; t <= t1; t++) acc = add(acc, load_pk(part, 2 * t));
  store_pk(buckets, b, acc);
}

// the same fixup, one quad of lanes per bucket (coop.h: 4 product latencies
// per addition instead of ~14): for the last window group of a lone call,
// whose fixup sits on the MSM's tail with one lone lane per bucket at ~2
// waves per CU
template <class F>
__global__ void __launch_bounds__(64) k_bucket_fixup_quad(const uint32_t* __restrict__ bstart,
                                                          const uint32_t* __restrict__ bend,
                                                          const uint32_t* __restrict__ order,
                                                          const uint32_t* __restrict__ hist, int lg,
                                                          const Xyzz<F>* __restrict__ part,
                                                          Xyzz<F>* __restrict__ buckets) {
  using C = typename AccField<F>::T;
  const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 2;
  const int qi = threadIdx.x & 3;
  if (i >= fixup_listed(hist)) return;  // quad-uniform
  const uint32_t b = order[i];
  const uint32_t s = bstart[b];
  const size_t t0 = (size_t)s >> lg, t1 = t0 + fixup_pieces(s, bend[b], lg);
  Xyzz<C> acc = load_pk(part, 2 * t0 + 1);
  for (size_t t = t0 + 1; t <= t1; t++) acc = add_quad(acc, load_pk(part, 2 * t), qi);
  if (qi == 0) store_pk(buckets, b, acc);
}

}  // namespace tpst
