// K1: the batched shared-base MSM of the commit (see msm.h for the pipeline).
#include "msm_sort.h"
#include "msm_acc.h"
#include "msm_reduce.h"

namespace tpst {

// ------------------------------------------------------------------ K1 ---
// T[w][j] = 2^(c w) B_j, one thread per base
__global__ void __launch_bounds__(64, 1) k_build_tables(const uint32_t* __restrict__ bases, size_t N, int c, int W, uint32_t* __restrict__ table) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= N) return;
  G1A p = load_affine<Fq>(bases, j);
  for (int w = 0; w < W; w++) {
    store_rec29(table, (size_t)w * N + j, p);  // an infinity base stays all-zero: x = y = 0
    if (w + 1 < W) {
      Xyzz<Fq> x = to_xyzz(p);
      for (int i = 0; i < c; i++) x = dbl(x);
      p = to_affine(x);
    }
  }
}

hipError_t batch_tables_build(hipStream_t s, const uint32_t* d_bases, size_t N, int c, BatchTables& t) {
  batch_tables_free(t);
  t.N = N;
  t.c = c;
  t.W = num_windows(c);
  TPST_TRY(hipMalloc(&t.d_table, (size_t)t.W * N * REC29_WORDS * sizeof(uint32_t)));
  k_build_tables<<<grid_for(N, 64), 64, 0, s>>>(d_bases, N, c, t.W, t.d_table);
  return hipGetLastError();
}

void batch_tables_free(BatchTables& t) {
  if (t.d_table) (void)hipFree(t.d_table);
  t.d_table = nullptr;
  t.N = 0;
}

// an empty bucket of the row MSMs = infinity (ZZ = 0): written by the sort,
// which knows the empty ones (no memset of all buckets)
__device__ __forceinline__ void zero_bucket(uint4* zb, size_t key) {
  constexpr int Q = sizeof(Xyzz<Fq>) / 16;
#pragma unroll
  for (int i = 0; i < Q; i++) zb[key * Q + i] = make_uint4(0, 0, 0, 0);
}

// one workgroup per row: LDS counting sort of the row's N*W signed digits
// by bucket; writes the row's entries and bucket bounds.
__global__ void __launch_bounds__(256) k_batch_sort(const uint32_t* __restrict__ scalars, size_t rows, size_t N,
                                                    size_t row_stride, size_t col_stride, int c, int W,
                                                    uint32_t* __restrict__ keys, uint32_t* __restrict__ entries,
                                                    uint32_t* __restrict__ bstart, uint32_t* __restrict__ bend,
                                                    uint4* __restrict__ zb) {
  extern __shared__ uint32_t cnt[];  // nb counters
  // XCD-aware: consecutive rows on the same XCD (blocks b, b+8, ... share one)
  const size_t nblk = gridDim.x;
  size_t r = blockIdx.x;
  if (nblk % 8 == 0) r = (blockIdx.x % 8) * (nblk / 8) + blockIdx.x / 8;
  if (r >= rows) return;
  const uint32_t nb = 1u << (c - 1);
  for (uint32_t b = threadIdx.x; b < nb; b += blockDim.x) cnt[b] = 0;
  __syncthreads();
  for (size_t j = threadIdx.x; j < N; j += blockDim.x) {
    uint32_t s[8];
    load_scalar(scalars + 8 * (r * row_stride + j * col_stride), s);
    uint32_t carry = 0;
    for (int w = 0; w < W; w++) {
      const int d = signed_digit(s, 8, w, c, W, carry);
      if (d) atomicAdd(&cnt[abs(d) - 1], 1u);
    }
  }
  __syncthreads();
  // exclusive scan of nb counters: thread t owns a contiguous slice
  __shared__ uint32_t part[256];
  __shared__ uint32_t total_sh;
  const uint32_t per = (nb + blockDim.x - 1) / blockDim.x;
  const uint32_t b0 = threadIdx.x * per;
  uint32_t local = 0;
  for (uint32_t b = b0; b < b0 + per && b < nb; b++) local += cnt[b];
  part[threadIdx.x] = local;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (unsigned t = 0; t < blockDim.x; t++) {
      const uint32_t v = part[t];
      part[t] = run;
      run += v;
    }
    total_sh = run;
  }
  __syncthreads();
  const size_t rowbase = r * N * (size_t)W;
  uint32_t run = part[threadIdx.x];
  for (uint32_t b = b0; b < b0 + per && b < nb; b++) {
    const uint32_t v = cnt[b];
    if (!v) zero_bucket(zb, r * nb + b);
    bstart[r * nb + b] = (uint32_t)(rowbase + run);
    bend[r * nb + b] = (uint32_t)(rowbase + run + v);
    cnt[b] = run;
    run += v;
  }
  __syncthreads();
  for (size_t j = threadIdx.x; j < N; j += blockDim.x) {
    uint32_t s[8];
    load_scalar(scalars + 8 * (r * row_stride + j * col_stride), s);
    uint32_t carry = 0;
    for (int w = 0; w < W; w++) {
      const int d = signed_digit(s, 8, w, c, W, carry);
      if (d) {
        const uint32_t b = (uint32_t)abs(d) - 1;
        const uint32_t pos = atomicAdd(&cnt[b], 1u);
        keys[rowbase + pos] = (uint32_t)(r * nb + b);
        entries[rowbase + pos] = (uint32_t)(w * N + j) | (d < 0 ? 0x80000000u : 0u);
      }
    }
  }
  // zero digits leave the row's region short: pad it with the sentinel
  const uint32_t total = total_sh;
  const uint32_t sent = (uint32_t)(rows * nb);
  for (size_t e = total + threadIdx.x; e < N * (size_t)W; e += blockDim.x) keys[rowbase + e] = sent;
}

// Staged variant (N <= SB_THREADS * SB_SPT, nb <= SB_NB): one 1024-thread
// workgroup per row.  After the LDS counting pass and the scan, the row's
// output is produced in position ranges of at most SB_STAGE entries: a pass
// takes the buckets [b_lo, b_hi) whose entries fit the range, recomputes the
// row's signed digits (the scalars are L2-resident after the counting pass),
// scatters the pass's digits into LDS and flushes the range to global memory
// with consecutive (coalesced) stores.  The direct scatter of k_batch_sort
// writes every 4-byte key and entry to a random position of a ~720 KB row
// region while dozens of rows per XCD are in flight (far over the L2), so
// nearly every store was a partial-line write; here the row's keys and
// entries are written once, contiguously.  A bucket larger than the stage
// (degenerate scalars) is scattered directly in a pass of its own.
constexpr int SB_THREADS = 1024;
constexpr int SB_SPT = 4;                 // scalars per thread: N <= 4096
constexpr uint32_t SB_NB = 2048;          // buckets per row (c <= 12)
constexpr uint32_t SB_STAGE = 15 * 1024;  // staged entries per pass (120 KB)

// WC > 0 (c = CC, W = WC: the commit's row MSMs, 12 / 22 at 2^24 and 11 /
// 24 at 2^20): the window loop is unrolled, so every digit is a funnel shift
// at a constant bit offset; with a runtime W the offset is runtime and the
// word select a chain of conditional moves over the scalar's 8 words (x 7
// passes over every digit of the row; 2^20 sort 172 -> 95 us)
template <int WC, int CC = 12>
__global__ void __launch_bounds__(SB_THREADS) k_batch_sort_staged(const uint32_t* __restrict__ scalars, size_t rows,
                                                                 size_t N, size_t row_stride, size_t col_stride, int c,
                                                                 int W, uint32_t* __restrict__ keys,
                                                                 uint32_t* __restrict__ entries,
                                                                 uint32_t* __restrict__ bstart,
                                                                 uint32_t* __restrict__ bend,
                                                                 uint4* __restrict__ zb) {
  __shared__ uint32_t start[SB_NB + 1];
  __shared__ uint32_t cur[SB_NB];
  __shared__ uint2 stage[SB_STAGE];
  __shared__ uint32_t part[SB_THREADS / 64];
  __shared__ uint32_t pass_lo, pass_hi;
  const size_t nblk = gridDim.x;
  size_t r = blockIdx.x;
  if (nblk % 8 == 0) r = (blockIdx.x % 8) * (nblk / 8) + blockIdx.x / 8;  // XCD-aware, as k_batch_sort
  if (r >= rows) return;
  const uint32_t nb = 1u << (c - 1);
  const int tid = threadIdx.x;
  for (uint32_t b = tid; b < nb; b += SB_THREADS) cur[b] = 0;
  __syncthreads();
  for (int k = 0; k < SB_SPT; k++) {
    const size_t j = (size_t)tid + (size_t)k * SB_THREADS;
    if (j >= N) break;
    uint32_t sc[8];
    load_scalar(scalars + 8 * (r * row_stride + j * col_stride), sc);
    uint32_t carry = 0;
    if constexpr (WC > 0) {
#pragma unroll
      for (int w = 0; w < WC; w++) {
        const int d = signed_digit(sc, 8, w, CC, WC, carry);
        if (d) atomicAdd(&cur[abs(d) - 1], 1u);
      }
    } else {
      for (int w = 0; w < W; w++) {
        const int d = signed_digit(sc, 8, w, c, W, carry);
        if (d) atomicAdd(&cur[abs(d) - 1], 1u);
      }
    }
  }
  __syncthreads();
  // exclusive scan of the counts -> start[] (row-relative)
  {
    const uint32_t per = (nb + SB_THREADS - 1) / SB_THREADS;
    const uint32_t b0 = tid * per;
    uint32_t local = 0;
    for (uint32_t b = b0; b < b0 + per && b < nb; b++) local += cur[b];
    const int lane = tid & 63, wv = tid >> 6;
    uint32_t incl = local;
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t v = __shfl_up(incl, o, 64);
      if (lane >= o) incl += v;
    }
    if (lane == 63) part[wv] = incl;
    __syncthreads();
    if (tid == 0) {
      uint32_t run = 0;
      for (int i = 0; i < SB_THREADS / 64; i++) {
        const uint32_t v = part[i];
        part[i] = run;
        run += v;
      }
      start[nb] = run;
    }
    __syncthreads();
    uint32_t run = part[wv] + incl - local;
    for (uint32_t b = b0; b < b0 + per && b < nb; b++) {
      const uint32_t v = cur[b];
      start[b] = run;
      run += v;
    }
  }
  __syncthreads();
  const size_t rowbase = r * N * (size_t)W;
  for (uint32_t b = tid; b < nb; b += SB_THREADS) {
    if (start[b + 1] == start[b]) zero_bucket(zb, r * nb + b);
    bstart[r * nb + b] = (uint32_t)(rowbase + start[b]);
    bend[r * nb + b] = (uint32_t)(rowbase + start[b + 1]);
    cur[b] = start[b];
  }
  const uint32_t total = start[nb];
  if (tid == 0) pass_hi = 0;
  __syncthreads();
  for (;;) {
    // next pass: buckets [lo, hi) from the end of the previous one, as many
    // as fit the stage (at least one)
    if (tid == 0) {
      const uint32_t lo = pass_hi;
      uint32_t hi = lo;
      if (lo < nb) {
        const uint32_t lim = start[lo] + SB_STAGE;
        uint32_t a = lo + 1, z = nb;  // largest hi in (lo, nb] with start[hi] <= lim
        while (a < z) {
          const uint32_t m = (a + z + 1) >> 1;
          if (start[m] <= lim) a = m; else z = m - 1;
        }
        hi = a;
      }
      pass_lo = lo;
      pass_hi = hi;
    }
    __syncthreads();
    const uint32_t lo = pass_lo, hi = pass_hi;
    if (lo >= nb) break;
    const uint32_t p0 = start[lo], cnt = start[hi] - p0;
    const bool direct = cnt > SB_STAGE;  // one oversized bucket
    auto place = [&](int d, int w, size_t j) {
      if (!d) return;
      const uint32_t b = (uint32_t)abs(d) - 1;
      if (b < lo || b >= hi) return;
      const uint32_t pos = atomicAdd(&cur[b], 1u);
      const uint2 e = make_uint2((uint32_t)(r * nb + b), (uint32_t)(w * N + j) | (d < 0 ? 0x80000000u : 0u));
      if (direct) {
        keys[rowbase + pos] = e.x;
        entries[rowbase + pos] = e.y;
      } else {
        stage[pos - p0] = e;
      }
    };
    for (int k = 0; k < SB_SPT; k++) {
      const size_t j = (size_t)tid + (size_t)k * SB_THREADS;
      if (j >= N) break;
      uint32_t sc[8];
      load_scalar(scalars + 8 * (r * row_stride + j * col_stride), sc);
      uint32_t carry = 0;
      if constexpr (WC > 0) {
#pragma unroll
        for (int w = 0; w < WC; w++) place(signed_digit(sc, 8, w, CC, WC, carry), w, j);
      } else {
        for (int w = 0; w < W; w++) place(signed_digit(sc, 8, w, c, W, carry), w, j);
      }
    }
    __syncthreads();
    if (!direct) {
      for (uint32_t i = tid; i < cnt; i += SB_THREADS) {
        const uint2 e = stage[i];
        keys[rowbase + p0 + i] = e.x;
        entries[rowbase + p0 + i] = e.y;
      }
    }
    __syncthreads();
  }
  // zero digits leave the row's region short: pad it with the sentinel
  const uint32_t sent = (uint32_t)(rows * nb);
  for (size_t e = total + tid; e < N * (size_t)W; e += SB_THREADS) keys[rowbase + e] = sent;
}

hipError_t msm_batch(Arena& ar, hipStream_t s, const BatchTables& t, const uint32_t* d_scalars, size_t rows,
                     size_t row_stride, size_t col_stride, Xyzz<Fq>* d_out) {
  if (rows == 0) return hipSuccess;
  const int c = t.c, W = t.W;
  const size_t N = t.N;
  const uint32_t nb = 1u << (c - 1);
  const size_t m = rows * N * (size_t)W;
  if (m >= (1ull << 32)) return hipErrorInvalidValue;  // entry offsets are u32
  const size_t nbk = rows * nb;
  // chunk length: at least 4 waves of chunks per SIMD (the
  // 2^20 commit's 26.6 M entries take 64-entry chunks, measured 8.7 -> 8.4 ms
  // against the 32-entry chunks 8 waves per SIMD would give)
  static const size_t k1_threads = (size_t)4 * 64 * device_simds();
  int lg = 5;
  while (lg < 8 && (m >> (lg + 1)) >= k1_threads) lg++;
  const size_t nchunk = (m + ((size_t)1 << lg) - 1) >> lg;
  const size_t nblk = (nchunk + ACC_BLOCK - 1) / ACC_BLOCK;
  size_t need = 2 * Arena::need(m, 4) + 2 * Arena::need(nbk, 4) + Arena::need(nbk, sizeof(Xyzz<Fq>)) +
                Arena::need(nchunk, sizeof(Xyzz<Fq>)) + Arena::need(nblk, sizeof(Xyzz<Fq>)) +
                reduce_scratch<Fq>(rows, nb) + (red2_ok(nb) ? reduce2_scratch<Fq>(rows, nb) : 0) + 4096;
  ar.reset();
  TPST_TRY(ar.reserve(need));
  uint32_t* keys = ar.take<uint32_t>(m);
  uint32_t* entries = ar.take<uint32_t>(m);
  Xyzz<Fq>* part = ar.take<Xyzz<Fq>>(nchunk);
  Xyzz<Fq>* bpart = ar.take<Xyzz<Fq>>(nblk);
  uint32_t* bstart = ar.take<uint32_t>(nbk);
  uint32_t* bend = ar.take<uint32_t>(nbk);
  Xyzz<Fq>* buckets = ar.take<Xyzz<Fq>>(nbk);
  const unsigned nrow_blk = (unsigned)rows;
  Profiler* pf = ar.prof;
  Profiler dummy;
  if (!pf) pf = &dummy;
  pf->begin(ST_BATCH_SORT, s);
  if (N <= (size_t)SB_THREADS * SB_SPT && c == 12 && W == 22)
    k_batch_sort_staged<22, 12><<<nrow_blk, SB_THREADS, 0, s>>>(d_scalars, rows, N, row_stride, col_stride, c, W, keys,
                                                                 entries, bstart, bend, reinterpret_cast<uint4*>(buckets));
  else if (N <= (size_t)SB_THREADS * SB_SPT && c == 11 && W == 24)
    k_batch_sort_staged<24, 11><<<nrow_blk, SB_THREADS, 0, s>>>(d_scalars, rows, N, row_stride, col_stride, c, W, keys,
                                                                 entries, bstart, bend, reinterpret_cast<uint4*>(buckets));
  else if (N <= (size_t)SB_THREADS * SB_SPT && nb <= SB_NB)
    k_batch_sort_staged<0><<<nrow_blk, SB_THREADS, 0, s>>>(d_scalars, rows, N, row_stride, col_stride, c, W, keys,
                                                            entries, bstart, bend, reinterpret_cast<uint4*>(buckets));
  else
    k_batch_sort<<<nrow_blk, 256, nb * sizeof(uint32_t), s>>>(d_scalars, rows, N, row_stride, col_stride, c, W, keys,
                                                          entries, bstart, bend, reinterpret_cast<uint4*>(buckets));
  TPST_TRY(hipGetLastError());
  pf->end(ST_BATCH_SORT, s);
  pf->begin(ST_BUCKET_ACC, s);
  // the LDS-staged gathers (2^24 commit 68.7-69.3 -> 68.6-68.8 ms against a
  // register prefetch of the next record, profiles/r05/l)
  k_bucket_acc_chunk_lds<TPST_K1_MINW><<<(unsigned)nblk, ACC_BLOCK, 0, s>>>(keys, entries, m, nullptr, (uint32_t)nbk, bstart, bend,
                                                                  t.d_table, lg, buckets, part, bpart);
  TPST_TRY(hipGetLastError());
  k_bucket_fixup<Fq><<<grid_for(nblk, 64), 64, 0, s>>>(keys, m, nullptr, (uint32_t)nbk, bstart, bend, lg, nblk,
                                                       part, bpart, buckets);
  TPST_TRY(hipGetLastError());
  pf->end(ST_BUCKET_ACC, s);
  pf->begin(ST_REDUCE, s);
  // the two-level reduction (no per-segment scalar multiplications; 2^20
  // commit 8.7 -> 8.2 ms, 2^24 unchanged)
  if (red2_ok(nb))
    TPST_TRY(reduce_buckets2<Fq>(ar, s, buckets, rows, nb, d_out, 0));
  else
    TPST_TRY(reduce_buckets<Fq>(ar, s, buckets, rows, nb, d_out));
  pf->end(ST_REDUCE, s);
  return hipSuccess;
}

}  // namespace tpst
