// Scalar decomposition and the two-pass bucket sort of the variable-base MSM.
#pragma once
#include "msm_common.h"
#include "msm_pieces.h"

namespace tpst {

// c-bit window of an nw-word canonical scalar starting at bit `off`
__device__ __forceinline__ uint32_t window_bits(const uint32_t* s, int nw, int off, int c) {
  const int w = off >> 5, b = off & 31;
  const uint64_t lo = (w < nw) ? s[w] : 0u;
  const uint64_t hi = (w + 1 < nw) ? s[w + 1] : 0u;
  return (uint32_t)(((lo | (hi << 32)) >> b) & ((1ull << c) - 1));
}

// signed digit of window w given the running carry (arkworks make_digits,
// except the top window keeps its carry instead of recentering)
__device__ __forceinline__ int signed_digit(const uint32_t* s, int nw, int w, int c, int W, uint32_t& carry) {
  const uint32_t coef = window_bits(s, nw, w * c, c) + carry;
  if (w == W - 1) {
    carry = 0;
    return (int)coef;
  }
  carry = (coef + (1u << (c - 1))) >> c;
  return (int)coef - (int)(carry << c);
}

__device__ __forceinline__ void load_scalar(const uint32_t* p, uint32_t* s) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 a = q[0], b = q[1];
  s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = a.w;
  s[4] = b.x; s[5] = b.y; s[6] = b.z; s[7] = b.w;
}

// ------------------------------------------------------- K2 bucket sort ---
// The decomposed entries (key = window*nb + |digit|-1, val = point index |
// sign<<31; with GLV, index i < n is P_i and n + i is phi(P_i); zero digits
// get the sentinel key nb*W) are grouped by key in two passes, no library sort:
//  * k_decompose_hist writes a tile of scalars' entries window-major and
//    counts them per bin (key >> lo) in LDS -> tab[tile][bin];
//  * k_sort_colscan / k_sort_binscan turn the counts into every tile's slot
//    range inside every bin and the bin starts;
//  * k_sort_scatter moves each tile's entries to its slots of their bins;
//  * k_sort_bin sorts one bin by the low lo key bits in LDS and writes the
//    entries in key order -- each value with the flags of the first and the
//    last entry of its bucket (msm_pieces.h entry_flags), which the G1
//    accumulation walks by --, the bucket bounds [bstart, bend), zeroes (=
//    infinity) the buckets without entries and the window starts range[w].
// Entries of one bucket land in an unspecified order: the bucket sum is a
// group element, so the MSM result does not depend on it.
// Workgroups of at most 256 threads (one wave per SIMD of a CU): a pipelined
// caller's next MSM decomposes and sorts while this one accumulates, and the
// accumulation's 2 waves per SIMD at ~200 VGPRs leave room for one more wave
// of <= 104 VGPRs per SIMD -- a wider workgroup waits for a whole CU to drain.
constexpr int SORT_THREADS = 256;                    // decomposition / scatter workgroup
constexpr uint32_t SORT_MAX_BINS = 16384;            // LDS histogram of a tile
constexpr int SORTB_THREADS = 256;                   // bin-sort workgroup
constexpr int SORTB_IT = 24;                         // entries per thread kept in registers
constexpr int SORTB_CAP = SORTB_THREADS * SORTB_IT;  // largest bin sorted in LDS
constexpr int SORTB_LO_MAX = 10;  // bin-sort LDS: 2^(lo+3) + 4 SORTB_CAP bytes <= 64 KB

struct SortPlan {
  int lo = 0;          // key bits sorted inside a bin
  uint32_t nbins = 0;  // (sent >> lo) + 1: the last bin holds the sentinel
  size_t tile = 0;     // scalars per decomposition tile
  uint32_t ntile = 0;
};

static bool sort_plan(uint32_t sent, size_t n, size_t m, SortPlan& p) {
  p.lo = 1;
  while ((sent >> p.lo) + 1 > SORT_MAX_BINS) p.lo++;
  // fewer, larger bins while a mean bin stays <= CAP/2 (headroom for skewed digits)
  while (p.lo < SORTB_LO_MAX && m / ((size_t)(sent >> (p.lo + 1)) + 1) <= (size_t)SORTB_CAP / 2) p.lo++;
  if (p.lo > SORTB_LO_MAX) return false;
  p.nbins = (sent >> p.lo) + 1;
  p.tile = 2048;
  while ((n + p.tile - 1) / p.tile > 1024) p.tile *= 2;
  p.ntile = (uint32_t)((n + p.tile - 1) / p.tile);
  return true;
}

// phi(P) = (beta x, y), the GLV endomorphism (phi(P) = [x^2 - 1] P on G1).
// On G2 (E'(Fq2), also j = 0) the same beta has eigenvalue lambda^2, so G2
// uses beta^2: (beta^2 x, y) = [x^2 - 1] Q, and one scalar decomposition
// serves both groups.
__constant__ uint32_t G2_GLV_BETA[12] = {0x5a7b8727u, 0x2c766f92u, 0x253d58b5u, 0x03d7f6b0u,
                                         0xec122131u, 0x838ec0deu, 0xf658bb10u, 0xbd5eb3e9u,
                                         0x6ed3e52eu, 0x6942bd12u, 0xdd04ed6au, 0x01673786u};  // Montgomery
template <class F>
__device__ __forceinline__ void glv_phi_point(const uint32_t* __restrict__ bases, size_t i, uint32_t* __restrict__ out) {
  Affine<F> p = load_affine<F>(bases, i);
  if (!is_inf(p)) {
    if constexpr (sizeof(F) == sizeof(Fq)) {
      p.x = mul(p.x, Fq::from_limbs(params::G1_BETA));
    } else {
      const Fq b2 = Fq::from_limbs(G2_GLV_BETA);
      p.x.c0 = mul(p.x.c0, b2);
      p.x.c1 = mul(p.x.c1, b2);
    }
  }
  store_affine(out, i, p);
}

// K2 (G1, GLV) gather records: P_i at index i and phi(P_i) at n + i in the
// accumulation field, fetch_rec29's 128-byte layout (written by the
// decomposition)
__device__ __forceinline__ void store_rec29(uint32_t* table, size_t idx, const Fq29& x, const Fq29& y) {
  uint32_t rec[REC29_WORDS];
#pragma unroll
  for (int i = 0; i < REC29_WORDS; i++) rec[i] = i < r29::N ? x.v[i] : i < 2 * r29::N ? y.v[i - r29::N] : 0u;
  uint4* dst = reinterpret_cast<uint4*>(table + idx * REC29_WORDS);
#pragma unroll
  for (int i = 0; i < REC29_WORDS / 4; i++) dst[i] = make_uint4(rec[4 * i], rec[4 * i + 1], rec[4 * i + 2], rec[4 * i + 3]);
}
__device__ __forceinline__ void store_rec29(uint32_t* table, size_t idx, const Affine<Fq>& p) {
  store_rec29(table, idx, from_std(p.x), from_std(p.y));
}

// one tile of scalars: signed digits (arkworks make_digits over the GLV
// halves), entries at slot (h W + w) n + i, bin counts, and phi of the bases
// (or, rec != nullptr, the gather records of P and phi(P))
template <class F>
static __global__ void __launch_bounds__(SORT_THREADS)
    k_decompose_hist(const uint32_t* __restrict__ scalars, size_t n, int c, int W, int glv, uint32_t sent, int lo,
                     uint32_t nbins, size_t tile, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                     uint32_t* __restrict__ tab, const uint32_t* __restrict__ bases, uint32_t* __restrict__ phib,
                     uint32_t* __restrict__ rec) {
  extern __shared__ uint32_t hist[];
  for (uint32_t b = threadIdx.x; b < nbins; b += SORT_THREADS) hist[b] = 0;
  __syncthreads();
  const uint32_t nb = 1u << (c - 1);
  const size_t i0 = (size_t)blockIdx.x * tile;
  const size_t i1 = (i0 + tile < n) ? i0 + tile : n;
  for (size_t i = i0 + threadIdx.x; i < i1; i += SORT_THREADS) {
    uint32_t s[8];
    load_scalar(scalars + 8 * i, s);
    const int halves = glv ? 2 : 1;
    uint32_t parts[2][4];
    if (glv) glv_split(s, parts[0], parts[1]);
    for (int h = 0; h < halves; h++) {
      const uint32_t* sc = glv ? parts[h] : s;
      const int nw = glv ? 4 : 8;
      const uint32_t idx = (uint32_t)(h * n + i);
      uint32_t carry = 0;
      for (int w = 0; w < W; w++) {
        const int d = signed_digit(sc, nw, w, c, W, carry);
        uint32_t key = sent, val = 0;
        if (d != 0) {
          key = (uint32_t)w * nb + (uint32_t)(abs(d) - 1);
          val = idx | (d < 0 ? 0x80000000u : 0u);
        }
        const size_t slot = ((size_t)h * W + w) * n + i;
        keys[slot] = key;
        vals[slot] = val;
        atomicAdd(&hist[key >> lo], 1u);
      }
    }
    if constexpr (sizeof(F) == sizeof(Fq)) {
      if (rec) {  // P and phi(P) = (beta x, y) in the accumulation field (infinity: x = y = 0 both)
        const Affine<Fq> p = load_affine<Fq>(bases, i);
        const Fq29 x = from_std(p.x), y = from_std(p.y);
        store_rec29(rec, i, x, y);
        store_rec29(rec, n + i, mul(x, from_std(Fq::from_limbs(params::G1_BETA))), y);
        continue;
      }
    }
    if (glv) glv_phi_point<F>(bases, i, phib);
  }
  __syncthreads();
  uint32_t* row = tab + (size_t)blockIdx.x * nbins;
  for (uint32_t b = threadIdx.x; b < nbins; b += SORT_THREADS) row[b] = hist[b];
}

// per bin: exclusive scan of the tiles' counts (in place: tab[t][bin] becomes
// tile t's first slot inside the bin) and the bin total.  64 bins x
// COLSCAN_CH tile chunks per workgroup.
constexpr int COLSCAN_CH = 4;
static __global__ void __launch_bounds__(64 * COLSCAN_CH) k_sort_colscan(uint32_t* __restrict__ tab, uint32_t ntile,
                                                                         uint32_t nbins, uint32_t* __restrict__ tot) {
  __shared__ uint32_t part[COLSCAN_CH][64];
  const uint32_t lane = threadIdx.x & 63, ch = threadIdx.x >> 6;
  const uint32_t bin = blockIdx.x * 64 + lane;
  const uint32_t per = (ntile + COLSCAN_CH - 1) / COLSCAN_CH;
  const uint32_t t0 = (ch * per < ntile) ? ch * per : ntile;
  const uint32_t t1 = (t0 + per < ntile) ? t0 + per : ntile;
  uint32_t sum = 0;
  if (bin < nbins)
    for (uint32_t t = t0; t < t1; t++) sum += tab[(size_t)t * nbins + bin];
  part[ch][lane] = sum;
  __syncthreads();
  if (ch == 0) {
    uint32_t acc = 0;
    for (int k = 0; k < COLSCAN_CH; k++) {
      const uint32_t v = part[k][lane];
      part[k][lane] = acc;
      acc += v;
    }
    if (bin < nbins) tot[bin] = acc;
  }
  __syncthreads();
  if (bin < nbins) {
    uint32_t acc = part[ch][lane];
    for (uint32_t t = t0; t < t1; t++) {
      const size_t o = (size_t)t * nbins + bin;
      const uint32_t v = tab[o];
      tab[o] = acc;
      acc += v;
    }
  }
}

// start[b] = sum of the totals of bins < b, start[nbins] = entry count (one workgroup)
constexpr int BINSCAN_THREADS = 256;
static __global__ void __launch_bounds__(BINSCAN_THREADS) k_sort_binscan(const uint32_t* __restrict__ tot,
                                                                         uint32_t nbins, uint32_t* __restrict__ start) {
  __shared__ uint32_t ws[BINSCAN_THREADS];
  const uint32_t t = threadIdx.x;
  const uint32_t per = (nbins + BINSCAN_THREADS - 1) / BINSCAN_THREADS;
  const uint32_t b0 = t * per;
  uint32_t sum = 0;
  for (uint32_t k = 0; k < per; k++)
    if (b0 + k < nbins) sum += tot[b0 + k];
  ws[t] = sum;
  __syncthreads();
  for (uint32_t off = 1; off < BINSCAN_THREADS; off <<= 1) {
    const uint32_t v = t >= off ? ws[t - off] : 0u;
    __syncthreads();
    ws[t] += v;
    __syncthreads();
  }
  uint32_t acc = ws[t] - sum;
  for (uint32_t k = 0; k < per; k++)
    if (b0 + k < nbins) {
      start[b0 + k] = acc;
      acc += tot[b0 + k];
    }
  if (t == BINSCAN_THREADS - 1) start[nbins] = ws[BINSCAN_THREADS - 1];
}

// tile -> bins: each entry takes the next slot of its bin from the tile's
// cursors in LDS (reads coalesced; writes in runs of the tile's entries per bin)
static __global__ void __launch_bounds__(SORT_THREADS)
    k_sort_scatter(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, size_t n, uint32_t segs,
                   int lo, uint32_t nbins, size_t tile, const uint32_t* __restrict__ tab,
                   const uint32_t* __restrict__ start, uint32_t* __restrict__ keys2, uint32_t* __restrict__ vals2) {
  extern __shared__ uint32_t cur[];
  const uint32_t* row = tab + (size_t)blockIdx.x * nbins;
  for (uint32_t b = threadIdx.x; b < nbins; b += SORT_THREADS) cur[b] = start[b] + row[b];
  __syncthreads();
  const size_t i0 = (size_t)blockIdx.x * tile;
  const uint32_t cnt = (uint32_t)((i0 + tile < n) ? tile : n - i0);
  const uint32_t total = segs * cnt;
  constexpr int U = 4;
  for (uint32_t q0 = 0; q0 < total; q0 += U * SORT_THREADS) {
    uint32_t k[U], v[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const uint32_t q = q0 + u * SORT_THREADS + threadIdx.x;
      if (q < total) {
        const uint32_t sg = q / cnt;
        const size_t slot = (size_t)sg * n + i0 + (q - sg * cnt);
        k[u] = keys[slot];
        v[u] = vals[slot];
      }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const uint32_t q = q0 + u * SORT_THREADS + threadIdx.x;
      if (q < total) {
        const uint32_t pos = atomicAdd(&cur[k[u] >> lo], 1u);
        keys2[pos] = k[u];
        vals2[pos] = v[u];
      }
    }
  }
}

// exclusive prefix sums of a[0, len) into o (may alias a) by NT threads:
// per-thread runs, wave scan, wave totals; returns the total
template <int NT>
__device__ uint32_t block_scan_excl(const uint32_t* a, uint32_t* o, uint32_t len, uint32_t* wsum) {
  const uint32_t t = threadIdx.x;
  const uint32_t per = (len + NT - 1) / NT, d0 = t * per;
  uint32_t sum = 0;
  for (uint32_t k = 0; k < per; k++)
    if (d0 + k < len) sum += a[d0 + k];
  uint32_t incl = sum;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const uint32_t v = __shfl_up(incl, s, 64);
    if ((t & 63) >= (uint32_t)s) incl += v;
  }
  if ((t & 63) == 63) wsum[t >> 6] = incl;
  __syncthreads();
  uint32_t acc = incl - sum, total = 0;
  for (uint32_t w = 0; w < NT / 64; w++) {
    if (w < (t >> 6)) acc += wsum[w];
    total += wsum[w];
  }
  for (uint32_t k = 0; k < per; k++)
    if (d0 + k < len) {
      const uint32_t v = a[d0 + k];
      o[d0 + k] = acc;
      acc += v;
    }
  __syncthreads();
  return total;
}

// k_sort_scatter with the tile staged per window through LDS (bins aligned to
// windows: lo <= c - 1): the tile's entries of window w (both GLV halves)
// are ordered by bin in LDS, then written out in per-bin runs, so a wave's
// store covers a few runs instead of 64 scattered words
template <int E>
static __global__ void __launch_bounds__(SORT_THREADS)
    k_sort_scatter_win(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, size_t n, int halves,
                       int W, uint32_t sent, int lo, uint32_t nbins, uint32_t bpw, size_t tile,
                       const uint32_t* __restrict__ tab, const uint32_t* __restrict__ start,
                       uint32_t* __restrict__ keys2, uint32_t* __restrict__ vals2) {
  extern __shared__ uint32_t sm[];
  __shared__ uint32_t wsum[SORT_THREADS / 64];
  uint32_t* cur = sm;              // global cursor of every bin
  uint32_t* lc = cur + nbins;      // the window's bins + the sentinel bin: counts
  uint32_t* lo_ = lc + bpw + 1;    //   and their first staged slot
  uint32_t* sk = lo_ + bpw + 1;    // staged keys / values
  uint32_t* sv = sk + (size_t)E * SORT_THREADS;
  const uint32_t t = threadIdx.x;
  const uint32_t* row = tab + (size_t)blockIdx.x * nbins;
  for (uint32_t b = t; b < nbins; b += SORT_THREADS) cur[b] = start[b] + row[b];
  const size_t sub = (size_t)E * SORT_THREADS / halves;
  const size_t t0 = (size_t)blockIdx.x * tile, t1 = (t0 + tile < n) ? t0 + tile : n;
  for (size_t i0 = t0; i0 < t1; i0 += sub)  // sub-tiles append at the tile's cursors
  for (int w = 0; w < W; w++) {
    const uint32_t cnt = (uint32_t)((i0 + sub < t1) ? sub : t1 - i0);
    const uint32_t tot = (uint32_t)halves * cnt;
    const uint32_t wb = (uint32_t)w * bpw;
    for (uint32_t j = t; j <= bpw; j += SORT_THREADS) lc[j] = 0;
    __syncthreads();
    uint32_t k[E], v[E], r[E];
#pragma unroll
    for (int u = 0; u < E; u++) {
      const uint32_t q = u * SORT_THREADS + t;
      if (q < tot) {
        const uint32_t h = q >= cnt ? 1u : 0u;
        const size_t slot = ((size_t)h * W + w) * n + i0 + (q - h * cnt);
        k[u] = keys[slot];
        v[u] = vals[slot];
      }
    }
#pragma unroll
    for (int u = 0; u < E; u++)
      if (u * SORT_THREADS + t < tot) r[u] = atomicAdd(&lc[k[u] >= sent ? bpw : (k[u] >> lo) - wb], 1u);
    __syncthreads();
    block_scan_excl<SORT_THREADS>(lc, lo_, bpw + 1, wsum);
#pragma unroll
    for (int u = 0; u < E; u++)
      if (u * SORT_THREADS + t < tot) {
        const uint32_t p = lo_[k[u] >= sent ? bpw : (k[u] >> lo) - wb] + r[u];
        sk[p] = k[u];
        sv[p] = v[u];
      }
    __syncthreads();
    for (uint32_t p = t; p < tot; p += SORT_THREADS) {
      const uint32_t key = sk[p];
      const bool z = key >= sent;
      const uint32_t lb = z ? bpw : (key >> lo) - wb;
      const uint32_t pos = cur[z ? nbins - 1 : key >> lo] + (p - lo_[lb]);
      keys2[pos] = key;
      vals2[pos] = sv[p];
    }
    __syncthreads();
    for (uint32_t j = t; j <= bpw; j += SORT_THREADS) cur[j == bpw ? nbins - 1 : wb + j] += lc[j];
    __syncthreads();
  }
}

// one bin: counting sort by the low lo key bits.  A bin of <= SORTB_CAP
// entries is staged in registers + LDS and written out contiguously; a larger
// one (skewed digits) scatters straight to its slots.  Either way an entry's
// rank inside its bucket and the bucket's count follow from the offsets off[]
// and give its flags.
static __global__ void __launch_bounds__(SORTB_THREADS)
    k_sort_bin(const uint32_t* __restrict__ keys2, const uint32_t* __restrict__ vals2,
               const uint32_t* __restrict__ start, int lo, uint32_t sent, uint32_t nb, int W,
               uint32_t* __restrict__ keys, uint32_t* __restrict__ vals, uint32_t* __restrict__ bstart,
               uint32_t* __restrict__ bend, uint4* __restrict__ buckets, uint32_t bucket_u4,
               uint32_t* __restrict__ range) {
  extern __shared__ uint32_t sm[];
  __shared__ uint32_t wsum[SORTB_THREADS / 64];
  const uint32_t D = 1u << lo, mask = D - 1;
  uint32_t* off = sm;           // bucket offsets inside the bin (counts first)
  uint32_t* cur = sm + D;       // placement cursors
  uint32_t* sval = sm + 2 * D;  // staged values
  const uint32_t b = blockIdx.x, t = threadIdx.x;
  const uint32_t s = start[b], len = start[b + 1] - s;
  if ((b << lo) >= sent) {
    // the sentinel bin (zero digits; sent = W nb is a multiple of 2^lo when
    // lo <= c - 1): nothing reads entries past range[W] -- the short chunks
    // stop at range[whi] -- so a bin that can hold most of m entries (small or
    // boolean scalars) costs nothing here
    if (t == 0 && (b << lo) == sent) range[W] = s;
    return;
  }
  for (uint32_t d = t; d < D; d += SORTB_THREADS) off[d] = 0;
  __syncthreads();
  const bool fits = len <= (uint32_t)SORTB_CAP;
  uint32_t kk[SORTB_IT], vv[SORTB_IT];
  // sentinel entries of a mixed last bin (lo > c - 1: small MSMs) are not
  // counted: they fill the bin's tail [nz, len) after the sorted entries
  if (fits) {
#pragma unroll
    for (int k = 0; k < SORTB_IT; k++) {
      const uint32_t p = k * SORTB_THREADS + t;
      if (p < len) {
        kk[k] = keys2[s + p];
        vv[k] = vals2[s + p];
      }
    }
#pragma unroll
    for (int k = 0; k < SORTB_IT; k++)
      if (k * SORTB_THREADS + t < len && kk[k] < sent) atomicAdd(&off[kk[k] & mask], 1u);
  } else {
    for (uint32_t p = t; p < len; p += SORTB_THREADS) {
      const uint32_t key = keys2[s + p];
      if (key < sent) atomicAdd(&off[key & mask], 1u);
    }
  }
  __syncthreads();
  // exclusive scan of the counts: per-thread runs, wave scan, wave totals
  const uint32_t per = (D + SORTB_THREADS - 1) / SORTB_THREADS;
  const uint32_t d0 = t * per;
  uint32_t sum = 0;
  for (uint32_t k = 0; k < per; k++)
    if (d0 + k < D) sum += off[d0 + k];
  uint32_t incl = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t v = __shfl_up(incl, o, 64);
    if ((t & 63) >= (uint32_t)o) incl += v;
  }
  if ((t & 63) == 63) wsum[t >> 6] = incl;
  __syncthreads();
  uint32_t acc = incl - sum, nz = 0;
  for (uint32_t w = 0; w < SORTB_THREADS / 64; w++) {
    if (w < (t >> 6)) acc += wsum[w];
    nz += wsum[w];  // entries with a bucket key
  }
  for (uint32_t k = 0; k < per; k++) {
    const uint32_t d = d0 + k;
    if (d >= D) break;
    const uint32_t cn = off[d];
    cur[d] = acc;
    const uint32_t key = (b << lo) | d;
    if (key < sent) {
      bstart[key] = s + acc;
      bend[key] = s + acc + cn;
      if (cn == 0 && buckets)
        for (uint32_t u = 0; u < bucket_u4; u++) buckets[(size_t)key * bucket_u4 + u] = make_uint4(0, 0, 0, 0);
    }
    acc += cn;
  }
  __syncthreads();
  for (uint32_t d = t; d < D; d += SORTB_THREADS) off[d] = cur[d];
  if (t <= (uint32_t)W) {
    const uint32_t target = t * nb;  // first key of window t (t = W: the sentinel)
    if ((target >> lo) == b) range[t] = s + cur[target & mask];
  }
  __syncthreads();
  if (fits) {
#pragma unroll
    for (int k = 0; k < SORTB_IT; k++)
      if (k * SORTB_THREADS + t < len && kk[k] < sent) sval[atomicAdd(&cur[kk[k] & mask], 1u)] = vv[k];
    __syncthreads();
    for (uint32_t p = t; p < nz; p += SORTB_THREADS) {
      uint32_t a = 0, z = D;  // first bucket offset > p
      while (a < z) {
        const uint32_t mid = (a + z) >> 1;
        if (off[mid] <= p)
          a = mid + 1;
        else
          z = mid;
      }
      const uint32_t b0 = off[a - 1], b1 = a < D ? off[a] : nz;  // the bucket's slots
      keys[s + p] = (b << lo) | (a - 1);
      vals[s + p] = sval[p] | entry_flags(p - b0, b1 - b0);
    }
  } else {
    for (uint32_t p = t; p < len; p += SORTB_THREADS) {
      const uint32_t key = keys2[s + p];
      if (key >= sent) continue;
      const uint32_t d = key & mask;
      const uint32_t b0 = off[d], b1 = d + 1 < D ? off[d + 1] : nz;
      const uint32_t q = atomicAdd(&cur[d], 1u);
      keys[s + q] = key;
      vals[s + q] = vals2[s + p] | entry_flags(q - b0, b1 - b0);
    }
  }
  for (uint32_t p = nz + t; p < len; p += SORTB_THREADS) keys[s + p] = sent;
}

}  // namespace tpst
