// Weighted bucket reductions and the window chain.
#pragma once
#include "msm_common.h"

namespace tpst {

// bucket-array input of a reduction kernel: the accumulation's packed format
// (PK) or a reduction's own output
template <bool PK, class F>
__device__ __forceinline__ Xyzz<typename AccField<F>::T> load_in(const Xyzz<F>* p, size_t i) {
  if constexpr (PK)
    return load_pk(p, i);
  else
    return load_acc(p, i);
}

// segment t of group g: sum_{b in seg} (b+1) * S_b with b the bucket index
// inside the group (bucket b holds digit value b+1): running sums over the L
// buckets plus (segment offset) * (segment sum).  One quad of lanes per
// segment (coop.h): 4 / 3 product latencies per addition / doubling.
template <class F, bool PK>
__global__ void __launch_bounds__(64) k_seg_reduce_quad(const Xyzz<F>* __restrict__ buckets, uint32_t nb, uint32_t L,
                                                        size_t nseg, Xyzz<F>* __restrict__ seg_out, int prio = 0) {
  using C = typename AccField<F>::T;
  set_wave_prio(prio);
  const size_t t = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 2;
  const int qi = threadIdx.x & 3;
  if (t >= nseg) return;  // quad-uniform
  const uint32_t S = nb / L;
  const size_t g = t / S;
  const uint32_t k = (uint32_t)(t % S);
  const size_t base = g * nb + (size_t)k * L;
  Xyzz<C> acc = Xyzz<C>::inf(), sum = Xyzz<C>::inf();
  for (int b = (int)L - 1; b >= 0; b--) {
    acc = add_quad(acc, load_in<PK>(buckets, base + b), qi);
    sum = add_quad(sum, acc, qi);
  }
  const uint32_t s0 = k * L;
  if (s0 != 0 && !is_inf(acc)) sum = add_quad(sum, scalar_mul_quad(acc, s0, 32 - __builtin_clz(s0), qi), qi);
  if (qi == 0) store_acc(seg_out, t, sum);
}

// the same segment sums, one lane per segment: for reductions with enough
// segments to fill the chip (the 4096-row commit at 2^24: 262 144 segments)
// the quad-cooperative form only adds exchange overhead to a throughput-bound
// pass
template <class F, bool PK>
__global__ void __launch_bounds__(64) k_seg_reduce_lane(const Xyzz<F>* __restrict__ buckets, uint32_t nb, uint32_t L,
                                                        size_t nseg, Xyzz<F>* __restrict__ seg_out) {
  using C = typename AccField<F>::T;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nseg) return;
  const uint32_t S = nb / L;
  const size_t g = t / S;
  const uint32_t k = (uint32_t)(t % S);
  const size_t base = g * nb + (size_t)k * L;
  Xyzz<C> acc = Xyzz<C>::inf(), sum = Xyzz<C>::inf();
  for (int b = (int)L - 1; b >= 0; b--) {
    acc = add(acc, load_in<PK>(buckets, base + b));
    sum = add(sum, acc);
  }
  const uint32_t s0 = k * L;
  if (s0 != 0 && !is_inf(acc)) sum = add(sum, scalar_mul_xyzz(acc, &s0, 32 - __builtin_clz(s0)));
  store_acc(seg_out, t, sum);
}

// one workgroup of BS / 4 quads per group: sum its S partial points
template <class F, int BS>
__global__ void __launch_bounds__(BS) k_group_reduce_quad(const Xyzz<F>* __restrict__ seg, uint32_t S,
                                                          Xyzz<F>* __restrict__ out, int prio = 0) {
  using C = typename AccField<F>::T;
  set_wave_prio(prio);
  constexpr int Q = BS / 4;
  __shared__ Xyzz<C> sh[Q];
  const size_t g = blockIdx.x;
  const int quad = threadIdx.x >> 2, qi = threadIdx.x & 3;
  Xyzz<C> acc = Xyzz<C>::inf();
  for (uint32_t k = quad; k < S; k += Q) acc = add_quad(acc, load_acc(seg, g * S + k), qi);
  if (qi == 0) sh[quad] = acc;
  __syncthreads();
  for (int h = Q / 2; h > 0; h >>= 1) {
    if (quad < h) {  // a quad reads its two operands before its lane 0 writes (one wave, in order)
      const Xyzz<C> v = add_quad(sh[quad], sh[quad + h], qi);
      if (qi == 0) sh[quad] = v;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) store_acc(out, g, sh[0]);
}

// Contribution of the window group [wlo, whi) on one wave:
// 2^(c wlo) sum_{wlo <= w < whi} 2^(c (w - wlo)) G_w (Horner, then c wlo more
// doublings), plus the `nextra` finished contributions of the other groups.
// Every quad runs the same chain, its doublings and additions
// quad-cooperative (coop.h: 3 / 4 product latencies).
template <class F>
static __global__ void __launch_bounds__(64, 1) k_window_chain(const Xyzz<F>* __restrict__ win, int wlo, int whi,
                                                              int c, const Xyzz<F>* __restrict__ extra, int nextra,
                                                              Xyzz<F>* __restrict__ out) {
  using C = typename AccField<F>::T;
  if (blockIdx.x != 0) return;
  __builtin_amdgcn_s_setprio(3);  // a lone latency chain beside accumulation waves
  const int qi = threadIdx.x & 3;
  Xyzz<C> acc = load_acc(win, whi - 1);
  for (int w = whi - 2; w >= wlo; w--) {
    for (int i = 0; i < c; i++) acc = dbl_quad(acc, qi);
    acc = add_quad(acc, load_acc(win, w), qi);
  }
  for (int i = 0; i < c * wlo; i++) acc = dbl_quad(acc, qi);
  for (int k = 0; k < nextra; k++) acc = add_quad(acc, load_acc(extra, k), qi);
  if (threadIdx.x == 0) store_acc(out, 0, acc);
}

// segment length of the weighted bucket reduction: short segments (L = 4)
// when the groups are few (latency-bound: many short chains); longer ones when
// there are enough segments to fill the chip anyway (throughput-bound: every
// segment pays one scalar multiplication by its offset, so fewer, longer
// segments do less work) -- the 4096-row commit at 2^24 runs L = 32
static uint32_t reduce_seg_len(size_t groups, uint32_t nb) {
  uint32_t L = 4;
  while (L < 32 && 2 * L <= nb && groups * (nb / (2 * L)) >= ((size_t)1 << 18)) L *= 2;
  return nb >= L ? L : nb;
}

template <class F>
static size_t reduce_scratch(size_t groups, uint32_t nb) {
  const uint32_t L = reduce_seg_len(groups, nb);
  const size_t nseg = groups * (nb / L);
  return Arena::need(nseg, sizeof(Xyzz<F>)) + Arena::need(nseg / 64 + groups + 1, sizeof(Xyzz<F>));
}

// sum of S points per group (tree passes of k_group_reduce_quad)
template <class F>
static hipError_t sum_groups(Arena& ar, hipStream_t s, const Xyzz<F>* in, size_t groups, uint32_t S, Xyzz<F>* out,
                             int prio) {
  if (S >= 256 && S % 64 == 0) {  // two-pass tree: 64 -> 1, then per group
    Xyzz<F>* mid = ar.take<Xyzz<F>>(groups * S / 64);
    k_group_reduce_quad<F, 256><<<(unsigned)(groups * S / 64), 256, 0, s>>>(in, 64, mid, prio);
    TPST_TRY(hipGetLastError());
    k_group_reduce_quad<F, 256><<<(unsigned)groups, 256, 0, s>>>(mid, S / 64, out, prio);
  } else {
    k_group_reduce_quad<F, 256><<<(unsigned)groups, 256, 0, s>>>(in, S, out, prio);
  }
  return hipGetLastError();
}

// reduce `groups` bucket sets of nb buckets each into one point per group:
// weighted segments of reduce_seg_len buckets, then the tree of sum_groups
template <class F>
static hipError_t reduce_buckets(Arena& ar, hipStream_t s, const Xyzz<F>* d_buckets, size_t groups, uint32_t nb,
                                 Xyzz<F>* d_group_out, int prio = 0, bool pk = true) {
  const uint32_t L = reduce_seg_len(groups, nb);
  const uint32_t S = nb / L;
  const size_t nseg = groups * S;
  Xyzz<F>* seg = ar.take<Xyzz<F>>(nseg);
  // d_buckets: the accumulation's bucket format (pk) or a reduction's output
  if (std::is_same<F, Fq>::value && nseg >= ((size_t)1 << 18)) {
    if (pk)
      k_seg_reduce_lane<F, true><<<grid_for(nseg, 64), 64, 0, s>>>(d_buckets, nb, L, nseg, seg);
    else
      k_seg_reduce_lane<F, false><<<grid_for(nseg, 64), 64, 0, s>>>(d_buckets, nb, L, nseg, seg);
  } else if (pk) {
    k_seg_reduce_quad<F, true><<<grid_for(4 * nseg, 64), 64, 0, s>>>(d_buckets, nb, L, nseg, seg, prio);
  } else {
    k_seg_reduce_quad<F, false><<<grid_for(4 * nseg, 64), 64, 0, s>>>(d_buckets, nb, L, nseg, seg, prio);
  }
  TPST_TRY(hipGetLastError());
  return sum_groups<F>(ar, s, seg, groups, S, d_group_out, prio);
}

// Two-level weighted reduction without per-segment scalar multiplications
// (work ~1/3 of reduce_buckets at the K2 shape, for the window groups whose
// reduction runs under other groups' accumulation -- throughput, not latency).
// Level 1: segments of L1 buckets -> S_k = sum_{b in seg} (b - k L1 + 1) X_b and
// T_k = sum_{b in seg} X_b; then sum_b (b+1) X_b = sum_k S_k + L1 sum_k k T_k,
// the second sum being the same weighted reduction over Tn_{k-1} = T_k.
template <class F, bool PK = true>
__global__ void __launch_bounds__(64) k_seg_run_quad(const Xyzz<F>* __restrict__ buckets, uint32_t nb, uint32_t L,
                                                     size_t nseg, Xyzz<F>* __restrict__ S_out,
                                                     Xyzz<F>* __restrict__ Tn, int prio = 0) {
  using C = typename AccField<F>::T;
  set_wave_prio(prio);
  const size_t t = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 2;
  const int qi = threadIdx.x & 3;
  if (t >= nseg) return;  // quad-uniform
  const uint32_t S = nb / L;
  const size_t g = t / S;
  const uint32_t k = (uint32_t)(t % S);
  const size_t base = g * nb + (size_t)k * L;
  Xyzz<C> acc = Xyzz<C>::inf(), sum = Xyzz<C>::inf();
  for (int b = (int)L - 1; b >= 0; b--) {
    acc = add_quad(acc, load_in<PK>(buckets, base + b), qi);
    sum = add_quad(sum, acc, qi);
  }
  if (qi == 0) {
    store_acc(S_out, t, sum);
    store_acc(Tn, g * S + (k ? k - 1 : S - 1), k ? acc : Xyzz<C>::inf());
  }
}

// k_seg_run_quad with one lane per segment (throughput shape: >= 2^18
// segments, e.g. the 2^24 commit's 4096 rows x 128 segments)
template <class F, bool PK = true>
__global__ void __launch_bounds__(64) k_seg_run_lane(const Xyzz<F>* __restrict__ buckets, uint32_t nb, uint32_t L,
                                                     size_t nseg, Xyzz<F>* __restrict__ S_out,
                                                     Xyzz<F>* __restrict__ Tn) {
  using C = typename AccField<F>::T;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nseg) return;
  const uint32_t S = nb / L;
  const size_t g = t / S;
  const uint32_t k = (uint32_t)(t % S);
  const size_t base = g * nb + (size_t)k * L;
  Xyzz<C> acc = Xyzz<C>::inf(), sum = Xyzz<C>::inf();
  for (int b = (int)L - 1; b >= 0; b--) {
    acc = add(acc, load_in<PK>(buckets, base + b));
    sum = add(sum, acc);
  }
  store_acc(S_out, t, sum);
  store_acc(Tn, g * S + (k ? k - 1 : S - 1), k ? acc : Xyzz<C>::inf());
}

// out[g] = a[g] + 2^lg b[g], one quad per group
template <class F>
__global__ void __launch_bounds__(64) k_lift_add_quad(const Xyzz<F>* __restrict__ a, const Xyzz<F>* __restrict__ b,
                                                      int lg, size_t groups, Xyzz<F>* __restrict__ out,
                                                      int prio = 0) {
  using C = typename AccField<F>::T;
  set_wave_prio(prio);
  const size_t g = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 2;
  const int qi = threadIdx.x & 3;
  if (g >= groups) return;
  Xyzz<C> r = load_acc(b, g);
  for (int i = 0; i < lg; i++) r = dbl_quad(r, qi);
  r = add_quad(r, load_acc(a, g), qi);
  if (qi == 0) store_acc(out, g, r);
}

constexpr int RED2_LG = 4;  // level-1 segment length 16

static bool red2_ok(uint32_t nb) { return nb >= (16u << RED2_LG); }

template <class F>
static size_t reduce2_scratch(size_t groups, uint32_t nb) {
  const uint32_t S1 = nb >> RED2_LG;
  return 2 * Arena::need(groups * S1, sizeof(Xyzz<F>)) + reduce_scratch<F>(groups, S1) +
         Arena::need(groups * S1 / 64 + 1, sizeof(Xyzz<F>)) + 2 * Arena::need(groups, sizeof(Xyzz<F>));
}

#ifndef TPST_RED2_LANE
#define TPST_RED2_LANE 1
#endif
// lane_ok: a throughput reduction (under other accumulation work) -- one lane
// per segment costs fewer VALU issue slots per addition than a quad
template <class F>
static hipError_t reduce_buckets2(Arena& ar, hipStream_t s, const Xyzz<F>* d_buckets, size_t groups, uint32_t nb,
                                  Xyzz<F>* d_group_out, int prio, bool lane_ok = false) {
  const uint32_t L1 = 1u << RED2_LG, S1 = nb / L1;
  const size_t nseg = groups * S1;
  Xyzz<F>* Sk = ar.take<Xyzz<F>>(nseg);
  Xyzz<F>* Tn = ar.take<Xyzz<F>>(nseg);
  Xyzz<F>* R = ar.take<Xyzz<F>>(groups);
  Xyzz<F>* SS = ar.take<Xyzz<F>>(groups);
  if (std::is_same<F, Fq>::value && (nseg >= ((size_t)1 << 18) || (TPST_RED2_LANE && lane_ok)))
    k_seg_run_lane<F><<<grid_for(nseg, 64), 64, 0, s>>>(d_buckets, nb, L1, nseg, Sk, Tn);
  else
    k_seg_run_quad<F><<<grid_for(4 * nseg, 64), 64, 0, s>>>(d_buckets, nb, L1, nseg, Sk, Tn, prio);
  TPST_TRY(hipGetLastError());
  TPST_TRY(reduce_buckets<F>(ar, s, Tn, groups, S1, R, prio, false));  // Tn: a reduction's output
  TPST_TRY(sum_groups<F>(ar, s, Sk, groups, S1, SS, prio));
  k_lift_add_quad<F><<<grid_for(4 * groups, 64), 64, 0, s>>>(SS, R, RED2_LG, groups, d_group_out, prio);
  return hipGetLastError();
}

}  // namespace tpst
