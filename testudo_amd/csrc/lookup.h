// Lookup argument on committed polynomials (lookup.hip; include/tpst.h,
// "lookup argument"): the device stages that build the LogUp helper tables
//   m(y)   = #{(l, x) : a_l(x) = t(y)}, credited to the first y holding the value
//   h_l(x) = 1 / (beta + a_l(x)),   h_t(y) = m(y) / (beta + t(y))
// and the sums of the h tables.  Internal interface of the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace tpst {

// most witness polynomials of one lookup (include/tpst.h)
constexpr size_t LOOKUP_MAX_WITNESSES = 8;
// an empty slot of the index; "no entry" of the two error cells
constexpr uint32_t LK_EMPTY = 0xFFFFFFFFu;
constexpr unsigned long long LK_NONE = ~0ull;

// workgroups of 256 lanes for `items` independent items (TPST_LOOKUP_GRID caps it; no result depends on it)
unsigned lookup_grid(size_t items);

// The index of the table: 2^slots_log2 >= N slots (n <= slots_log2 <= 31), each LK_EMPTY or the LEAST index y whose
// value hashes and probes there (open addressing, linear probing; keys are compared on all 8 words of t[y]).
// d_slots must hold LK_EMPTY everywhere before the call.  d_t: N canonical Fr, 16-byte aligned, never written.
hipError_t lookup_index_build(hipStream_t s, const uint32_t* d_t, size_t N, uint32_t* d_slots, int slots_log2);

// One probe per witness entry: d_cnt[y] += 1 for the slot index y of a_l[x] (d_cnt zeroed by the caller; equal
// destinations are combined inside a wave before the atomic), or *d_miss = min(*d_miss, l N + x) when the value
// is not in the table (*d_miss = LK_NONE before the call).  d_wits: device array of L tables of N Fr.  L N < 2^32.
hipError_t lookup_count(hipStream_t s, const uint32_t* const* d_wits, int L, size_t N, const uint32_t* d_t,
                        const uint32_t* d_slots, int slots_log2, uint32_t* d_cnt, unsigned long long* d_miss);

// d_m[y] = the Fr of d_cnt[y], canonical
hipError_t lookup_counts_fr(hipStream_t s, const uint32_t* d_cnt, size_t N, uint32_t* d_m);

// d_out[i] = d_num[i] / (beta + d_f[i]) (d_num null: 1 / ...), all canonical, exact: Montgomery's trick per lane
// over the lane's grid-strided entries -- one inversion per lane, d_out holds the prefix products in between, so
// d_out must not alias d_f or d_num.  A zero denominator is replaced by 1 for the products (it does not poison
// its lane) and reported: *d_zero = min(*d_zero, i) (LK_NONE before the call); the outputs are then not valid.
hipError_t lookup_inverse(hipStream_t s, const uint32_t* d_f, const uint32_t* d_num, const uint32_t* d_beta, size_t N,
                          uint32_t* d_out, unsigned long long* d_zero);

// d_out[0] = sum_i d_x[i], canonical, exact (LDS tree, no atomics); d_partial: lookup_grid(N) Fr
hipError_t lookup_sum(hipStream_t s, const uint32_t* d_x, size_t N, uint32_t* d_partial, uint32_t* d_out);

}  // namespace tpst
