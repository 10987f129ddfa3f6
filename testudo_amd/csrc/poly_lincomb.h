// Linear combinations with one weight vector shared by every output
// (poly_lincomb.hip): the two device stages of opening B committed
// polynomials at one point with a single sqrt-PST proof,
//   Z*[i]         = sum_j w_j Z_j[i]          (evaluation tables, Fr)
//   comm_list*[i] = sum_j w_j comm_list_j[i]  (row commitments, G1).
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include "msm.h"

namespace tpst {

// most terms of one combination (include/tpst.h)
constexpr size_t LINCOMB_MAX_TERMS = 256;

// d_tabs: B device pointers (a device array) to tables of n canonical Fr (8
// u32 each, 16-byte aligned); d_w: B weights in Montgomery form; d_out: n
// canonical Fr.  d_out may not alias a table.
hipError_t fr_lincomb(hipStream_t s, const uint32_t* const* d_tabs, const uint32_t* d_w, size_t B, size_t n,
                      uint32_t* d_out);

// The bit schedule of a joint double-and-add over B canonical weights (4 u64
// each), split over G chains (chain g takes the terms j = g mod G): for chain g
// and step t (bit nbits - 1 - t) the terms whose weight has that bit set.
// Layout (u32): G x (nbits + 1) offsets into the index list, then the list.
struct RowSchedule {
  int nbits = 1, G = 1;
  std::vector<uint32_t> words;
};
RowSchedule row_schedule(const uint64_t* w, size_t B, size_t C);

// d_P: B lists of C affine Montgomery G1 points, list-major (24 u32 each,
// all-zero = infinity); d_sched: the schedule's words; d_part: G x C XYZZ
// scratch; d_out: C XYZZ (Montgomery).  With G == 1 d_part is not used.
hipError_t g1_lincomb_rows(hipStream_t s, const uint32_t* d_P, size_t C, const uint32_t* d_sched, int nbits, int G,
                           Xyzz<Fq>* d_part, Xyzz<Fq>* d_out);

}  // namespace tpst
