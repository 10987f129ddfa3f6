// Shared by the MSM sources (msm.h lists them): window counts, the device's
// size and the constants the stages agree on.
#pragma once
#include <cstdlib>
#include <string>
#include "device_util.h"
#include "coop.h"
#include "msm.h"
#include "pair_fq2.h"
#include "glv.h"
#include "acc_field.h"
#include "inv_wave.h"
#include <type_traits>

namespace tpst {

static inline int bit_length(uint64_t v) {
  int b = 0;
  while (v) {
    b++;
    v >>= 1;
  }
  return b;
}

// signed-digit windows covering `bits` bits: ceil(bits / c) keeps the top
// digit <= 2^(c-1) (bits = 254 for full scalars, 128 for GLV halves)
static inline int num_windows_bits(int c, int bits) { return (bits + c - 1) / c; }
static inline int num_windows(int c) { return num_windows_bits(c, 254); }

// SIMDs of the current device (4 per CU on CDNA): the chunk lengths of the
// accumulation launches are sized to keep a number of waves on each
static size_t device_simds() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
    cus = 256;  // MI355X
  return (size_t)cus * 4;
}

constexpr int ACC_BLOCK_LG = 6;  // chunks (threads) per accumulation workgroup: one wave
constexpr int ACC_BLOCK = 1 << ACC_BLOCK_LG;

// words of a gather record: one affine point in the accumulation field, a
// 128-byte line (store_rec29 in msm_sort.h writes it, fetch_rec29 in msm_acc.h reads it)
constexpr int REC29_WORDS = 32;

// wave issue priority on its SIMD (s_setprio): the latency-bound reduction and
// chain kernels of the window-grouped MSM share SIMDs with accumulation waves
__device__ __forceinline__ void set_wave_prio(int prio) {
  if (prio == 1)
    __builtin_amdgcn_s_setprio(1);
  else if (prio == 2)
    __builtin_amdgcn_s_setprio(2);
  else if (prio >= 3)
    __builtin_amdgcn_s_setprio(3);
}

}  // namespace tpst
