// Device-resident R1CS instance shared by the Spartan sum-checks (r1cs.hip)
// and the Groth16 prover (groth16.hip).  The owning device buffer (DevBuf) and
// the host Fr helpers (fr_canon / fr_out / fr_ok) are pst_state.h's.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/tpst.h"
#include "pst_state.h"

namespace tpst {

inline int log2_exact(size_t n) {
  int l = 0;
  while (((size_t)1 << l) < n) l++;
  return ((size_t)1 << l) == n ? l : -1;
}

}  // namespace tpst

// ================================================================ state ==
struct tpst_r1cs {
  const tpst_ctx* owner = nullptr;  // the context whose device holds the tables
  size_t num_cons = 0, num_vars = 0, num_inputs = 0, ncols = 0;
  size_t nnz[3] = {0, 0, 0};
  tpst::DevBuf rptr[3], ridx[3], rval[3];  // CSR over rows (multiply_vec)
  tpst::DevBuf cptr[3], cidx[3], cval[3];  // CSC over the 2 num_vars columns of z (eval table)
  tpst::DevBuf orow[3], ocol[3], oval[3];  // the entries in the caller's order (SPARK dense rep)
  void* pin = nullptr;            // 4 KiB pinned host staging of the sum-check rounds
  void* pinned() {
    if (!pin && hipHostMalloc(&pin, 4096, hipHostMallocDefault) != hipSuccess) pin = nullptr;
    return pin;
  }
  ~tpst_r1cs() {
    if (pin) (void)hipHostFree(pin);
  }
};

