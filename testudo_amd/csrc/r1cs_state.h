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

// ---------------------------- r1cs.hip, for the batched sum-checks of
// product_tree.hip
// UniPoly::from_evals (unipoly.rs:15-45): n = 3 or 4 evaluations at 0..n-1 ->
// coefficients, constant first; UniPoly::evaluate (:66-74).  Host, Montgomery.
void from_evals(const Fr* e, int n, Fr* cs);
Fr uni_eval(const Fr* cs, int n, const Fr& r);
// EqPolynomial::evals of ell Montgomery coordinates at d_r (MSB-first) into
// d_out (2^ell Fr, 32-byte aligned) by the k_eq_evals / k_eq_outer path;
// d_half: eq_table_scratch(ell) Fr of scratch
constexpr int EQ_SPLIT_MIN = 10;  // below: one k_eq_evals launch, ell products per entry
inline size_t eq_table_scratch(int ell) {
  return ell < EQ_SPLIT_MIN ? 0 : ((size_t)1 << (ell - ell / 2)) + ((size_t)1 << (ell / 2));
}
hipError_t eq_table(hipStream_t s, const uint32_t* d_r, int ell, uint32_t* d_half, uint32_t* d_out);

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

