// State behind the opaque handles of the SPARK evaluation proofs
// (sparse_eval.hip): the generators of R1CSCommitmentGens::setup and the
// device-resident decommitment (MultiSparseMatPolynomialAsDense) that
// r1cs.hip's dense-representation builder fills.  Internal: nothing here is
// part of include/tpst.h.
#pragma once
#include <vector>

#include "../../include/tpst.h"
#include "pst_state.h"

// SparseMatPolyCommitmentGens (sparse_mlpoly.rs:290-323): three Hyrax
// generator sets, k = 0 ops, 1 mem, 2 derefs
struct tpst_r1cs_gens {
  const tpst_ctx* owner = nullptr;
  size_t num_cons = 0, num_vars = 0, num_inputs = 0, N = 0, cells = 0;
  int ell[3] = {0, 0, 0};
  tpst_gens* g[3] = {nullptr, nullptr, nullptr};  // over G[0..R) with h
  uint64_t Q[3][12] = {};                         // G[R], canonical affine
  ~tpst_r1cs_gens() {
    for (int k = 0; k < 3; k++)
      if (g[k]) tpst_gens_free(g[k]);
  }
};

// R1CSDecommitment: what tpst_r1cs_commit builds, kept on the device
struct tpst_r1cs_decomm {
  const tpst_ctx* owner = nullptr;
  size_t num_cons = 0, num_vars = 0, num_inputs = 0;
  size_t N = 0, cells = 0;  // ops per matrix (padded), memory cells
  int vx = 0, vy = 0;
  // comb_ops: 16 N canonical Fr, row.ops_addr | row.read_ts | col.ops_addr |
  // col.read_ts | val | 0, each of the five 3 N (matrix after matrix);
  // comb_mem: row.audit_ts | col.audit_ts, 2 cells
  tpst::DevBuf ops, mem;
  // the same addresses and timestamps as u32: [0] rows, [1] columns
  tpst::DevBuf addr[2], rts[2], audit[2];
};

namespace tpst {
// r1cs.hip: the dense representation of R (multi_sparse_to_dense_rep) into d
int r1cs_dense_rep(tpst_ctx* ctx, tpst_r1cs* R, tpst_r1cs_decomm& d);
}  // namespace tpst
