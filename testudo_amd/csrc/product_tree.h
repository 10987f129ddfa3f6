// The two-step form of the batched product-circuit prover (product_tree.hip),
// for sparse_eval.hip: ProductLayerProof::prove (sparse_mlpoly.rs:1053-1236)
// appends the claims of BOTH batched proofs to the transcript before the first
// of them runs, so the claims have to exist before any round does.
// tpst_prodcircuit_prove(_dev) is build followed by rounds.  Internal: nothing
// here is part of include/tpst.h.
#pragma once
#include <vector>

#include "../../include/tpst.h"
#include "pst_state.h"

namespace tpst {

struct ProdCircuitProver {
  int ell = 0;
  size_t P = 0, D = 0;
  DevBuf arena;  // every layer, the dot-product tables, eq pair, partials, slots (Fr)
  std::vector<size_t> loff;
  size_t o_dot = 0, o_eq = 0, o_eqs = 0, o_part = 0, o_sums = 0, o_r = 0, o_lay = 0, o_fin = 0;
  std::vector<Fr> claims, cdot;
  // allocates the arena, builds the layers over the device inputs (canonical
  // Fr, laid out as tpst_prodcircuit_prove_dev takes them) and returns
  // claims_prod (P Fr) and claims_dotp (D Fr).  Dimensions are the caller's to
  // check; the caller holds the context lock.
  int build(tpst_ctx* ctx, int ell, size_t P, const uint32_t* d_polys, size_t D, const uint32_t* d_left,
            const uint32_t* d_right, const uint32_t* d_weight, uint64_t* claims_prod, uint64_t* claims_dotp);
  // the layer proofs over `tr` (updated in place) into the flat proof, and rand.
  // Allocates nothing on the device.
  int rounds(tpst_ctx* ctx, tpst_transcript_fr* tr, uint64_t* proof, uint64_t* rand_out);
};

}  // namespace tpst
