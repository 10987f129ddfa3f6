// The state behind the opaque tpst_gens handle (gens_api.hip), shared with the
// Hyrax evaluation proofs (hyrax.hip).  Internal: not part of include/tpst.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/tpst.h"
#include "msm.h"

struct tpst_gens {
  tpst_ctx* ctx = nullptr;
  size_t n = 0;
  bool has_h = false;
  uint32_t* d_G = nullptr;   // n affine G1, Montgomery
  uint32_t* d_h = nullptr;   // 1 affine G1, Montgomery
  tpst::BatchTables tables;  // K1 window tables over G
  ~tpst_gens() {
    if (d_G) (void)hipFree(d_G);
    if (d_h) (void)hipFree(d_h);
    tpst::batch_tables_free(tables);
  }
};
