// The op programs of the radix wave engine's live kernels (pairing_wave.hip:
// k_final_wave, k_gt_pow_wave) and its Fq12 inversion, shared with the tower
// self-test (selftest.hip), which runs the same programs and the same
// inversion on chosen operands.
#pragma once
#include "wave_tower.h"

namespace tpst {

constexpr int FE_OPS[] = {wave::OP_F12_MUL, wave::OP_CYC_SQR, wave::OP_FROB1, wave::OP_FROB2,
                          wave::OP_CONJ,    wave::OP_INV1,    wave::OP_INV2,  wave::OP_INV3,
                          wave::OP_INV4,    wave::OP_INV5,    wave::OP_INV6,  wave::OP_INV7};
constexpr int N_FE_OPS = sizeof(FE_OPS) / sizeof(FE_OPS[0]);
constexpr wave::OpSet<N_FE_OPS> FE_SET(FE_OPS);
constexpr int FW_PROG = FE_SET.words;

enum { FE_MUL, FE_CYC, FE_FROB1, FE_FROB2, FE_CONJ, FE_INV1 };  // FE_INV1 + k: OP_INV(1 + k), k < 7
static_assert(FE_OPS[FE_MUL] == wave::OP_F12_MUL && FE_OPS[FE_CONJ] == wave::OP_CONJ &&
                  FE_OPS[FE_INV1] == wave::OP_INV1 && FE_OPS[FE_INV1 + 6] == wave::OP_INV7 &&
                  FE_INV1 + 7 == N_FE_OPS,
              "FE_* index FE_OPS");

// f (register F) -> f^-1 in the twelve slots from D, through the tower norms
// and one Fq inversion on lane 0 (field.h inv(Fq12)).  prog: FE_SET in LDS,
// I: 24 slots of temporaries.  f = 0 gives 0: the norm is 0 and inv(0) = 0.
__device__ __forceinline__ void fe_inv(const wave::Eng& e, const wave::lds_t* prog, int F, int I, int D) {
  const int lane = threadIdx.x & 63;
  wave::run(e, prog + FE_SET.off[FE_INV1 + 0], F, 0, I + 0);        // t = c0^2 - v c1^2
  wave::run(e, prog + FE_SET.off[FE_INV1 + 1], I + 0, 0, I + 6);    // Fq6 adjugate c'
  wave::run(e, prog + FE_SET.off[FE_INV1 + 2], I + 6, I + 0, I + 12);  // Fq6 norm t'
  wave::run(e, prog + FE_SET.off[FE_INV1 + 3], I + 12, 0, I + 14);  // Fq2 norm n
  if (lane == 0) wave::put_slot(e.lds, I + 15, inv(wave::get_slot(e.lds, I + 14)));
  wave::wave_sync();
  wave::run(e, prog + FE_SET.off[FE_INV1 + 4], I + 12, I + 15, I + 16);  // t'^-1
  wave::run(e, prog + FE_SET.off[FE_INV1 + 5], I + 6, I + 16, I + 18);   // t^-1
  wave::run(e, prog + FE_SET.off[FE_INV1 + 6], F, I + 18, D);            // f^-1
}

}  // namespace tpst
