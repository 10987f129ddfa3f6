// G2 (Fq2) instantiations of the MSM pipeline, compiled as a separate
// translation unit so the build parallelises.  The G2 variable-base MSM
// serves the verifier, tpst_g2_msm and Groth16's B (groth16.hip; the opening's
// G2 MSMs run on fixed-base tables, fbt.hip).  Its Fq2 products stay out of
// line (see field.h): inlined, the XYZZ mixed addition spills ~420 VGPRs and
// the unit takes ~9 min to compile.
#define TPST_FQ2_ATTR __host__ __device__ inline __attribute__((noinline))
#include "msm_var.h"

namespace tpst {

// explicit instantiations (G2)
template hipError_t msm_var<Fq2>(Arena&, hipStream_t, const uint32_t*, const uint32_t*, size_t, Xyzz<Fq2>*,
                                 hipStream_t, bool*, hipStream_t, bool);
template hipError_t points_to_mont<Fq2>(hipStream_t, const uint32_t*, uint32_t*, size_t);
template hipError_t affine_from_mont<Fq2>(hipStream_t, const uint32_t*, uint32_t*, size_t);
template hipError_t xyzz_to_affine_canonical<Fq2>(hipStream_t, const Xyzz<Fq2>*, uint32_t*, size_t);

}  // namespace tpst
