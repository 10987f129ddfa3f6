// Instruction-count probe for the mixed add (cross-compiles without a GPU):
//   hipcc -std=c++17 -O3 --offload-arch=gfx950 -I testudo_amd/csrc --cuda-device-only -S \
//         profiles/chain_start/madd_count.hip -o madd_count.s
//   python tools/isa_blocks.py madd_count.s k_madd_full     (then k_madd_step1, k_mul)
// k_madd_full loops add_affine; k_madd_step1 loops the shared body with the
// wave-uniform `unit` flag set at step 1, as the accumulation kernels do.
#include <hip/hip_runtime.h>
#include "acc_field.h"
using namespace tpst;

__device__ __forceinline__ void load_ops(const uint32_t* in, uint32_t t, Affine<Fq29>& g, Xyzz<Fq29>& acc) {
  for (int i = 0; i < 13; i++) {
    g.x.v[i] = in[i + 26 * t];
    g.y.v[i] = in[13 + i + 26 * t];
    acc.X.v[i] = in[100 + i + t];
    acc.Y.v[i] = in[200 + i + t];
    acc.ZZ.v[i] = in[300 + i + t];
    acc.ZZZ.v[i] = in[400 + i + t];
  }
}

__global__ void k_mul(int iters, uint32_t* out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  Fq29 a = Fq29::one(), b = Fq29::one();
  a.v[0] ^= t & 0xffffu;
  b.v[1] ^= (t * 7u + 1) & 0xffffu;
#pragma unroll 1
  for (int i = 0; i < iters; i++) a = mul(a, b);
#pragma unroll
  for (int i = 0; i < 13; i++) out[13 * (size_t)t + i] = a.v[i];
}

__global__ void __launch_bounds__(64, 2) k_madd_full(int iters, const uint32_t* in, uint32_t* out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  Affine<Fq29> g;
  Xyzz<Fq29> acc;
  load_ops(in, t, g, acc);
#pragma unroll 1
  for (int i = 0; i < iters; i++) acc = add_affine(acc, g);
#pragma unroll
  for (int i = 0; i < 13; i++) out[13 * (size_t)t + i] = acc.X.v[i] ^ acc.Y.v[i] ^ acc.ZZ.v[i] ^ acc.ZZZ.v[i];
}

__global__ void __launch_bounds__(64, 2) k_madd_step1(int iters, const uint32_t* in, uint32_t* out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  Affine<Fq29> g;
  Xyzz<Fq29> acc;
  load_ops(in, t, g, acc);
#pragma unroll 1
  for (int i = 0; i < iters; i++) acc = add_affine(acc, g, i == 1);
#pragma unroll
  for (int i = 0; i < 13; i++) out[13 * (size_t)t + i] = acc.X.v[i] ^ acc.Y.v[i] ^ acc.ZZ.v[i] ^ acc.ZZZ.v[i];
}
