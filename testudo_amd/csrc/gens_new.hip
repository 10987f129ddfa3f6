// MultiCommitGens::new (commitments.rs:17-39) on the device: the Pedersen /
// Hyrax generators of a label.
//
//   sponge = PoseidonSponge<Fr>(poseidon_params())   (parameters.rs:156-186)
//   sponge.absorb(label); sponge.absorb(G1 generator, compressed)
//   G_i = Affine::rand(StdRng::from_seed(sponge.squeeze_bytes(32)))  i = 0..n
//
// The sponge is sequential and cheap (one permutation per generator): host.
// Each generator's StdRng (= ChaCha12) stream, Fq::rand rejection sampling,
// square root and cofactor clearing are independent: one device lane each
// (a 2^12-generator set costs milliseconds instead of seconds on the host).
// Algorithms restated from the published crates (rand 0.8 / rand_chacha 0.3 /
// ark 0.4, not vendored here) -- see oracle/py/gens.py; parity unpinned.
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/tpst.h"
#include "ctx.h"
#include "device_util.h"
#include "fq_sqrt.h"
#include "fr_sponge.h" // the host sponge (also PoseidonTranscript<Fr>, hyrax.hip)

using namespace tpst;

namespace {

// ----------------------------------------------------------- device side --
// (the square root, lt_p_words and cmp_canon: fq_sqrt.h)
__device__ __forceinline__ uint32_t rotl32(uint32_t v, int c) { return (v << c) | (v >> (32 - c)); }

// ChaCha12 keystream (rand_chacha 0.3 ChaCha12Rng: key = seed, counter from 0,
// nonce 0), consumed word by word
struct ChaChaDev {
  uint32_t key[8];
  uint32_t ctr = 0;
  uint32_t buf[16];
  int pos = 16;
  __device__ void refill() {
    uint32_t x[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key[0], key[1], key[2], key[3],
                      key[4],      key[5],      key[6],      key[7],      ctr,    0u,     0u,     0u};
    uint32_t s[16];
#pragma unroll
    for (int i = 0; i < 16; i++) s[i] = x[i];
#define QR(a, b, c, d)                \
  x[a] += x[b];                       \
  x[d] = rotl32(x[d] ^ x[a], 16);     \
  x[c] += x[d];                       \
  x[b] = rotl32(x[b] ^ x[c], 12);     \
  x[a] += x[b];                       \
  x[d] = rotl32(x[d] ^ x[a], 8);      \
  x[c] += x[d];                       \
  x[b] = rotl32(x[b] ^ x[c], 7);
    for (int r = 0; r < 6; r++) {
      QR(0, 4, 8, 12) QR(1, 5, 9, 13) QR(2, 6, 10, 14) QR(3, 7, 11, 15)
      QR(0, 5, 10, 15) QR(1, 6, 11, 12) QR(2, 7, 8, 13) QR(3, 4, 9, 14)
    }
#undef QR
#pragma unroll
    for (int i = 0; i < 16; i++) buf[i] = x[i] + s[i];
    ctr++;
    pos = 0;
  }
  __device__ uint32_t next_u32() {
    if (pos == 16) refill();
    return buf[pos++];
  }
};

// G1 cofactor (x - 1)^2 / 3 = 0x170b5d44300000000000000000000000 (125 bits)
__constant__ uint32_t G1_COFACTOR[4] = {0x00000000u, 0x00000000u, 0x30000000u, 0x170b5d44u};

// one lane per generator: Affine::rand over ChaCha12(seed); canonical x || y out
__global__ void __launch_bounds__(64) k_gens_from_seeds(const uint8_t* __restrict__ seeds, size_t n, SqrtConsts K,
                                                       uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  ChaChaDev rng;
  for (int k = 0; k < 8; k++) {
    const uint8_t* s = seeds + 32 * i + 4 * k;
    rng.key[k] = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
  }
  G1A pt;
  for (;;) {
    Fq x;  // Fq::rand: 6 u64 limbs = the Montgomery form, top limb to 57 bits, < p
    for (;;) {
      for (int k = 0; k < 12; k++) x.v[k] = rng.next_u32();
      x.v[11] &= (1u << 25) - 1;
      if (lt_p_words(x.v)) break;
    }
    const bool greatest = (rng.next_u32() >> 31) != 0;
    Fq y;
    if (!fq_sqrt_dev(add(mul(mul(x, x), x), Fq::one()), K, y)) continue;
    const Fq ny = neg(y);
    const bool y_larger = cmp_canon(y, ny) > 0;
    pt = {x, (greatest == y_larger) ? y : ny};
    break;
  }
  const G1A r = to_affine(scalar_mul(pt, G1_COFACTOR, 125));
  store_f<Fq>(out + 24 * i, from_mont(r.x));
  store_f<Fq>(out + 24 * i + 12, from_mont(r.y));
}

// compressed G1 generator (48 bytes): canonical x with the YIsNegative flag
// (params hold the generator in Montgomery form)
void g1_gen_compressed(uint8_t* b) {
  const Fq xm = Fq::from_limbs(params::G1_GEN_X), ym = Fq::from_limbs(params::G1_GEN_Y);
  const Fq xc = from_mont(xm), yc = from_mont(ym), nyc = from_mont(neg(ym));
  memcpy(b, xc.v, 48);
  bool negf = false;
  for (int i = 11; i >= 0; i--)
    if (yc.v[i] != nyc.v[i]) {
      negf = yc.v[i] > nyc.v[i];
      break;
    }
  if (negf) b[47] |= 0x80;
}

}  // namespace

// the n + 1 StdRng seeds of MultiCommitGens::new (host only)
static void gens_seeds(size_t n, const uint8_t* label, size_t label_len, uint8_t* seeds) {
  FrSponge sp;
  sp.absorb_bytes(label, label_len);
  uint8_t gb[48];
  g1_gen_compressed(gb);
  sp.absorb_bytes(gb, 48);
  for (size_t i = 0; i <= n; i++) sp.squeeze32(seeds + 32 * i);
}

extern "C" int tpst_gens_seeds(size_t n, const uint8_t* label, size_t label_len, uint8_t* seeds) {
  if (!seeds || (label_len && !label)) return TPST_E_ARG;
  gens_seeds(n, label, label_len, seeds);
  return TPST_OK;
}

extern "C" int tpst_gens_new(tpst_ctx* ctx, size_t n, const uint8_t* label, size_t label_len, uint64_t* G_out,
                             uint64_t* h_out, tpst_gens** out) {
  if (!ctx || !G_out || !h_out || (label_len && !label)) return fail(ctx, TPST_E_ARG, "null argument");
  if (n == 0 || n > ((size_t)1 << 26)) return fail(ctx, TPST_E_ARG, "n out of range");
  std::vector<uint8_t> seeds(32 * (n + 1));
  gens_seeds(n, label, label_len, seeds.data());
  static const SqrtConsts K = sqrt_consts();
  std::vector<uint64_t> pts(12 * (n + 1));
  {
    std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
    TPST_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    void *d_seeds = nullptr, *d_out = nullptr;
    TPST_HIP(ctx, hipMalloc(&d_seeds, seeds.size()));
    if (hipMalloc(&d_out, pts.size() * 8) != hipSuccess) {
      (void)hipFree(d_seeds);
      return fail(ctx, TPST_E_HIP, "hipMalloc");
    }
    hipError_t e = hipMemcpyAsync(d_seeds, seeds.data(), seeds.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
      k_gens_from_seeds<<<grid_for(n + 1, 64), 64, 0, s>>>((const uint8_t*)d_seeds, n + 1, K, (uint32_t*)d_out);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(pts.data(), d_out, pts.size() * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d_seeds);
    (void)hipFree(d_out);
    if (e != hipSuccess) return hip_fail(ctx, e, "gens_new");
  }
  memcpy(G_out, pts.data(), n * 96);
  memcpy(h_out, &pts[12 * n], 96);
  if (out) return tpst_gens_load(ctx, G_out, n, h_out, out);
  return TPST_OK;
}
