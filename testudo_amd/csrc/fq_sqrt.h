// Square roots over Fq on the device (Tonelli-Shanks, p - 1 = 2^46 q) and the
// canonical ordering arkworks' point compression uses, one lane per element:
// shared by the generator sampler (gens_new.hip) and the point codec
// (point_codec.hip).  The constants are computed on the host and passed by value.
#pragma once
#include <cstring>

#include "field.h"

namespace tpst {

struct SqrtConsts {
  uint32_t e[12];   // (q - 1) / 2, q = (p - 1) / 2^46
  uint32_t zq[12];  // z^q (Montgomery), z the least non-residue
};

#if defined(__HIPCC__)
__device__ inline Fq fq_pow_dev(const Fq& a, const uint32_t* e, int nbits) {
  Fq r = Fq::one();
  for (int b = nbits - 1; b >= 0; b--) {
    r = mul(r, r);
    if ((e[b >> 5] >> (b & 31)) & 1) r = mul(r, a);
  }
  return r;
}

// Tonelli-Shanks (2-adicity 46); false for a non-residue
__device__ inline bool fq_sqrt_dev(const Fq& a, const SqrtConsts& K, Fq& out) {
  if (is_zero(a)) {
    out = a;
    return true;
  }
  const Fq w = fq_pow_dev(a, K.e, 330);
  Fq r = mul(a, w), t = mul(r, w), c = Fq::from_limbs(K.zq);
  int m = 46;
  while (!eq(t, Fq::one())) {
    int i = 0;
    Fq t2 = t;
    while (!eq(t2, Fq::one())) {
      t2 = mul(t2, t2);
      if (++i == m) return false;
    }
    Fq b = c;
    for (int k = 0; k < m - i - 1; k++) b = mul(b, b);
    m = i;
    c = mul(b, b);
    t = mul(t, c);
    r = mul(r, b);
  }
  out = r;
  return true;
}

__device__ inline bool lt_p_words(const uint32_t* w) {
  for (int i = 11; i >= 0; i--)
    if (w[i] != params::FQ_P[i]) return w[i] < params::FQ_P[i];
  return false;
}

__device__ inline int cmp_canon(const Fq& a, const Fq& b) {
  const Fq x = from_mont(a), y = from_mont(b);
  for (int i = 11; i >= 0; i--)
    if (x.v[i] != y.v[i]) return x.v[i] < y.v[i] ? -1 : 1;
  return 0;
}
#endif  // __HIPCC__

inline SqrtConsts sqrt_consts() {
  // e = (q - 1) / 2 with q = (p - 1) >> 46 (p - 1 = p with limb 0 cleared: p's low word is 1)
  uint32_t pm1[12];
  for (int i = 0; i < 12; i++) pm1[i] = params::FQ_P[i];
  pm1[0] -= 1;
  auto shr = [](uint32_t* a, int s) {
    for (int k = 0; k < s; k++)
      for (int i = 0; i < 12; i++) a[i] = (a[i] >> 1) | (i < 11 ? a[i + 1] << 31 : 0);
  };
  SqrtConsts K;
  uint32_t q[12];
  memcpy(q, pm1, 48);
  shr(q, 46);
  memcpy(K.e, q, 48);
  K.e[0] -= 1;  // q odd
  shr(K.e, 1);
  // z = least quadratic non-residue: z^((p-1)/2) = -1
  uint32_t half[12];
  memcpy(half, pm1, 48);
  shr(half, 1);
  auto powh = [](const Fq& a, const uint32_t* e, int nb) {
    Fq r = Fq::one();
    for (int b = nb - 1; b >= 0; b--) {
      r = mul(r, r);
      if ((e[b >> 5] >> (b & 31)) & 1) r = mul(r, a);
    }
    return r;
  };
  Fq z = Fq::one();
  const Fq minus1 = neg(Fq::one());
  do {
    z = add(z, Fq::one());
  } while (!eq(powh(z, half, 377), minus1));
  const Fq zq = powh(z, q, 331);
  memcpy(K.zq, zq.v, 48);
  return K;
}

}  // namespace tpst
