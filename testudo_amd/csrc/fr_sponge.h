// PoseidonSponge<Fr> over poseidon_params() (parameters.rs:156-186) on the host:
// the sponge of MultiCommitGens::new (commitments.rs:17-39, gens_new.hip) and
// of PoseidonTranscript<Fr> (poseidon_transcript.rs), which the Hyrax
// evaluation proofs run over (hyrax.hip, tpst_transcript_fr_*).
//
// Not to be included beside poseidon_host.h (the Fq sponge of the MIPP): both
// pull in poseidon_constants.inc.
#pragma once
#include <cstring>
#include <vector>

#include "../../include/tpst.h"
#include "field.h"

namespace tpst {

#include "poseidon_constants.inc"

inline bool fr_ge_r(const uint64_t* v) {
  static const uint64_t FR_P64[4] = {0x0a11800000000001ull, 0x59aa76fed0000001ull, 0x60b44d1e5c37b001ull,
                                     0x12ab655e9a2ca556ull};
  for (int k = 3; k >= 0; k--)
    if (v[k] != FR_P64[k]) return v[k] > FR_P64[k];
  return true;
}

// a < 2^256 canonical -> Montgomery Fr (reduced mod r)
inline Fr fr_from_u256(const uint64_t* a) {
  static const uint64_t FR_P64[4] = {0x0a11800000000001ull, 0x59aa76fed0000001ull, 0x60b44d1e5c37b001ull,
                                     0x12ab655e9a2ca556ull};
  uint64_t v[4] = {a[0], a[1], a[2], a[3]};
  while (fr_ge_r(v)) {
    unsigned __int128 br = 0;
    for (int k = 0; k < 4; k++) {
      const unsigned __int128 d = (unsigned __int128)v[k] - FR_P64[k] - (uint64_t)br;
      v[k] = (uint64_t)d;
      br = (d >> 64) & 1;
    }
  }
  Fr f;
  memcpy(f.v, v, 32);
  return to_mont(f);
}

struct FrPoseidon {
  Fr ark[39][3], mds[3][3];
  FrPoseidon() {
    for (int r = 0; r < 39; r++)
      for (int i = 0; i < 3; i++) ark[r][i] = fr_from_u256(POSEIDON_ARK[r][i]);
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) mds[i][j] = fr_from_u256(POSEIDON_MDS[i][j]);
  }
};

inline const FrPoseidon& frp() {
  static FrPoseidon p;
  return p;
}

// PoseidonSponge<Fr>: rate 2, capacity 1, alpha 17, 8 full + 31 partial rounds
struct FrSponge {
  Fr st[3] = {Fr::zero(), Fr::zero(), Fr::zero()};
  bool squeezing = false;
  int idx = 0;
  void permute() {
    const FrPoseidon& P = frp();
    for (int r = 0; r < 39; r++) {
      for (int i = 0; i < 3; i++) st[i] = add(st[i], P.ark[r][i]);
      const bool full = r < 4 || r >= 35;
      for (int i = 0; i < (full ? 3 : 1); i++) {
        const Fr x = st[i], x2 = mul(x, x), x4 = mul(x2, x2), x8 = mul(x4, x4), x16 = mul(x8, x8);
        st[i] = mul(x16, x);
      }
      Fr ns[3];
      for (int i = 0; i < 3; i++) ns[i] = add(add(mul(P.mds[i][0], st[0]), mul(P.mds[i][1], st[1])), mul(P.mds[i][2], st[2]));
      for (int i = 0; i < 3; i++) st[i] = ns[i];
    }
  }
  void absorb(const Fr* e, size_t n) {
    if (!n) return;
    if (squeezing || idx == 2) {
      permute();
      idx = 0;
    }
    for (size_t k = 0; k < n; k++) {
      if (idx == 2) {
        permute();
        idx = 0;
      }
      st[1 + idx] = add(st[1 + idx], e[k]);
      idx++;
    }
    squeezing = false;
  }
  void absorb(const std::vector<Fr>& e) { absorb(e.data(), e.size()); }
  // Absorb for byte slices: u64 LE length prefix, 31-byte LE chunks
  void absorb_bytes(const uint8_t* d, size_t n) {
    std::vector<uint8_t> buf(8 + n);
    const uint64_t len = n;
    memcpy(buf.data(), &len, 8);
    if (n) memcpy(buf.data() + 8, d, n);
    std::vector<Fr> e;
    for (size_t o = 0; o < buf.size(); o += 31) {
      uint64_t l[4] = {0, 0, 0, 0};
      memcpy(l, buf.data() + o, buf.size() - o < 31 ? buf.size() - o : 31);
      e.push_back(fr_from_u256(l));
    }
    absorb(e);
  }
  Fr squeeze1() {
    if (!squeezing || idx == 2) {
      permute();
      idx = 0;
    }
    squeezing = true;
    return st[1 + idx++];
  }
  // squeeze_bytes(32): two native elements, 31 LE bytes of each, truncated
  void squeeze32(uint8_t* out) {
    uint8_t b[62];
    for (int k = 0; k < 2; k++) {
      const Fr c = from_mont(squeeze1());
      memcpy(b + 31 * k, c.v, 31);
    }
    memcpy(out, b, 32);
  }
  // the caller-held state of tpst_transcript_fr (canonical limbs); false for a
  // state no sponge can be in
  bool load(const tpst_transcript_fr* t) {
    if (t->squeezing > 1 || t->index > 2) return false;
    for (int i = 0; i < 3; i++) {
      if (fr_ge_r(t->state[i])) return false;
      st[i] = fr_from_u256(t->state[i]);
    }
    squeezing = t->squeezing != 0;
    idx = (int)t->index;
    return true;
  }
  void store(tpst_transcript_fr* t) const {
    for (int i = 0; i < 3; i++) {
      const Fr c = from_mont(st[i]);
      memcpy(t->state[i], c.v, 32);
    }
    t->squeezing = squeezing ? 1 : 0;
    t->index = (uint32_t)idx;
  }
};

}  // namespace tpst
