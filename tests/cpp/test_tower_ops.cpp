// Host run of the tower arithmetic the device engines implement, for
// tests/test_tower_vectors.py: field.h / pairing.h's own host functions (mul,
// cyclotomic_sqr, frobenius, conj, inv, final_exponentiation, g2_prepare) on
// the vectors of tests/tower_vectors.py -- a second reference, independent of
// the Python oracle and of both engines' tables.  Binary records on stdin until
// EOF:
//   i32 index (csrc/selftest_ops.h T_*), i32 n, n x words of a, n x words of b
//   (F12_MUL only)
// with a, b and the result as 144-word field.h Montgomery Fq12 (G2_PREPARE: 48
// words in, 69 x 72 words out, point-major), and per record n x result words on
// stdout.  inv(0) = 0, as on the device.  Exit status 2: not a host op.
// With the argument `table`: for ops 0 .. 1023 four i32 each: tower_op_valid,
// tower_a_words, tower_b_words, tower_out_words.
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
#include "pairing.h"
#include "selftest_ops.h"

using namespace tpst;
namespace st = tpst::selftest;

static bool get(void* p, size_t bytes) { return fread(p, 1, bytes, stdin) == bytes; }

static Fq12 load12(const uint32_t* w) {
  Fq12 f;
  Fq* c = reinterpret_cast<Fq*>(&f);
  for (int k = 0; k < 12; k++) c[k] = Fq::from_limbs(w + 12 * k);
  return f;
}
static void store12(uint32_t* w, const Fq12& f) {
  const Fq* c = reinterpret_cast<const Fq*>(&f);
  for (int k = 0; k < 12; k++)
    for (int i = 0; i < 12; i++) w[12 * k + i] = c[k].v[i];
}

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "table")) {  // the header's tables for ops [0, 1024)
    for (int o = 0; o < 1024; o++) {
      const int32_t row[4] = {st::tower_op_valid(o), st::tower_a_words(o), st::tower_b_words(o), st::tower_out_words(o)};
      fwrite(row, 4, 4, stdout);
    }
    return 0;
  }
  static_assert(sizeof(Fq12) == 144 * 4 && sizeof(LineCoeff) == 72 * 4, "word layouts");
  int32_t hdr[2];
  while (get(hdr, sizeof hdr)) {
    const int idx = hdr[0];
    const size_t n = (size_t)hdr[1];
    if (idx < 0 || idx > st::T_G2_PREPARE) return 2;
    const size_t wa = idx == st::T_G2_PREPARE ? st::TOWER_G2_WORDS : st::TOWER_FQ_WORDS;
    const size_t wb = idx == st::T_F12_MUL ? wa : 0;
    const size_t wo = idx == st::T_G2_PREPARE ? st::TOWER_LINES_WORDS : st::TOWER_FQ_WORDS;
    std::vector<uint32_t> a(n * wa), b(n * wb + 1), out(n * wo);
    if (!get(a.data(), 4 * n * wa) || (wb && !get(b.data(), 4 * n * wb))) return 1;
    for (size_t i = 0; i < n; i++) {
      if (idx == st::T_G2_PREPARE) {
        const uint32_t* w = &a[wa * i];
        const G2A q = {st::load_fq2(w), st::load_fq2(w + 24)};
        std::vector<LineCoeff> co(N_LINE_COEFFS);
        g2_prepare(q, co.data(), 1);
        std::memcpy(&out[wo * i], co.data(), wo * 4);
        continue;
      }
      const Fq12 x = load12(&a[wa * i]);
      Fq12 r;
      switch (idx) {
        case st::T_F12_MUL: r = mul(x, load12(&b[wb * i])); break;
        case st::T_F12_SQR: r = sqr(x); break;
        case st::T_CYC_SQR: r = cyclotomic_sqr(x); break;
        case st::T_FROB1: r = frobenius(x, 1); break;
        case st::T_FROB2: r = frobenius(x, 2); break;
        case st::T_FROB3: r = frobenius(x, 3); break;
        case st::T_CONJ: r = conj(x); break;
        case st::T_COPY: r = x; break;
        case st::T_INV: r = inv(x); break;
        default: r = final_exponentiation(x); break;  // T_FINAL_EXP
      }
      store12(&out[wo * i], r);
    }
    fwrite(out.data(), 4, n * wo, stdout);
  }
  return 0;
}
