// Host run of the self-test dispatch of csrc/selftest_ops.h (the lane forms of
// tpst_selftest_field / tpst_selftest_curve) for tests/test_selftest_ops.py:
// the same vectors and expected values as the GPU test, so that on the device
// only the device code is unknown.  Binary records on stdin until EOF:
//   i32 kind (0 field, 1 curve), i32 op, i32 n, n x words of a (p), n x words of b (q)
// and per record n x result words on stdout.  Exit status 2: not a lane op.
// kind 2 (no operands): for ops op .. op + n - 1, five i32 each:
//   field_op_valid, field_in_words, field_out_words, curve_op_valid, curve_words.
#include <cstdio>
#include <cstdint>
#include <vector>
#include "selftest_ops.h"

using namespace tpst;

static bool get(void* p, size_t bytes) { return fread(p, 1, bytes, stdin) == bytes; }

int main() {
  int32_t hdr[3];
  while (get(hdr, sizeof hdr)) {
    const int kind = hdr[0], op = hdr[1];
    const size_t n = (size_t)hdr[2];
    if (kind == 2) {  // the header's tables for ops [op, op + n): validity and word counts
      for (int o = op; o < op + (int)n; o++) {
        const int32_t row[5] = {selftest::field_op_valid(o), selftest::field_in_words(o), selftest::field_out_words(o),
                                selftest::curve_op_valid(o), selftest::curve_words(o)};
        fwrite(row, 4, 5, stdout);
      }
      continue;
    }
    if (kind == 0 ? !selftest::field_op_valid(op) : !selftest::curve_op_valid(op)) return 2;
    const size_t wi = kind == 0 ? selftest::field_in_words(op) : selftest::curve_words(op);
    const size_t wo = kind == 0 ? selftest::field_out_words(op) : selftest::curve_words(op);
    std::vector<uint32_t> a(n * wi), b(n * wi), out(n * wo);
    if (!get(a.data(), 4 * n * wi) || !get(b.data(), 4 * n * wi)) return 1;
    for (size_t i = 0; i < n; i++) {
      const bool ok = kind == 0 ? selftest::field_lane_op(op, &a[wi * i], &b[wi * i], &out[wo * i])
                                : selftest::curve_lane_op(op, &a[wi * i], &b[wi * i], &out[wo * i]);
      if (!ok) return 2;
    }
    fwrite(out.data(), 4, n * wo, stdout);
  }
  return 0;
}
