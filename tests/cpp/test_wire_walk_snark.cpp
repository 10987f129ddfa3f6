// Stand-alone check of the byte-level structure walk of R1CSProof and of the
// SNARK proof (csrc/wire_snark.h over csrc/wire_spark.h, no HIP, no library):
// built with -fsanitize=address,undefined by tests/test_wire_walk_snark.py,
// which passes the golden byte strings as files and the dimensions as numbers.
//
//   test_wire_walk_snark SNARK_PROOF R1CS_PROOF num_cons num_vars derefs_rows ell_ops ell_mem ell_derefs
//                        log_ops log_cells
//
// For both layouts the walk must accept the original and reject every
// truncation to 0 .. len - 1 bytes, one appended byte, and every length prefix
// replaced by itself +- 1, by 0 and by 2^63 + 1.  Every candidate is walked in a
// heap buffer of exactly its own length, so that a read past the end is an
// AddressSanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "wire_snark.h"

using namespace tpst::wire;
typedef std::vector<uint8_t> Bytes;

static long cases = 0, bad = 0;

static void expect(bool got, bool want, const char* what, size_t at) {
  cases++;
  if (got != want) {
    bad++;
    fprintf(stderr, "FAIL %s at %zu: walk returned %d\n", what, at, (int)got);
  }
}

// the walk over an exact-size heap copy
static bool walk_copy(const std::vector<Item>& items, const uint8_t* p, size_t n) {
  uint8_t* h = (uint8_t*)malloc(n ? n : 1);
  if (n) memcpy(h, p, n);
  std::vector<size_t> o;
  const bool ok = walk_snark_items(h, n, items, o);
  free(h);
  return ok;
}

static bool check(const char* name, const Bytes& b, const std::vector<Item>& items) {
  std::vector<size_t> offs;
  if (!walk_snark_items(b.data(), b.size(), items, offs) || snark_items_bytes(items) != b.size()) {
    fprintf(stderr, "the golden %s does not walk\n", name);
    return false;
  }
  expect(walk_copy(items, b.data(), b.size()), true, name, b.size());
  for (size_t n = 0; n < b.size(); n++) expect(walk_copy(items, b.data(), n), false, "truncation", n);
  Bytes more(b);
  more.push_back(0);
  expect(walk_copy(items, more.data(), more.size()), false, "appended byte", more.size());
  size_t prefixes = 0;
  for (size_t i = 0; i < items.size(); i++) {
    if (items[i].kind != LEN) continue;
    prefixes++;
    uint64_t v;
    memcpy(&v, &b[offs[i]], 8);
    const uint64_t repl[4] = {v + 1, v - 1, 0, (1ull << 63) + 1};
    for (uint64_t r : repl) {
      if (r == v) continue;
      Bytes m(b);
      memcpy(&m[offs[i]], &r, 8);
      expect(walk_copy(items, m.data(), m.size()), false, "length prefix", offs[i]);
    }
  }
  return prefixes > 0;
}

static Bytes read_file(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    exit(2);
  }
  Bytes b;
  uint8_t buf[4096];
  size_t k;
  while ((k = fread(buf, 1, sizeof(buf), f)) > 0) b.insert(b.end(), buf, buf + k);
  fclose(f);
  return b;
}

int main(int argc, char** argv) {
  if (argc != 11) {
    fprintf(stderr,
            "usage: %s SNARK_PROOF R1CS_PROOF num_cons num_vars derefs_rows ell_ops ell_mem ell_derefs log_ops "
            "log_cells\n",
            argv[0]);
    return 2;
  }
  const Bytes snark = read_file(argv[1]), sat = read_file(argv[2]);
  SatDims d;
  if (!sat_dims((uint64_t)atol(argv[3]), (uint64_t)atol(argv[4]), d)) {
    fprintf(stderr, "dimensions no R1CSProof has\n");
    return 1;
  }
  tpst_r1cs_eval_sizes z;
  memset(&z, 0, sizeof(z));
  z.derefs_rows = (size_t)atol(argv[5]);
  z.ell_ops = atoi(argv[6]), z.ell_mem = atoi(argv[7]), z.ell_derefs = atoi(argv[8]);
  z.log_ops = atoi(argv[9]), z.log_cells = atoi(argv[10]);
  // tpst_prodcircuit_proof_len(ell, P, D) = 2 ell (ell - 1) + 2 ell P + 3 D at (12, 6) and (4, 0)
  const size_t lo = (size_t)z.log_ops, lc = (size_t)z.log_cells;
  z.prod_ops_len = 2 * lo * (lo - 1) + 2 * lo * 12 + 18;
  z.prod_mem_len = 2 * lc * (lc - 1) + 2 * lc * 4;

  std::vector<Item> items;
  if (!r1cs_proof_items(d, items) || !check("R1CSProof", sat, items)) return 1;
  if (!snark_items(d, z, items) || !check("SNARK proof", snark, items)) return 1;

  // dimensions no proof has are refused before any byte is read
  SatDims none;
  const uint64_t bad_dims[5][2] = {{0, 16}, {16, 2}, {3, 16}, {16, 24}, {(uint64_t)1 << 63, 16}};
  for (const uint64_t* v : bad_dims) {
    cases++;
    if (sat_dims(v[0], v[1], none)) bad++, fprintf(stderr, "FAIL dimensions %llu x %llu accepted\n",
                                                   (unsigned long long)v[0], (unsigned long long)v[1]);
  }

  printf("cases %ld bad %ld\n", cases, bad);
  return bad ? 1 : 0;
}
