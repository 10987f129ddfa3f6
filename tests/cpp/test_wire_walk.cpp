// Stand-alone check of the byte-level structure walk (csrc/wire_spark.h alone,
// no HIP, no library): built with -fsanitize=address,undefined by
// tests/test_wire_walk.py, which passes the golden proof and commitment as
// files and the proof's sizes as numbers.
//
//   test_wire_walk PROOF COMMITMENT derefs_rows ell_ops ell_mem ell_derefs log_ops log_cells
//
// For the proof, the commitment and a synthetic CommitterKey (nv = 3, zero
// elements: the walk reads lengths only) the walk must accept the original and
// reject every truncation to 0 .. len - 1 bytes, one appended byte, and every
// Vec length prefix replaced by itself +- 1, by 0 and by 2^63 + 1.  Every
// candidate is walked in a heap buffer of exactly its own length, so that a
// read past the end is an AddressSanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "wire_spark.h"

using namespace tpst::wire;
typedef std::vector<uint8_t> Bytes;
typedef std::function<bool(const uint8_t*, size_t)> Walk;

static long cases = 0, bad = 0;

static void expect(bool got, bool want, const char* what, size_t at) {
  cases++;
  if (got != want) {
    bad++;
    fprintf(stderr, "FAIL %s at %zu: walk returned %d\n", what, at, (int)got);
  }
}

// the walk over an exact-size heap copy
static bool walk_copy(const Walk& walk, const uint8_t* p, size_t n) {
  uint8_t* h = (uint8_t*)malloc(n ? n : 1);
  if (n) memcpy(h, p, n);
  const bool ok = walk(h, n);
  free(h);
  return ok;
}

static void check(const char* name, const Bytes& b, const std::vector<size_t>& prefixes, const Walk& walk) {
  expect(walk_copy(walk, b.data(), b.size()), true, name, b.size());
  for (size_t n = 0; n < b.size(); n++) expect(walk_copy(walk, b.data(), n), false, "truncation", n);
  Bytes more(b);
  more.push_back(0);
  expect(walk_copy(walk, more.data(), more.size()), false, "appended byte", more.size());
  for (size_t off : prefixes) {
    uint64_t v;
    memcpy(&v, &b[off], 8);
    const uint64_t repl[4] = {v + 1, v - 1, 0, (1ull << 63) + 1};
    for (uint64_t r : repl) {
      if (r == v) continue;
      Bytes m(b);
      memcpy(&m[off], &r, 8);
      expect(walk_copy(walk, m.data(), m.size()), false, "length prefix", off);
    }
  }
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

static std::vector<size_t> len_offsets(const std::vector<Item>& items, const std::vector<size_t>& offs, size_t skip) {
  std::vector<size_t> out;
  for (size_t i = skip; i < items.size(); i++)
    if (items[i].kind == LEN) out.push_back(offs[i]);
  return out;
}

int main(int argc, char** argv) {
  if (argc != 9) {
    fprintf(stderr, "usage: %s PROOF COMMITMENT derefs_rows ell_ops ell_mem ell_derefs log_ops log_cells\n", argv[0]);
    return 2;
  }
  const Bytes proof = read_file(argv[1]), comm = read_file(argv[2]);
  tpst_r1cs_eval_sizes z;
  memset(&z, 0, sizeof(z));
  z.derefs_rows = (size_t)atol(argv[3]);
  z.ell_ops = atoi(argv[4]), z.ell_mem = atoi(argv[5]), z.ell_derefs = atoi(argv[6]);
  z.log_ops = atoi(argv[7]), z.log_cells = atoi(argv[8]);
  // tpst_prodcircuit_proof_len(ell, P, D) = 2 ell (ell - 1) + 2 ell P + 3 D at (12, 6) and (4, 0)
  const size_t lo = (size_t)z.log_ops, lc = (size_t)z.log_cells;
  z.prod_ops_len = 2 * lo * (lo - 1) + 2 * lo * 12 + 18;
  z.prod_mem_len = 2 * lc * (lc - 1) + 2 * lc * 4;

  // ---- R1CSEvalProof
  std::vector<Item> items;
  std::vector<size_t> offs;
  if (!proof_items(z, items) || !walk_items(proof.data(), proof.size(), items, offs)) {
    fprintf(stderr, "the golden proof does not walk\n");
    return 1;
  }
  if (items_bytes(items) != proof.size()) {
    fprintf(stderr, "items_bytes disagrees with the proof's length\n");
    return 1;
  }
  check("proof", proof, len_offsets(items, offs, 0), [&](const uint8_t* p, size_t n) {
    std::vector<size_t> o;
    return walk_items(p, n, items, o);
  });

  // ---- R1CSCommitment
  CommitmentWalk cw;
  if (!walk_commitment(comm.data(), comm.size(), cw)) {
    fprintf(stderr, "the golden commitment does not walk\n");
    return 1;
  }
  check("commitment", comm, {cw.len_off[0], cw.len_off[1]}, [](const uint8_t* p, size_t n) {
    CommitmentWalk w;
    return walk_commitment(p, n, w);
  });
  {  // batch_size other than 3
    Bytes m(comm);
    m[24] = 4;
    cases++;
    CommitmentWalk w;
    if (walk_commitment(m.data(), m.size(), w)) bad++, fprintf(stderr, "FAIL batch_size 4 accepted\n");
  }

  // ---- CommitterKey, nv = 3: lengths over zero elements
  std::vector<Item> kitems;
  committer_key_items(3, kitems);
  Bytes key;
  for (const Item& it : kitems) {
    if (it.kind == LEN) {
      const uint64_t v = it.count;
      key.insert(key.end(), (const uint8_t*)&v, (const uint8_t*)&v + 8);
    } else {
      key.insert(key.end(), it.count * KIND_BYTES[it.kind], 0);
    }
  }
  std::vector<size_t> koffs;
  int nv = 0;
  std::vector<Item> got;
  if (!walk_committer_key(key.data(), key.size(), &nv, got, koffs) || nv != 3) {
    fprintf(stderr, "the synthetic key does not walk\n");
    return 1;
  }
  // item 0 is the nv field itself (1 .. TPST_MAX_VARS picks the layout): a Vec prefix from item 1 on
  check("committer key", key, len_offsets(got, koffs, 1), [](const uint8_t* p, size_t n) {
    int v;
    std::vector<Item> it;
    std::vector<size_t> o;
    return walk_committer_key(p, n, &v, it, o);
  });
  const uint64_t bad_nv[5] = {0, 2, 4, TPST_MAX_VARS + 1, ((uint64_t)1 << 63) + 1};
  for (uint64_t v : bad_nv) {
    Bytes m(key);
    memcpy(&m[0], &v, 8);
    int x;
    std::vector<Item> it;
    std::vector<size_t> o;
    cases++;
    if (walk_committer_key(m.data(), m.size(), &x, it, o)) bad++, fprintf(stderr, "FAIL nv %llu accepted\n", (unsigned long long)v);
  }

  printf("cases %ld bad %ld\n", cases, bad);
  return bad ? 1 : 0;
}
