// Byte-level structure walk of the arkworks wire format (ark-serialize 0.4,
// Compress::Yes) of R1CSCommitment, R1CSEvalProof and CommitterKey: lengths,
// offsets and bounds only, no field or curve arithmetic and no HIP, so that it
// compiles alone (tests/cpp/test_wire_walk.cpp runs it under the sanitizers).
// serialize.hip writes and reads the elements at the places found here.
//
// A layout is a list of items in wire order.  LEN is a u64 LE whose value the
// sizes fix (a usize field or a Vec length prefix); FR / G1 / G2 are runs of
// 32 / 48 / 96-byte elements that live at `word` (u64 index) of caller buffer
// `buf`.  Field order is declaration order, Vec<T> = length || elements, tuples
// field by field; G: CurveGroup values serialise as their affine form.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/tpst.h"

namespace tpst {
namespace wire {

enum Kind : uint8_t { LEN = 0, FR, G1, G2 };
constexpr size_t KIND_BYTES[4] = {8, 32, 48, 96};
constexpr size_t KIND_WORDS[4] = {1, 4, 12, 24};  // u64 per element in the caller's buffer

struct Item {
  Kind kind;
  uint8_t buf;   // which caller buffer (the layout's own numbering)
  size_t count;  // LEN: the value; otherwise the number of elements
  size_t word;   // first u64 of the run in that buffer
};

// bounds-checked reads; n <= len always, and no product of an unchecked count
struct Cursor {
  const uint8_t* in;
  size_t len, n = 0;
  bool take(size_t count, size_t elem, size_t* off) {
    if (count > (len - n) / elem) return false;
    *off = n;
    n += count * elem;
    return true;
  }
  bool u64(uint64_t* v) {
    size_t o;
    if (!take(1, 8, &o)) return false;
    memcpy(v, in + o, 8);
    return true;
  }
};

// places every item: offs[i] = byte offset of item i (of the prefix itself for
// LEN).  False for a truncated input, a prefix of another value, trailing bytes.
inline bool walk_items(const uint8_t* in, size_t len, const std::vector<Item>& items, std::vector<size_t>& offs) {
  Cursor c{in, len};
  offs.assign(items.size(), 0);
  for (size_t i = 0; i < items.size(); i++) {
    const Item& it = items[i];
    if (it.kind == LEN) {
      uint64_t v;
      offs[i] = c.n;
      if (!c.u64(&v) || v != (uint64_t)it.count) return false;
    } else if (!c.take(it.count, KIND_BYTES[it.kind], &offs[i])) {
      return false;
    }
  }
  return c.n == len;
}

inline size_t items_bytes(const std::vector<Item>& items) {
  size_t n = 0;
  for (const Item& it : items) n += it.kind == LEN ? 8 : it.count * KIND_BYTES[it.kind];
  return n;
}

// ------------------------------------------------------------ R1CSEvalProof --
enum ProofBuf : uint8_t { B_PROOF = 0, B_DEREFS, B_PROD_OPS, B_PROD_MEM };
constexpr size_t BATCH_SIZE = 3;  // (A, B, C)

// rounds of the three openings: log2 of the columns of a polynomial of ell variables
inline int open_rounds(int ell) { return ell - ell / 2; }

inline bool proof_sizes_ok(const tpst_r1cs_eval_sizes& z) {
  const int ells[3] = {z.ell_ops, z.ell_mem, z.ell_derefs};
  for (int e : ells)
    if (e < 1 || e > 2 * TPST_HYRAX_MAX_ROUNDS || open_rounds(e) > TPST_HYRAX_MAX_ROUNDS) return false;
  if (z.log_ops < 1 || z.log_ops > 30 || z.log_cells < 1 || z.log_cells > 30) return false;
  const size_t lo = (size_t)z.log_ops, lc = (size_t)z.log_cells;
  return z.derefs_rows == (size_t)1 << (z.ell_derefs / 2) &&
         z.prod_ops_len == 2 * lo * (lo - 1) + 2 * lo * 4 * BATCH_SIZE + 3 * 2 * BATCH_SIZE &&
         z.prod_mem_len == 2 * lc * (lc - 1) + 2 * lc * 4;
}

// ProductCircuitEvalProofBatched { proof: Vec<LayerProofBatched { proof: SumcheckInstanceProof { polys:
// Vec<UniPoly { coeffs }> }, claims_prod_left, claims_prod_right }>, claims_dotp: (Vec, Vec, Vec) } from the
// flat buffer of tpst_prodcircuit_proof_len: all round polynomials, then all lefts, then all rights, then
// the 3 x D dot-product claims -- interleaved per layer here
inline void prodcircuit_items(std::vector<Item>& it, uint8_t buf, int ell, size_t P, size_t D) {
  const size_t L = (size_t)ell, left0 = 4 * (L * (L - 1) / 2), right0 = left0 + L * P, dotp0 = right0 + L * P;
  it.push_back({LEN, buf, L, 0});
  size_t poly = 0;
  for (size_t i = 0; i < L; i++) {
    it.push_back({LEN, buf, i, 0});
    for (size_t r = 0; r < i; r++, poly++) {
      it.push_back({LEN, buf, 4, 0});
      it.push_back({FR, buf, 4, 4 * (4 * poly)});
    }
    it.push_back({LEN, buf, P, 0});
    it.push_back({FR, buf, P, 4 * (left0 + i * P)});
    it.push_back({LEN, buf, P, 0});
    it.push_back({FR, buf, P, 4 * (right0 + i * P)});
  }
  for (size_t k = 0; k < 3; k++) {
    it.push_back({LEN, buf, D, 0});
    it.push_back({FR, buf, D, 4 * (dotp0 + k * D)});
  }
}

// PolyEvalProof { DotProductProofLog { BulletReductionProof { L_vec, R_vec }, delta, beta, z1, z2 } }
inline void dotprod_items(std::vector<Item>& it, size_t base_bytes, int rounds) {
  const size_t w = base_bytes / 8, R = (size_t)rounds;
  it.push_back({LEN, B_PROOF, R, 0});
  it.push_back({G1, B_PROOF, R, w + offsetof(tpst_dotprod_proof, L) / 8});
  it.push_back({LEN, B_PROOF, R, 0});
  it.push_back({G1, B_PROOF, R, w + offsetof(tpst_dotprod_proof, R) / 8});
  it.push_back({G1, B_PROOF, 1, w + offsetof(tpst_dotprod_proof, delta) / 8});
  it.push_back({G1, B_PROOF, 1, w + offsetof(tpst_dotprod_proof, beta) / 8});
  it.push_back({FR, B_PROOF, 1, w + offsetof(tpst_dotprod_proof, z1) / 8});
  it.push_back({FR, B_PROOF, 1, w + offsetof(tpst_dotprod_proof, z2) / 8});
}

// R1CSEvalProof { SparseMatPolyEvalProof { comm_derefs: DerefsCommitment { PolyCommitment { C: Vec<G1> } },
// PolyEvalNetworkProof { ProductLayerProof, HashLayerProof } } }; false for sizes no proof has
inline bool proof_items(const tpst_r1cs_eval_sizes& z, std::vector<Item>& it) {
  it.clear();
  if (!proof_sizes_ok(z)) return false;
  typedef tpst_r1cs_eval_proof P;
  const auto fr = [&](size_t byte_off, size_t count) { it.push_back({FR, B_PROOF, count, byte_off / 8}); };
  const auto vec = [&](size_t byte_off, size_t count) {
    it.push_back({LEN, B_PROOF, count, 0});
    fr(byte_off, count);
  };
  it.push_back({LEN, B_DEREFS, z.derefs_rows, 0});
  it.push_back({G1, B_DEREFS, z.derefs_rows, 0});
  // ProductLayerProof: eval_row / eval_col = (init, Vec read, Vec write, audit); eval_val = (Vec left, Vec
  // right); proof_mem, then proof_ops
  for (size_t side : {offsetof(P, prod_row), offsetof(P, prod_col)}) {
    fr(side, 1);
    vec(side + 32, BATCH_SIZE);
    vec(side + 4 * 32, BATCH_SIZE);
    fr(side + 7 * 32, 1);
  }
  vec(offsetof(P, prod_val), BATCH_SIZE);
  vec(offsetof(P, prod_val) + BATCH_SIZE * 32, BATCH_SIZE);
  prodcircuit_items(it, B_PROD_MEM, z.log_cells, 4, 0);
  prodcircuit_items(it, B_PROD_OPS, z.log_ops, 4 * BATCH_SIZE, 2 * BATCH_SIZE);
  // HashLayerProof: eval_row / eval_col = (Vec ops_addr, Vec read_ts, audit_ts); eval_val; eval_derefs = (Vec
  // row_ops_val, Vec col_ops_val); proof_ops, proof_mem, proof_derefs
  for (size_t side : {offsetof(P, hash_row), offsetof(P, hash_col)}) {
    vec(side, BATCH_SIZE);
    vec(side + 3 * 32, BATCH_SIZE);
    fr(side + 6 * 32, 1);
  }
  vec(offsetof(P, hash_val), BATCH_SIZE);
  vec(offsetof(P, hash_derefs), BATCH_SIZE);
  vec(offsetof(P, hash_derefs) + BATCH_SIZE * 32, BATCH_SIZE);
  dotprod_items(it, offsetof(P, proof_ops), open_rounds(z.ell_ops));
  dotprod_items(it, offsetof(P, proof_mem), open_rounds(z.ell_mem));
  dotprod_items(it, offsetof(P, proof_derefs), open_rounds(z.ell_derefs));
  return true;
}

// ----------------------------------------------------------- R1CSCommitment --
// R1CSCommitment { num_cons, num_vars, num_inputs, SparseMatPolyCommitment { batch_size, num_ops,
// num_mem_cells, comm_comb_ops: PolyCommitment { C }, comm_comb_mem: PolyCommitment { C } } }
struct CommitmentWalk {
  uint64_t dims[5];  // num_cons, num_vars, num_inputs, num_ops, num_mem_cells
  size_t ops_rows, ops_off, mem_rows, mem_off;
  size_t len_off[2];  // byte offsets of the two Vec length prefixes
};

inline int log2_pow2(uint64_t v) {  // -1 unless v is a power of two
  if (!v || (v & (v - 1))) return -1;
  int l = 0;
  while (!((v >> l) & 1)) l++;
  return l;
}

// rows of the two committed polynomials: comb_ops has log2(num_ops) + 4 variables, comb_mem
// log2(num_mem_cells) + 1, and ell variables commit as 2^(ell / 2) rows; false for dimensions no
// commitment has
inline bool commitment_rows(uint64_t num_ops, uint64_t num_mem_cells, size_t* ops_rows, size_t* mem_rows) {
  const int lo = log2_pow2(num_ops), lc = log2_pow2(num_mem_cells);
  if (lo < 1 || lc < 1 || lo > 40 || lc > 40) return false;
  *ops_rows = (size_t)1 << ((lo + 4) / 2);
  *mem_rows = (size_t)1 << ((lc + 1) / 2);
  return true;
}

inline bool walk_commitment(const uint8_t* in, size_t len, CommitmentWalk& w) {
  Cursor c{in, len};
  uint64_t batch, rows;
  size_t want_ops, want_mem;
  for (int k = 0; k < 3; k++)
    if (!c.u64(&w.dims[k])) return false;
  if (!c.u64(&batch) || batch != BATCH_SIZE) return false;
  if (!c.u64(&w.dims[3]) || !c.u64(&w.dims[4])) return false;
  if (!commitment_rows(w.dims[3], w.dims[4], &want_ops, &want_mem)) return false;
  w.len_off[0] = c.n;
  if (!c.u64(&rows) || rows != want_ops || !c.take(want_ops, KIND_BYTES[G1], &w.ops_off)) return false;
  w.ops_rows = want_ops;
  w.len_off[1] = c.n;
  if (!c.u64(&rows) || rows != want_mem || !c.take(want_mem, KIND_BYTES[G1], &w.mem_off)) return false;
  w.mem_rows = want_mem;
  return c.n == len;
}

// ------------------------------------------------------------- CommitterKey --
// CommitterKey { nv, powers_of_g: Vec<Vec<G1>>, powers_of_h: Vec<Vec<G2>>, g, h }: level i holds
// 2^(nv - i) points.  Buffer 0 = the flat SRS of tpst_srs_export (g | h | per level powers_of_g[i] |
// powers_of_h[i] | g_mask | h_mask; the masks are not part of the key).
inline void committer_key_items(int nv, std::vector<Item>& it) {
  it.clear();
  std::vector<size_t> pg(nv), ph(nv);
  size_t off = 36;
  for (int i = 0; i < nv; i++) {
    pg[i] = off;
    off += ((size_t)1 << (nv - i)) * 12;
    ph[i] = off;
    off += ((size_t)1 << (nv - i)) * 24;
  }
  it.push_back({LEN, 0, (size_t)nv, 0});
  it.push_back({LEN, 0, (size_t)nv, 0});
  for (int i = 0; i < nv; i++) {
    it.push_back({LEN, 0, (size_t)1 << (nv - i), 0});
    it.push_back({G1, 0, (size_t)1 << (nv - i), pg[i]});
  }
  it.push_back({LEN, 0, (size_t)nv, 0});
  for (int i = 0; i < nv; i++) {
    it.push_back({LEN, 0, (size_t)1 << (nv - i), 0});
    it.push_back({G2, 0, (size_t)1 << (nv - i), ph[i]});
  }
  it.push_back({G1, 0, 1, 0});
  it.push_back({G2, 0, 1, 12});
}

// nv from the first field (1 .. TPST_MAX_VARS), then the layout it implies
inline bool walk_committer_key(const uint8_t* in, size_t len, int* nv, std::vector<Item>& items,
                               std::vector<size_t>& offs) {
  Cursor c{in, len};
  uint64_t v;
  if (!c.u64(&v) || v < 1 || v > TPST_MAX_VARS) return false;
  *nv = (int)v;
  committer_key_items(*nv, items);
  return walk_items(in, len, items, offs);
}

}  // namespace wire
}  // namespace tpst
