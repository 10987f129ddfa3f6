// Byte-level structure walk of the arkworks wire format (ark-serialize 0.4,
// Compress::Yes) of R1CSProof and of this library's SNARK proof: lengths,
// offsets and bounds only, no field or curve arithmetic and no HIP, so that it
// compiles alone (tests/cpp/test_wire_walk_snark.cpp runs it under the
// sanitizers).  The item lists and the cursor are wire_spark.h's; this header
// adds the one element kind those layouts do not have, the 576-byte Fq12 of
// R1CSProof.t and MippProof.comms_t, with a walk that knows it, so that
// wire_spark.h and its users stay as they are.
//
// R1CSProof (r1csproof.rs:32-53), fields in declaration order, from a
// tpst_r1cs_proof (buffer 0 of the layout):
//    1. comm: Commitment { nv, g_product }       nv = q.num_vars = m_row (sqrt_pst.rs:201-204), open.U
//    2. sc_proof_phase1: SumcheckInstanceProof { polys: Vec<UniPoly { coeffs: Vec<F> }> }
//                                                rounds_x polynomials of 4 coefficients, sc1
//    3. claims_phase2: (F, F, F, F)              no prefix
//    4. sc_proof_phase2                          rounds_y polynomials of 3 coefficients, sc2
//    5. eval_vars_at_ry: F
//    6. proof_eval_vars_at_ry: Proof { proofs: Vec<G2> }   m_row points, open.pst_proof
//    7. rx: Vec<F>                               rounds_x
//    8. ry: Vec<F>                               rounds_y
//    9. transcript_sat_state: F
//   10. initial_state: F
//   11. t: Fq12                                  T
//   12. mipp_proof: MippProof { comms_t: Vec<(Fq12, Fq12)>, comms_u: Vec<(G1, G1)>, final_a: G1,
//                               final_h: G2, pst_proof_h: ProofG1 { proofs: Vec<G1> } }   (mipp.rs:21-28)
// r_abc and claims_phase2_z_abc are not fields of the reference's struct: not
// written, zero after a read, read by no verifier.
//
// The SNARK proof is OUR layout, R1CSProof || R1CSEvalProof || Ar || Br || Cr:
// the reference's TestudoSnark (testudo_snark.rs:22-29, commented out there)
// starts with an R1CSVerifierProof, whose first field is a Groth16 proof this
// library does not produce, and repeats (rx, ry), which R1CSProof
// already carries.
#pragma once
#include "wire_spark.h"

namespace tpst {
namespace wire {

constexpr Kind GT = (Kind)4;  // an Fq12: 12 Fq of 48 bytes, no flags
constexpr size_t SNARK_KIND_BYTES[5] = {8, 32, 48, 96, 576};
constexpr size_t SNARK_KIND_WORDS[5] = {1, 4, 12, 24, 72};

// walk_items over the five kinds
inline bool walk_snark_items(const uint8_t* in, size_t len, const std::vector<Item>& items,
                             std::vector<size_t>& offs) {
  Cursor c{in, len};
  offs.assign(items.size(), 0);
  for (size_t i = 0; i < items.size(); i++) {
    const Item& it = items[i];
    if (it.kind == LEN) {
      uint64_t v;
      offs[i] = c.n;
      if (!c.u64(&v) || v != (uint64_t)it.count) return false;
    } else if (it.kind > GT || !c.take(it.count, SNARK_KIND_BYTES[it.kind], &offs[i])) {
      return false;
    }
  }
  return c.n == len;
}

inline size_t snark_items_bytes(const std::vector<Item>& items) {
  size_t n = 0;
  for (const Item& it : items) n += it.kind == LEN ? 8 : it.count * SNARK_KIND_BYTES[it.kind];
  return n;
}

// the dimensions an R1CSProof of a num_cons x num_vars instance has
struct SatDims {
  int rounds_x, rounds_y, m_col, m_row;
};

inline bool sat_dims(uint64_t num_cons, uint64_t num_vars, SatDims& d) {
  const int lx = log2_pow2(num_cons), lv = log2_pow2(num_vars);
  if (lx < 1 || lv < 2 || lx > TPST_R1CS_MAX_ROUNDS || lv + 1 > TPST_R1CS_MAX_ROUNDS || lv > 2 * TPST_MAX_VARS)
    return false;
  d.rounds_x = lx, d.rounds_y = lv + 1, d.m_col = lv / 2, d.m_row = lv - lv / 2;
  return true;
}

inline bool sat_dims_ok(const SatDims& d) {
  return d.rounds_x >= 1 && d.rounds_x <= TPST_R1CS_MAX_ROUNDS && d.rounds_y >= 3 &&
         d.rounds_y <= TPST_R1CS_MAX_ROUNDS && d.m_col >= 1 && d.m_col <= TPST_MAX_VARS &&
         (d.m_row == d.m_col || d.m_row == d.m_col + 1) && d.m_row <= TPST_MAX_VARS &&
         d.m_col + d.m_row == d.rounds_y - 1;
}

// appends the items of an R1CSProof held in caller buffer `buf`
inline bool sat_items(const SatDims& d, uint8_t buf, std::vector<Item>& it) {
  if (!sat_dims_ok(d)) return false;
  typedef tpst_r1cs_proof P;
  const size_t rx = (size_t)d.rounds_x, ry = (size_t)d.rounds_y, mc = (size_t)d.m_col, mr = (size_t)d.m_row;
  const size_t open = offsetof(P, open) / 8;
  const auto w = [](size_t byte_off) { return byte_off / 8; };
  it.push_back({LEN, buf, mr, 0});
  it.push_back({G1, buf, 1, open + w(offsetof(tpst_open_proof, U))});
  it.push_back({LEN, buf, rx, 0});
  for (size_t j = 0; j < rx; j++) {
    it.push_back({LEN, buf, 4, 0});
    it.push_back({FR, buf, 4, w(offsetof(P, sc1)) + 16 * j});
  }
  it.push_back({FR, buf, 4, w(offsetof(P, claims_phase2))});
  it.push_back({LEN, buf, ry, 0});
  for (size_t j = 0; j < ry; j++) {
    it.push_back({LEN, buf, 3, 0});
    it.push_back({FR, buf, 3, w(offsetof(P, sc2)) + 12 * j});
  }
  it.push_back({FR, buf, 1, w(offsetof(P, eval_vars_at_ry))});
  it.push_back({LEN, buf, mr, 0});
  it.push_back({G2, buf, mr, open + w(offsetof(tpst_open_proof, pst_proof))});
  it.push_back({LEN, buf, rx, 0});
  it.push_back({FR, buf, rx, w(offsetof(P, rx))});
  it.push_back({LEN, buf, ry, 0});
  it.push_back({FR, buf, ry, w(offsetof(P, ry))});
  it.push_back({FR, buf, 1, w(offsetof(P, transcript_sat_state))});
  it.push_back({FR, buf, 1, w(offsetof(P, initial_state))});
  it.push_back({GT, buf, 1, w(offsetof(P, T))});
  it.push_back({LEN, buf, mc, 0});
  it.push_back({GT, buf, 2 * mc, open + w(offsetof(tpst_open_proof, comms_t))});
  it.push_back({LEN, buf, mc, 0});
  it.push_back({G1, buf, 2 * mc, open + w(offsetof(tpst_open_proof, comms_u))});
  it.push_back({G1, buf, 1, open + w(offsetof(tpst_open_proof, final_a))});
  it.push_back({G2, buf, 1, open + w(offsetof(tpst_open_proof, final_h))});
  it.push_back({LEN, buf, mc, 0});
  it.push_back({G1, buf, mc, open + w(offsetof(tpst_open_proof, pst_proof_h))});
  return true;
}

// buffers of the SNARK layout: the two fixed-size structs, the three variable
// parts of the evaluation proof, the three matrix evaluations
enum SnarkBuf : uint8_t { S_SAT = 0, S_EVAL, S_DEREFS, S_PROD_OPS, S_PROD_MEM, S_EVALS, S_NBUF };

inline bool r1cs_proof_items(const SatDims& d, std::vector<Item>& it) {
  it.clear();
  return sat_items(d, S_SAT, it);
}

// R1CSProof || R1CSEvalProof || Ar || Br || Cr
inline bool snark_items(const SatDims& d, const tpst_r1cs_eval_sizes& z, std::vector<Item>& it) {
  it.clear();
  std::vector<Item> ev;
  if (!sat_items(d, S_SAT, it) || !proof_items(z, ev)) return false;
  for (Item e : ev) {
    e.buf = (uint8_t)(e.buf + S_EVAL);  // B_PROOF .. B_PROD_MEM -> S_EVAL .. S_PROD_MEM
    it.push_back(e);
  }
  it.push_back({FR, S_EVALS, 3, 0});
  return true;
}

}  // namespace wire
}  // namespace tpst
