// TestudoSnark / TestudoNizk: the end-to-end composition (testudo_snark.rs:
// 120-235, testudo_nizk.rs:80-157) of the library's own entry points --
// tpst_r1cs_prove / tpst_r1cs_verify_evals / tpst_r1cs_verify, tpst_r1cs_evaluate,
// tpst_r1cs_eval_prove / _verify -- with the transcript calls between them
// that bind the parts: SparseMatPolyEvalProof::prove absorbs neither the
// commitment nor (rx, ry) nor the claimed evaluations (sparse_mlpoly.rs:1473-
// 1568); only this layer does.
//
// Host code only, no kernel: every device stage runs behind one of those entry
// points, each of which takes the context's lock for itself (the way
// tpst_r1cs_prove composes tpst_poly_commit / tpst_poly_open).  The protocol,
// step by step, is the comment of this section in include/tpst.h.
//
// F, the caller's PoseidonTranscript<Fr>, is worked on as a copy and stored
// back only on success; Q, the PoseidonTranscript<Fq> of the satisfiability
// proof, lives and dies inside a call.
#include <cstring>
#include <vector>

#include "../../include/tpst.h"
#include "ctx.h"
#include "fr_sponge.h"
#include "r1cs_state.h"
#include "sparse_eval_state.h"
#include "wire_spark.h"

using namespace tpst;

namespace {

constexpr uint64_t BATCH_SIZE = 3;  // (A, B, C)

void absorb_u64(FrSponge& sp, uint64_t x) {
  const uint64_t c[4] = {x, 0, 0, 0};
  const Fr f = fr_canon(c);
  sp.absorb(&f, 1);
}

void absorb_scalars(FrSponge& sp, const uint64_t* c, size_t n) {
  for (size_t i = 0; i < n; i++) {
    const Fr f = fr_canon(c + 4 * i);
    sp.absorb(&f, 1);
  }
}

bool frs_ok(const uint64_t* p, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!fr_ok(p + 4 * i)) return false;
  return true;
}

// the pointers and row counts of a caller's commitment
bool commitment_shape_ok(const tpst_r1cs_commitment* c) {
  size_t ops_rows, mem_rows;
  return c && c->comm_ops && c->comm_mem && wire::commitment_rows(c->num_ops, c->num_mem_cells, &ops_rows, &mem_rows) &&
         c->ops_rows == ops_rows && c->mem_rows == mem_rows;
}

// step 1: R1CSCommitment::write_to_transcript; false for a point that is not canonical
bool absorb_commitment(FrSponge& sp, const tpst_r1cs_commitment* c) {
  for (uint64_t v : {(uint64_t)c->num_cons, (uint64_t)c->num_vars, (uint64_t)c->num_inputs, BATCH_SIZE,
                     (uint64_t)c->num_ops, (uint64_t)c->num_mem_cells})
    absorb_u64(sp, v);
  const uint64_t* lists[2] = {c->comm_ops, c->comm_mem};
  const size_t rows[2] = {c->ops_rows, c->mem_rows};
  for (int k = 0; k < 2; k++)
    for (size_t i = 0; i < rows[k]; i++) {
      uint8_t b[48];
      if (tpst_ser_g1(lists[k] + 12 * i, b) != TPST_OK) return false;
      sp.absorb_bytes(b, 48);
    }
  return true;
}

// steps 2-4: c, F.new_from_state(&c), Q = fresh + new_from_state2(&c)
void fork(FrSponge& F, tpst_transcript* Q) {
  const Fr c = F.squeeze1();
  uint64_t cc[4];
  fr_out(c, cc);
  F = FrSponge();
  F.absorb(&c, 1);
  tpst_transcript_init(Q);
  tpst_transcript_reset_fr(Q, cc);
}

// step 8: what ties F to the satisfiability proof made over Q; evals NULL in NIZK mode
void bind(FrSponge& F, const tpst_r1cs_proof* sat, const uint64_t* evals) {
  absorb_scalars(F, sat->transcript_sat_state, 1);
  absorb_scalars(F, &sat->rx[0][0], (size_t)sat->rounds_x);
  absorb_scalars(F, &sat->ry[0][0], (size_t)sat->rounds_y);
  if (evals) absorb_scalars(F, evals, 3);
}

// what both provers settle first; the padded witness into `padded`
int prover_precheck(tpst_ctx* ctx, const tpst_r1cs* R, const uint64_t* vars, size_t n_vars, const uint64_t* inputs,
                    std::vector<uint64_t>& padded) {
  if (R->owner != ctx) return fail(ctx, TPST_E_ARG, "instance belongs to another context");
  const int nvar_bits = log2_exact(R->num_vars);
  if (nvar_bits < 2) return fail(ctx, TPST_E_ARG, "the witness commitment needs num_vars >= 4");
  if (n_vars > R->num_vars) return fail(ctx, TPST_E_ARG, "more witness values than the instance has variables");
  if ((n_vars && !vars) || (R->num_inputs && !inputs)) return fail(ctx, TPST_E_ARG, "null argument");
  if (!frs_ok(vars, n_vars)) return fail(ctx, TPST_E_ARG, "witness value >= r");
  if (!frs_ok(inputs, R->num_inputs)) return fail(ctx, TPST_E_ARG, "input value >= r");
  if (srs_nv(ctx) != nvar_bits - nvar_bits / 2)
    return fail(ctx, TPST_E_STATE, "no SRS loaded for ceil(log2(num_vars) / 2) variables");
  padded.assign(4 * R->num_vars, 0);  // step 5 (lib.rs:99-113)
  if (n_vars) memcpy(padded.data(), vars, n_vars * 32);
  return TPST_OK;
}

bool same_dims(const tpst_r1cs_commitment* c, const tpst_r1cs_gens* g) {
  return c->num_cons == g->num_cons && c->num_vars == g->num_vars && c->num_inputs == g->num_inputs &&
         c->num_ops == g->N && c->num_mem_cells == g->cells;
}

}  // namespace

extern "C" int tpst_transcript_fr_append_u64(tpst_transcript_fr* t, uint64_t x) {
  if (!t) return TPST_E_ARG;
  FrSponge sp;
  if (!sp.load(t)) return TPST_E_ARG;
  absorb_u64(sp, x);
  sp.store(t);
  return TPST_OK;
}

extern "C" int tpst_transcript_fr_new_from_state(tpst_transcript_fr* t, const uint64_t* fr) {
  if (!t || !fr || !fr_ok(fr)) return TPST_E_ARG;
  FrSponge sp;
  absorb_scalars(sp, fr, 1);
  sp.store(t);
  return TPST_OK;
}

extern "C" int tpst_r1cs_commitment_absorb(const tpst_r1cs_commitment* comm, tpst_transcript_fr* tr) {
  if (!tr || !commitment_shape_ok(comm)) return TPST_E_ARG;
  FrSponge sp;
  if (!sp.load(tr) || !absorb_commitment(sp, comm)) return TPST_E_ARG;
  sp.store(tr);
  return TPST_OK;
}

// TestudoSnark::prove (testudo_snark.rs:120-196)
extern "C" int tpst_snark_prove(tpst_ctx* ctx, tpst_r1cs* R, const tpst_r1cs_commitment* comm,
                                const tpst_r1cs_decomm* decomm, const tpst_r1cs_gens* gens, const uint64_t* vars,
                                size_t n_vars, const uint64_t* inputs, const uint64_t* rnd_derefs,
                                const uint64_t* rnd_ops, const uint64_t* rnd_mem, tpst_transcript_fr* tr,
                                tpst_snark_proof* proof, uint64_t* comm_derefs, uint64_t* prod_ops,
                                uint64_t* prod_mem) {
  if (!ctx || !R || !comm || !decomm || !gens || !rnd_derefs || !rnd_ops || !rnd_mem || !tr || !proof ||
      !comm_derefs || !prod_ops || !prod_mem)
    return fail(ctx, TPST_E_ARG, "null argument");
  if (gens->owner != ctx) return fail(ctx, TPST_E_ARG, "generators belong to another context");
  if (decomm->owner != ctx) return fail(ctx, TPST_E_ARG, "decommitment belongs to another context");
  std::vector<uint64_t> padded;
  if (int rc = prover_precheck(ctx, R, vars, n_vars, inputs, padded)) return rc;
  if (!commitment_shape_ok(comm)) return fail(ctx, TPST_E_ARG, "commitment rows do not follow from its dimensions");
  if (!same_dims(comm, gens) || R->num_cons != gens->num_cons || R->num_vars != gens->num_vars ||
      R->num_inputs != gens->num_inputs || decomm->num_cons != gens->num_cons || decomm->num_vars != gens->num_vars ||
      decomm->N != gens->N || decomm->cells != gens->cells)
    return fail(ctx, TPST_E_ARG, "instance, commitment, decommitment and generators of different shapes");
  FrSponge F;
  if (!F.load(tr)) return fail(ctx, TPST_E_ARG, "bad transcript state");
  if (!absorb_commitment(F, comm)) return fail(ctx, TPST_E_ARG, "commitment point is not canonical");
  tpst_transcript Q;
  fork(F, &Q);
  if (int rc = tpst_r1cs_prove(ctx, R, padded.data(), inputs, &Q, &proof->sat)) return rc;
  const uint64_t *rx = &proof->sat.rx[0][0], *ry = &proof->sat.ry[0][0];
  if (int rc = tpst_r1cs_evaluate(ctx, R, rx, ry, &proof->inst_evals[0][0])) return rc;
  bind(F, &proof->sat, &proof->inst_evals[0][0]);
  tpst_transcript_fr t;
  F.store(&t);
  if (int rc = tpst_r1cs_eval_prove(ctx, decomm, gens, rx, ry, &proof->inst_evals[0][0], rnd_derefs, rnd_ops, rnd_mem,
                                    &t, &proof->eval, comm_derefs, prod_ops, prod_mem))
    return rc;
  *tr = t;
  return TPST_OK;
}

// TestudoSnark::verify (testudo_snark.rs:198-235)
extern "C" int tpst_snark_verify(tpst_ctx* ctx, const tpst_r1cs_commitment* comm, const tpst_r1cs_gens* gens,
                                 const uint64_t* inputs, size_t num_inputs, tpst_transcript_fr* tr,
                                 const tpst_snark_proof* proof, const uint64_t* comm_derefs, const uint64_t* prod_ops,
                                 const uint64_t* prod_mem) {
  if (!ctx || !comm || !gens || (num_inputs && !inputs) || !tr || !proof || !comm_derefs || !prod_ops || !prod_mem)
    return fail(ctx, TPST_E_ARG, "null argument");
  if (gens->owner != ctx) return fail(ctx, TPST_E_ARG, "generators belong to another context");
  if (!commitment_shape_ok(comm)) return fail(ctx, TPST_E_ARG, "commitment rows do not follow from its dimensions");
  if (!same_dims(comm, gens)) return fail(ctx, TPST_E_ARG, "commitment dimensions do not match the generators");
  if (num_inputs != comm->num_inputs)
    return fail(ctx, TPST_E_VERIFY, "snark verify: the number of inputs is not the commitment's");
  FrSponge F;
  if (!F.load(tr)) return fail(ctx, TPST_E_ARG, "bad transcript state");
  if (!absorb_commitment(F, comm)) return fail(ctx, TPST_E_VERIFY, "snark verify: commitment point is not canonical");
  tpst_transcript Q;
  fork(F, &Q);
  if (int rc = tpst_r1cs_verify_evals(ctx, comm->num_cons, comm->num_vars, inputs, num_inputs,
                                      &proof->inst_evals[0][0], &Q, &proof->sat))
    return rc;
  // rx, ry and transcript_sat_state equal values the verifier derived: canonical from here on
  bind(F, &proof->sat, &proof->inst_evals[0][0]);
  tpst_transcript_fr t;
  F.store(&t);
  if (int rc = tpst_r1cs_eval_verify(ctx, comm->comm_ops, comm->comm_mem, comm->num_ops, comm->num_mem_cells, gens,
                                     &proof->sat.rx[0][0], &proof->sat.ry[0][0], &proof->inst_evals[0][0], &t,
                                     &proof->eval, comm_derefs, prod_ops, prod_mem))
    return rc;
  *tr = t;
  return TPST_OK;
}

// TestudoNizk::prove (testudo_nizk.rs:80-130)
extern "C" int tpst_nizk_prove(tpst_ctx* ctx, tpst_r1cs* R, const uint8_t* digest, size_t digest_len,
                               const uint64_t* vars, size_t n_vars, const uint64_t* inputs, tpst_transcript_fr* tr,
                               tpst_r1cs_proof* proof) {
  if (!ctx || !R || (digest_len && !digest) || !tr || !proof) return fail(ctx, TPST_E_ARG, "null argument");
  std::vector<uint64_t> padded;
  if (int rc = prover_precheck(ctx, R, vars, n_vars, inputs, padded)) return rc;
  FrSponge F;
  if (!F.load(tr)) return fail(ctx, TPST_E_ARG, "bad transcript state");
  F.absorb_bytes(digest, digest_len);
  tpst_transcript Q;
  fork(F, &Q);
  if (int rc = tpst_r1cs_prove(ctx, R, padded.data(), inputs, &Q, proof)) return rc;
  bind(F, proof, nullptr);
  F.store(tr);
  return TPST_OK;
}

// TestudoNizk::verify (testudo_nizk.rs:136-157), with the squeeze of c that the
// reference's verifier omits and its prover does
extern "C" int tpst_nizk_verify(tpst_ctx* ctx, tpst_r1cs* R, const uint8_t* digest, size_t digest_len,
                                const uint64_t* inputs, tpst_transcript_fr* tr, const tpst_r1cs_proof* proof) {
  if (!ctx || !R || (digest_len && !digest) || (R->num_inputs && !inputs) || !tr || !proof)
    return fail(ctx, TPST_E_ARG, "null argument");
  FrSponge F;
  if (!F.load(tr)) return fail(ctx, TPST_E_ARG, "bad transcript state");
  F.absorb_bytes(digest, digest_len);
  tpst_transcript Q;
  fork(F, &Q);
  if (int rc = tpst_r1cs_verify(ctx, R, inputs, &Q, proof)) return rc;
  bind(F, proof, nullptr);
  F.store(tr);
  return TPST_OK;
}
