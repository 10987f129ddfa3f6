/*
 * tpst.h -- C ABI of the MI355X-native sqrt-PST engine (libtpst.so).
 *
 * Drop-in boundary for the BLS12-377 hot path of Testudo's sqrt-PST
 * polynomial commitment (reference: rosariocannavo/testudo).  The reference
 * has no FFI of its own; every entry point below replaces one Rust call
 * site (file:line under the reference tree), see INTEGRATION.md.
 *
 * Conventions
 *  - Field elements are CANONICAL (non-Montgomery) little-endian u64 limbs:
 *      Fr  = 4 x u64 (value < r),  Fq = 6 x u64 (value < p).
 *  - G1 affine = x || y (12 u64, 96 bytes); G2 affine = x.c0 || x.c1 ||
 *    y.c0 || y.c1 (24 u64, 192 bytes).  The point at infinity is all zero
 *    (x = y = 0 lies on neither curve), i.e. arkworks' Affine with the
 *    `infinity` flag mapped to (0, 0).
 *  - GT / Fq12 = 12 Fq in arkworks order c0.c0.c0, c0.c0.c1, c0.c1.c0, ...,
 *    c1.c2.c1 (72 u64, 576 bytes).
 *  - Caller owns every host buffer; the library reads inputs and writes
 *    outputs only.  `_dev` entry points take device pointers (hipMalloc /
 *    torch allocations on the context's device) and run on the context's
 *    stream; bases passed to `_dev` calls are in Montgomery form (the same
 *    bytes as arkworks' in-memory G1Affine x/y), scalars canonical (what
 *    arkworks' msm_bigint consumes).
 *  - Return 0 (TPST_OK) or a negative TPST_E_* code; tpst_last_error()
 *    gives the message.  No exceptions or aborts cross the ABI.  One call
 *    in flight per context (internally serialised by a mutex).
 */
#ifndef TPST_H
#define TPST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TPST_OK 0
#define TPST_E_ARG -1     /* bad length / null pointer / out-of-range value */
#define TPST_E_NODEV -2   /* no HIP device */
#define TPST_E_HIP -3     /* HIP runtime failure */
#define TPST_E_STATE -4   /* e.g. no SRS loaded */
#define TPST_E_VERIFY -5  /* verification failed */

typedef struct tpst_ctx tpst_ctx;

/* ---- context ---------------------------------------------------------- */
int tpst_device_count(void);
int tpst_create(int device, tpst_ctx** out);
void tpst_destroy(tpst_ctx* ctx);
const char* tpst_last_error(const tpst_ctx* ctx);
/* hipStream_t of the context, for callers that order their own work */
void* tpst_stream(tpst_ctx* ctx);
int tpst_synchronize(tpst_ctx* ctx);
/* Ordering against a caller's stream (e.g. the framework stream that wrote a
 * device buffer handed to a _dev call, or will read one a _dev call fills).
 * The library's stream is non-blocking, so without these the two streams are
 * unordered.  tpst_wait_stream: work the library queues from now on starts
 * after everything queued on `stream` so far.  tpst_join_stream: work queued
 * on `stream` from now on starts after everything the library queued so far.
 * Both are asynchronous (one event each); stream == NULL is the legacy
 * default stream. */
int tpst_wait_stream(tpst_ctx* ctx, void* stream);
int tpst_join_stream(tpst_ctx* ctx, void* stream);

/* ---- K2: variable-base MSM ---------------------------------------------
 * sum_i scalars[i] * bases[i] over min(n_bases, n_scalars) terms.
 * Replaces <G1 as VariableBaseMSM>::msm_unchecked (sqrt_pst.rs:198,
 * mipp.rs:393 via multiexponentiation mipp.rs:385-394) and msm_bigint inside
 * MultilinearPC::commit / open. */
int tpst_g1_msm(tpst_ctx* ctx, const uint64_t* bases, size_t n_bases, const uint64_t* scalars,
                size_t n_scalars, uint64_t* out);
int tpst_g2_msm(tpst_ctx* ctx, const uint64_t* bases, size_t n_bases, const uint64_t* scalars,
                size_t n_scalars, uint64_t* out);
/* device-resident form: d_bases Montgomery affine (24 u32 each), d_scalars
 * canonical Fr (8 u32 each), d_out one canonical affine G1.  Stream-ordered:
 * the call starts after the work already queued on tpst_stream and the MSM's
 * end is ordered before anything queued on tpst_stream after it (the host
 * returns at once; consecutive calls run one after another on the device). */
int tpst_g1_msm_dev(tpst_ctx* ctx, const void* d_bases, const void* d_scalars, size_t n, void* d_out);
/* Pipelined form (opt-in): consecutive calls overlap on the library's
 * internal streams (call i+1 decomposes and sorts while call i accumulates).
 * The call starts after the work already queued on tpst_stream, but its work
 * is NOT ordered before work the caller queues directly on tpst_stream
 * afterwards.  LIFETIME RULE: d_bases, d_scalars and d_out must stay
 * allocated and unmodified (and d_out unread) until tpst_synchronize,
 * tpst_join_stream or the next call of any other tpst_* entry point (each of
 * which waits for every pending pipelined MSM) -- a framework's caching
 * allocator must not recycle them before that. */
int tpst_g1_msm_dev_async(tpst_ctx* ctx, const void* d_bases, const void* d_scalars, size_t n, void* d_out);
/* One MSM split over ranks (sqrt_pst.rs:198 / mipp.rs:393 at 1/2/4/8 GPUs):
 * each rank's share of the points as the raw XYZZ sum (192 B: X, Y, ZZ, ZZZ,
 * Montgomery u64 limbs; no per-rank affine inversion), gathered as bytes,
 * then summed on one device to one canonical affine G1 (k shares, stride_bytes
 * apart in d_parts; d_parts and stride_bytes 16-byte aligned, else TPST_E_ARG). */
int tpst_g1_msm_xyzz_dev(tpst_ctx* ctx, const void* d_bases, const void* d_scalars, size_t n, void* d_out_xyzz);
int tpst_g1_xyzz_sum_dev(tpst_ctx* ctx, const void* d_parts, size_t k, size_t stride_bytes, void* d_out);

/* Length-checked form: mipp.rs:385-394 `multiexponentiation` returns
 * Err(InvalidIPVectorLength) when the lengths differ -> TPST_E_ARG here. */
int tpst_g1_multiexp(tpst_ctx* ctx, const uint64_t* bases, size_t n_bases, const uint64_t* scalars,
                     size_t n_scalars, uint64_t* out);
int tpst_g2_multiexp(tpst_ctx* ctx, const uint64_t* bases, size_t n_bases, const uint64_t* scalars,
                     size_t n_scalars, uint64_t* out);

/* ---- shared-base batch MSM and Pedersen/Hyrax commitments -----------------
 * A generator set = MultiCommitGens {n, G[n], h} (commitments.rs:9-15),
 * uploaded once (K1 window tables built here).  h may be NULL when only the
 * batch MSM is used. */
typedef struct tpst_gens tpst_gens;
int tpst_gens_load(tpst_ctx* ctx, const uint64_t* G, size_t n, const uint64_t* h, tpst_gens** out);
void tpst_gens_free(tpst_gens* gens);
/* out[r] = sum_{j < cols} scalars[r*row_stride + j*col_stride] * G[j] for
 * r < rows (canonical affine G1 each); cols must equal gens->n.  The strides
 * let one call consume a row split of Z without a host transpose: this is
 * the whole par_iter row loop of sqrt_pst.rs:121-125 / dense_mlpoly.rs:323-327
 * in one launch. */
int tpst_g1_msm_batch(tpst_ctx* ctx, const tpst_gens* gens, const uint64_t* scalars, size_t rows, size_t cols,
                      size_t row_stride, size_t col_stride, uint64_t* out);
int tpst_g1_msm_batch_dev(tpst_ctx* ctx, const tpst_gens* gens, const void* d_scalars, size_t rows, size_t cols,
                          size_t row_stride, size_t col_stride, void* d_out);
/* MultiCommitGens::new (commitments.rs:17-39): Poseidon<Fr> over label || the
 * compressed G1 generator, 32 squeezed bytes per generator -> StdRng (ChaCha12)
 * -> Affine::rand (Fq::rand rejection sampling, square root, cofactor
 * clearing; one device lane per generator).  Writes G_out (n G1) and h_out
 * (the (n+1)-th), canonical affine; with out != NULL also loads them as a
 * generator set (tpst_gens_load). */
int tpst_gens_new(tpst_ctx* ctx, size_t n, const uint8_t* label, size_t label_len, uint64_t* G_out,
                  uint64_t* h_out, tpst_gens** out);
/* its n + 1 32-byte StdRng seeds (host only; the squeezed sponge bytes) */
int tpst_gens_seeds(size_t n, const uint8_t* label, size_t label_len, uint8_t* seeds);
/* PedersenCommit::commit_slice (commitments.rs:79-86): msm(G, scalars) + h * blind;
 * n must equal gens->n (the reference assert_eq!s, here TPST_E_ARG). */
int tpst_pedersen_commit_slice(tpst_ctx* ctx, const tpst_gens* gens, const uint64_t* scalars, size_t n,
                               const uint64_t* blind, uint64_t* out);
/* DensePolynomial::commit_inner (dense_mlpoly.rs:314-329): n_rows = |blinds|
 * rows of R = n_z / n_rows contiguous evaluations, row i -> commit_slice(Z[R i ..
 * R (i+1)], blinds[i]); out = n_rows canonical affine G1. */
int tpst_pedersen_commit_rows(tpst_ctx* ctx, const tpst_gens* gens, const uint64_t* Z, size_t n_z,
                              const uint64_t* blinds, size_t n_rows, uint64_t* out);

/* ---- fixed-base grouped MSM (csrc/fbt.h) --------------------------------
 * Builds the 64-window x 8-multiple lookup table of the n bases, then
 * out[g] = sum over k in group g of scalars[k] * bases[k] for L/D groups,
 * k(g, m) = (m / D) * L + g * D + m % D  (n % L == 0, L % D == 0).
 * L = D = n is a plain MSM; D = 1 is the MIPP fold a_i + sum_t w_t a_{i+tL}
 * (mipp.rs:124-136 applied over all rounds at once). */
int tpst_g1_msm_fixed(tpst_ctx* ctx, const uint64_t* bases, size_t n, const uint64_t* scalars, size_t L, size_t D,
                      uint64_t* out);
int tpst_g2_msm_fixed(tpst_ctx* ctx, const uint64_t* bases, size_t n, const uint64_t* scalars, size_t L, size_t D,
                      uint64_t* out);

/* ---- K4: multi-pairing ---------------------------------------------------
 * prod_i e(g1[i], g2[i]) after final exponentiation (ark-ec
 * Pairing::multi_pairing(...).0; sqrt_pst.rs:143, mipp.rs:397). */
int tpst_multi_pairing(tpst_ctx* ctx, const uint64_t* g1, const uint64_t* g2, size_t n, uint64_t* out_gt);
/* Valid::check of a canonical affine point (ark-serialize Validate::Yes):
 * coordinates < p, on the curve, in the r-torsion subgroup (infinity = all
 * zero is valid).  TPST_OK or TPST_E_VERIFY; host only, no context. */
int tpst_g1_check(const uint64_t* p);
int tpst_g2_check(const uint64_t* p);


/* ---- sqrt-PST protocol ----------------------------------------------------
 * Mirrors sqrt_pst.rs:14-265 (Polynomial), mipp.rs:21-320 (MippProof) and
 * the ark-poly-commit fork's MultilinearPC keys.  n = number of variables,
 * m_col = n/2, m_row = n - m_col. */
#define TPST_MAX_VARS 20

/* Poseidon sponge state of PoseidonTranscript<Fq> (poseidon_transcript.rs:12-15):
 * state = capacity || rate (3 canonical Fq), duplex mode and index. */
typedef struct {
  uint64_t state[3][6];
  uint32_t squeezing; /* 0 = absorbing, 1 = squeezing */
  uint32_t index;     /* next absorb / squeeze position in the rate */
} tpst_transcript;

/* (Commitment U, Proof{m_row G2}, MippProof) returned by Polynomial::open */
typedef struct {
  int32_t m_col, m_row;
  uint64_t U[12];                              /* c_u, sqrt_pst.rs:198 */
  uint64_t pst_proof[TPST_MAX_VARS][24];       /* PST proof of q (G2) */
  uint64_t comms_t[TPST_MAX_VARS][2][72];      /* MippProof.comms_t */
  uint64_t comms_u[TPST_MAX_VARS][2][12];      /* MippProof.comms_u */
  uint64_t final_a[12];                        /* MippProof.final_a */
  uint64_t final_h[24];                        /* MippProof.final_h */
  uint64_t pst_proof_h[TPST_MAX_VARS][12];     /* MippProof.pst_proof_h (G1) */
} tpst_open_proof;

typedef struct tpst_poly tpst_poly;

/* Poseidon transcript (host): new / append(G1 | GT) / challenge_scalar */
void tpst_transcript_init(tpst_transcript* t);
int tpst_transcript_append_g1(tpst_transcript* t, const uint64_t* g1);
int tpst_transcript_append_gt(tpst_transcript* t, const uint64_t* gt);
int tpst_transcript_challenge(tpst_transcript* t, uint64_t* out_fr);

/* SRS / CommitterKey + VerifierKey of MultilinearPC (setup + trim to nv vars).
 * Flat canonical layout: g | h | for i < nv: powers_of_g[i] (2^(nv-i) G1) |
 * powers_of_h[i] (2^(nv-i) G2) | g_mask (nv G1) | h_mask (nv G2). */
size_t tpst_srs_flat_len(int nv);
int tpst_srs_setup(tpst_ctx* ctx, int nv, uint64_t seed);   /* seeded trapdoor, on the GPU */
int tpst_srs_load(tpst_ctx* ctx, int nv, const uint64_t* flat);
int tpst_srs_export(tpst_ctx* ctx, uint64_t* flat);
/* SplitMix64 uniform-Fr stream used for synthetic inputs; returns next index */
uint64_t tpst_fr_stream(uint64_t seed, size_t n, uint64_t start, uint64_t* out);

/* Polynomial::from_evaluations (sqrt_pst.rs:32-75): Z = 2^n canonical Fr.
 * The row split is a strided view of Z on the device (no host transpose). */
int tpst_poly_from_evaluations(tpst_ctx* ctx, const uint64_t* Z, int n, tpst_poly** out);
int tpst_poly_from_evaluations_dev(tpst_ctx* ctx, const void* d_Z, int n, tpst_poly** out);
/* Rank-local shard: upload only the columns [c0, c1) of the
 * strided view (for every j: Z[j 2^m_col + c0 .. j 2^m_col + c1), one 2D copy).
 * Such a handle serves tpst_poly_commit_rows[_partial] for rows inside
 * [c0, c1); eval / commit / open need the whole polynomial (TPST_E_STATE). */
int tpst_poly_from_evaluations_cols(tpst_ctx* ctx, const uint64_t* Z, int n, size_t c0, size_t c1,
                                    tpst_poly** out);
void tpst_poly_free(tpst_poly* p);
/* Polynomial::eval (sqrt_pst.rs:105-115); computes and caches q, chi(b) */
int tpst_poly_eval(tpst_ctx* ctx, tpst_poly* p, const uint64_t* point, uint64_t* out_v);
/* Polynomial::commit (sqrt_pst.rs:117-149): comms = 2^m_col G1, T = GT */
int tpst_poly_commit(tpst_ctx* ctx, tpst_poly* p, uint64_t* comms, uint64_t* T);
int tpst_poly_commit_dev(tpst_ctx* ctx, tpst_poly* p, void* d_comms, void* d_T);
/* Row-sharded commit (multi-GPU): the MSMs of rows [r0, r1)
 * of the sqrt_pst.rs:121-125 loop -> (r1-r0) canonical G1; and the IPP of a
 * gathered commitment list (sqrt_pst.rs:128-143) -> T. */
int tpst_poly_commit_rows(tpst_ctx* ctx, tpst_poly* p, size_t r0, size_t r1, uint64_t* comms);
int tpst_poly_ipp(tpst_ctx* ctx, int n, const uint64_t* comms, uint64_t* T);
/* Same row range with the IPP split across ranks: also returns this share's
 * Miller-loop product prod_{r0<=i<r1} ml(C_i, h_i) BEFORE final
 * exponentiation (canonical Fq12, 72 u64).  T = FE(product of every rank's
 * partial) via tpst_gt_final_exp_product (sqrt_pst.rs:128-143 split by rows). */
int tpst_poly_commit_rows_partial(tpst_ctx* ctx, tpst_poly* p, size_t r0, size_t r1, uint64_t* comms,
                                  uint64_t* miller);
int tpst_gt_final_exp_product(tpst_ctx* ctx, const uint64_t* partials, size_t k, uint64_t* T);
/* Device-resident variants for the RCCL path (no host round trip): the share
 * [comms (R x 12) | Miller partial (72)] written into a device buffer of
 * R * 96 + 576 bytes; k partials read from device memory `stride_bytes` apart
 * (an all-gather of those buffers). */
int tpst_poly_commit_rows_partial_dev(tpst_ctx* ctx, tpst_poly* p, size_t r0, size_t r1, void* d_out);
int tpst_gt_final_exp_product_dev(tpst_ctx* ctx, const void* d_partials, size_t stride_bytes, size_t k, uint64_t* T);

/* Row-sharded opening (sqrt_pst.rs:81-101, 198).  Rank g
 * (rows [r0, r1) resident, e.g. a from_evaluations_cols handle) computes its
 * share of get_q, zq_g[j] = sum_{r0 <= i < r1} Z_i[j] chi_i(b) (2^m_row
 * canonical Fr), and of c_u = sum_{r0 <= i < r1} chi_i(b) C_i (canonical
 * affine, from its own row commitments).  The shares are summed on rank 0
 * (tpst_fr_sum_dev: k device vectors of n canonical Fr, mod r; c_u: a G1 sum),
 * which opens from an opening-only handle: tpst_poly_from_q_dev (q on the
 * device, chi(b) from the point, c_u optional -- NULL computes it) serves
 * tpst_poly_eval and tpst_poly_open without the evaluations. */
int tpst_poly_get_q_partial(tpst_ctx* ctx, tpst_poly* p, const uint64_t* point, size_t r0, size_t r1, uint64_t* zq);
int tpst_poly_get_q_partial_dev(tpst_ctx* ctx, tpst_poly* p, const uint64_t* point, size_t r0, size_t r1, void* d_zq);
int tpst_fr_sum_dev(tpst_ctx* ctx, const void* d_parts, size_t k, size_t n, void* d_out);
int tpst_poly_cu_partial(tpst_ctx* ctx, int n, const uint64_t* point, size_t r0, size_t r1, const uint64_t* comms,
                         uint64_t* out);
int tpst_poly_from_q_dev(tpst_ctx* ctx, int n, const uint64_t* point, const void* d_zq, const uint64_t* U,
                         tpst_poly** out);
/* Polynomial::open (sqrt_pst.rs:168-230); the transcript is updated in place.
 * U = MSM(comms, chi(b)) over the caller's comm_list (sqrt_pst.rs:198). */
int tpst_poly_open(tpst_ctx* ctx, tpst_poly* p, tpst_transcript* tr, const uint64_t* comms,
                   const uint64_t* point, const uint64_t* T, tpst_open_proof* proof);
/* Row-sharded Polynomial::open (the MIPP rounds of
 * mipp.rs:58-120 split across `world` ranks, one process per GPU).  Rank g
 * owns the rows i = g mod world of comm_list (and of h, y): while a round's
 * length is >= 4 world its cross MSMs, folds, h preparations and look-ahead
 * pairings run on the rank's own rows, and one all-gather per product
 * combines them (cross partials summed, Miller partials multiplied before
 * the final exponentiation); every rank replays the transcript.  At the first
 * shorter round the folded a-vector (2 world points) is gathered to rank 0,
 * which finishes the rounds and the epilogue alone.  Same proof bytes as
 * tpst_poly_open on the same inputs.
 *
 * The library does no communication: `allgather` is the caller's transport
 * (RCCL, gloo, MPI, ...).  It must gather `bytes` from d_arena + send_off of
 * every rank into d_arena + recv_off (world x bytes, rank-major) ordered
 * after the work queued on `stream` (a hipStream_t of the library) and before
 * work queued on it afterwards -- e.g. an RCCL all-gather enqueued on that
 * stream; return 0 on success.  Every rank issues the same gathers in the
 * same order.  d_arena: device memory of arena_bytes >=
 * tpst_open_sharded_arena_bytes(n, world), reachable by the transport.
 *
 * rank 0: p = the opening handle (tpst_poly_from_q_dev, or a whole
 * polynomial) and `proof`; other ranks: p and proof may be NULL.  Every
 * rank: the whole comm_list, the point, U = c_u (canonical affine, e.g. the
 * combined tpst_poly_cu_partial shares) and its own transcript copy.  With
 * fewer than 4 world rows rank 0 opens alone (the others return at once).
 *
 * After the call only rank 0's transcript is the reference's end state: the
 * other ranks stop at the hand-over round and leave theirs mid-protocol (a
 * prover that keeps using the transcript on every rank must take rank 0's).
 * The allgather callback runs while the context's lock is held: it must not
 * call back into libtpst on the same context.  A rank that returns an error
 * stops issuing gathers, so its peers would wait in their next collective:
 * on any non-OK return the caller must abort the whole group (e.g.
 * ncclCommAbort / destroying the process group), not retry the call. */
typedef int (*tpst_allgather_fn)(void* user, size_t send_off, size_t recv_off, size_t bytes, void* stream);
typedef struct {
  int world, rank;
  tpst_allgather_fn allgather;
  void* user;
  void* d_arena;
  size_t arena_bytes;
} tpst_exchange;
size_t tpst_open_sharded_arena_bytes(int n, int world);
int tpst_poly_open_sharded(tpst_ctx* ctx, tpst_poly* p, tpst_transcript* tr, int n, const uint64_t* comms,
                           const uint64_t* point, const uint64_t* U, const tpst_exchange* x, tpst_open_proof* proof);
/* Polynomial::verify (sqrt_pst.rs:232-264): TPST_OK if valid, TPST_E_VERIFY if
 * not, including any proof element that is non-canonical, off its curve or
 * outside the prime-order subgroup (checked before the transcript absorbs it). */
int tpst_pst_verify(tpst_ctx* ctx, tpst_transcript* tr, int n, const uint64_t* point, const uint64_t* v,
                    const uint64_t* T, const tpst_open_proof* proof);

/* Batch verification: B openings of n-variable polynomials against the loaded
 * SRS, decided by ONE combined check -- one multi-pairing with a single final
 * exponentiation over B (3 + m_col + m_row) pairs, one GT-power launch over
 * B (2 m_col + 1) bases and one G1 MSM over B (2 m_col + 2) points -- instead
 * of B calls of tpst_pst_verify (three final exponentiations and a stream
 * synchronisation each).  Every item is what one tpst_pst_verify call takes,
 * with its own transcript (distinct per item).
 *
 * rho: four 128-bit multipliers per item, B x 4 x 2 u64 (little-endian limb
 * pairs), in the order rho_T, rho_2, rho_1, rho_U: the weights of the item's T
 * check, check_2, check and U check in the combination.  They are an argument,
 * like every other random draw of this library, and THEY MUST BE DRAWN
 * UNIFORMLY AT RANDOM AFTER ALL PROOFS OF THE BATCH ARE FIXED (a CSPRNG, never
 * a value the prover can predict or influence, never reused across batches a
 * prover sees): under that condition a batch that holds an invalid item passes
 * with probability about 2^-128.  With predictable or repeated multipliers
 * invalid items can be made to cancel each other.  A zero multiplier is
 * TPST_E_ARG.
 *
 * Returns TPST_OK iff every item is valid, TPST_E_VERIFY otherwise; B == 0 is
 * TPST_OK.  TPST_E_ARG: a null argument (items, rho, any field of an item),
 * bad n, an item whose proof->m_col / m_row do not match n, a zero multiplier.
 * TPST_E_STATE: no SRS loaded.
 *
 * Per item, as tpst_pst_verify: every element is validated before a sponge
 * absorbs anything (scalars < r, Fq limbs < p, G1 / G2 points on their curve
 * and in the subgroup, GT coefficients < p; T and comms_t in GT).  An item with
 * a malformed element is invalid and left out of the combination; the others
 * go on.
 *
 * ok (B bytes, or NULL): ok[j] = 1 iff item j is valid -- what tpst_pst_verify
 * returns for it alone (up to the 2^-128 above).  When the combined check
 * fails they are found by bisection over it.  With ok == NULL a failing batch
 * returns TPST_E_VERIFY at once.
 *
 * Transcripts: a valid item's tr ends exactly as tpst_pst_verify leaves it; an
 * invalid item's tr is untouched, also when the batch as a whole fails.  With
 * ok == NULL and a failing combined check no verdicts exist and every tr is
 * left untouched.
 *
 * The context lock is held once for the whole call.  Callers with one proof
 * keep tpst_pst_verify. */
typedef struct {
  const uint64_t* point;        /* n Fr */
  const uint64_t* v;            /* Fr */
  const uint64_t* T;            /* GT */
  const tpst_open_proof* proof;
  tpst_transcript* tr;          /* this item's own transcript */
} tpst_verify_item;
int tpst_pst_verify_batch(tpst_ctx* ctx, int n, const tpst_verify_item* items, size_t B, const uint64_t* rho,
                          uint8_t* ok);

/* Combined opening: B polynomials of the same n (1 <= B <= 256), committed one
 * by one, opened at ONE common point with ONE proof.  No counterpart in the
 * reference.  The commitment is linear in the polynomial (the row list and
 * T), so for weights w (B canonical Fr)
 *   Z* = sum_j w_j Z_j,   comm_list*[i] = sum_j w_j comm_list_j[i],
 *   T* = prod_j T_j^(w_j), v* = sum_j w_j v_j
 * is a committed polynomial and its value at the point; one ordinary opening
 * of Z* against (comm_list*, T*) proves all B values.  The verifier forms T*
 * and v* from the B commitments T_j and the claimed v_j and runs the ordinary
 * verifier once.
 *
 * SOUNDNESS: the weights are an argument, like every other draw of this
 * library, and THEY MUST BE FIXED ONLY AFTER EVERY T_j, THE POINT AND EVERY
 * CLAIMED v_j ARE FIXED: either derived from a transcript that has absorbed
 * all of them (tpst_pst_combine_challenge, called at the same place by prover
 * and verifier) or drawn uniformly at random by the verifier afterwards.  With
 * weights the prover can predict, wrong values can be made to cancel in v*.
 *
 * tpst_poly_lincomb: a new whole-polynomial handle holding Z* (free it with
 *   tpst_poly_free).  Arithmetic only: zero weights are allowed.  TPST_E_ARG:
 *   null argument, B out of range, differing n, a weight >= r, a handle of
 *   another context; TPST_E_STATE: a handle that is not a whole polynomial
 *   (tpst_poly_from_evaluations_cols, tpst_poly_from_q_dev).
 * tpst_g1_lincomb_rows: out[i] = sum_j w_j lists[j][i] for i < C (C >= 1,
 *   B C <= 2^26); lists[j] = C canonical affine G1, all-zero = infinity;
 *   validation as tpst_g1_lincomb_batch (canonical, on the curve, no subgroup
 *   test).  The doublings of the chain are shared by all B terms and it is as
 *   long as the longest weight: 128-bit weights cost half.
 * tpst_commit_lincomb: the combined row list (comms[j] = 2^m_col G1 ->
 *   comms_out), the combined T (Ts[j] = GT -> T_out), or both; comms or Ts may
 *   be NULL (with its output), not both -- the verifier has only the T_j.
 *   TPST_E_ARG as above, and for a T_j with a coefficient >= p or outside GT.
 * tpst_pst_combine_challenge: host only.  The Fiat-Shamir weights: on the
 *   caller's transcript, append_gt of T_0..T_{B-1}, tpst_transcript_append_fr
 *   of the n point coordinates and of v_0..v_{B-1}, one challenge rho;
 *   w_j = rho^j (w_0 = 1).  TPST_E_ARG: null argument, B out of range, a
 *   coordinate or value >= r.
 * tpst_poly_open_combined: tpst_poly_lincomb, tpst_commit_lincomb,
 *   tpst_poly_eval and tpst_poly_open of the combination, under those calls'
 *   rules; writes comm_list* (2^m_col G1), T*, v* and the proof.  A zero
 *   weight is TPST_E_ARG (that polynomial would not be bound).  tr ends
 *   exactly as tpst_poly_open of Z* leaves it.
 * tpst_pst_verify_combined: T* and v* from (Ts, vs, w), then tpst_pst_verify.
 *   TPST_OK or TPST_E_VERIFY -- the latter also for a v_j or w_j >= r, a zero
 *   weight, a T_j with a coefficient >= p or outside GT, all checked before the
 *   sponge absorbs anything.  tr is changed only on TPST_OK, and then as
 *   tpst_pst_verify on (T*, v*) leaves it.  TPST_E_ARG: null argument, B out
 *   of range, sizes that do not match n; TPST_E_STATE: no SRS loaded. */
int tpst_poly_lincomb(tpst_ctx* ctx, tpst_poly* const* polys, size_t B, const uint64_t* w, tpst_poly** out);
/* The 2^n evaluations of a whole polynomial (canonical Fr, the order of
 * tpst_poly_from_evaluations) copied to the host, e.g. Z* of tpst_poly_lincomb.
 * TPST_E_STATE: not a whole polynomial. */
int tpst_poly_evaluations(tpst_ctx* ctx, const tpst_poly* p, uint64_t* Z);
int tpst_g1_lincomb_rows(tpst_ctx* ctx, const uint64_t* const* lists, size_t B, size_t C, const uint64_t* w,
                         uint64_t* out);
int tpst_commit_lincomb(tpst_ctx* ctx, int n, const uint64_t* const* comms, const uint64_t* const* Ts, size_t B,
                        const uint64_t* w, uint64_t* comms_out, uint64_t* T_out);
int tpst_pst_combine_challenge(tpst_transcript* tr, int n, const uint64_t* point, const uint64_t* const* Ts,
                               const uint64_t* vs, size_t B, uint64_t* w_out);
int tpst_poly_open_combined(tpst_ctx* ctx, tpst_poly* const* polys, const uint64_t* const* comms,
                            const uint64_t* const* Ts, size_t B, const uint64_t* w, tpst_transcript* tr,
                            const uint64_t* point, uint64_t* comms_out, uint64_t* T_out, uint64_t* v_out,
                            tpst_open_proof* proof);
int tpst_pst_verify_combined(tpst_ctx* ctx, tpst_transcript* tr, int n, const uint64_t* point, const uint64_t* vs,
                             const uint64_t* const* Ts, size_t B, const uint64_t* w, const tpst_open_proof* proof);

/* Multi-point opening: B polynomials of the same n (1 <= B <= 256), committed
 * one by one, opened at MANY points with ONE proof: K claims (1 <= K <= 4096)
 *   f_{j_k}(r_k) = v_k,  k < K,  j_k < B,  r_k in Fr^n,
 * every polynomial in at least one claim; a polynomial may occur in several
 * claims and a point may repeat.  This protocol is this library's own: the
 * reference has no counterpart.  Points and tables are in tpst_poly_eval's
 * order (v = sum_x Z[x] eq(r, x), r[0] the most significant bit of x).
 *
 * A sum-check reduces the K claims to B claims at one random point rho, which
 * one combined opening (above) then proves.  On the caller's transcript,
 * prover and verifier alike:
 *  1. statement: tpst_transcript_append_fr of B, K and n (the Fr of each
 *     integer); append_gt of T_0..T_{B-1}; per claim in order append_fr of
 *     j_k, of the n coordinates of r_k and of v_k; one challenge gamma;
 *     a_k = gamma^k (a_0 = 1).
 *  2. sum-check of e_0 = sum_k a_k v_k over g(x) = sum_j D_j(x) f_j(x) with
 *     D_j(x) = sum_{k: j_k = j} a_k eq(r_k, x): n rounds, round i binds
 *     variable i (the most significant first).  The round polynomial s_i has
 *     s_i(0) + s_i(1) = e_i; its coefficients c0, c1, c2 (UniPoly::from_evals
 *     of s_i(0), s_i(1), s_i(2), constant first) are the proof's and are
 *     absorbed with append_fr; one challenge rho_i; e_{i+1} = s_i(rho_i).
 *  3. final values: the proof carries u_j = f_j(rho); the check is
 *     e_n = sum_j u_j D_j(rho),
 *     D_j(rho) = sum_{k: j_k = j} a_k prod_i (r_ki rho_i + (1 - r_ki)(1 - rho_i)).
 *  4. tpst_pst_combine_challenge(tr, n, rho, Ts, u) gives the weights w of the
 *     combined opening of all B polynomials at rho with values u.
 * The proof: the n x 3 round coefficients, the B values u_j, one
 * tpst_open_proof.  Its wire format, a sharded (multi-rank) form and merging
 * claims that share a point are not part of this interface.
 *
 * SOUNDNESS: the sum-check bound (2n / r) plus the two random linear
 * combinations ((K - 1) / r and (B - 1) / r).  IT HOLDS ONLY BECAUSE gamma IS
 * DRAWN AFTER EVERY T_j, EVERY POINT AND EVERY CLAIMED VALUE ARE ABSORBED, AND
 * THE WEIGHTS OF STEP 4 AFTER EVERY u_j: a caller that replays these steps
 * itself must keep that order, and whatever fixed the commitments must be on
 * the transcript before the call.  With a gamma the prover can predict, wrong
 * values can be made to cancel in e_0.
 *
 * Claim k is (claim_poly[k], points + 4 n k, vals + 4 k); rounds is n x 3 Fr,
 * u B Fr, rho n Fr.
 *
 * tpst_poly_open_multi: the prover.  Steps 1-3 with the reduction on the
 *   device (the handles' tables are read, never written), then step 4 and
 *   tpst_poly_open_combined at rho; writes rounds, u, rho and what that call
 *   writes (comm_list*, T*, v*, the proof).  tr ends as tpst_poly_open_combined
 *   at rho leaves it, and is unchanged on any error.  THE PROVER DOES NOT CHECK
 *   THAT v_k IS RIGHT: a wrong claim yields a proof the verifier rejects.
 *   TPST_E_ARG: a null argument, B = 0, K = 0, B > 256, K > 4096, an index
 *   >= B, a polynomial with no claim, polynomials of different n or of another
 *   context, a coordinate or value >= r.  TPST_E_STATE: a handle that is not a
 *   whole polynomial, no SRS loaded.
 * tpst_pst_multi_reduce: HOST ONLY, no context: the verifier's steps 1-3.  On
 *   TPST_OK rho is written and tr stands where step 4 starts.  TPST_E_VERIFY: a
 *   failed round check or final identity, or any scalar (coordinate, value,
 *   round coefficient, u_j) >= r or T_j coefficient >= p.  TPST_E_ARG: misuse
 *   (null argument, bad n, B or K out of range, an index >= B, a polynomial
 *   with no claim).  tr is unchanged on any failure.
 * tpst_pst_verify_multi: tpst_pst_multi_reduce, tpst_pst_combine_challenge,
 *   tpst_pst_verify_combined.  TPST_OK or TPST_E_VERIFY; TPST_E_ARG also for
 *   sizes that do not match n; TPST_E_STATE: no SRS loaded.  tr is changed only
 *   on TPST_OK.
 * tpst_poly_multi_sumcheck_stages: test entry.  The device reduction alone --
 *   the prover's own round loop -- with the caller's weights a (K Fr, zero
 *   allowed) and challenges rho (n Fr): sums = n x 2 Fr, s_i(0) and s_i(2) of
 *   every round; u as above.  Errors as tpst_poly_open_multi (no SRS needed). */
int tpst_poly_open_multi(tpst_ctx* ctx, tpst_poly* const* polys, const uint64_t* const* comms,
                         const uint64_t* const* Ts, size_t B, const uint32_t* claim_poly, const uint64_t* points,
                         const uint64_t* vals, size_t K, tpst_transcript* tr, uint64_t* rounds, uint64_t* u,
                         uint64_t* rho, uint64_t* comms_out, uint64_t* T_out, uint64_t* v_out, tpst_open_proof* proof);
int tpst_pst_multi_reduce(tpst_transcript* tr, int n, const uint64_t* const* Ts, size_t B, const uint32_t* claim_poly,
                          const uint64_t* points, const uint64_t* vals, size_t K, const uint64_t* rounds,
                          const uint64_t* u, uint64_t* rho);
int tpst_pst_verify_multi(tpst_ctx* ctx, tpst_transcript* tr, int n, const uint64_t* const* Ts, size_t B,
                          const uint32_t* claim_poly, const uint64_t* points, const uint64_t* vals, size_t K,
                          const uint64_t* rounds, const uint64_t* u, const tpst_open_proof* proof);
int tpst_poly_multi_sumcheck_stages(tpst_ctx* ctx, tpst_poly* const* polys, size_t B, const uint32_t* claim_poly,
                                    const uint64_t* points, const uint64_t* a, size_t K, const uint64_t* rho,
                                    uint64_t* sums, uint64_t* u);

/* Product sum-check: a relation between B committed polynomials of the same n
 * (1 <= B <= 256), each committed on its own as (comm_list_j, T_j), proved by
 * a sum-check over a sum of products of their tables and ONE combined opening.
 * M terms (1 <= M <= 64); term t is (deg_t in {1, 2, 3}, idx_t[0..deg_t) < B,
 * c_t in Fr).  An index may repeat inside a term (f f, f f f), every polynomial
 * occurs in at least one term, c_t = 0 is allowed.  With
 *   g(x) = sum_t c_t prod_{i < deg_t} f_{idx_t[i]}(x)
 * and an optional point tau in Fr^n the claim is
 *   e_0 = sum_{x in {0,1}^n} eq(tau, x) g(x)      (without tau: sum_x g(x)).
 * a o b = c is g = f_0 f_1 - f_2 with tau and e_0 = 0; sum a b = s is
 * g = f_0 f_1; sum a b c = s is g = f_0 f_1 f_2.  Points and tables are in
 * tpst_poly_eval's order, tau[0] the most significant bit of x.  The round
 * degree is D = max_t deg_t + (tau given ? 1 : 0); D > 3 is TPST_E_ARG and
 * D = 1 is run as D = 2 (UniPoly::from_evals takes 3 or 4 evaluations).  This
 * protocol is this library's own: the reference's sum-checks are private to
 * R1CSProof and the product tree.
 *
 * On the caller's transcript, prover and verifier alike:
 *  1. statement: tpst_transcript_append_fr of B, M, n and has_tau (0 or 1),
 *     each as the Fr of the integer; append_gt of T_0..T_{B-1}; per term in
 *     order append_fr of deg_t, of each of its deg_t indices and of c_t; the n
 *     coordinates of tau, if given; append_fr of e_0.
 *  2. rounds: n rounds, round i binds variable i (the most significant
 *     first).  The round polynomial s_i has degree <= D and
 *     s_i(0) + s_i(1) = e_i; its D + 1 coefficients (UniPoly::from_evals of
 *     s_i(0..D), constant first) are the proof's and are absorbed with
 *     append_fr; one challenge rho_i; e_{i+1} = s_i(rho_i).
 *  3. final values: the proof carries u_j = f_j(rho); the check is
 *     e_n = [prod_i (tau_i rho_i + (1 - tau_i)(1 - rho_i))]
 *           sum_t c_t prod_i u_{idx_t[i]}       (the bracket only with tau).
 *  4. tpst_pst_combine_challenge(tr, n, rho, Ts, u) gives the weights w of the
 *     combined opening of all B polynomials at rho with values u.
 * The proof: the n x (D + 1) round coefficients, the B values u_j, one
 * tpst_open_proof.  Its wire format, a sharded (multi-rank) form, degrees
 * above 3 and terms over polynomials of different n are not part of this
 * interface.
 *
 * SOUNDNESS: the sum-check bound (D n / r) plus the combination ((B - 1) / r).
 * IT HOLDS ONLY BECAUSE EVERY T_j, EVERY TERM, tau AND e_0 ARE ABSORBED BEFORE
 * rho_0 IS DRAWN, AND THE WEIGHTS OF STEP 4 AFTER EVERY u_j: a caller that
 * replays these steps itself must keep that order, and whatever fixed the
 * commitments must be on the transcript before the call.  A tau MEANT AS
 * ZERO-CHECK RANDOMNESS (a o b = c for every x, not just under one weighting)
 * MUST BE DRAWN BY THE CALLER AFTER THE COMMITMENTS ARE FIXED, e.g. squeezed
 * from the transcript once every T_j is on it: that is the caller's protocol,
 * not this call's, which takes tau as part of the statement.
 *
 * terms: M tpst_sc_term (idx entries past deg are ignored); tau: n Fr or NULL;
 * rounds is n x (D + 1) Fr, u B Fr, rho n Fr, e0 one Fr.
 *
 * tpst_poly_sumcheck_open: the prover.  e_0 is an OUTPUT: round 0 computes
 *   s_0(0) and s_0(1) on the device and their sum is the claim; the statement
 *   is absorbed once that is known.  Then steps 2-3 with the rounds on the
 *   device (the handles' tables are read, never written), step 4 and
 *   tpst_poly_open_combined at rho; writes e0, rounds, u, rho and what that
 *   call writes (comm_list*, T*, v*, the proof).  tr ends as
 *   tpst_poly_open_combined at rho leaves it, and is unchanged on any error.
 *   TPST_E_ARG: a null argument (tau may be NULL), B, M or a degree out of
 *   range, D > 3, an index >= B, a polynomial in no term, polynomials of
 *   different n or of another context, a coefficient or coordinate >= r.
 *   TPST_E_STATE: a handle that is not a whole polynomial, no SRS loaded.
 * tpst_pst_sumcheck_reduce: HOST ONLY, no context: the verifier's steps 1-3 on
 *   a claimed e_0.  On TPST_OK rho is written and tr stands where step 4
 *   starts.  TPST_E_VERIFY: a failed round check or final identity, or any
 *   scalar (coefficient, coordinate, e_0, round coefficient, u_j) >= r or T_j
 *   coefficient >= p.  TPST_E_ARG: misuse (null argument, bad n, B, M or a
 *   degree out of range, D > 3, an index >= B, a polynomial in no term).  tr is
 *   unchanged on any failure.
 * tpst_pst_verify_sumcheck: tpst_pst_sumcheck_reduce,
 *   tpst_pst_combine_challenge, tpst_pst_verify_combined.  TPST_OK or
 *   TPST_E_VERIFY; TPST_E_ARG also for sizes that do not match n;
 *   TPST_E_STATE: no SRS loaded.  tr is changed only on TPST_OK.
 * tpst_poly_sumcheck_stages: test entry.  The device rounds alone -- the
 *   prover's own loop -- on the caller's challenges rho (n Fr): sums =
 *   n x (D + 1) Fr, s_i(0..D) of every round (s_i(1) of a round after the
 *   first is e_i - s_i(0), as the prover takes it); u as above.  Errors as
 *   tpst_poly_sumcheck_open (no SRS needed). */
typedef struct tpst_sc_term {
  uint32_t deg;      /* 1..3 */
  uint32_t idx[3];   /* polynomial indices, the first deg are used */
  uint64_t coeff[4]; /* c_t, canonical Fr */
} tpst_sc_term;
int tpst_poly_sumcheck_open(tpst_ctx* ctx, tpst_poly* const* polys, const uint64_t* const* comms,
                            const uint64_t* const* Ts, size_t B, const tpst_sc_term* terms, size_t M,
                            const uint64_t* tau, tpst_transcript* tr, uint64_t* e0, uint64_t* rounds, uint64_t* u,
                            uint64_t* rho, uint64_t* comms_out, uint64_t* T_out, uint64_t* v_out,
                            tpst_open_proof* proof);
int tpst_pst_sumcheck_reduce(tpst_transcript* tr, int n, const uint64_t* const* Ts, size_t B, const tpst_sc_term* terms,
                             size_t M, const uint64_t* tau, const uint64_t* e0, const uint64_t* rounds,
                             const uint64_t* u, uint64_t* rho);
int tpst_pst_verify_sumcheck(tpst_ctx* ctx, tpst_transcript* tr, int n, const uint64_t* const* Ts, size_t B,
                             const tpst_sc_term* terms, size_t M, const uint64_t* tau, const uint64_t* e0,
                             const uint64_t* rounds, const uint64_t* u, const tpst_open_proof* proof);
int tpst_poly_sumcheck_stages(tpst_ctx* ctx, tpst_poly* const* polys, size_t B, const tpst_sc_term* terms, size_t M,
                              const uint64_t* tau, const uint64_t* rho, uint64_t* sums, uint64_t* u);

/* Lookup argument (LogUp): L witness polynomials a_0..a_{L-1} (1 <= L <= 8)
 * and one table polynomial t, all whole polynomials of one n in one context,
 * each committed on its own as (comm_list, T).  The claim: for every l and
 * every x in {0,1}^n there is a y with a_l(x) = t(y).  The table may hold
 * repeated values.  A range check is t(y) = y; an opcode or fixed-table lookup
 * and set membership are the same call.  This protocol is this library's own:
 * the reference has no counterpart.  It is closed by ONE opening.
 *
 * Helper polynomials, built on the device by the prover:
 *   m(y)   = #{(l, x) : a_l(x) = t(y)}, credited to the FIRST y (lowest index)
 *            that holds the value and 0 at its repeats: a function of (a, t)
 *            alone, bit-identical across runs, grids and index capacities;
 *   h_l(x) = 1 / (beta + a_l(x)),   h_t(y) = m(y) / (beta + t(y)).
 * The polynomial order used below is a_0..a_{L-1}, t, m, h_0..h_{L-1}, h_t;
 * B = 2L + 3.
 *
 * On the caller's transcript, prover and verifier alike:
 *  1. tpst_transcript_append_fr of L and n (the Fr of each integer); append_gt
 *     of T_{a_0}..T_{a_{L-1}}, T_t.
 *  2. append_gt of T_m; one challenge beta.
 *  3. append_gt of T_{h_0}..T_{h_{L-1}}, T_{h_t}; n challenges tau_0..tau_{n-1};
 *     one challenge lambda.
 *  4. the product sum-check (above), exactly its steps 1-3, on the B
 *     polynomials with tau (has_tau = 1, D = 3) and the M = 2L + 3 terms
 *       per l < L: (lambda^l, [h_l, a_l]), (lambda^l beta, [h_l]);
 *       then (lambda^L, [h_t, t]), (lambda^L beta, [h_t]), (-lambda^L, [m]).
 *     Its claim is e_0 = sum_{l < L} lambda^l: THE VERIFIER COMPUTES IT, it is
 *     not taken from the proof.  (Under eq(tau, .) every h_l (beta + a_l) is
 *     1 and h_t (beta + t) - m is 0.)  It ends in rho and u_j = f_j(rho).
 *  5. s_l = h_l(1/2, .., 1/2) and s_t = h_t(1/2, .., 1/2), 1/2 = (r + 1) / 2;
 *     the check is sum_l s_l = s_t.  For a multilinear h,
 *     sum_x h(x) = 2^n h(1/2, .., 1/2): this is the LogUp identity
 *     sum_l sum_x 1 / (beta + a_l(x)) = sum_y m(y) / (beta + t(y)) without a
 *     second sum-check.
 *  6. the multi-point opening (above), exactly its steps 1-4, on all B
 *     polynomials with the K = 3L + 4 claims f_j(rho) = u_j for j = 0..B-1,
 *     then h_l(1/2, .., 1/2) = s_l for l < L, then h_t(1/2, .., 1/2) = s_t.
 *     It ends in one combined opening at its own point rho'.
 * The proof: T_m and T_{h_0}..T_{h_t} (T_helpers, (L + 2) x 72); the n x 4
 * round coefficients (sc_rounds) and the 2L + 3 values u; the L + 1 values s
 * (s_0..s_{L-1}, s_t); the multi-point reduction's n x 3 coefficients
 * (mp_rounds) and its 2L + 3 final values (mp_u); one tpst_open_proof.  comms
 * and Ts are the L + 1 commitments of a_0..a_{L-1}, t in that order.  NOT PART
 * OF THIS INTERFACE: the proof's wire format, a sharded (multi-rank) form,
 * tables of another n than the witnesses, vector (multi-column) lookups, and
 * merging with a caller's own sum-check.
 *
 * SOUNDNESS: (L + 1) 2^n / r for the identity in beta (it needs L 2^n < r,
 * which always holds), (n + L) / r for tau and lambda, plus the bounds of the
 * product sum-check and of the multi-point opening.  IT HOLDS ONLY BECAUSE
 * beta IS DRAWN AFTER T_m IS ABSORBED, tau AND lambda ARE DRAWN AFTER EVERY T_h
 * IS ABSORBED, AND WHATEVER FIXED T_a AND T_t IS ON THE TRANSCRIPT BEFORE THE
 * CALL: a caller that replays these steps itself must keep that order.  With a
 * beta the prover knows before it commits to m, a false m can be made to
 * satisfy the identity.
 *
 * tpst_poly_lookup_open: the prover.  Builds m (an index of the table, one
 *   probe per witness entry), commits it, draws beta, builds every h (a
 *   batched inversion) and commits it, draws tau and lambda, runs the product
 *   sum-check's rounds on the device and tpst_poly_open_multi on the claims of
 *   step 6; writes every proof part, rho' (rho, n Fr) and what the combined
 *   opening writes (comm_list*, T*, v*, the proof).  The handles' tables are
 *   read, never written; the helper handles are freed before return.  tr ends
 *   as tpst_poly_open_multi leaves it and is unchanged on any error.
 *   THE PROVER DOES CHECK MEMBERSHIP (m does not exist otherwise): a witness
 *   entry that is not in the table is TPST_E_ARG, and tpst_last_error names the
 *   least (l, x).  beta + value = 0 (probability <= (L + 1) 2^n / r) is
 *   TPST_E_ARG too.  TPST_E_ARG also: a null argument, L out of range,
 *   polynomials of different n or of another context, n + 3 > 32 or
 *   L 2^n >= 2^32 (the counts are u32), a T with a coefficient >= p.
 *   TPST_E_STATE: a handle that is not a whole polynomial, no SRS loaded.
 * tpst_pst_lookup_reduce: HOST ONLY, no context: the verifier's steps 1-5 and
 *   the multi-point reduction (steps 1-3 of step 6), composed from
 *   tpst_pst_sumcheck_reduce and tpst_pst_multi_reduce.  On TPST_OK rho' is
 *   written and tr stands where the combined opening's challenge
 *   (tpst_pst_combine_challenge on rho', all B T and mp_u) starts.
 *   TPST_E_VERIFY: any failed check, any scalar >= r, any T with a coefficient
 *   >= p.  TPST_E_ARG: misuse (null argument, bad n, n + 3 > 32, L out of
 *   range).  tr is unchanged on any failure.
 * tpst_pst_verify_lookup: tpst_pst_lookup_reduce, tpst_pst_combine_challenge,
 *   tpst_pst_verify_combined.  TPST_OK or TPST_E_VERIFY; TPST_E_ARG also for
 *   sizes that do not match n; TPST_E_STATE: no SRS loaded.  tr is changed only
 *   on TPST_OK.
 * tpst_poly_lookup_stages: test entry.  The device stages alone on the
 *   caller's beta (no SRS needed): m (2^n Fr), h = h_0..h_{L-1}, h_t
 *   ((L + 1) x 2^n Fr) and s = s_0..s_{L-1}, s_t (L + 1 Fr), all canonical.
 *   Errors as tpst_poly_lookup_open; beta >= r is TPST_E_ARG.
 * Test hooks (environment): TPST_LOOKUP_GRID=g caps the workgroups of the
 * lookup kernels; TPST_LOOKUP_SLOTS_LOG2=k sets the index capacity to 2^k
 * slots (default n + 1, twice the table; k = n is load factor 1; k < n or
 * k > 31 is TPST_E_ARG).  No output depends on either. */
int tpst_poly_lookup_open(tpst_ctx* ctx, tpst_poly* const* wits, size_t L, tpst_poly* table,
                          const uint64_t* const* comms, const uint64_t* const* Ts, tpst_transcript* tr,
                          uint64_t* T_helpers, uint64_t* sc_rounds, uint64_t* u, uint64_t* s, uint64_t* mp_rounds,
                          uint64_t* mp_u, uint64_t* rho, uint64_t* comms_out, uint64_t* T_out, uint64_t* v_out,
                          tpst_open_proof* proof);
int tpst_pst_lookup_reduce(tpst_transcript* tr, int n, size_t L, const uint64_t* const* Ts, const uint64_t* T_helpers,
                           const uint64_t* sc_rounds, const uint64_t* u, const uint64_t* s, const uint64_t* mp_rounds,
                           const uint64_t* mp_u, uint64_t* rho);
int tpst_pst_verify_lookup(tpst_ctx* ctx, tpst_transcript* tr, int n, size_t L, const uint64_t* const* Ts,
                           const uint64_t* T_helpers, const uint64_t* sc_rounds, const uint64_t* u, const uint64_t* s,
                           const uint64_t* mp_rounds, const uint64_t* mp_u, const tpst_open_proof* proof);
int tpst_poly_lookup_stages(tpst_ctx* ctx, tpst_poly* const* wits, size_t L, tpst_poly* table, const uint64_t* beta,
                            uint64_t* m, uint64_t* h, uint64_t* s);

/* ---- MultilinearPC single calls (ark-poly-commit fork) --
 * Against the loaded SRS; a polynomial of nv <= ck.nv variables uses level
 * ck.nv - nv.  evals: 2^nv canonical Fr (to_evaluations order); point: nv Fr,
 * LSB-first (as MultilinearPC takes it, cf. a_rev at sqrt_pst.rs:218-225).
 * commit  (sqrt_pst.rs:124)  -> g_product (G1)
 * commit_g2 (mipp.rs:133)     -> h_product (G2)
 * open    (sqrt_pst.rs:225)   -> nv G2 proofs;  open_g1 (mipp.rs:144) -> nv G1
 * check   (sqrt_pst.rs:261)   -> TPST_OK / TPST_E_VERIFY
 * check_2 (mipp.rs:307)       -> TPST_OK / TPST_E_VERIFY
 * The checks reject non-canonical, off-curve or non-subgroup inputs. */
int tpst_mlpc_commit(tpst_ctx* ctx, const uint64_t* evals, int nv, uint64_t* g_product);
int tpst_mlpc_commit_g2(tpst_ctx* ctx, const uint64_t* evals, int nv, uint64_t* h_product);
int tpst_mlpc_open(tpst_ctx* ctx, const uint64_t* evals, int nv, const uint64_t* point, uint64_t* proofs);
int tpst_mlpc_open_g1(tpst_ctx* ctx, const uint64_t* evals, int nv, const uint64_t* point, uint64_t* proofs);
int tpst_mlpc_check(tpst_ctx* ctx, int nv, const uint64_t* comm, const uint64_t* point, const uint64_t* value,
                    const uint64_t* proofs);
int tpst_mlpc_check_2(tpst_ctx* ctx, int nv, const uint64_t* comm_h, const uint64_t* point, const uint64_t* value,
                      const uint64_t* proofs);

/* Transcript calls of the R1CS prover (poseidon_transcript.rs:55-60, 83-85):
 * append_scalar -- an Fr absorbed as one Fq element of the same value;
 * new_from_state2 -- a fresh sponge that absorbs the 32-byte uncompressed Fr. */
int tpst_transcript_append_fr(tpst_transcript* t, const uint64_t* fr);
int tpst_transcript_reset_fr(tpst_transcript* t, const uint64_t* fr);
/* append_bytes (poseidon_transcript.rs:67-69): absorb a byte vector (u64
 * length prefix, 47-byte chunks); `append` of any value = this over its
 * Compress::No serialisation (poseidon_transcript.rs:22-28). */
int tpst_transcript_append_bytes(tpst_transcript* t, const uint8_t* bytes, size_t n);

/* ---- Spartan R1CS sum-checks (csrc/r1cs.hip) ------
 * R1CSInstance (r1csinstance.rs): num_cons x (2 num_vars) sparse A, B, C;
 * z = vars || 1 || inputs || 0.  Matrices as (row u32, col u32, canonical Fr)
 * triples, any order; kept on the device as CSR (multiply_vec) + CSC
 * (compute_eval_table_sparse).  num_cons and num_vars are powers of two >= 2;
 * the provers over the witness (tpst_r1cs_prove, tpst_groth16_setup) and
 * tpst_r1cs_synthetic need num_vars >= 4. */
typedef struct tpst_r1cs tpst_r1cs;
int tpst_r1cs_load(tpst_ctx* ctx, size_t num_cons, size_t num_vars, size_t num_inputs, const size_t* nnz /*[3]*/,
                   const uint32_t* const* rows /*[3]*/, const uint32_t* const* cols /*[3]*/,
                   const uint64_t* const* vals /*[3]*/, tpst_r1cs** out);
/* produce_synthetic_r1cs (r1csinstance.rs:166-242) over the SplitMix64 Fr
 * stream of `seed` (the reference draws thread_rng): also returns the
 * satisfying vars (num_vars Fr) and inputs (num_inputs Fr) */
int tpst_r1cs_synthetic(tpst_ctx* ctx, size_t num_cons, size_t num_vars, size_t num_inputs, uint64_t seed,
                        tpst_r1cs** out, uint64_t* vars, uint64_t* inputs);
void tpst_r1cs_free(tpst_r1cs* r);
/* UniPoly::from_evals (unipoly.rs:15-45): n = 3 or 4 canonical evaluations at
 * 0..n-1 -> n coefficients, constant first (host; the sum-check round encoding). */
int tpst_unipoly_from_evals(const uint64_t* evals, int n, uint64_t* coeffs);
/* EqPolynomial::evals (dense_mlpoly.rs:231-250): the MSB-first chi table of
 * r[0..ell) (ell <= 30), computed on the device; out = 2^ell canonical Fr. */
int tpst_eq_evals(tpst_ctx* ctx, const uint64_t* r, int ell, uint64_t* out);

/* R1CSInstance::commit (r1csinstance.rs:313-344) = SparseMatPolynomial::
 * multi_commit over (A, B, C) (sparse_mlpoly.rs:490-517): the SPARK dense
 * representation (addresses, memory-checking read / audit timestamps, values)
 * built on the device, comb_ops and comb_mem each committed with
 * DensePolynomial::commit (Hyrax rows, zero blinds) over the generators of
 * PolyCommitmentGens::setup(num_vars, label).  ops_rows / mem_rows receive the
 * row counts (the G1 points of each PolyCommitment); with comm_ops or
 * comm_mem NULL only the sizes are reported. */
int tpst_r1cs_commit(tpst_ctx* ctx, tpst_r1cs* r1cs, const uint8_t* label, size_t label_len, uint64_t* comm_ops,
                     size_t* ops_rows, uint64_t* comm_mem, size_t* mem_rows);

#define TPST_R1CS_MAX_ROUNDS 48
/* R1CSProof (r1csproof.rs:24-38) without the Groth16 part; canonical Fr.
 * sc1: cubic round polynomials (4 coefficients, constant first), sc2: quad
 * (3); claims_phase2 = (Az, Bz, Cz, Az Bz)(rx); claims_phase2_z_abc = the
 * phase-two finals (z(ry), ABC(ry)); open = (comm U, proof_eval_vars_at_ry,
 * mipp_proof) of the witness polynomial at ry[1..]. */
typedef struct {
  int32_t rounds_x, rounds_y, num_vars_log, pad;
  uint64_t T[72];
  uint64_t initial_state[4];
  uint64_t sc1[TPST_R1CS_MAX_ROUNDS][4][4];
  uint64_t claims_phase2[4][4];
  uint64_t claims_phase2_z_abc[2][4];
  uint64_t r_abc[3][4];
  uint64_t sc2[TPST_R1CS_MAX_ROUNDS][3][4];
  uint64_t rx[TPST_R1CS_MAX_ROUNDS][4];
  uint64_t ry[TPST_R1CS_MAX_ROUNDS][4];
  uint64_t transcript_sat_state[4];
  uint64_t eval_vars_at_ry[4];
  tpst_open_proof open;
} tpst_r1cs_proof;
/* R1CSProof::prove (r1csproof.rs:237-370) minus prove_verifier: needs the SRS
 * loaded for ceil(log2(num_vars) / 2) variables; `tr` is updated in place. */
int tpst_r1cs_prove(tpst_ctx* ctx, tpst_r1cs* r1cs, const uint64_t* vars, const uint64_t* inputs,
                    tpst_transcript* tr, tpst_r1cs_proof* out);

/* R1CSInstance::evaluate (r1csinstance.rs:308-311, SparseMatPolynomial::
 * multi_evaluate): evals = (A, B, C)(rx, ry), 3 x 4 u64 canonical.  rx has
 * log2(num_cons) entries, ry log2(2 num_vars), both MSB-first as tpst_eq_evals
 * takes them.  Both eq tables and the gather-multiply-reduce over the resident
 * CSR run on the device (no atomics: the value does not depend on the launch).
 * TPST_E_ARG: a coordinate >= r, or an instance of another context. */
int tpst_r1cs_evaluate(tpst_ctx* ctx, tpst_r1cs* r1cs, const uint64_t* rx, const uint64_t* ry, uint64_t* evals);
/* R1CSInstance::is_sat (r1csinstance.rs:244-274): TPST_OK if Az * Bz = Cz in
 * every row for z = vars || 1 || inputs || 0, TPST_E_VERIFY if not;
 * TPST_E_ARG for a value >= r. */
int tpst_r1cs_is_sat(tpst_ctx* ctx, tpst_r1cs* r1cs, const uint64_t* vars, const uint64_t* inputs);
/* R1CSVerifierProof::verify as intended (r1csproof.rs:443-486) with the checks
 * of R1CSVerificationCircuit::generate_constraints (constraints.rs:263-397)
 * run natively on the host -- the transcript replay of tpst_r1cs_prove, both
 * SumcheckInstanceProof::verify (sumcheck.rs:29-66), the derived rx / ry
 * against the proof's (:317-319, :362-364), the two final claims (:328-340,
 * :376-388 with z(ry) from eval_vars_at_ry and the sparse (1, inputs)
 * polynomial of r1csproof.rs:390-398), the transcript state after the
 * sum-checks -- then Polynomial::verify of the witness opening at ry[1..]
 * (r1csproof.rs:469-480, tpst_pst_verify).  evals = (A, B, C)(rx, ry) is the
 * caller's (SNARK mode, tests); `tr` is updated in place.  The fields r_abc
 * and claims_phase2_z_abc are not read (the reference's verifier never sees
 * them).
 * TPST_OK: the proof verifies.  TPST_E_VERIFY: any failed check, a
 * non-canonical Fr in the proof, the inputs or evals, or rounds_x / rounds_y /
 * num_vars_log / the opening's m_col, m_row not matching the dimensions.
 * TPST_E_ARG: null arguments, dimensions that are not powers of two or beyond
 * TPST_R1CS_MAX_ROUNDS.  TPST_E_STATE: the SRS is not loaded for
 * ceil(log2(num_vars) / 2) variables (as for tpst_r1cs_prove). */
int tpst_r1cs_verify_evals(tpst_ctx* ctx, size_t num_cons, size_t num_vars, const uint64_t* inputs,
                           size_t num_inputs, const uint64_t* evals, tpst_transcript* tr,
                           const tpst_r1cs_proof* proof);
/* TestudoNizk::verify (testudo_nizk.rs:136-157) minus the digest append:
 * tpst_r1cs_evaluate at the proof's (rx, ry), then tpst_r1cs_verify_evals.
 * Also TPST_E_ARG for an instance of another context. */
int tpst_r1cs_verify(tpst_ctx* ctx, tpst_r1cs* r1cs, const uint64_t* inputs, tpst_transcript* tr,
                     const tpst_r1cs_proof* proof);

/* ---- Hyrax evaluation proofs (csrc/hyrax.hip) -------------------------------
 * PolyEvalProof (dense_mlpoly.rs:473-575) over DotProductProofLog
 * (nizk/mod.rs:32-180) and BulletReductionProof (nizk/bullet.rs): the opening
 * of the Hyrax commitments of tpst_pedersen_commit_rows / tpst_r1cs_commit.
 *
 * These proofs run over PoseidonTranscript<Fr> (poseidon_transcript.rs), the
 * sponge of MultiCommitGens::new -- not the Fq sponge of tpst_transcript.
 * state = capacity || rate (3 canonical Fr).  Host only, no context;
 * TPST_E_ARG for a null pointer, a value >= r or a non-canonical point. */
typedef struct {
  uint64_t state[3][4];
  uint32_t squeezing; /* 0 = absorbing, 1 = squeezing */
  uint32_t index;     /* next absorb / squeeze position in the rate */
} tpst_transcript_fr;
void tpst_transcript_fr_init(tpst_transcript_fr* t);
/* append_scalar (poseidon_transcript.rs:73-75): one native absorb */
int tpst_transcript_fr_append_scalar(tpst_transcript_fr* t, const uint64_t* fr);
/* append_scalar_vector (:88-96): n absorbs of one element each */
int tpst_transcript_fr_append_scalars(tpst_transcript_fr* t, const uint64_t* fr, size_t n);
/* append_point (:77-86): the 48 Compress::Yes bytes absorbed as a Vec<u8> */
int tpst_transcript_fr_append_point(tpst_transcript_fr* t, const uint64_t* g1);
/* append_bytes (:69-71): u64 length prefix, then 31-byte chunks */
int tpst_transcript_fr_append_bytes(tpst_transcript_fr* t, const uint8_t* bytes, size_t n);
/* challenge_scalar (:30-32): squeeze_field_elements(1) */
int tpst_transcript_fr_challenge(tpst_transcript_fr* t, uint64_t* out_fr);

/* Generators = PolyCommitmentGens::setup(num_vars, label) (dense_mlpoly.rs:
 * 185-187) = DotProductProofGens::new(R, label), R = 2^(ell - ell/2):
 * MultiCommitGens::new(R + 1, label) split at R -- `gens` a generator set over
 * G[0..R) with h (tpst_gens_new(R + 1) then tpst_gens_load of the first R),
 * Q = G[R] canonical affine (gens_1.G[0]).
 *
 * rnd: the reference's thread_rng draws, 3 + 4 log2(n) canonical Fr in draw
 * order: d, r_delta, r_beta, then 2 log2(n) pairs (blind_L, blind_R) -- the
 * reference draws twice the pairs it uses (nizk/mod.rs:65); round k consumes
 * pair k, the rest are only range-checked.
 *
 * Errors.  TPST_E_ARG: a null argument, a value >= r, gens->n not a power of
 * two <= 2^16 (or != R for the evaluation calls), a generator set of another
 * context.  TPST_E_STATE: a generator set without h.  Verifiers return
 * TPST_E_VERIFY for a failed equation, rounds != log2(n), a zero challenge, or
 * any proof or commitment element that is non-canonical, off the curve or
 * outside the subgroup (checked before the transcript absorbs anything).
 * `tr` is updated in place. */
#define TPST_HYRAX_MAX_ROUNDS 16
/* DotProductProofLog { BulletReductionProof { L_vec, R_vec }, delta, beta, z1, z2 } */
typedef struct {
  int32_t rounds, pad;
  uint64_t L[TPST_HYRAX_MAX_ROUNDS][12], R[TPST_HYRAX_MAX_ROUNDS][12];
  uint64_t delta[12], beta[12], z1[4], z2[4];
} tpst_dotprod_proof;
/* DotProductProofLog::prove (nizk/mod.rs:45-125): x, a = n = gens->n canonical
 * Fr (n = 1: zero rounds); returns Cx = commit(x, blind_x), Cy = y Q + blind_y h */
int tpst_dotprod_prove(tpst_ctx* ctx, const tpst_gens* gens, const uint64_t* Q, const uint64_t* x,
                       const uint64_t* blind_x, const uint64_t* a, const uint64_t* y, const uint64_t* blind_y,
                       const uint64_t* rnd, tpst_transcript_fr* tr, tpst_dotprod_proof* proof, uint64_t* Cx,
                       uint64_t* Cy);
/* DotProductProofLog::verify (nizk/mod.rs:127-179) */
int tpst_dotprod_verify(tpst_ctx* ctx, const tpst_gens* gens, const uint64_t* Q, const uint64_t* a,
                        const uint64_t* Cx, const uint64_t* Cy, tpst_transcript_fr* tr,
                        const tpst_dotprod_proof* proof);
/* PolyEvalProof::prove (dense_mlpoly.rs:482-534): Z = 2^ell canonical Fr
 * (1 <= ell <= 32), blinds = 2^(ell/2) Fr or NULL (zero), r = ell Fr
 * (MSB-first), blind_Zr may be NULL (zero); returns C_Zr'.  _dev: d_Z on the
 * context's device, ordered after the work queued on tpst_stream. */
int tpst_hyrax_eval_prove(tpst_ctx* ctx, const tpst_gens* gens, const uint64_t* Q, const uint64_t* Z, int ell,
                          const uint64_t* blinds, const uint64_t* r, const uint64_t* Zr, const uint64_t* blind_Zr,
                          const uint64_t* rnd, tpst_transcript_fr* tr, tpst_dotprod_proof* proof, uint64_t* C_Zr);
int tpst_hyrax_eval_prove_dev(tpst_ctx* ctx, const tpst_gens* gens, const uint64_t* Q, const void* d_Z, int ell,
                              const uint64_t* blinds, const uint64_t* r, const uint64_t* Zr,
                              const uint64_t* blind_Zr, const uint64_t* rnd, tpst_transcript_fr* tr,
                              tpst_dotprod_proof* proof, uint64_t* C_Zr);
/* PolyEvalProof::verify (dense_mlpoly.rs:536-560): comm = the 2^(ell/2) row
 * commitments; verify_plain (:562-574): C_Zr = Zr Q */
int tpst_hyrax_eval_verify(tpst_ctx* ctx, const tpst_gens* gens, const uint64_t* Q, int ell, const uint64_t* r,
                           const uint64_t* C_Zr, const uint64_t* comm, tpst_transcript_fr* tr,
                           const tpst_dotprod_proof* proof);
int tpst_hyrax_eval_verify_plain(tpst_ctx* ctx, const tpst_gens* gens, const uint64_t* Q, int ell, const uint64_t* r,
                                 const uint64_t* Zr, const uint64_t* comm, tpst_transcript_fr* tr,
                                 const tpst_dotprod_proof* proof);
/* DensePolynomial::evaluate (dense_mlpoly.rs:408-414) on the device */
int tpst_dense_evaluate(tpst_ctx* ctx, const uint64_t* Z, int ell, const uint64_t* r, uint64_t* out_fr);

/* ---- SPARK grand products (csrc/product_tree.hip) ---------------------------
 * ProductCircuitEvalProofBatched::{prove, verify} (product_tree.rs:255-476)
 * over SumcheckInstanceProof::prove_cubic_batched (sumcheck.rs:220-385) and
 * PoseidonTranscript<Fr>: the memory-checking argument ProductLayerProof::prove
 * (sparse_mlpoly.rs:1053-1236) runs twice per R1CSEvalProof.
 *
 * P product circuits over 2^ell entries each (ProductCircuit::new, 1 <= ell <=
 * 30, P >= 1) and D dot-product circuits (DotProductCircuit, already split:
 * D is 0 or even, circuits 2k and 2k + 1 the halves of one unsplit triple) of
 * 2^(ell - 1) entries each; P + D <= TPST_PRODCIRCUIT_MAX_INSTANCES.
 *
 * The proof is one caller-owned flat buffer of tpst_prodcircuit_proof_len(ell,
 * P, D) canonical Fr (4 u64 each), in this order:
 *   1. the layer proofs in the reference's push order (from the top layer
 *      down): layer proof i, i = 0 .. ell - 1, has i rounds of 4 coefficients,
 *      constant first -- ell (ell - 1) / 2 round polynomials in all;
 *   2. ell x P claims_prod_left (layer proof i, then instance), then ell x P
 *      claims_prod_right;
 *   3. the 3 x D final dot-product claims: D left, D right, D weight.
 * `tr` is updated in place. */
#define TPST_PRODCIRCUIT_MAX_INSTANCES 4096
/* Fr count of the flat proof = 2 ell (ell - 1) + 2 ell P + 3 D; 0 for
 * dimensions the calls below reject */
size_t tpst_prodcircuit_proof_len(int ell, size_t P, size_t D);
/* prove: polys = P x 2^ell canonical Fr, dotp_left / dotp_right / dotp_weight =
 * D x 2^(ell - 1) each (NULL with claims_dotp when D == 0).  Returns
 * claims_prod = every circuit's ProductCircuit::evaluate (P Fr), claims_dotp =
 * every DotProductCircuit::evaluate (D Fr) and rand (ell Fr).  The inputs are
 * not modified: the layers are built in a library-owned device arena.
 * _dev: the four inputs are device buffers on the context's device, ordered
 * after the work queued on tpst_stream; their values must be canonical (not
 * checked, as for tpst_hyrax_eval_prove_dev).
 * TPST_E_ARG: a null argument, a value >= r, ell or P out of range, odd D, a
 * transcript state no sponge can be in.  TPST_E_HIP: a HIP runtime failure
 * (the arena needs about 32 (2 P + 1.5 D + 1) 2^ell bytes). */
int tpst_prodcircuit_prove(tpst_ctx* ctx, int ell, size_t P, const uint64_t* polys, size_t D,
                           const uint64_t* dotp_left, const uint64_t* dotp_right, const uint64_t* dotp_weight,
                           tpst_transcript_fr* tr, uint64_t* proof, uint64_t* claims_prod, uint64_t* claims_dotp,
                           uint64_t* rand);
int tpst_prodcircuit_prove_dev(tpst_ctx* ctx, int ell, size_t P, const void* d_polys, size_t D,
                               const void* d_dotp_left, const void* d_dotp_right, const void* d_dotp_weight,
                               tpst_transcript_fr* tr, uint64_t* proof, uint64_t* claims_prod, uint64_t* claims_dotp,
                               uint64_t* rand);
/* verify (product_tree.rs:379-476 with SumcheckInstanceProof::verify,
 * sumcheck.rs:29-63): host only, no context.  Returns claims_out = the P
 * product claims at rand, claims_dotp_out = 3 D / 2 Fr, (left, right, weight)
 * of every unsplit dot-product triple at rand, and rand (ell Fr); the caller
 * checks those against its polynomials.
 * TPST_OK: every round and layer check holds.  TPST_E_VERIFY: a failed round
 * check (G(0) + G(1) = e), a failed layer equation, or a non-canonical Fr in
 * the proof or the claims (checked before the transcript absorbs anything; on
 * any failure `tr` and the outputs are left untouched).  TPST_E_ARG: a null
 * argument or dimensions as above. */
int tpst_prodcircuit_verify(int ell, size_t P, size_t D, const uint64_t* claims_prod, const uint64_t* claims_dotp,
                            const uint64_t* proof, tpst_transcript_fr* tr, uint64_t* claims_out,
                            uint64_t* claims_dotp_out, uint64_t* rand);

/* ---- SPARK evaluation proofs (csrc/sparse_eval.hip) --------------------------
 * R1CSEvalProof = SparseMatPolyEvalProof::{prove, verify} (r1csinstance.rs:
 * 336-386, sparse_mlpoly.rs:1441-1569): the opening of the computational
 * commitment of tpst_r1cs_commit at (rx, ry), over PoseidonTranscript<Fr>.
 * Unblinded, as the reference (it passes None); batch size 3 = (A, B, C).
 *
 * Dimensions.  N = num_nz_entries.next_power_of_two() ops per matrix (>= 2),
 * cells = max(num_cons, 2 num_vars) memory cells; comb_ops has ell_ops = log2 N
 * + 4 variables, comb_mem ell_mem = log2 cells + 1, comb_derefs ell_derefs =
 * log2 N + 3; a polynomial of ell variables is committed as 2^(ell / 2) rows.
 * rx has log2(num_cons) entries, ry log2(2 num_vars), MSB-first. */
/* R1CSCommitmentGens::setup (r1csinstance.rs:33-52, sparse_mlpoly.rs:296-323):
 * the three Hyrax generator sets (ops, mem, derefs), each tpst_gens_new(R + 1,
 * label) loaded over its first R points with h, Q = G[R]; built once here.
 * TPST_E_ARG: dimensions that are not powers of two, num_inputs >= num_vars,
 * fewer than 2 entries. */
typedef struct tpst_r1cs_gens tpst_r1cs_gens;
int tpst_r1cs_gens_setup(tpst_ctx* ctx, const uint8_t* label, size_t label_len, size_t num_cons, size_t num_vars,
                         size_t num_inputs, size_t num_nz_entries, tpst_r1cs_gens** out);
void tpst_r1cs_gens_free(tpst_r1cs_gens* gens);
/* R1CSDecommitment (MultiSparseMatPolynomialAsDense) on the device: comb_ops
 * (16 N canonical Fr: row.ops_addr | row.read_ts | col.ops_addr | col.read_ts |
 * val | 0), comb_mem (row.audit_ts | col.audit_ts) and the addresses and
 * timestamps as u32. */
typedef struct tpst_r1cs_decomm tpst_r1cs_decomm;
/* R1CSInstance::commit (r1csinstance.rs:313-333) over `gens`, keeping the
 * decommitment: comm_ops / comm_mem as tpst_r1cs_commit returns them for the
 * same label; with comm_ops or comm_mem NULL only the row counts are reported.
 * TPST_E_ARG: an instance or generators of another context, generators of
 * another shape. */
int tpst_r1cs_commit_decomm(tpst_ctx* ctx, tpst_r1cs* r1cs, const tpst_r1cs_gens* gens, uint64_t* comm_ops,
                            size_t* ops_rows, uint64_t* comm_mem, size_t* mem_rows, tpst_r1cs_decomm** out);
void tpst_r1cs_decomm_free(tpst_r1cs_decomm* decomm);

/* The fixed-size part of the proof, canonical Fr.  The variable parts are
 * caller-owned buffers: comm_derefs (derefs_rows G1 points) and the two flat
 * product-circuit proofs, laid out as tpst_prodcircuit_proof_len defines them:
 * prod_ops for (log2 N, 12, 6), prod_mem for (log2 cells, 4, 0). */
typedef struct {
  /* ProductLayerProof: eval_row / eval_col = init, read A B C, write A B C,
   * audit; eval_val = the split dot-product claims, [0] left, [1] right */
  uint64_t prod_row[8][4], prod_col[8][4], prod_val[2][3][4];
  /* HashLayerProof: eval_row / eval_col = ops_addr A B C, read_ts A B C,
   * audit_ts; eval_val; eval_derefs = [0] row_ops_val, [1] col_ops_val */
  uint64_t hash_row[7][4], hash_col[7][4], hash_val[3][4], hash_derefs[2][3][4];
  /* DerefsEvalProof.proof_derefs, HashLayerProof.proof_ops / proof_mem */
  tpst_dotprod_proof proof_derefs, proof_ops, proof_mem;
} tpst_r1cs_eval_proof;
typedef struct {
  size_t num_ops, num_mem_cells;            /* N, cells */
  int32_t ell_ops, ell_mem, ell_derefs;     /* variables of the three committed polynomials */
  int32_t log_ops, log_cells;               /* ell of the two batched product proofs */
  size_t ops_rows, mem_rows, derefs_rows;   /* G1 points of comm_ops / comm_mem / comm_derefs */
  size_t prod_ops_len, prod_mem_len;        /* Fr of the two flat product proofs */
  size_t rnd_len[3];                        /* Fr of the draws, in proving order: derefs, ops, mem */
} tpst_r1cs_eval_sizes;
/* host only, no context; TPST_E_ARG for dimensions tpst_r1cs_gens_setup rejects */
int tpst_r1cs_eval_proof_sizes(size_t num_cons, size_t num_vars, size_t num_nz_entries, tpst_r1cs_eval_sizes* out);
/* SparseMatPolyEvalProof::prove (sparse_mlpoly.rs:1473-1532): evals = 3 Fr =
 * (A, B, C)(rx, ry); rnd_derefs / rnd_ops / rnd_mem = the reference's
 * thread_rng draws of the three openings in proving order, each 3 + 4 log2(R_k)
 * Fr as tpst_hyrax_eval_prove documents.  `tr` is updated in place, and only on
 * success.  The eq tables, the dereference, the hash layer, both batched
 * product proofs, the 23 evaluations and the three openings run on the device.
 * TPST_E_ARG: a null argument, a value >= r, a handle of another context,
 * generators of another shape, or one of the prover's assertions (the message
 * says which): init * writes != reads * audit over the rows or the columns,
 * left + right != evals[m]. */
int tpst_r1cs_eval_prove(tpst_ctx* ctx, const tpst_r1cs_decomm* decomm, const tpst_r1cs_gens* gens,
                         const uint64_t* rx, const uint64_t* ry, const uint64_t* evals, const uint64_t* rnd_derefs,
                         const uint64_t* rnd_ops, const uint64_t* rnd_mem, tpst_transcript_fr* tr,
                         tpst_r1cs_eval_proof* proof, uint64_t* comm_derefs, uint64_t* prod_ops, uint64_t* prod_mem);
/* SparseMatPolyEvalProof::verify (sparse_mlpoly.rs:1534-1568 with :1377-1438,
 * :1238-1334, :896-1040): needs no instance and no decommitment.  The
 * transcript, both tpst_prodcircuit_verify, the subset and claim checks and the
 * n-to-1 reductions are host work; the three tpst_hyrax_eval_verify_plain run
 * on the device.  `tr` is updated in place, and only on success.
 * TPST_E_VERIFY: any failed check of the reference's verifier, or any Fr (of
 * the proof, evals, rx, ry) or point (of the proof or the commitment) that is
 * non-canonical, off the curve or outside the subgroup, all checked before the
 * transcript absorbs anything.  TPST_E_ARG: a null argument, generators of
 * another context, num_ops / num_mem_cells that do not match the generators. */
int tpst_r1cs_eval_verify(tpst_ctx* ctx, const uint64_t* comm_ops, const uint64_t* comm_mem, size_t num_ops,
                          size_t num_mem_cells, const tpst_r1cs_gens* gens, const uint64_t* rx, const uint64_t* ry,
                          const uint64_t* evals, tpst_transcript_fr* tr, const tpst_r1cs_eval_proof* proof,
                          const uint64_t* comm_derefs, const uint64_t* prod_ops, const uint64_t* prod_mem);
/* The prover's stages alone (tests, tools); any output may be NULL.  derefs:
 * comb_derefs, 8 N Fr; r_mem_check = (r_hash, gamma) -> hash_ops: 12 N Fr (row
 * read | row write | col read | col write, A B C each) and hash_mem: 4 cells
 * (row init | row audit | col init | col audit); seg: the 15 evaluations of
 * comb_ops' segments and the 6 of comb_derefs' at rand_ops (log2 N Fr), then
 * the 2 of comb_mem's halves at rand_mem (log2 cells Fr). */
int tpst_r1cs_eval_stages(tpst_ctx* ctx, const tpst_r1cs_decomm* decomm, const uint64_t* rx, const uint64_t* ry,
                          const uint64_t* r_mem_check, const uint64_t* rand_ops, const uint64_t* rand_mem,
                          uint64_t* derefs, uint64_t* hash_ops, uint64_t* hash_mem, uint64_t* seg);

/* ---- TestudoSnark / TestudoNizk (csrc/snark.hip) ----------------------------
 * The composition of the calls above into the two end-to-end proofs of
 * testudo_snark.rs:120-235 and testudo_nizk.rs:80-157, with the transcript
 * calls between the parts that bind them.  Host code: every device stage is
 * one of the entry points above, called without the context's lock held across
 * them.  There is no prove_verifier: the Groth16 wrap stays replaced by the
 * native checks of tpst_r1cs_verify_evals.
 *
 * Two sponges.  F = the caller's PoseidonTranscript<Fr> (`tr`), Q = a
 * PoseidonTranscript<Fq> owned by the call.  The reference (commented out
 * there) passes one PoseidonTranscript<ScalarField> to R1CSProof::prove, which
 * since takes a PoseidonTranscript<BaseField> (r1csproof.rs:242); the bridge
 * between the two is stated here.
 *   SNARK prove:
 *    1. tpst_r1cs_commitment_absorb(comm, F)        comm.write_to_transcript
 *    2. c = F.challenge_scalar()
 *    3. F.new_from_state(&c)                        tpst_transcript_fr_new_from_state
 *    4. Q = fresh + new_from_state2(&c)             tpst_transcript_init, tpst_transcript_reset_fr
 *                                                   (the Fr-into-Fq call of r1csproof.rs:262)
 *    5. vars padded with zeros to num_vars          lib.rs:99-113
 *    6. sat = tpst_r1cs_prove over Q -> rx, ry
 *    7. inst_evals = tpst_r1cs_evaluate(rx, ry)
 *    8. F absorbs append_scalar(sat.transcript_sat_state), append_scalar_vector(rx),
 *       append_scalar_vector(ry), append_scalar(Ar), (Br), (Cr)   (testudo_snark.rs:156-162; the
 *       reference binds by continuing on its one transcript)
 *    9. tpst_r1cs_eval_prove(decomm, rx, ry, inst_evals, gens, F, rnd)
 *   SNARK verify: 1-4 over the commitment; tpst_r1cs_verify_evals on Q with the
 *   commitment's dimensions, the caller's inputs and the proof's inst_evals; the
 *   absorbs of 8 from the proof's fields; tpst_r1cs_eval_verify at the proof's
 *   (rx, ry).  It needs no instance and no decommitment.
 *   NIZK prove: F.append_bytes(digest), 2-6, then the first three absorbs of 8,
 *   so that the caller's transcript is bound to the proof.  NIZK verify mirrors
 *   it and evaluates (A, B, C) itself (tpst_r1cs_verify).  The reference's NIZK
 *   verifier omits the squeeze of c that its prover does (testudo_nizk.rs:90,
 *   :144-147); this one mirrors the prover.
 * Every call works on a copy of `tr` and stores it back only on TPST_OK; prover
 * and verifier leave it in the same state.  Parity of the Fr transcript is
 * unpinned against arkworks, as for the calls above.
 *
 * Errors.  TPST_E_ARG: a null argument, a value >= r, n_vars > num_vars,
 * num_vars < 4, a handle of another context, an instance, commitment,
 * decommitment or generators whose dimensions differ, a commitment point that
 * is not canonical (provers), the assertions of tpst_r1cs_eval_prove.
 * TPST_E_STATE: no SRS loaded for ceil(log2(num_vars) / 2) variables.
 * TPST_E_VERIFY (verifiers): anything either verifier rejects -- a failed
 * check, a malformed element of the proof, the inputs or the commitment, a
 * number of inputs other than the commitment's. */

/* append_u64 (poseidon_transcript.rs:65-67): one native absorb of the field
 * element x (ark-crypto-primitives 0.4 `Absorb for u64`).  Host only. */
int tpst_transcript_fr_append_u64(tpst_transcript_fr* t, uint64_t x);
/* new_from_state (poseidon_transcript.rs:50-53): a fresh sponge that absorbs
 * the scalar.  Host only; TPST_E_ARG for a value >= r. */
int tpst_transcript_fr_new_from_state(tpst_transcript_fr* t, const uint64_t* fr);

/* R1CSCommitment (r1csinstance.rs:55-61) as the caller holds it: the
 * dimensions and the two row-commitment lists of tpst_r1cs_commit_decomm. */
typedef struct {
  size_t num_cons, num_vars, num_inputs, num_ops, num_mem_cells;
  const uint64_t* comm_ops; /* ops_rows canonical affine G1 */
  size_t ops_rows;
  const uint64_t* comm_mem; /* mem_rows canonical affine G1 */
  size_t mem_rows;
} tpst_r1cs_commitment;
/* R1CSCommitment::write_to_transcript (r1csinstance.rs:63-70, sparse_mlpoly.rs:
 * 335-341, dense_mlpoly.rs:464-470): append_u64 of num_cons, num_vars,
 * num_inputs, then of batch_size (3), num_ops, num_mem_cells, then append_point
 * of every row of comm_comb_ops, then of comm_comb_mem.  Host only (one
 * permutation or two per point).  TPST_E_ARG: a null pointer, row counts other
 * than the ones num_ops / num_mem_cells imply, a point that is not canonical;
 * `tr` is then untouched. */
int tpst_r1cs_commitment_absorb(const tpst_r1cs_commitment* comm, tpst_transcript_fr* tr);

/* The SNARK proof: (R1CSProof, inst_evals = (A, B, C)(rx, ry), R1CSEvalProof).
 * rx and ry live in `sat`.  The variable parts of the evaluation proof stay
 * caller-owned buffers, as for tpst_r1cs_eval_prove. */
typedef struct {
  tpst_r1cs_proof sat;
  uint64_t inst_evals[3][4];
  tpst_r1cs_eval_proof eval;
} tpst_snark_proof;
/* TestudoSnark::prove (testudo_snark.rs:120-196), steps 1-9 above.  vars =
 * n_vars <= num_vars witness values (may be NULL when n_vars is 0); rnd_derefs /
 * rnd_ops / rnd_mem and the three output buffers as tpst_r1cs_eval_prove takes
 * them. */
int tpst_snark_prove(tpst_ctx* ctx, tpst_r1cs* r1cs, const tpst_r1cs_commitment* comm,
                     const tpst_r1cs_decomm* decomm, const tpst_r1cs_gens* gens, const uint64_t* vars, size_t n_vars,
                     const uint64_t* inputs, const uint64_t* rnd_derefs, const uint64_t* rnd_ops,
                     const uint64_t* rnd_mem, tpst_transcript_fr* tr, tpst_snark_proof* proof, uint64_t* comm_derefs,
                     uint64_t* prod_ops, uint64_t* prod_mem);
/* TestudoSnark::verify (testudo_snark.rs:198-235): TPST_OK only if both the
 * satisfiability proof and the evaluation proof verify. */
int tpst_snark_verify(tpst_ctx* ctx, const tpst_r1cs_commitment* comm, const tpst_r1cs_gens* gens,
                      const uint64_t* inputs, size_t num_inputs, tpst_transcript_fr* tr,
                      const tpst_snark_proof* proof, const uint64_t* comm_derefs, const uint64_t* prod_ops,
                      const uint64_t* prod_mem);
/* TestudoNizk::prove / verify (testudo_nizk.rs:80-157): digest = the instance's
 * digest bytes (r1csinstance.rs:155-164), absorbed with append_bytes. */
int tpst_nizk_prove(tpst_ctx* ctx, tpst_r1cs* r1cs, const uint8_t* digest, size_t digest_len, const uint64_t* vars,
                    size_t n_vars, const uint64_t* inputs, tpst_transcript_fr* tr, tpst_r1cs_proof* proof);
int tpst_nizk_verify(tpst_ctx* ctx, tpst_r1cs* r1cs, const uint8_t* digest, size_t digest_len,
                     const uint64_t* inputs, tpst_transcript_fr* tr, const tpst_r1cs_proof* proof);

/* ---- Groth16 over BLS12-377 (csrc/groth16.hip) ----
 * The prover behind R1CSProof::prove_verifier (r1csproof.rs:374-434,
 * Groth16::<E>::prove at :421): ark-groth16 create_proof with the
 * LibsnarkReduction QAP, over any tpst_r1cs instance (variables in the
 * Spartan z order: witness z[0..num_vars), instance (1, inputs)).  The
 * reference's thread_rng draws are arguments here. */
typedef struct tpst_groth16_pk tpst_groth16_pk;
/* generate_random_parameters_with_reduction: toxic = (tau, alpha, beta,
 * gamma, delta) canonical Fr (5 x 4 u64, nonzero, tau outside the domain).
 * Keeps the proving key (query points) on the device. */
int tpst_groth16_setup(tpst_ctx* ctx, tpst_r1cs* r1cs, const uint64_t* toxic, tpst_groth16_pk** out);
void tpst_groth16_pk_free(tpst_groth16_pk* pk);
/* QAP domain size n = next_pow2(num_cons + num_inputs + 1) */
int tpst_groth16_domain(const tpst_groth16_pk* pk, size_t* n);
/* VerifyingKey: alpha_g1 (12 u64), beta_g2 / gamma_g2 / delta_g2 (24 u64
 * each), gamma_abc_g1 (num_inputs + 1 points), affine canonical */
int tpst_groth16_vk(tpst_ctx* ctx, const tpst_groth16_pk* pk, uint64_t* alpha_g1, uint64_t* beta_g2,
                    uint64_t* gamma_g2, uint64_t* delta_g2, uint64_t* gamma_abc_g1);
/* LibsnarkReduction::witness_map: the first n - 1 coefficients of h (canonical) */
int tpst_groth16_witness_map(tpst_ctx* ctx, tpst_groth16_pk* pk, tpst_r1cs* r1cs, const uint64_t* vars,
                             const uint64_t* inputs, uint64_t* h);
/* create_proof_with_reduction: rs = (r, s) canonical; Proof { a: G1, b: G2, c: G1 } */
int tpst_groth16_prove(tpst_ctx* ctx, tpst_groth16_pk* pk, tpst_r1cs* r1cs, const uint64_t* vars,
                       const uint64_t* inputs, const uint64_t* rs, uint64_t* A, uint64_t* B, uint64_t* C);
/* Groth16::verify_proof (ark-groth16 verifier.rs): TPST_OK if the proof
 * verifies, TPST_E_VERIFY if it does not or if any element is malformed
 * (coordinate >= p, off the curve, outside the r-torsion subgroup, input >= r:
 * what Validate::Yes deserialisation rejects); TPST_E_ARG if n_abc !=
 * n_inputs + 1.  Canonical affine points, vk as tpst_groth16_vk returns it. */
int tpst_groth16_verify(tpst_ctx* ctx, const uint64_t* alpha_g1, const uint64_t* beta_g2, const uint64_t* gamma_g2,
                        const uint64_t* delta_g2, const uint64_t* gamma_abc_g1, size_t n_abc, const uint64_t* inputs,
                        size_t n_inputs, const uint64_t* A, const uint64_t* B, const uint64_t* C);

/* ---- arkworks wire format (csrc/serialize.hip; host only, no context) ------
 * CanonicalSerialize with Compress::Yes (ark-serialize 0.4): G1 48 B, G2 96 B
 * (x with SWFlags in the top bits of the last byte: 0x80 y negative, 0x40
 * infinity), GT 576 B, usize / Vec length as u64 LE.  The byte strings of
 * benches/pst.rs:43-46,64-74 (commiter_key_size, proof_size = |Proof| +
 * |MippProof|).  Writers: out == NULL only reports the length in *len;
 * TPST_E_ARG if cap is too small or an element is not canonical.  Readers
 * validate like Validate::Yes (canonical, on curve, prime-order subgroup). */
int tpst_ser_g1(const uint64_t* p, uint8_t* out48);
int tpst_ser_g2(const uint64_t* p, uint8_t* out96);
int tpst_de_g1(const uint8_t* in48, uint64_t* p);
int tpst_de_g2(const uint8_t* in96, uint64_t* p);
/* Commitment { nv, g_product } (sqrt_pst.rs:201 U, :121-125 comm_list entries) */
int tpst_ser_commitment(int nv, const uint64_t* g1, uint8_t* out, size_t cap, size_t* len);
/* Proof { proofs: Vec<G2> } -- the pst_proof of Polynomial::open (sqrt_pst.rs:225) */
int tpst_ser_pst_proof(const tpst_open_proof* p, uint8_t* out, size_t cap, size_t* len);
/* MippProof (mipp.rs:21-28) */
int tpst_ser_mipp_proof(const tpst_open_proof* p, uint8_t* out, size_t cap, size_t* len);
/* both back into a tpst_open_proof (U left zero) */
int tpst_de_open_proof(const uint8_t* pst, size_t pst_len, const uint8_t* mipp, size_t mipp_len,
                       tpst_open_proof* out);
/* CommitterKey { nv, powers_of_g, powers_of_h, g, h } from the flat SRS of
 * tpst_srs_export (benches/pst.rs:43-46) */
int tpst_ser_committer_key(int nv, const uint64_t* srs_flat, size_t flat_len, uint8_t* out, size_t cap,
                           size_t* len);  /* flat_len == tpst_srs_flat_len(nv) */

/* ---- batched point decompression and validation (csrc/point_codec.hip) ------
 * One device lane per point, at any n: the steps of tpst_de_g1 / tpst_de_g2
 * and of tpst_g1_check / tpst_g2_check, with the same verdict on every input.
 * n compressed points -> n x 12 (G1) / n x 24 (G2) canonical limbs, Validate::Yes on the device.
 * TPST_E_ARG if any point is rejected: *first_bad (may be NULL) = lowest rejected index, out is
 * then not to be used.  n == 0 is TPST_OK. */
int tpst_de_g1_batch(tpst_ctx* ctx, const uint8_t* in, size_t n, uint64_t* out, size_t* first_bad);
int tpst_de_g2_batch(tpst_ctx* ctx, const uint8_t* in, size_t n, uint64_t* out, size_t* first_bad);
/* n canonical affine points -> TPST_OK, or TPST_E_VERIFY with *first_bad */
int tpst_g1_check_batch(tpst_ctx* ctx, const uint64_t* pts, size_t n, size_t* first_bad);
int tpst_g2_check_batch(tpst_ctx* ctx, const uint64_t* pts, size_t n, size_t* first_bad);

/* ---- batched double-scalar multiplication (csrc/lincomb.hip) ----------------
 * out[i] = s_i P_i + t_i Q_i for n pairs of canonical affine points (12 / 24
 * u64 each, all-zero = infinity) and canonical Fr scalars; out: n canonical
 * affine points.  Q and t may both be NULL: out[i] = s_i P_i.  One quad of
 * lanes per output, joint double-and-add over the bit length of the longest
 * scalar of the call (128-bit scalars cost half of full ones).  Every case is
 * computed exactly: zero scalars, P = Q, P = -Q, inputs and results at
 * infinity.  TPST_E_ARG: a null argument (or only one of Q, t), a scalar >= r,
 * a non-canonical coordinate, a point off its curve.  Subgroup membership is
 * not required (as for tpst_g1_msm).  n = 0 returns TPST_OK. */
int tpst_g1_lincomb_batch(tpst_ctx* ctx, const uint64_t* P, const uint64_t* s, const uint64_t* Q, const uint64_t* t,
                          size_t n, uint64_t* out);
int tpst_g2_lincomb_batch(tpst_ctx* ctx, const uint64_t* P, const uint64_t* s, const uint64_t* Q, const uint64_t* t,
                          size_t n, uint64_t* out);

/* ---- arkworks wire format of the SPARK objects (csrc/serialize.hip) ---------
 * Compress::Yes, as above.  The writers are host only; the readers walk the
 * structure on the host (csrc/wire_spark.h) and validate all the object's
 * points in one device batch.  Readers return TPST_E_ARG for a truncated input,
 * trailing bytes, a length prefix other than the one the sizes imply or beyond
 * the input or a caller capacity (checked before anything is allocated or
 * copied), batch_size != 3, an Fr >= r, or a rejected point.
 *
 * R1CSCommitment { num_cons, num_vars, num_inputs, SparseMatPolyCommitment {
 * batch_size, num_ops, num_mem_cells, comm_comb_ops: Vec<G1>, comm_comb_mem:
 * Vec<G1> } } (r1csinstance.rs:55-61, sparse_mlpoly.rs:325-332). */
int tpst_ser_r1cs_commitment(size_t num_cons, size_t num_vars, size_t num_inputs, size_t num_ops,
                             size_t num_mem_cells, const uint64_t* comm_ops, size_t ops_rows,
                             const uint64_t* comm_mem, size_t mem_rows, uint8_t* out, size_t cap, size_t* len);
/* dims = num_cons, num_vars, num_inputs, num_ops, num_mem_cells.  With comm_ops
 * and comm_mem NULL and both capacities 0 only dims and the row counts are
 * reported (no point is validated). */
int tpst_de_r1cs_commitment(tpst_ctx* ctx, const uint8_t* in, size_t len, size_t dims[5], uint64_t* comm_ops,
                            size_t ops_cap, size_t* ops_rows, uint64_t* comm_mem, size_t mem_cap, size_t* mem_rows);
/* R1CSEvalProof (r1csinstance.rs:336-339, sparse_mlpoly.rs:1441-1445, :1337-
 * 1341, :1043-1050, :691-700; product_tree.rs:138-170; nizk/mod.rs:31-38) from
 * and to the buffers of tpst_r1cs_eval_prove / _verify of these sizes. */
int tpst_ser_r1cs_eval_proof(const tpst_r1cs_eval_sizes* sizes, const tpst_r1cs_eval_proof* proof,
                             const uint64_t* comm_derefs, const uint64_t* prod_ops, const uint64_t* prod_mem,
                             uint8_t* out, size_t cap, size_t* len);
int tpst_de_r1cs_eval_proof(tpst_ctx* ctx, const uint8_t* in, size_t len, const tpst_r1cs_eval_sizes* sizes,
                            tpst_r1cs_eval_proof* proof, uint64_t* comm_derefs, uint64_t* prod_ops,
                            uint64_t* prod_mem);
/* R1CSProof (r1csproof.rs:32-53) in declaration order: comm (nv = m_row),
 * sc_proof_phase1, claims_phase2, sc_proof_phase2, eval_vars_at_ry,
 * proof_eval_vars_at_ry, rx, ry, transcript_sat_state, initial_state, t,
 * mipp_proof; the layout list is csrc/wire_snark.h.  r_abc and
 * claims_phase2_z_abc are not fields of the reference's struct: not written,
 * zero after a read, read by no verifier.  The writer is host only and takes
 * the dimensions from the proof's own fields; the reader takes them from
 * num_cons / num_vars and validates as the readers above (TPST_E_ARG also for
 * an Fq12 coefficient >= p). */
int tpst_ser_r1cs_proof(const tpst_r1cs_proof* proof, uint8_t* out, size_t cap, size_t* len);
int tpst_de_r1cs_proof(tpst_ctx* ctx, const uint8_t* in, size_t len, size_t num_cons, size_t num_vars,
                       tpst_r1cs_proof* proof);
/* The SNARK proof = R1CSProof || R1CSEvalProof || Ar || Br || Cr.  This is
 * this library's layout: the reference's TestudoSnark (testudo_snark.rs:22-29)
 * would start with a Groth16 proof that is not produced here. */
int tpst_ser_snark_proof(const tpst_r1cs_eval_sizes* sizes, const tpst_snark_proof* proof,
                         const uint64_t* comm_derefs, const uint64_t* prod_ops, const uint64_t* prod_mem,
                         uint8_t* out, size_t cap, size_t* len);
int tpst_de_snark_proof(tpst_ctx* ctx, const uint8_t* in, size_t len, size_t num_cons, size_t num_vars,
                        const tpst_r1cs_eval_sizes* sizes, tpst_snark_proof* proof, uint64_t* comm_derefs,
                        uint64_t* prod_ops, uint64_t* prod_mem);
/* inverse of tpst_ser_committer_key: flat = the tpst_srs_export layout, so
 * tpst_srs_load takes it.  With flat NULL and flat_cap 0 only *nv and
 * *flat_len are reported. */
int tpst_de_committer_key(tpst_ctx* ctx, const uint8_t* in, size_t len, int* nv, uint64_t* flat, size_t flat_cap,
                          size_t* flat_len);

/* ---- utilities ----------------------------------------------------------- */
/* out[i] = scalars[i] * G1 generator (affine, canonical); synthetic bases */
int tpst_g1_mul_generator(tpst_ctx* ctx, const uint64_t* scalars, size_t n, uint64_t* out);
int tpst_g2_mul_generator(tpst_ctx* ctx, const uint64_t* scalars, size_t n, uint64_t* out);
/* device forms: d_out Montgomery (for _dev MSM bases) */
int tpst_g1_mul_generator_dev(tpst_ctx* ctx, const void* d_scalars, size_t n, void* d_out_mont);

/* Field microbenchmark (measured peak for the roofline's compute column):
 * kind 0 = Fq Montgomery multiply, 1 = G1 XYZZ mixed add, 2 = Fq inverse, 3 / 4 = Fq multiply
 * variants (two interleaved accumulation chains / independent columns), 5 = G1 XYZZ doubling, 15 = Fq inverse
 * by a whole wave (csrc/inv_wave.h; one chain per 64 threads), 16 + op = one wave
 * running `iters` stages of wave-engine op `op` (csrc/wave_ops.inc), 13 = G1 XYZZ mixed add
 * over the radix-2^29 field, 116 = its chain-start form (ZZ = ZZZ = 1), 20 = the verifiers' host
 * check of `threads` row commitments (up to 16 host threads; host milliseconds of one pass).  Runs `threads`
 * threads x `iters` dependent ops each; returns kernel milliseconds. */
int tpst_microbench(tpst_ctx* ctx, int kind, size_t threads, int iters, double* ms);
/* shader-clock cycles of the parts of `iters` stages of wave op `op` (forms,
 * product, product store, output forms, output reduce/store) */
int tpst_microbench_wave_phases(tpst_ctx* ctx, int op, int iters, uint64_t* cycles5);
/* Self-test of the two device Fq inverses: n Montgomery-form values (6 words
 * each) -> their inverses by the lone-lane routine and by the wave routine. */
int tpst_selftest_inv(tpst_ctx* ctx, size_t n, const uint64_t* in, uint64_t* out_lane, uint64_t* out_wave);
/* Self-tests of the device arithmetic below the kernels: one field operation
 * (op = family * 32 + index) or one curve operation (op = form * 16 + index)
 * per element on n caller-chosen operands, words exactly as the kernels hold
 * them.  The op numbers and the words per operand and result are those of
 * csrc/selftest_ops.h (field_in_words / field_out_words / curve_words).  A bad
 * op, a null pointer or n == 0 is TPST_E_ARG (q may be null for glv_split). */
int tpst_selftest_field(tpst_ctx* ctx, int op, size_t n, const uint64_t* a, const uint64_t* b, uint64_t* out);
int tpst_selftest_curve(tpst_ctx* ctx, int op, size_t n, const uint64_t* p, const uint64_t* q, uint64_t* out);
/* Self-test of the pairing's two Fq12 engines on n caller-chosen operands: the
 * RNS chain engine (csrc/rns_engine.h, engine 0) and the radix wave engine
 * (csrc/wave_tower.h, engine 1), run through the engines' own loads, stages
 * and stores.  op = engine << 8 | in codec << 7 | out codec << 6 | index
 * (csrc/selftest_ops.h: tower_op / tower_op_valid / tower_a_words /
 * tower_b_words / tower_out_words).
 *   codec 0 (FQ): an Fq12 as 12 field.h Montgomery Fq in tower order, 144 u32
 *     words per element; results canonical (< p).
 *   codec 1 (RES, RNS engine only): the engine's 12 x 32 raw residue words
 *     (word 32 k + c = channel c of coefficient k; channels 0..14 base B, 15
 *     mod 2^32, 16..30 base B', 31 idle: ignored going in, unspecified coming
 *     out): any integer < 16 p per coefficient going in, the stage's
 *     bit-exact residues coming out.
 *   index 0 F12_MUL (a b), 1 F12_SQR, 2 CYC_SQR (the Granger-Scott formula, a
 *     polynomial identity on any a), 3 / 4 / 5 FROB1 / FROB2 / FROB3, 6 CONJ,
 *     7 COPY (under FQ -> FQ the load / store round trip): single stages;
 *   8 INV: the inversion both final exponentiations start with (rc_inv /
 *     fe_inv).  a = 0 gives 0 (the tower norm is 0 and the device Fq inverses
 *     map 0 to 0, tpst_selftest_inv), where arkworks' Field::inverse returns
 *     None: callers that can meet 0 test for it first.  A final
 *     exponentiation of 0 is therefore 0 on both engines; no entry point of
 *     this library feeds it one from valid inputs.
 *   9 FINAL_EXP (RNS, FQ only): the final exponentiation of a alone.
 *   10 G2_PREPARE (RNS, FQ only): a = n affine G2 points (Montgomery x, y: 48
 *     words each) -> 69 line coefficients (c0, c1, c2: 72 words) per point,
 *     coefficient-major: coefficient j of point i at out + 72 (j n + i) words.
 *   11 GT_POW (wave only): a = base, b = 4 u64 base-x exponent digits (8
 *     words) -> n x 144 result words, then n words ok[i] (1: base[i] is in
 *     GT), then one zero word if n is odd; the result of a non-member is 0.
 *   12 PASS (RNS only): no stage, the load straight into the store: FQ -> RES
 *     is the engine's load alone, RES -> FQ its store alone on a's integers.
 * The wave engine runs F12_MUL, CYC_SQR, FROB1, FROB2, CONJ, INV and GT_POW.
 * b is read by F12_MUL and GT_POW only and may be null otherwise.  A bad op, a
 * null pointer, n == 0 or n > 2^16 is TPST_E_ARG. */
int tpst_selftest_tower(tpst_ctx* ctx, int op, size_t n, const uint64_t* a, const uint64_t* b, uint64_t* out);
/* Self-test of the fixed-base table engine (csrc/fbt.h): the opening's own
 * fbt_build and fbt_msm on caller-chosen bases, scalars and groups, with
 * everything an FbGroups can say.  No kernel of its own.
 *   group 1 / 2: G1 / G2.  glv 0 / 1: the plain table (64 windows per base) or
 *     the GLV table (32 windows, G1 only: glv = 1 with group = 2 is
 *     TPST_E_ARG).
 *   bases: n canonical affine points in tpst_g1_msm's layout (12 / 24 u64 each,
 *     infinity = all zero), 1 <= n <= 2^14.
 *   mode 0, the grouped MSM: scalars = n_scalars canonical Fr (4 u64 each,
 *     1 <= n_scalars <= 2^20); out[q groups + g] = sum over the members m <
 *     `members` of group g of scalars[k + q set_stride] * bases[k], as
 *     canonical affine points (sets * groups of them), where
 *       seg == NULL (strided): k = (m / D) L + g D + m % D;
 *       seg != NULL: groups + 1 u32, k = seg[g] + m for m < seg[g+1] - seg[g]
 *         (L and D are not read; an empty segment gives infinity).
 *     Checked on the host before anything is launched, each violation
 *     TPST_E_ARG: groups, sets >= 1; sets * groups * max(members, 1) <= 2^16;
 *     strided: 1 <= L, D <= 2^14; every k is below n and every k + q set_stride
 *     below n_scalars (set_stride <= 2^20); seg is non-decreasing, ends at or
 *     below n, and no segment is longer than `members`.  members = 0 is
 *     allowed and gives infinity.
 *   mode 1, the table: scalars, the group arguments and seg are not read;
 *     out = the n * nw * 8 table entries as canonical affine points, nw = 64
 *     (plain) or 32 (GLV): entry ((k nw + w) 8 + m) = (m + 1) 16^w bases[k].
 * A null ctx, bases or out, a group, glv or mode outside the values above, or
 * n outside its range is TPST_E_ARG. */
int tpst_selftest_fbt(tpst_ctx* ctx, int group, int glv, int mode, const uint64_t* bases, size_t n,
                      const uint64_t* scalars, size_t n_scalars, size_t groups, size_t members, size_t L, size_t D,
                      const uint32_t* seg, size_t sets, size_t set_stride, uint64_t* out);

/* Per-stage HIP-event timing of the MSM pipeline on the context's stream.
 * stage: 0 decompose, 1 sort, 2 bucket bounds, 3 bucket accumulation (the
 * dominant kernel), 4 bucket reduction, 5 window combine, 6 K1 row sort;
 * 15 / 16: tpst_r1cs_evaluate's eq tables / its reduction and partial sum;
 * 17 / 18 / 19: tpst_hyrax_eval_prove's eq tables / bound / dot-product proof
 * (first launch to last result, the host work between launches included);
 * 20 / 21: tpst_prodcircuit_prove's layer build / all layer proofs (host work
 * between launches included); 22 / 23: round 0 / round 1 of its layer 0 alone
 * (round kernel and reduce); 24 / 25 / 26 / 27: tpst_r1cs_eval_prove's
 * k_deref / k_hash_ops / k_hash_mem / k_seg_eval (both groups, with their
 * partial sums); 28: the batched point decompression / validation kernels
 * (tpst_de_g1_batch and its kin, the wire-format readers, the verifiers' row
 * checks from POINT_CHECK_DEVICE_MIN points up). */
int tpst_profile_enable(tpst_ctx* ctx, int on);
int tpst_profile_reset(tpst_ctx* ctx);
int tpst_profile_read(tpst_ctx* ctx, int stage, double* total_ms, uint64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* TPST_H */
