// Scratch plan of the pairing entry points: how many elements each
// Arena::take of multi_pairing_prepared, mipp_lookahead, multi_pairing and
// gt_product_final asks for, the levels of their product trees, and the
// *_scratch sums of exactly those takes.  Arena::take checks no bound, so the
// sums are what keeps a take inside its reservation: the launch code takes
// through the counts and levels below and the sums add the same ones, in the
// order of the takes.  Host only (a stand-alone host test includes this header
// alone, tests/cpp/test_pairing_scratch.cpp); the pairing units assert that
// the sizes written here are those of the device types.
// A sum covers its entry point's takes from an arena the caller has reset.
// What a caller takes from the same arena before the call, itself or through
// another function, is the caller's to add or to reset away (the opening's
// look-ahead resets after its table MSM, pst_open.hip enqueue_lookahead).
#pragma once
#include <stddef.h>

namespace tpst {
namespace plan {

constexpr size_t F12_BYTES = 12 * 48;       // sizeof(Fq12)
constexpr size_t LINE_BYTES = 6 * 48;       // sizeof(LineCoeff): three Fq2
constexpr size_t RES_WORDS = 12 * 32;       // u32 per Fq12 in RNS form (rns::RES_WORDS)
constexpr size_t N_LINES = 69;              // line values per pair (N_LINE_COEFFS)
constexpr size_t NBLK = 8;                  // block multipliers per group (63 Miller bits, 8 per block)
constexpr size_t TREE_CHUNK = 4;            // factors per product of the line tree
constexpr size_t RW_CHUNK = 8;              // factors per product of the partial tree
constexpr size_t FW = 2;                    // waves of k_final_wave; each multiplies its share of the partials
constexpr size_t SLACK = 4096 + 256 * 16;   // fixed slack of every *_scratch sum

// bytes one Arena::take of count elements moves the arena by (Arena::need)
constexpr size_t need(size_t count, size_t elem) { return (count * elem + 255) & ~size_t(255); }

// A chunked product tree: n factors per group become ceil(n / chunk) until at
// most `stop` are left.  for (Tree t = ...; t.more(); t.step()) visits the
// levels; t.n factors go in and t.nout() products come out of each.
struct Tree {
  size_t n, chunk, stop;
  bool more() const { return n > stop; }
  size_t nout() const { return (n + chunk - 1) / chunk; }
  void step() { n = nout(); }
};
// over the pair products of a group's lines (pairing_from_lines), down to one
inline Tree line_tree(size_t n) { return {n, TREE_CHUNK, 1}; }
// over Miller partials (gt_product_final), down to what k_final_wave multiplies itself
inline Tree partial_tree(size_t n) { return {n, RW_CHUNK, 2 * FW}; }

// -- element counts of the takes ---------------------------------------------
// Fq12 line buffer of groups x n pairs (one entry per group when n = 0)
inline size_t lines_count(size_t groups, size_t n) { return groups * N_LINES * (n ? n : 1); }
// pair products k_line_pair leaves per (group, line): what the line tree starts from
inline size_t pair_products(size_t n) { return n ? (n + 1) / 2 : 1; }
// u32 of one line-tree level with nout products per (group, line)
inline size_t level_words(size_t groups, size_t nout) { return groups * N_LINES * nout * RES_WORDS; }
// u32 of the block multipliers
inline size_t mbr_words(size_t groups) { return groups * NBLK * RES_WORDS; }
// u32 of the residue lines the G2 preparation of n points writes
inline size_t prepare_words(size_t n) { return n * N_LINES * 6 * 32; }

// takes of pairing_from_lines over n pair products per (group, line): one per
// tree level, then the block multipliers
inline size_t from_lines_bytes(size_t groups, size_t n) {
  size_t b = 0;
  for (Tree t = line_tree(n); t.more(); t.step()) b += need(level_words(groups, t.nout()), 4);
  return b + need(mbr_words(groups), 4);
}

}  // namespace plan

// multi_pairing_prepared: the lines, then pairing_from_lines
inline size_t multi_pairing_scratch(size_t groups, size_t n) {
  return plan::need(plan::lines_count(groups, n), plan::F12_BYTES) +
         plan::from_lines_bytes(groups, plan::pair_products(n)) + plan::SLACK;
}

// mipp_lookahead over len = 4 sp, E fold sets: 8 groups of sp E >= 1 pairs,
// the same takes as multi_pairing_prepared's
inline size_t mipp_lookahead_scratch(size_t sp, int E) { return multi_pairing_scratch(8, sp * (size_t)E); }

// g2_prepare_batch of n points: the residue lines (the caller's buffer)
inline size_t g2_prepare_scratch(size_t n) { return plan::prepare_words(n) * 4; }

// multi_pairing reserves this itself: the prepared coefficients and the
// residue lines of all groups x n pairs, then multi_pairing_prepared
inline size_t multi_pairing_reserve(size_t groups, size_t n) {
  const size_t np = groups * n;
  return plan::need(np * plan::N_LINES, plan::LINE_BYTES) + plan::need(plan::prepare_words(np), 4) +
         multi_pairing_scratch(groups, n);
}

// gt_product_final: one take per level of the partial tree
inline size_t gt_product_scratch(size_t groups, size_t n) {
  size_t b = 0;
  for (plan::Tree t = plan::partial_tree(n); t.more(); t.step()) b += plan::need(groups * t.nout(), plan::F12_BYTES);
  return b + plan::SLACK;
}

}  // namespace tpst
