// pairing_plan.h on the host: every *_scratch sum against a replay of the
// Arena takes of its entry point.  The replays below are written out from the
// launch code (pairing.hip, pairing_wave.hip) with literal sizes and their own
// 256-byte rounding, not through the header, so a formula that loses or gains
// a term, or a tree that stops at another level, shows up as a difference.
// For every case: replayed <= scratch <= replayed + the fixed slack.
// Stand-alone (g++ -I testudo_amd/csrc; also clean under
// -fsanitize=address,undefined).  Prints "cases N bad 0" and exits 0, or names
// the first failing case and exits 1.
#include <cstdio>
#include <cstdlib>
#include "pairing_plan.h"

using namespace tpst;

static int bad = 0, cases = 0;

constexpr size_t F12 = 576, LINE = 288, LINES = 69, RES = 384, BLOCKS = 8, SLACK = 4096 + 256 * 16;

struct Replay {  // Arena::take's bookkeeping
  size_t off = 0;
  void take(size_t count, size_t elem) { off += (count * elem + 255) / 256 * 256; }
};

static void expect(const char* what, size_t a, size_t b, size_t replayed, size_t scratch) {
  cases++;
  if (scratch < replayed || scratch > replayed + SLACK) {
    if (!bad) fprintf(stderr, "%s(%zu, %zu): takes %zu bytes, scratch %zu\n", what, a, b, replayed, scratch);
    bad++;
  }
}

// pairing_from_lines: one u32 buffer per level of the chunk-4 tree down to
// one product per (group, line), then the block multipliers
static void from_lines(Replay& r, size_t groups, size_t n) {
  while (n > 1) {
    const size_t nout = (n + 3) / 4;
    r.take(groups * LINES * nout * RES, 4);
    n = nout;
  }
  r.take(groups * BLOCKS * RES, 4);
}

static void multi_pairing_prepared(Replay& r, size_t groups, size_t n) {
  r.take(groups * LINES * (n ? n : 1), F12);
  from_lines(r, groups, n ? (n + 1) / 2 : 1);
}

static void mipp_lookahead(Replay& r, size_t sp, size_t E) {
  const size_t n = sp * E;
  r.take(8 * LINES * n, F12);
  from_lines(r, 8, (n + 1) / 2);
}

static void multi_pairing(Replay& r, size_t groups, size_t n) {
  const size_t np = groups * n;
  r.take(np * LINES, LINE);
  r.take(np * LINES * 6 * 32, 4);
  multi_pairing_prepared(r, groups, n);
}

// gt_product_final: one Fq12 buffer per level of the chunk-8 tree down to the
// 4 partials k_final_wave multiplies itself
static size_t gt_product_final(Replay& r, size_t groups, size_t n) {
  size_t levels = 0;
  while (n > 4) {
    const size_t nout = (n + 7) / 8;
    r.take(groups * nout, F12);
    n = nout;
    levels++;
  }
  return levels;
}

int main() {
  const size_t G[] = {1, 2, 8};
  const size_t N[] = {0, 1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 63, 64, 65, 2048, 4096, 4097};
  for (size_t groups : G)
    for (size_t n : N) {
      Replay a, b, c;
      multi_pairing_prepared(a, groups, n);
      expect("multi_pairing_prepared", groups, n, a.off, multi_pairing_scratch(groups, n));
      multi_pairing(b, groups, n);
      expect("multi_pairing", groups, n, b.off, multi_pairing_reserve(groups, n));
      gt_product_final(c, groups, n);
      expect("gt_product_final", groups, n, c.off, gt_product_scratch(groups, n));
    }
  // the look-ahead has 8 groups; sp = len / 4 = 0 is rejected before any take
  for (size_t E = 1; E <= 8; E *= 2)
    for (size_t sp : N) {
      if (!sp) continue;
      Replay a;
      mipp_lookahead(a, sp, E);
      expect("mipp_lookahead", sp, E, a.off, mipp_lookahead_scratch(sp, (int)E));
    }
  // the levels the GPU test of tpst_gt_final_exp_product walks: none up to 4
  // partials, one for 5 (5 -> 1), two for 40 (40 -> 5 -> 1)
  const size_t want_levels[][2] = {{0, 0}, {4, 0}, {5, 1}, {32, 1}, {33, 2}, {40, 2}};
  for (auto& w : want_levels) {
    size_t levels = 0;  // as the launch loop of gt_product_final walks the header's tree
    for (plan::Tree t = plan::partial_tree(w[0]); t.more(); t.step()) levels++;
    Replay r;
    cases++;
    if (levels != w[1] || gt_product_final(r, 1, w[0]) != w[1]) {
      if (!bad) fprintf(stderr, "gt_product_final: %zu partials do not take %zu levels\n", w[0], w[1]);
      bad++;
    }
  }
  // the sizes the header states, against the replay's
  cases++;
  if (plan::F12_BYTES != F12 || plan::LINE_BYTES != LINE || plan::N_LINES != LINES || plan::RES_WORDS != RES ||
      plan::NBLK != BLOCKS || plan::SLACK != SLACK || g2_prepare_scratch(3) != 3 * LINES * 6 * 32 * 4) {
    if (!bad) fprintf(stderr, "pairing_plan.h sizes differ from the replay's\n");
    bad++;
  }
  printf("cases %d bad %d\n", cases, bad);
  return bad ? 1 : 0;
}
