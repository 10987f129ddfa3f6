// msm_pieces.h on the host: the first / last-of-bucket flags of the sorted
// values (entry_flags, set by k_sort_bin) and the flag-driven walk of the
// short-chunk accumulation (run_ends / run_slot) against the predicate it
// replaced (bstart[key] >= c0, bend[key] <= c1), on random sorted key arrays
// with empty buckets and windows, several windows, a sentinel tail, chunks of
// 2^3 .. 2^5 entries and window groups whose bounds cut chunks.
// Stand-alone (g++ -I testudo_amd/csrc; also clean under
// -fsanitize=address,undefined).  Prints "cases N bad 0" and exits 0, or
// names the first failing case and exits 1.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "msm_pieces.h"

using namespace tpst;

static int bad = 0, cases = 0;

static void fail(const char* what, int trial, size_t a, size_t b) {
  if (!bad) fprintf(stderr, "trial %d: %s (%zu, %zu)\n", trial, what, a, b);
  bad++;
}

struct Sorted {
  int W;
  uint32_t nb, sent;
  std::vector<uint32_t> keys, vals, bstart, bend, range;
};

// bucket sizes drawn per window: empty windows, sparse windows (many empty
// buckets, one- and two-entry ones), windows of mid-sized buckets and windows
// with one bucket far longer than a chunk
static Sorted make(std::mt19937& rng, int trial) {
  Sorted a;
  a.W = 1 + (int)(rng() % 5);
  a.nb = 1u << (rng() % 4);
  a.sent = (uint32_t)a.W * a.nb;
  a.bstart.assign(a.sent, 0);
  a.bend.assign(a.sent, 0);
  a.range.assign(a.W + 1, 0);
  for (int w = 0; w < a.W; w++) {
    a.range[w] = (uint32_t)a.keys.size();
    const int shape = (int)(rng() % 4);
    for (uint32_t d = 0; d < a.nb; d++) {
      uint32_t cnt = 0;
      if (shape == 1) cnt = rng() % 3;
      if (shape == 2) cnt = rng() % 40;
      if (shape == 3) cnt = (rng() % 4 == 0) ? 60 + rng() % 200 : rng() % 4;
      const uint32_t key = (uint32_t)w * a.nb + d;
      a.bstart[key] = (uint32_t)a.keys.size();
      // both sort paths put the entry of rank r at bstart + r
      for (uint32_t r = 0; r < cnt; r++) {
        a.keys.push_back(key);
        a.vals.push_back((rng() & (VAL_INDEX | VAL_SIGN)) | entry_flags(r, cnt));
      }
      a.bend[key] = (uint32_t)a.keys.size();
    }
  }
  a.range[a.W] = (uint32_t)a.keys.size();
  const uint32_t tail = rng() % 70;  // zero digits: sentinel keys, values never written
  for (uint32_t i = 0; i < tail; i++) {
    a.keys.push_back(a.sent);
    a.vals.push_back(rng());
  }
  return a;
}

// entry_flags marks exactly the first and the last entry of every bucket
static void check_flags(const Sorted& a, int trial) {
  const size_t m = a.range[a.W];
  for (size_t e = 0; e < m; e++) {
    const bool first = e == 0 || a.keys[e - 1] != a.keys[e];
    const bool last = e + 1 == m || a.keys[e + 1] != a.keys[e];
    cases++;
    if (first != ((a.vals[e] & VAL_FIRST) != 0)) fail("first flag", trial, e, a.keys[e]);
    if (last != ((a.vals[e] & VAL_LAST) != 0)) fail("last flag", trial, e, a.keys[e]);
  }
}

// one launch over windows [wlo, whi) with chunks of 2^lg entries: every run's
// destination by the flags and by the bucket bounds
static void check_walk(const Sorted& a, int wlo, int whi, int lg, int trial) {
  const size_t e_lo = a.range[wlo], e_hi = a.range[whi];
  for (size_t t = e_lo >> lg; (t << lg) < e_hi; t++) {
    size_t c0 = t << lg;
    const size_t c1 = (c0 + ((size_t)1 << lg) < e_hi) ? c0 + ((size_t)1 << lg) : e_hi;
    if (c0 < e_lo) c0 = e_lo;
    const size_t steps = c1 - c0;
    // the kernels' state: the value one entry ahead, the first value of the
    // current run, and the key of a bucket stored whole, loaded one step early
    const uint32_t none = ~0u;
    uint32_t val = a.vals[c0], val_n = steps > 1 ? a.vals[c0 + 1] : 0u;
    uint32_t first_val = val;
    uint32_t held = a.keys[c0];
    for (size_t s = 0; s < steps; s++) {
      const size_t e = c0 + s;
      const uint32_t key = a.keys[e];
      const uint32_t val_nn = s + 2 < steps ? a.vals[e + 2] : 0u;
      const uint32_t first_n = run_ends(val, s + 1 == steps) ? val_n : first_val;
      const uint32_t held_n = s + 1 < steps && run_slot(first_n, val_n) == RUN_BUCKET ? a.keys[e + 1] : none;
      if (val != a.vals[e]) fail("value pipeline", trial, e, t);
      if (key >= a.sent) fail("sentinel inside the range", trial, e, key);
      const bool end_old = e + 1 >= c1 || a.keys[e + 1] != key;
      const bool end_new = run_ends(val, s + 1 == steps);
      if (end_old != end_new) fail("run end", trial, e, t);
      if (end_new) {
        cases++;
        const bool starts = a.bstart[key] >= c0, ends = a.bend[key] <= c1;
        const uint32_t want = starts && ends ? RUN_BUCKET : (starts ? 1u : 0u);
        if (run_slot(first_val, val) != want) fail("destination", trial, e, t);
        if (want == RUN_BUCKET && held != key) fail("key of a whole bucket", trial, e, held);
      }
      val = val_n;
      val_n = val_nn;
      first_val = first_n;
      held = held_n;
    }
  }
}

int main() {
  // the rule itself
  cases += 4;
  if (entry_flags(0, 1) != (VAL_FIRST | VAL_LAST)) fail("single entry", -1, 0, 1);
  if (entry_flags(0, 5) != VAL_FIRST) fail("first of five", -1, 0, 5);
  if (entry_flags(4, 5) != VAL_LAST) fail("last of five", -1, 4, 5);
  if (entry_flags(2, 5) != 0) fail("inside", -1, 2, 5);
  // sign, flags and a 28-bit index (2 x 2^27 points with GLV) do not overlap
  cases++;
  if ((VAL_SIGN & VAL_FIRST) || (VAL_SIGN & VAL_LAST) || (VAL_FIRST & VAL_LAST) ||
      ((VAL_SIGN | VAL_FIRST | VAL_LAST) & VAL_INDEX) || VAL_INDEX < (1u << 28) - 1 || (VAL_INDEX & (VAL_INDEX + 1)))
    fail("bit layout", -1, VAL_INDEX, VAL_LAST);
  std::mt19937 rng(20240607);
  for (int trial = 0; trial < 400; trial++) {
    const Sorted a = make(rng, trial);
    check_flags(a, trial);
    for (int lg = 3; lg <= 5; lg++) {
      check_walk(a, 0, a.W, lg, trial);  // one group
      for (int cut = 1; cut < a.W; cut++) {  // two groups: the bound cuts a chunk
        check_walk(a, 0, cut, lg, trial);
        check_walk(a, cut, a.W, lg, trial);
      }
    }
  }
  printf("cases %d bad %d\n", cases, bad);
  return bad ? 1 : 0;
}
