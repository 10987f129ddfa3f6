// msm_pieces.h on the host: fixup_pieces / fixup_class on the bucket shapes
// the short-chunk fixup meets, and against a direct count of the chunks a
// bucket touches.  Stand-alone (g++ -I testudo_amd/csrc; also clean under
// -fsanitize=address,undefined).  Prints "cases N bad 0" and exits 0, or
// names the first failing case and exits 1.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "msm_pieces.h"

using namespace tpst;

static int bad = 0, cases = 0;

static void expect(const char* what, uint32_t s, uint32_t e, int lg, uint32_t pieces, uint32_t cls) {
  cases++;
  const uint32_t p = fixup_pieces(s, e, lg), c = fixup_class(p);
  if (p != pieces || c != cls) {
    if (!bad) fprintf(stderr, "%s: [%u, %u) lg %d: pieces %u (want %u) class %u (want %u)\n", what, s, e, lg, p, pieces, c, cls);
    bad++;
  }
}

// chunks holding an entry of [s, e), minus one: marks them one by one
static uint32_t direct(uint32_t s, uint32_t e, int lg) {
  if (e <= s) return 0;
  std::vector<char> hit(((size_t)e >> lg) + 1, 0);
  for (uint32_t i = s; i < e; i++) hit[i >> lg] = 1;
  uint32_t n = 0;
  for (char h : hit) n += h;
  return n - 1;
}

int main() {
  const int lg = 4;  // 16-entry chunks, the window-grouped path's
  const uint32_t L = 1u << lg;
  expect("inside one chunk", 3 * L + 2, 3 * L + 9, lg, 0, 0);
  expect("a whole chunk", 3 * L, 4 * L, lg, 0, 0);
  expect("one entry", 5 * L + 15, 5 * L + 16, lg, 0, 0);
  expect("ends on a chunk boundary", 3 * L + 5, 5 * L, lg, 1, 1);
  expect("one entry past the boundary", 3 * L + 5, 5 * L + 1, lg, 2, 2);
  expect("starts on a boundary", 4 * L, 5 * L + 1, lg, 1, 1);
  expect("empty", 77, 77, lg, 0, 0);
  expect("empty at 0", 0, 0, lg, 0, 0);
  expect("empty, bounds reversed", 80, 64, lg, 0, 0);
  // t1 - t0 = LONG_PARTS: the last bucket a lane walks; one chunk more: the long list's
  expect("LONG_PARTS chunks past the first", 2 * L + 7, (2 + LONG_PARTS) * L + 1, lg, LONG_PARTS, FIXUP_CAP);
  expect("LONG_PARTS, ending on a boundary", 2 * L + 7, (3 + LONG_PARTS) * L, lg, LONG_PARTS, FIXUP_CAP);
  expect("LONG_PARTS + 1", 2 * L + 7, (3 + LONG_PARTS) * L + 1, lg, LONG_PARTS + 1, FIXUP_LONG);
  expect("FIXUP_CAP - 1", L - 1, (FIXUP_CAP - 1) * L + 1, lg, FIXUP_CAP - 1, FIXUP_CAP - 1);
  expect("FIXUP_CAP", L - 1, FIXUP_CAP * L + 1, lg, FIXUP_CAP, FIXUP_CAP);
  expect("FIXUP_CAP + 1", L - 1, (FIXUP_CAP + 1) * L + 1, lg, FIXUP_CAP + 1, FIXUP_CAP);
  expect("top of the entry range", 0x7fffffe0u, 0x7fffffffu, lg, 1, 1);
  expect("a window of one bucket", 0, 1u << 21, lg, (1u << 17) - 1, FIXUP_LONG);
  expect("32-entry chunks", 31, 65, 5, 2, 2);
  // every bucket of a small range, three chunk lengths, against the direct count
  for (int g = 0; g <= 5; g += (g ? 1 : 3))  // lg 0, 3, 4, 5
    for (uint32_t s = 0; s < 100; s++)
      for (uint32_t e = s; e < s + 80; e++) {
        const uint32_t d = direct(s, e, g);
        expect("sweep", s, e, g, d, d > LONG_PARTS ? FIXUP_LONG : (d < FIXUP_CAP ? d : FIXUP_CAP));
      }
  printf("cases %d bad %d\n", cases, bad);
  return bad ? 1 : 0;
}
