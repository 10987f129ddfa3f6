// Host check of curve.h's chain-start mixed add (add_affine_unit: p is
// infinity or has ZZ = ZZZ = 1) against add_affine, over Fq (field.h) and
// Fq29 (field29.h), for tests/test_add_affine_unit.py.  Binary stdin:
//   i32 n, n x 48 words of p (XYZZ, field.h Montgomery words), n x 48 words of
//   q (X, Y the affine point, infinity X = Y = 0; the rest ignored)
// Every pair must meet the contract (exit status 3 otherwise).  Equality is
// equality of all four coordinates, word for word.  Prints
//   pairs N fq_bad A fq29_bad B
// and the index of the first few mismatches; exit status 1 on any mismatch.
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
#include "curve.h"

using namespace tpst;

template <class F>
static bool same(const Xyzz<F>& a, const Xyzz<F>& b) {
  return !memcmp(a.X.v, b.X.v, sizeof a.X.v) && !memcmp(a.Y.v, b.Y.v, sizeof a.Y.v) &&
         !memcmp(a.ZZ.v, b.ZZ.v, sizeof a.ZZ.v) && !memcmp(a.ZZZ.v, b.ZZZ.v, sizeof a.ZZZ.v);
}

int main() {
  int32_t n;
  if (fread(&n, 4, 1, stdin) != 1 || n <= 0) return 2;
  std::vector<uint32_t> p(48 * (size_t)n), q(48 * (size_t)n);
  if (fread(p.data(), 4, p.size(), stdin) != p.size() || fread(q.data(), 4, q.size(), stdin) != q.size()) return 2;
  int fq_bad = 0, f29_bad = 0;
  for (int i = 0; i < n; i++) {
    const uint32_t *pw = &p[48 * (size_t)i], *qw = &q[48 * (size_t)i];
    const Xyzz<Fq> a = {Fq::from_limbs(pw), Fq::from_limbs(pw + 12), Fq::from_limbs(pw + 24), Fq::from_limbs(pw + 36)};
    const Affine<Fq> b = {Fq::from_limbs(qw), Fq::from_limbs(qw + 12)};
    if (!is_zero(a.ZZ) && !(eq(a.ZZ, Fq::one()) && eq(a.ZZZ, Fq::one()))) return 3;
    if (!same(add_affine(a, b), add_affine_unit(a, b))) {
      if (fq_bad++ < 5) fprintf(stderr, "fq mismatch at pair %d\n", i);
    }
    const Xyzz<Fq29> a29 = {from_std(a.X), from_std(a.Y), from_std(a.ZZ), from_std(a.ZZZ)};
    const Affine<Fq29> b29 = {from_std(b.x), from_std(b.y)};
    if (!is_zero(a29.ZZ) && !(eq(a29.ZZ, Fq29::one()) && eq(a29.ZZZ, Fq29::one()))) return 3;
    if (!same(add_affine(a29, b29), add_affine_unit(a29, b29))) {
      if (f29_bad++ < 5) fprintf(stderr, "fq29 mismatch at pair %d\n", i);
    }
  }
  printf("pairs %d fq_bad %d fq29_bad %d\n", n, fq_bad, f29_bad);
  return fq_bad || f29_bad ? 1 : 0;
}
