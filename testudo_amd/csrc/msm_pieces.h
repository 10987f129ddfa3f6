// How many parked pieces the short-chunk fixup owes a bucket, and the class
// the fixup's visiting order sorts it into; the layout of a sorted K2 value
// and where the accumulation sends a run of entries.  Host and device
// (stand-alone host tests include this header alone).
#pragma once
#include <stdint.h>
#include "field.h"  // TPST_HD

namespace tpst {

// Buckets spanning more than LONG_PARTS chunks (many equal digits: small or
// boolean scalars put most entries of a window into one bucket) are not
// walked by one lane of the fixups -- 2^20 entries of one bucket would be a
// 32 768-add serial chain -- but appended to a per-group list and summed by
// k_bucket_fixup_long, one workgroup per bucket.
constexpr uint32_t LONG_PARTS = 64;

// Additions the fixup owes the bucket of sorted entries [s, e) under chunks of
// 2^lg entries: the trailing piece of its first chunk plus one leading piece
// per further chunk it reaches, t1 - t0 with t0 / t1 the chunks of its first /
// last entry.  0 for an empty bucket and for one inside a single chunk (the
// accumulation stored it itself); a bucket ending exactly on a chunk boundary
// does not reach the next chunk.
TPST_HD uint32_t fixup_pieces(uint32_t s, uint32_t e, int lg) { return e <= s ? 0u : ((e - 1) >> lg) - (s >> lg); }

// A value of the K2 bucket sort (msm_sort.h): the point's index (with GLV
// below 2 MSM_MAX_POINTS = 2^28), bit 31 set for the negated point, and, in
// the sorted array only, whether the entry is the first / the last of its
// bucket.  k_sort_bin sets the two flags on every value it writes, so the
// accumulation finds the ends of a bucket in the entries themselves instead of
// loading the bucket's bounds.
constexpr uint32_t VAL_SIGN = 1u << 31;
constexpr uint32_t VAL_FIRST = 1u << 30;
constexpr uint32_t VAL_LAST = 1u << 29;
constexpr uint32_t VAL_INDEX = (1u << 28) - 1;

// flags of the entry at position `rank` of a bucket of `count` sorted entries
TPST_HD uint32_t entry_flags(uint32_t rank, uint32_t count) {
  return (rank == 0 ? VAL_FIRST : 0u) | (rank + 1 == count ? VAL_LAST : 0u);
}

// The short-chunk accumulation walks its chunk in runs of one bucket's
// entries.  A run ends at the bucket's last entry or at the chunk's
// (chunk_last; a chunk clamped to its window group's entries ends at a
// bucket's end).  run_slot: where the sum of a run goes, from the values of
// its first and last entry -- a bucket lying wholly inside the chunk is stored
// to buckets[key] (RUN_BUCKET); otherwise the piece is parked in part[2t + 1]
// when the bucket starts in chunk t (its trailing piece) and in part[2t] when
// it began in an earlier chunk.
TPST_HD bool run_ends(uint32_t v, bool chunk_last) { return (v & VAL_LAST) != 0 || chunk_last; }
constexpr uint32_t RUN_BUCKET = 2;
TPST_HD uint32_t run_slot(uint32_t v_first, uint32_t v_last) {
  const bool starts = (v_first & VAL_FIRST) != 0, ends = (v_last & VAL_LAST) != 0;
  return starts && ends ? RUN_BUCKET : (starts ? 1u : 0u);
}

// Classes of the fixup's visiting order: 0 = nothing to do, 1 .. FIXUP_CAP =
// that many additions (FIXUP_CAP: that many or more, up to LONG_PARTS),
// FIXUP_LONG = the long list's.
constexpr uint32_t FIXUP_CAP = 8;
constexpr uint32_t FIXUP_LONG = FIXUP_CAP + 1;
constexpr uint32_t FIXUP_CLASSES = FIXUP_CAP + 1;  // 0 .. FIXUP_CAP: the ordered ones
TPST_HD uint32_t fixup_class(uint32_t pieces) {
  return pieces > LONG_PARTS ? FIXUP_LONG : (pieces < FIXUP_CAP ? pieces : FIXUP_CAP);
}

}  // namespace tpst
