// How many parked pieces the short-chunk fixup owes a bucket, and the class
// the fixup's visiting order sorts it into.  Host and device (a stand-alone
// host test includes this header alone).
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
