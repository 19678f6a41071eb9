// decode_kbest_list.hpp — what the two k-list decoders (decode_kbest.hip: the K best derivations of a line;
// decode_pairs_kbest.hip: the K best alignments of a pair) share: the bound on K, a candidate's tag and the bisection that finds
// an arc's next candidate.  A list is K doubles, sorted non-increasing and padded with -inf; a candidate is (arc a, rank r of a's
// source list S) with value S[r] + w(a), and candidates are ordered by
//   value, descending; then arcs whose matched symbol is not epsilon before arcs whose matched symbol is; then arc id, ascending;
//   then r, ascending
// (decode_kbest.hip's header).  The tag packs the middle two keys: (0 matched, 1 epsilon) << 32 | arc id.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace carmel_hip {
constexpr uint32_t kMaxK = 1024;
constexpr uint64_t kEpsTag = 1ull << 32;  // a candidate's tag: (0 matched, 1 epsilon) << 32 | arc id

// the first rank r of the source list S (sorted, padded with -inf) whose candidate (S[r] + w, tag, r) comes after the candidate
// picked last, (vl, tagl, rl); K if none does.  "After" is monotone in r: S is non-increasing and so is S[r] + w.
__device__ inline uint32_t kb_next(const double* S, double w, uint32_t K, uint64_t tag, double vl, uint64_t tagl, uint32_t rl) {
  uint32_t lo = 0, hi = K;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    const double v = S[mid] + w;
    if (v < vl || (v == vl && (tag > tagl || (tag == tagl && mid > rl))))
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo;
}
}  // namespace carmel_hip
