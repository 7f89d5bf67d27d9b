// bloom_search.h — the searches over a run's entries that the batched GET
// (bloom_get.hip) and the batched RANGE (bloom_range.hip) share.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bloomhip {

// Largest power of two <= x (x >= 1).
__device__ __forceinline__ uint32_t floor_pow2(uint32_t x) { return 1u << (31 - __clz((int)x)); }

// The entry with the largest key <= k among p[pos .. pos + 2 * st0 - 1]
// (indices clamped below len), given that p[pos].key <= k: a branchless
// halving search, one dependent 8-byte read per step.  pos leaves as that
// entry's index and best as the entry; when no step is taken both stay as
// they came (best = p[pos] is the caller's to supply).
__device__ __forceinline__ void halving_search(const int2 *__restrict__ p, uint32_t &pos, uint32_t len,
                                               uint32_t st0, int32_t k, int2 &best) {
    for (uint32_t st = st0; st; st >>= 1) {
        const uint32_t c = pos + st;
        const int2 v = p[min(c, len - 1)];  // clamped: an index past the interval counts as > k
        const bool take = c < len && v.x <= k;
        pos = take ? c : pos;
        best = take ? v : best;
    }
}

}  // namespace bloomhip
