// bloom_range.h — the batched RANGE (bloomhip_range_batch); see bloom_range.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bloom_kernels.h"  // kMaxRouteRuns, kFenceStride

namespace bloomhip {

// A query's candidate count ub = the entries of every run inside its bounds.
// Up to kRangeWaveCap candidates one wave merges them in LDS, up to
// kRangeBlockCap a workgroup of 256 does (kRangePerLane per lane: 4 KiB and
// 16 KiB of entries); above that the query is a compaction of its sub-ranges.
// bloomhip.RANGE_WAVE_CAP / RANGE_BLOCK_CAP mirror the two.
constexpr int kRangePerLane = 8;
constexpr uint32_t kRangeWaveCap = 512;
constexpr uint32_t kRangeBlockCap = 2048;
static_assert(kRangeWaveCap == 64 * kRangePerLane && kRangeBlockCap == 256 * kRangePerLane,
              "the caps are the merge kernels' block sizes times kRangePerLane");

// The runs of a RANGE call: entries on the device (keys strictly ascending),
// and the fences of the runs that have them (meta[r][0] = max key, meta[r][1
// ..] = the fences; nfences[r] == 0: the run is searched whole).
struct RangeRuns {
    const void *entries[kMaxRouteRuns];
    uint64_t nentries[kMaxRouteRuns];
    const int32_t *meta[kMaxRouteRuns];
    uint32_t nfences[kMaxRouteRuns];
    uint32_t fence_off[kMaxRouteRuns];  // offset of run r's fences in the LDS copy
    uint32_t total_fences;
    int nruns;
};

// The three class lists (query indices, any order) and their lengths.
enum { RANGE_WAVE = 0, RANGE_BLOCK = 1, RANGE_LARGE = 2 };
struct RangeLists {
    uint32_t *list[3];  // nq u32 each
    uint32_t *count;    // 3 u32, zeroed before the bounds kernel
};

// k_range_bounds: per (query, run) lo = lower_bound(start), len =
// lower_bound(end) - lo (0 when end <= start; saturated at 2^32 - 1), row
// major [nq][nruns]; ub[q] = the sum of the query's lens; counts[q] = 0; q
// appended to its class list (none when ub == 0; the large list for every
// non-empty query when force_large).
hipError_t launch_range_bounds(const RangeRuns &R, const int32_t *starts, const int32_t *ends,
                               uint64_t nq, bool force_large, uint64_t *lo, uint32_t *len,
                               uint64_t *ub, uint64_t *counts, const RangeLists &L,
                               hipStream_t stream);

// k_range_merge over one class list (cls = RANGE_WAVE or RANGE_BLOCK, n
// queries).  out == nullptr: the count pass, counts[q] = the kept entries of
// query q.  Otherwise the write pass: counts holds the scanned offsets (nq + 1)
// and query q's entries go to out[counts[q] ..).
hipError_t launch_range_merge(const RangeRuns &R, int cls, const uint32_t *list, uint32_t n,
                              const uint64_t *lo, const uint32_t *len, uint64_t *counts, void *out,
                              hipStream_t stream);

// Exclusive scan of counts[0 .. nq) in place, the total in counts[nq].
hipError_t launch_range_scan(uint64_t *counts, uint64_t nq, hipStream_t stream);

// Large queries: rows of lo / len / ub gathered for the host (n_large x nruns,
// n_large), kept counts scattered into counts, and the compacted slices copied
// to their offsets.
hipError_t launch_range_gather(const uint32_t *list, uint32_t n, int nruns, const uint64_t *lo,
                               const uint32_t *len, const uint64_t *ub, uint64_t *lo_rows,
                               uint32_t *len_rows, uint64_t *ub_rows, hipStream_t stream);
hipError_t launch_range_set_counts(const uint32_t *list, uint32_t n, const uint64_t *kept,
                                   uint64_t *counts, hipStream_t stream);
hipError_t launch_range_copy_large(const uint32_t *list, uint32_t n, const uint64_t *slice_off,
                                   const uint64_t *offsets, const void *scratch, void *out,
                                   hipStream_t stream);

}  // namespace bloomhip
