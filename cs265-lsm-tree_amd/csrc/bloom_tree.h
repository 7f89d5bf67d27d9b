// bloom_tree.h — the flush cut points of an op stream (bloomhip_flush_cuts);
// see bloom_tree.hip.  The tree handle built on them is bloom_tree_host.cpp.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bloomhip {

// The walk takes the op stream in chunks of kTreeCutChunk ops, one op per lane
// of its single workgroup, on a fixed grid: chunk c is ops [c * kTreeCutChunk,
// (c + 1) * kTreeCutChunk).  bloomhip.TREE_CUT_CHUNK mirrors it.
constexpr uint32_t kTreeCutChunk = 1024;
constexpr uint32_t kTreeCutNone = 0xFFFFFFFFu;  // prev[i]: no earlier op on the key

// u32 words of workspace beside the sort's (bloom_flush.h): prev[n], the cut
// count, the cuts (at most (n - 1) / B of them).
uint64_t cut_workspace_words(uint64_t n, uint64_t B);
inline uint64_t cut_max_cuts(uint64_t n, uint64_t B) { return n > B ? (n - 1) / B : 0; }

// rec[i] = {key of ops[i], i}: the sort's input (the index rides in the value slot).
hipError_t launch_cut_records(const void *ops, uint64_t n, void *rec, hipStream_t stream);
// sorted: rec stably sorted on the key.  prev[i] = the index of the previous
// op with op i's key, kTreeCutNone when there is none.
hipError_t launch_cut_links(const void *sorted, uint64_t n, uint32_t *prev, hipStream_t stream);
// The walk: *count = the number of realised cuts, cuts[0..min(count, cap)) the
// cuts themselves, ascending.  B < n < 2^32 - 1.
hipError_t launch_cut_walk(const uint32_t *prev, uint64_t n, uint64_t B, uint32_t *cuts,
                           uint32_t cap, uint32_t *count, hipStream_t stream);

}  // namespace bloomhip
