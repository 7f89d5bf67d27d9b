// bloom_tree.hip — where the reference's buffer flushes: the cut points of an
// op stream, found on the device for the whole batch (bloomhip_flush_cuts).
//
// Reference: Buffer::put (src/buffer.cpp:37-58) replaces the value of a key it
// holds and refuses once it holds max_size distinct keys, even a key it holds
// (:42); LSMTree::put (src/lsm_tree.cpp:104-139) then flushes and puts the
// refused op into the empty buffer.  A segment therefore ends right after the
// op that brought its B-th distinct key, and the cut is realised only when
// another op follows.
//
// On the GPU, three steps.
//   k_cut_records  rec[i] = {key_i, i}; the caller sorts them stably on the
//                  key with the batched PUT's radix sort (bloom_flush.hip).
//   k_cut_links    neighbours in sorted order with one key are consecutive
//                  ops on that key: prev[i] = the index of the previous op
//                  with op i's key, kTreeCutNone without one.
//   k_cut_walk     op i brings a new distinct key to the segment that starts
//                  at s iff prev[i] is none or < s.  Segments depend on each
//                  other in sequence, so one workgroup walks the stream: per
//                  step a chunk of kTreeCutChunk ops, one op per lane, the
//                  flags counted by ballot per wave and summed over the waves
//                  through LDS.  Below B new keys the walk moves to the next
//                  chunk; otherwise the lane holding the B-th new key is found
//                  by its rank in the ballot, cut = its index + 1, and the
//                  chunk is counted again for the segment that starts at the
//                  cut.  Every step moves on a chunk or records a cut: no
//                  waiting on another workgroup.
// An index read from memory is clamped before it is an address; a key never
// is one.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "bloom_tree.h"

namespace bloomhip {
namespace {

constexpr int kCutWaves = kTreeCutChunk / 64;
constexpr int kCutGroup = 8;  // chunks whose links are loaded together
static_assert(kTreeCutChunk % 64 == 0 && kTreeCutChunk <= 1024, "one op per lane of one workgroup");

__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__global__ void __launch_bounds__(256) k_cut_records(const uint2 *__restrict__ ops, uint32_t n,
                                                     uint2 *__restrict__ rec) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
        rec[i] = make_uint2(ops[i].x, (uint32_t)i);
}

__global__ void __launch_bounds__(256) k_cut_links(const uint2 *__restrict__ sorted, uint32_t n,
                                                   uint32_t *__restrict__ prev) {
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (uint64_t)gridDim.x * 256) {
        const uint2 cur = sorted[j];
        uint32_t p = kTreeCutNone;
        if (j > 0) {
            const uint2 before = sorted[j - 1];
            // stable sort: equal keys keep arrival order, so before.y < cur.y
            if (before.x == cur.x && before.y < cur.y) p = before.y;
        }
        if (cur.y < n) prev[cur.y] = p;
    }
}

// One workgroup of kTreeCutChunk lanes.  Chunks lie on a fixed grid (p a
// multiple of kTreeCutChunk).  The links of kCutGroup chunks are loaded
// together into a register each, so the walk meets the memory latency once per
// group, not once per chunk.  A cut inside a chunk moves the segment start s
// and the same chunk is counted again from s on, out of the same register:
// nothing is loaded twice.  Every step either moves to the next chunk or
// records a cut past s, so the walk ends after at most n / kTreeCutChunk +
// ncuts + 1 steps.  Uniform state (s, p, count, ncuts) is kept by every lane;
// the LDS wave counts are double-buffered by step parity, so a wave writing
// step k + 2's counts has passed step k + 1's barrier, which every wave
// reaches only after reading step k's.
__global__ void __launch_bounds__(kTreeCutChunk) k_cut_walk(const uint32_t *__restrict__ prev,
                                                           uint32_t n, uint32_t B,
                                                           uint32_t *__restrict__ cuts, uint32_t cap,
                                                           uint32_t *__restrict__ count_out) {
    __shared__ uint32_t s_cnt[2][kCutWaves];
    __shared__ uint32_t s_cut;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t s = 0, count = 0, ncuts = 0, parity = 0;
    uint64_t p = 0;  // 64-bit: p + kCutGroup * kTreeCutChunk passes 2^32 for the largest n
    // the index clamped into the stream; a link past the end is never used:
    // its op fails i < n
    auto link_at = [&](uint64_t base) -> uint32_t {
        const uint64_t i = base + threadIdx.x;
        return prev[i < n ? i : n - 1];
    };
    if (threadIdx.x == 0) s_cut = 0;  // ordered before any cut's store by the step's first barrier
    // One chunk, its links in `slot`: its cuts, then on to the next chunk.
    // Returns false when the walk is over.
    auto chunk = [&](const uint32_t slot) -> bool {
        if (p >= n) return false;
        const uint64_t i = p + threadIdx.x;
        for (;;) {
            // op i brings a new key to the segment [s, ..): no earlier op on its key, or one before s
            const bool fresh = i < n && i >= s && (slot == kTreeCutNone || slot < s);
            const uint64_t m = __ballot(fresh);
            if (lane == 0) s_cnt[parity][wave] = (uint32_t)__popcll(m);
            __syncthreads();
            uint32_t below = 0, total = 0;
#pragma unroll
            for (uint32_t w = 0; w < (uint32_t)kCutWaves; w++) {
                const uint32_t t = s_cnt[parity][w];
                if (w < wave) below += t;
                total += t;
            }
            parity ^= 1;
            if (count + total < B) {  // uniform: the buffer is not full after this chunk
                count += total;
                break;
            }
            // the B-th new key of the segment is new key number `want` of this chunk
            const uint32_t want = B - count;  // 1 <= want <= total
            if (fresh && below + lanes_below(m) + 1 == want) s_cut = (uint32_t)i + 1;
            __syncthreads();
            const uint32_t cut = s_cut;  // s < cut <= n
            if (cut >= n || cut <= s) return false;  // the stream ends on a full buffer: no flush
            if (threadIdx.x == 0 && ncuts < cap) cuts[ncuts] = cut;
            ncuts++;
            s = cut;  // the same chunk again, from the cut on
            count = 0;
        }
        p += kTreeCutChunk;
        return true;
    };
    for (bool more = true; more;) {
        uint32_t links[kCutGroup];
#pragma unroll
        for (int j = 0; j < kCutGroup; j++) links[j] = link_at(p + (uint64_t)j * kTreeCutChunk);
#pragma unroll
        for (int j = 0; j < kCutGroup; j++)
            if (more) more = chunk(links[j]);
    }
    if (threadIdx.x == 0) *count_out = ncuts;
}

}  // namespace

uint64_t cut_workspace_words(uint64_t n, uint64_t B) { return n + 2 + cut_max_cuts(n, B); }

hipError_t launch_cut_records(const void *ops, uint64_t n, void *rec, hipStream_t stream) {
    if (n == 0 || n >= 0xFFFFFFFFull) return hipErrorInvalidValue;
    const uint64_t blocks = std::min<uint64_t>((n + 255) / 256, 4096);
    k_cut_records<<<(unsigned)blocks, 256, 0, stream>>>(reinterpret_cast<const uint2 *>(ops),
                                                        (uint32_t)n, reinterpret_cast<uint2 *>(rec));
    return hipGetLastError();
}

hipError_t launch_cut_links(const void *sorted, uint64_t n, uint32_t *prev, hipStream_t stream) {
    if (n == 0 || n >= 0xFFFFFFFFull) return hipErrorInvalidValue;
    const uint64_t blocks = std::min<uint64_t>((n + 255) / 256, 4096);
    k_cut_links<<<(unsigned)blocks, 256, 0, stream>>>(reinterpret_cast<const uint2 *>(sorted),
                                                      (uint32_t)n, prev);
    return hipGetLastError();
}

hipError_t launch_cut_walk(const uint32_t *prev, uint64_t n, uint64_t B, uint32_t *cuts,
                           uint32_t cap, uint32_t *count, hipStream_t stream) {
    if (B == 0 || n <= B || n >= 0xFFFFFFFFull) return hipErrorInvalidValue;
    k_cut_walk<<<1, kTreeCutChunk, 0, stream>>>(prev, (uint32_t)n, (uint32_t)B, cuts, cap, count);
    return hipGetLastError();
}

}  // namespace bloomhip
