// bloom_range.hip — the batched RANGE: newest-wins range scans over the runs.
//
// Reference: LSMTree::range (src/lsm_tree.cpp:218-290) collects Buffer::range
// and every Run::range (src/run.cpp:115-157) of the bounds [start, end), merges
// them with MergeContext precedence (the newest run's entry of a key wins,
// src/merge.cpp) and drops tombstones (:273-279); end <= start answers nothing
// (:226-229).
//
// On the GPU, for many queries at once: k_range_bounds finds each query's
// sub-range [lo, lo + len) of every run (the page from the fences, then the
// halving search inside the fence interval: the chain k_get_resolve uses; a
// run without fences is searched whole) and sorts the queries into three
// classes by their candidate count.  k_range_merge gives the short ones to
// one wave or one workgroup each: the sub-ranges staged in LDS back to back,
// every element ranked in (key, run) order by binary searches in the other
// runs' shares, duplicates of a newer run and tombstones dropped, the kept
// ones placed by a block scan.  It runs twice, once for the counts and, after
// k_range_scan has turned them into offsets, once to write.  The long queries
// are compactions of their sub-ranges (bloom_merge.hip, driven from
// bloom_capi.cpp) and are copied to their offsets by k_range_copy_large.
//
// (Run::range maps num_pages * 4096 BYTES at byte offset page * 4096 while
// the fences sit every 4096 ENTRIES, src/run.cpp:164: past 512 entries it
// scans the wrong place.  Here every entry of the run inside the bounds
// counts)
#include "bloom_range.h"

#include <algorithm>

#include "bloom_combine.h"  // route_page
#include "bloom_search.h"   // halving_search, floor_pow2

namespace bloomhip {
namespace {

constexpr int kBoundsBlock = 256;
constexpr int32_t kTombstone = INT32_MIN;  // VAL_TOMBSTONE, src/types.h:12

__device__ __forceinline__ uint32_t lane_id() {
    return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}

// The number of entries of run r with key < x (lower_bound), in [0, nent].
// x == INT32_MIN: none.  Otherwise the entries with key <= k = x - 1: the page
// of k from the fences, then the largest entry <= k of that fence interval,
// every index clamped as k_get_resolve clamps it.
template <bool LDS_FENCES>
__device__ __forceinline__ uint64_t range_lower_bound(const int2 *__restrict__ ent, uint64_t nent,
                                                      const int32_t *fz, int nf, float f0,
                                                      float scale, int32_t x) {
    if (x == INT32_MIN || nent == 0) return 0;
    const int32_t k = x - 1;
    if (nf > 0) {
        if (fz[0] > k) return 0;
        int pg;
        if constexpr (LDS_FENCES) {
            pg = route_page(fz, nf, k, f0, scale);
        } else {
            int l = 1, h = nf;  // upper_bound; k >= fences[0]
            while (l < h) {
                const int mid = (l + h) >> 1;
                if (fz[mid] <= k) l = mid + 1;
                else h = mid;
            }
            pg = l - 1;
        }
        pg = max(pg, 0);
        const uint64_t base = min((uint64_t)pg * kFenceStride, (nent - 1) & ~(kFenceStride - 1ull));
        const uint32_t len = (uint32_t)min((uint64_t)kFenceStride, nent - base);
        const int2 *p = ent + base;
        int2 best = p[0];
        uint32_t pos = 0;
        halving_search(p, pos, len, len > 1 ? floor_pow2(len - 1) : 0, k, best);
        // p[0] is the page's fence, <= k; entries that disagree with their
        // fences: nothing of this interval counts
        return best.x <= k ? base + pos + 1 : base;
    }
    if (ent[0].x > k) return 0;
    if (nent <= 0xFFFFFFFFull) {
        const uint32_t len = (uint32_t)nent;
        int2 best = ent[0];
        uint32_t pos = 0;
        halving_search(ent, pos, len, len > 1 ? floor_pow2(len - 1) : 0, k, best);
        return (uint64_t)pos + 1;
    }
    uint64_t l = 1, h = nent;  // ent[0] <= k
    while (l < h) {
        const uint64_t mid = (l + h) >> 1;
        if (ent[mid].x <= k) l = mid + 1;
        else h = mid;
    }
    return l;
}

// One lane per (query, run): a workgroup takes qpb = 256 / nruns queries per
// step, lane t the run t % nruns of query t / nruns.  The lens meet in LDS,
// lane t < qpb sums query t's, and the lanes of a wave that hold queries of
// one class append them to its list with one atomic per wave.  Persistent
// workgroups: the fences are staged once.
template <bool LDS_FENCES>
__global__ void __launch_bounds__(kBoundsBlock) k_range_bounds(
    RangeRuns R, const int32_t *__restrict__ starts, const int32_t *__restrict__ ends, uint64_t nq,
    int force_large, uint64_t *__restrict__ lo_out, uint32_t *__restrict__ len_out,
    uint64_t *__restrict__ ub_out, uint64_t *__restrict__ counts, RangeLists L) {
    extern __shared__ int32_t s_fences[];
    __shared__ uint32_t s_len[kBoundsBlock];
    __shared__ float s_f0[kMaxRouteRuns], s_scale[kMaxRouteRuns];
    const int nruns = R.nruns;
    for (int r = threadIdx.x; r < nruns; r += kBoundsBlock) {
        const uint32_t nf = R.nfences[r];
        const int32_t f0 = nf ? R.meta[r][1] : 0, fl = nf ? R.meta[r][nf] : 0;
        s_f0[r] = (float)f0;
        s_scale[r] = (nf > 1 && fl > f0) ? (float)(nf - 1) / ((float)fl - (float)f0) : 0.0f;
    }
    if constexpr (LDS_FENCES) {
        for (int r = 0; r < nruns; r++) {
            const uint32_t nf = R.nfences[r];
            const int32_t *src = R.meta[r] + 1;
            int32_t *dst = s_fences + R.fence_off[r];
            for (uint32_t i = threadIdx.x; i < nf; i += kBoundsBlock) dst[i] = src[i];
        }
    }
    __syncthreads();
    const uint32_t qpb = kBoundsBlock / (uint32_t)nruns;
    const uint32_t ql = threadIdx.x / (uint32_t)nruns;
    const int r = (int)(threadIdx.x - ql * (uint32_t)nruns);
    const uint64_t tiles = (nq + qpb - 1) / qpb;
    const int2 *ent = reinterpret_cast<const int2 *>(R.entries[r]);
    const uint64_t nent = R.nentries[r];
    const int nf = (int)R.nfences[r];
    const int32_t *fz;
    if constexpr (LDS_FENCES) fz = s_fences + R.fence_off[r];
    else fz = R.meta[r] + 1;  // only read when nf > 0
    const float f0 = s_f0[r], scale = s_scale[r];
    const uint32_t lane = lane_id();
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t q = tile * qpb + ql;
        const bool active = ql < qpb && q < nq;
        uint32_t len32 = 0;
        if (active) {
            const int32_t st = starts[q], en = ends[q];
            uint64_t lo = 0, len = 0;
            if (en > st) {
                lo = min(range_lower_bound<LDS_FENCES>(ent, nent, fz, nf, f0, scale, st), nent);
                const uint64_t hi =
                    min(range_lower_bound<LDS_FENCES>(ent, nent, fz, nf, f0, scale, en), nent);
                len = hi > lo ? hi - lo : 0;
            }
            len32 = (uint32_t)min(len, (uint64_t)0xFFFFFFFFull);
            lo_out[q * (uint64_t)nruns + r] = lo;
            len_out[q * (uint64_t)nruns + r] = len32;
        }
        s_len[threadIdx.x] = len32;
        __syncthreads();
        const uint64_t q2 = tile * qpb + threadIdx.x;
        int cls = -1;
        if (threadIdx.x < qpb && q2 < nq) {
            uint64_t ub = 0;
            for (int j = 0; j < nruns; j++) ub += s_len[threadIdx.x * nruns + j];
            ub_out[q2] = ub;
            counts[q2] = 0;
            if (ub) cls = (force_large || ub > kRangeBlockCap) ? RANGE_LARGE
                          : ub > kRangeWaveCap                 ? RANGE_BLOCK
                                                               : RANGE_WAVE;
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const uint64_t mask = __ballot(cls == c);
            if (mask == 0) continue;  // wave-uniform
            const int leader = __ffsll((unsigned long long)mask) - 1;
            uint32_t base = 0;
            if ((int)lane == leader) base = atomicAdd(L.count + c, (uint32_t)__popcll(mask));
            base = __shfl(base, leader, 64);
            if (cls == c) L.list[c][base + __popcll(mask & ((1ull << lane) - 1ull))] = (uint32_t)q2;
        }
        __syncthreads();  // s_len is rewritten by the next step
    }
}

// The first index of the sorted LDS share p[0 .. n) whose key is >= k (UPPER:
// > k).
template <bool UPPER>
__device__ __forceinline__ uint32_t lds_bound(const int2 *p, uint32_t n, int32_t k) {
    uint32_t l = 0, h = n;
    while (l < h) {
        const uint32_t mid = (l + h) >> 1;
        const int32_t v = p[mid].x;
        if (UPPER ? v <= k : v < k) l = mid + 1;
        else h = mid;
    }
    return l;
}

template <int BLOCK>
__device__ __forceinline__ uint32_t range_block_scan(uint32_t v, uint32_t *s_w, uint32_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t base = 0, all = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; w++) {
        if (w < wave) base += s_w[w];
        all += s_w[w];
    }
    __syncthreads();
    *total = all;
    return base + incl - v;
}

// One workgroup per listed query, looping over the list.  Phases, a
// __syncthreads() between each two:
//   0  wave 0 packs the query's non-empty sub-ranges: share c of the LDS
//      image is s_ent[s_start[c] .. s_start[c + 1]), shares in run order
//      (newest first);
//   A  the shares are staged, s_perm cleared;
//   B  element (c, i) with key k gets its rank in (key, run) order: i, plus
//      upper_bound(k) in every newer share, plus lower_bound(k) in every older
//      one; it is a duplicate when a newer share holds k; kept elements store
//      their LDS index at s_perm[rank];
//   C  lane t owns ranks 8t .. 8t + 7; a block scan of the lanes' kept counts
//      places them.  WRITE = false stores the query's count; WRITE = true
//      stores the entries at out + offsets[q] + place.
// Entries that break the contract (keys not strictly ascending) can make
// ranks collide: s_perm then misses elements, never points outside the image
// (cleared to kNoElem, checked < ub), and the write pass never leaves the
// query's slice of out (place < offsets[q + 1] - offsets[q]).
template <int BLOCK, bool WRITE>
__global__ void __launch_bounds__(BLOCK) k_range_merge(
    RangeRuns R, const uint32_t *__restrict__ list, uint32_t nlist,
    const uint64_t *__restrict__ lo, const uint32_t *__restrict__ len,
    uint64_t *__restrict__ counts, int2 *__restrict__ out) {
    constexpr uint32_t CAP = BLOCK * kRangePerLane;
    constexpr uint16_t kNoElem = 0xFFFF;
    static_assert(CAP < kNoElem, "LDS indices are u16");
    __shared__ int2 s_ent[CAP];
    __shared__ uint16_t s_perm[CAP];
    __shared__ uint32_t s_start[kMaxRouteRuns + 1];
    __shared__ const int2 *s_ptr[kMaxRouteRuns];
    __shared__ uint32_t s_w[BLOCK / 64];
    __shared__ uint32_t s_nne;
    const int nruns = R.nruns;
    // the share that holds LDS index j: the largest c with s_start[c] <= j
    auto share_of = [&](uint32_t j, uint32_t nne) -> uint32_t {
        uint32_t l = 0, h = nne;  // answer in [l, h)
        while (h - l > 1) {
            const uint32_t mid = (l + h) >> 1;
            if (s_start[mid] <= j) l = mid;
            else h = mid;
        }
        return l;
    };
    for (uint32_t it = blockIdx.x; it < nlist; it += gridDim.x) {
        const uint32_t q = list[it];
        if (threadIdx.x < 64) {
            const int r = (int)threadIdx.x;
            const uint64_t row = (uint64_t)q * (uint64_t)nruns;
            const uint32_t l = r < nruns ? len[row + r] : 0u;
            const uint64_t mask = __ballot(l > 0);
            const uint32_t c = (uint32_t)__popcll(mask & ((1ull << r) - 1ull));
            uint32_t incl = l;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t o = __shfl_up(incl, off, 64);
                if (r >= off) incl += o;
            }
            if (l > 0) {
                s_start[c] = min(incl - l, CAP);
                s_ptr[c] = reinterpret_cast<const int2 *>(R.entries[r]) + lo[row + r];
            }
            if (r == 63) {
                s_start[__popcll(mask)] = min(incl, CAP);  // ub <= CAP by the query's class
                s_nne = (uint32_t)__popcll(mask);
            }
        }
        __syncthreads();
        const uint32_t nne = s_nne;
        const uint32_t ub = s_start[nne];
        for (uint32_t j = threadIdx.x; j < ub; j += BLOCK) {
            const uint32_t c = share_of(j, nne);
            s_ent[j] = s_ptr[c][j - s_start[c]];
            s_perm[j] = kNoElem;
        }
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < ub; j += BLOCK) {
            const uint32_t c = share_of(j, nne);
            const int2 e = s_ent[j];
            uint32_t rank = j - s_start[c];
            bool dup = false;
            for (uint32_t c2 = 0; c2 < nne; c2++) {
                if (c2 == c) continue;
                const uint32_t a = s_start[c2], n2 = s_start[c2 + 1] - a;
                if (c2 < c) {
                    const uint32_t u = lds_bound<true>(s_ent + a, n2, e.x);
                    dup = dup || (u > 0 && s_ent[a + u - 1].x == e.x);
                    rank += u;
                } else {
                    rank += lds_bound<false>(s_ent + a, n2, e.x);
                }
            }
            if (!dup && e.y != kTombstone) s_perm[min(rank, ub - 1)] = (uint16_t)j;
        }
        __syncthreads();
        uint16_t p[kRangePerLane];
        uint32_t cnt = 0;
#pragma unroll
        for (int k = 0; k < kRangePerLane; k++) {
            const uint32_t rho = threadIdx.x * kRangePerLane + k;
            p[k] = rho < ub ? s_perm[rho] : kNoElem;
            cnt += p[k] < ub;
        }
        uint32_t total;
        uint32_t place = range_block_scan<BLOCK>(cnt, s_w, &total);
        if constexpr (WRITE) {
            const uint64_t off = counts[q];
            const uint64_t room = counts[q + 1] - off;
#pragma unroll
            for (int k = 0; k < kRangePerLane; k++) {
                if (p[k] < ub && place < room) out[off + place++] = s_ent[p[k]];
            }
        } else {
            if (threadIdx.x == 0) counts[q] = total;
        }
        __syncthreads();  // the LDS image is rebuilt by the next query
    }
}

// Exclusive scan of counts[0 .. n) in place by one workgroup, kScanItems
// consecutive values per lane and step; the total lands in counts[n].
constexpr int kScanBlock = 1024;
constexpr int kScanItems = 4;

__global__ void __launch_bounds__(kScanBlock) k_range_scan(uint64_t *__restrict__ counts, uint64_t n) {
    __shared__ uint64_t s_w[kScanBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t carry = 0;
    for (uint64_t b0 = 0; b0 < n; b0 += (uint64_t)kScanBlock * kScanItems) {
        const uint64_t i0 = b0 + (uint64_t)threadIdx.x * kScanItems;
        uint64_t v[kScanItems], sum = 0;
#pragma unroll
        for (int k = 0; k < kScanItems; k++) {
            v[k] = i0 + k < n ? counts[i0 + k] : 0ull;
            sum += v[k];
        }
        uint64_t incl = sum;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint64_t o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        if (lane == 63) s_w[wave] = incl;
        __syncthreads();
        uint64_t base = 0, all = 0;
#pragma unroll
        for (int w = 0; w < kScanBlock / 64; w++) {
            if (w < wave) base += s_w[w];
            all += s_w[w];
        }
        __syncthreads();
        uint64_t run = carry + base + incl - sum;
#pragma unroll
        for (int k = 0; k < kScanItems; k++) {
            if (i0 + k < n) counts[i0 + k] = run;
            run += v[k];
        }
        carry += all;
    }
    if (threadIdx.x == 0) counts[n] = carry;
}

__global__ void k_range_gather(const uint32_t *__restrict__ list, uint32_t n, int nruns,
                               const uint64_t *__restrict__ lo, const uint32_t *__restrict__ len,
                               const uint64_t *__restrict__ ub, uint64_t *__restrict__ lo_rows,
                               uint32_t *__restrict__ len_rows, uint64_t *__restrict__ ub_rows) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint64_t)n * (uint64_t)nruns) return;
    const uint64_t i = t / (uint64_t)nruns, r = t - i * (uint64_t)nruns;
    const uint64_t q = list[i];
    lo_rows[t] = lo[q * (uint64_t)nruns + r];
    len_rows[t] = len[q * (uint64_t)nruns + r];
    if (r == 0) ub_rows[i] = ub[q];
}

__global__ void k_range_set_counts(const uint32_t *__restrict__ list, uint32_t n,
                                   const uint64_t *__restrict__ kept, uint64_t *__restrict__ counts) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) counts[list[i]] = kept[i];
}

// Large query i's compacted slice, scratch[slice_off[i] ..), to its place.
__global__ void __launch_bounds__(256) k_range_copy_large(
    const uint32_t *__restrict__ list, uint32_t n, const uint64_t *__restrict__ slice_off,
    const uint64_t *__restrict__ offsets, const int2 *__restrict__ scratch, int2 *__restrict__ out) {
    for (uint32_t i = blockIdx.y; i < n; i += gridDim.y) {
        const uint64_t q = list[i];
        const uint64_t off = offsets[q], cnt = offsets[q + 1] - off;
        const int2 *src = scratch + slice_off[i];
        for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < cnt; j += (uint64_t)gridDim.x * 256)
            out[off + j] = src[j];
    }
}

}  // namespace

hipError_t launch_range_bounds(const RangeRuns &R, const int32_t *starts, const int32_t *ends,
                               uint64_t nq, bool force_large, uint64_t *lo, uint32_t *len,
                               uint64_t *ub, uint64_t *counts, const RangeLists &L,
                               hipStream_t stream) {
    if (nq == 0) return hipSuccess;
    if (R.nruns < 1 || R.nruns > kMaxRouteRuns) return hipErrorInvalidValue;
    const size_t lds = (size_t)R.total_fences * 4;
    const bool in_lds = lds <= kRouteLdsFenceBytesMax;
    const size_t per_block = (in_lds ? lds : 0) + 2048;
    int per_cu = (int)(kLdsBitmapBytes / per_block);
    per_cu = per_cu < 1 ? 1 : per_cu > 8 ? 8 : per_cu;  // 8 x 256 threads = 32 waves per CU
    const uint64_t qpb = (uint64_t)kBoundsBlock / (uint64_t)R.nruns;
    const uint64_t tiles = (nq + qpb - 1) / qpb;
    const unsigned grid = (unsigned)std::min<uint64_t>(tiles, (uint64_t)device_cu_count() * per_cu);
    if (in_lds)
        k_range_bounds<true><<<grid, kBoundsBlock, lds, stream>>>(R, starts, ends, nq, force_large ? 1 : 0,
                                                                  lo, len, ub, counts, L);
    else
        k_range_bounds<false><<<grid, kBoundsBlock, 0, stream>>>(R, starts, ends, nq, force_large ? 1 : 0,
                                                                 lo, len, ub, counts, L);
    return hipGetLastError();
}

hipError_t launch_range_merge(const RangeRuns &R, int cls, const uint32_t *list, uint32_t n,
                              const uint64_t *lo, const uint32_t *len, uint64_t *counts, void *out,
                              hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (cls != RANGE_WAVE && cls != RANGE_BLOCK) return hipErrorInvalidValue;
    int2 *o = reinterpret_cast<int2 *>(out);
    // what the chip holds at once: 32 waves per CU, within its LDS
    const unsigned cus = (unsigned)device_cu_count();
    if (cls == RANGE_WAVE) {
        const unsigned grid = std::min<unsigned>(n, cus * 24);  // ~5.5 KiB of LDS each
        if (o) k_range_merge<64, true><<<grid, 64, 0, stream>>>(R, list, n, lo, len, counts, o);
        else k_range_merge<64, false><<<grid, 64, 0, stream>>>(R, list, n, lo, len, counts, o);
    } else {
        const unsigned grid = std::min<unsigned>(n, cus * 7);  // ~21 KiB of LDS each
        if (o) k_range_merge<256, true><<<grid, 256, 0, stream>>>(R, list, n, lo, len, counts, o);
        else k_range_merge<256, false><<<grid, 256, 0, stream>>>(R, list, n, lo, len, counts, o);
    }
    return hipGetLastError();
}

hipError_t launch_range_scan(uint64_t *counts, uint64_t nq, hipStream_t stream) {
    k_range_scan<<<1, kScanBlock, 0, stream>>>(counts, nq);
    return hipGetLastError();
}

hipError_t launch_range_gather(const uint32_t *list, uint32_t n, int nruns, const uint64_t *lo,
                               const uint32_t *len, const uint64_t *ub, uint64_t *lo_rows,
                               uint32_t *len_rows, uint64_t *ub_rows, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint64_t t = (uint64_t)n * (uint64_t)nruns;
    k_range_gather<<<(unsigned)((t + 255) / 256), 256, 0, stream>>>(list, n, nruns, lo, len, ub, lo_rows,
                                                                    len_rows, ub_rows);
    return hipGetLastError();
}

hipError_t launch_range_set_counts(const uint32_t *list, uint32_t n, const uint64_t *kept,
                                   uint64_t *counts, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    k_range_set_counts<<<(n + 255) / 256, 256, 0, stream>>>(list, n, kept, counts);
    return hipGetLastError();
}

hipError_t launch_range_copy_large(const uint32_t *list, uint32_t n, const uint64_t *slice_off,
                                   const uint64_t *offsets, const void *scratch, void *out,
                                   hipStream_t stream) {
    if (n == 0) return hipSuccess;
    // a query's blocks along x (a large query has > kRangeBlockCap candidates;
    // its kept entries may be few), the queries along y
    const unsigned gx = std::max(1u, std::min(64u, (unsigned)device_cu_count() * 4 / n));
    const dim3 grid(gx, std::min(n, 65535u));
    k_range_copy_large<<<grid, 256, 0, stream>>>(list, n, slice_off, offsets,
                                                  reinterpret_cast<const int2 *>(scratch),
                                                  reinterpret_cast<int2 *>(out));
    return hipGetLastError();
}

}  // namespace bloomhip
