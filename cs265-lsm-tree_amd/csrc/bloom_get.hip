// bloom_get.hip — the batched GET past routing: from candidate runs to values.
//
// Reference: LSMTree::get past the buffer (src/lsm_tree.cpp:173-215) visits
// the runs newest first; Run::get (src/run.cpp:85-113) range-checks the key,
// asks the filter, finds the page with upper_bound over the fence pointers,
// reads it and searches it for the key.  A run that answers nullptr (a filter
// false positive) sends the search on to the next run; the first run that
// holds the key settles the GET, a tombstone included (:214).
//
// On the GPU: routing (k_route, or the stacked probe's combine with routing
// fused in) has left the range-checked candidate rows `cand`, bit i%64 of
// row r word i/64 = "Run::get would read a page of run r for key i".
// k_get_resolve walks each key's candidates in run order, finds the page from
// the fences (staged in LDS when they fit) and searches the fence interval
// [page * 4096, min((page + 1) * 4096, nentries)) of the run's entries in
// device memory.  (Run::get itself reads 4096 BYTES at byte offset page *
// 4096, src/run.cpp:101-103, while Run::put places a fence every 4096
// ENTRIES, :164: 512 entries at the wrong place for every page > 0.  The
// interval the fences describe is searched here)
#include "bloom_combine.h"  // route_page
#include "bloom_search.h"   // halving_search, floor_pow2

#include <algorithm>

namespace bloomhip {
namespace {

constexpr int kGetBlock = 256;
constexpr int32_t kGetNone = INT32_MIN;  // vals[i] when no run holds the key (= VAL_TOMBSTONE)
// The interpolated interval search looks in a window of kGetWindow entries
// around its guess: the rank of a key among the 4096 of a uniformly filled
// interval deviates from the straight line by at most sqrt(4096) / 2 = 32
// (one sigma), so +-128 is four sigma, and a wave of 64 lanes takes the exact
// fallback in under 1 % of its searches.
constexpr uint32_t kGetWindow = 256;

// One wave handles 64 consecutive keys per step, fetched one step ahead with
// the step's candidate words (lane r < nruns loads run r's word), as k_route
// does.  Each lane gathers its own nruns-bit candidate mask from the words
// (bit r = bit `lane` of lane r's word), then the wave loops while any lane
// has a candidate left and no answer: the lane takes its newest candidate
// run, finds the page, searches the fence interval, and either finishes or
// clears the bit (a false positive).  At most nruns rounds of at most 12
// dependent reads (13 loads with the interval's first entry, which is
// independent of them), twice that where an interpolation guess misses.
//
// Interval search: the chain of dependent reads at a random place of the
// run's entries is the cost (each one may miss every cache).  INTERP = false:
// a branchless binary search over the interval, 12 steps for 4096 entries.
// INTERP = true: a guess from the interval's two fences (the next fence, or
// the run's max key for its last interval) places a window of kGetWindow
// entries, and 8 halving steps search it; a result strictly inside the
// window proves itself (its neighbour above was read and is > k), a result
// at either end costs one more read to tell whether the answer lay outside,
// and then the binary search over the whole interval does.  Exact either way.
//
// Stats: per run, the wave's page reads and false reads are ballot popcounts
// accumulated by lane r; each wave adds its sums to the workgroup's LDS
// counters once, and the workgroup adds those to the global counters once.
template <int LAYOUT, bool LDS_FENCES, bool INTERP>
__global__ void __launch_bounds__(kGetBlock) k_get_resolve(
    KeySpan ks, RouteTable t, GetTable g, const uint64_t *__restrict__ cand, size_t nw,
    int32_t *__restrict__ vals, int32_t *__restrict__ found, unsigned long long *__restrict__ stats) {
    extern __shared__ int32_t s_fences[];
    __shared__ int32_t s_lo[kMaxRouteRuns], s_hi[kMaxRouteRuns];
    __shared__ uint32_t s_nf[kMaxRouteRuns], s_off[kMaxRouteRuns];
    __shared__ float s_scale[kMaxRouteRuns];
    __shared__ const int32_t *s_fz[kMaxRouteRuns];  // the run's fences in global memory
    __shared__ const int2 *s_ent[kMaxRouteRuns];
    __shared__ unsigned long long s_nent[kMaxRouteRuns];
    __shared__ unsigned long long s_stat[2 * kMaxRouteRuns];
    const int nruns = t.nruns;
    for (int r = threadIdx.x; r < nruns; r += kGetBlock) {
        const uint32_t nf = t.nfences[r];
        const int32_t f0 = nf ? t.meta[r][1] : 0, fl = nf ? t.meta[r][nf] : 0;
        s_hi[r] = nf ? t.meta[r][0] : INT32_MIN;
        s_lo[r] = nf ? f0 : INT32_MAX;
        s_nf[r] = nf;
        s_off[r] = t.fence_off[r];
        s_scale[r] = (nf > 1 && fl > f0) ? (float)(nf - 1) / ((float)fl - (float)f0) : 0.0f;
        s_fz[r] = t.meta[r] + 1;
        s_ent[r] = reinterpret_cast<const int2 *>(g.entries[r]);
        s_nent[r] = g.nentries[r];
        s_stat[2 * r] = s_stat[2 * r + 1] = 0;
    }
    if constexpr (LDS_FENCES) {
        constexpr int kBatch = 8;  // independent loads in flight per thread
        for (int r = 0; r < nruns; r++) {
            const uint32_t nf = t.nfences[r];
            const int32_t *src = t.meta[r] + 1;
            int32_t *dst = s_fences + t.fence_off[r];
            for (uint32_t b = 0; b < nf; b += kBatch * kGetBlock) {
                int32_t v[kBatch];
#pragma unroll
                for (int q = 0; q < kBatch; q++) {
                    const uint32_t i = b + q * kGetBlock + threadIdx.x;
                    v[q] = i < nf ? src[i] : 0;
                }
#pragma unroll
                for (int q = 0; q < kBatch; q++) {
                    const uint32_t i = b + q * kGetBlock + threadIdx.x;
                    if (i < nf) dst[i] = v[q];
                }
            }
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const size_t wstep = ((size_t)gridDim.x * kGetBlock) >> 6;
    size_t w = __builtin_amdgcn_readfirstlane(
        (uint32_t)(((size_t)blockIdx.x * kGetBlock + threadIdx.x) >> 6));
    // Unconditional (clamped) loads, as in k_route.
    auto load_key_at = [&](size_t ww) -> int32_t {
        const size_t i = min(min(ww, nw - 1) * 64 + lane, ks.n - 1);  // ks.n >= 1 here
        if constexpr (LAYOUT == KEYS_PACKED) return reinterpret_cast<const int32_t *>(ks.base)[i];
        else return load_key<LAYOUT>(ks, i);
    };
    auto load_cand_at = [&](size_t ww) -> uint64_t {
        return cand[(size_t)min(lane, nruns - 1) * nw + min(ww, nw - 1)];
    };
    unsigned long long acc_read = 0, acc_false = 0;  // lane r: run r's counts of this wave
    auto step = [&](size_t w, int32_t k, uint64_t cw) {
        const size_t i = w * 64 + lane;
        const bool valid = i < ks.n;
        uint64_t m0 = 0;  // this lane's candidate runs (bits past n are 0 in the rows)
        for (int r = 0; r < nruns; r++) {
            const uint32_t blo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)cw, r);
            const uint32_t bhi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(cw >> 32), r);
            const uint64_t word = ((uint64_t)bhi << 32) | blo;
            m0 |= ((word >> lane) & 1ull) << r;
        }
        if (!valid) m0 = 0;
        uint64_t m = m0;
        int32_t fr = -1, val = kGetNone;
        while (__ballot(m != 0) != 0) {  // at most nruns rounds: every round clears a bit or m
            if (m != 0) {
                const int r = __ffsll((unsigned long long)m) - 1;
                const int nf = (int)s_nf[r];  // >= 1: the run passed the range check
                const int32_t *fz;
                int pg;
                if constexpr (LDS_FENCES) {
                    fz = s_fences + s_off[r];
                    pg = route_page(fz, nf, k, (float)s_lo[r], s_scale[r]);
                } else {
                    fz = s_fz[r];
                    int l = 1, h = nf;  // upper_bound; k >= fences[0]
                    while (l < h) {
                        const int mid = (l + h) >> 1;
                        if (fz[mid] <= k) l = mid + 1;
                        else h = mid;
                    }
                    pg = l - 1;
                }
                pg = max(pg, 0);  // k >= fences[0] for a candidate; kept in range regardless
                const unsigned long long nent = s_nent[r];
                bool hit = false;
                if (nent) {
                    // every index stays in [0, nent): base is clamped to the
                    // last interval, offsets to the interval's length
                    const unsigned long long base =
                        min((unsigned long long)pg * kFenceStride, (nent - 1) & ~(kFenceStride - 1ull));
                    const uint32_t len = (uint32_t)min((unsigned long long)kFenceStride, nent - base);
                    const int2 *p = s_ent[r] + base;
                    int2 best;
                    uint32_t pos = 0;
                    bool ok = true;
                    if (INTERP && len > kGetWindow) {
                        // straight line from (0, fence[pg]) to (len, fence[pg + 1]), or to
                        // (len - 1, max key) in the run's last interval; differences
                        // in unsigned integers (exact), then float
                        const bool last = pg + 1 >= nf;
                        const int32_t f_lo = fz[min(pg, nf - 1)];
                        const int32_t f_hi = last ? s_hi[r] : fz[min(pg + 1, nf - 1)];
                        const float span = (float)((uint32_t)f_hi - (uint32_t)f_lo);
                        const float d = (float)((uint32_t)k - (uint32_t)f_lo);
                        const float cnt = (float)(last ? len - 1 : len);
                        const float gf = span > 0.0f ? d * cnt / span : 0.0f;
                        const uint32_t gi = (uint32_t)fminf(fmaxf(gf, 0.0f), (float)kFenceStride);
                        const uint32_t a = min(gi > kGetWindow / 2 ? gi - kGetWindow / 2 : 0u,
                                               len - kGetWindow);
                        // The answer is in the window [a, a + kGetWindow) iff p[a] <= k <
                        // p[a + kGetWindow].  Searched as if it were, the window gives
                        // an index strictly inside it whenever that holds with room to
                        // spare; only a result at either end needs a read to tell.
                        pos = a;
                        halving_search(p, pos, len, kGetWindow / 2, k, best);
                        if (pos == a) {  // no step taken: the window's first entry decides
                            best = p[a];
                            ok = a == 0 || best.x <= k;
                        } else if (pos == a + kGetWindow - 1 && a + kGetWindow < len) {
                            ok = p[a + kGetWindow].x > k;
                        }
                    } else {
                        best = p[0];
                        halving_search(p, pos, len, len > 1 ? floor_pow2(len - 1) : 0, k, best);
                    }
                    if (!ok) {  // the guess missed: binary search over the whole interval
                        pos = 0;
                        best = p[0];
                        halving_search(p, pos, len, floor_pow2(len - 1), k, best);
                    }
                    hit = best.x == k;
                    if (hit) val = best.y;
                }
                if (hit) {
                    fr = r;
                    m = 0;
                } else {
                    m &= m - 1;
                }
            }
        }
        if (valid) {
            if (vals) vals[i] = val;
            if (found) found[i] = fr;
        }
        if (stats) {
            // pages read: the candidates up to and including the run that answered
            const uint64_t rd = fr >= 0 ? m0 & ((2ull << fr) - 1ull) : m0;
            const uint64_t fl = fr >= 0 ? rd & ~(1ull << fr) : rd;
            for (int r = 0; r < nruns; r++) {
                const unsigned nr = (unsigned)__popcll(__ballot((rd >> r) & 1ull));
                const unsigned nfl = (unsigned)__popcll(__ballot((fl >> r) & 1ull));
                if (lane == r) {
                    acc_read += nr;
                    acc_false += nfl;
                }
            }
        }
    };
    int32_t ka = load_key_at(w);
    uint64_t ca = load_cand_at(w);
    while (w < nw) {
        const int32_t kb = load_key_at(w + wstep);
        const uint64_t cb = load_cand_at(w + wstep);
        step(w, ka, ca);
        w += wstep;
        if (w >= nw) break;
        ka = load_key_at(w + wstep);
        ca = load_cand_at(w + wstep);
        step(w, kb, cb);
        w += wstep;
    }
    if (stats) {
        if (lane < nruns) {
            if (acc_read) atomicAdd(&s_stat[2 * lane], acc_read);
            if (acc_false) atomicAdd(&s_stat[2 * lane + 1], acc_false);
        }
        __syncthreads();
        for (int j = threadIdx.x; j < 2 * nruns; j += kGetBlock)
            if (s_stat[j]) atomicAdd(stats + j, s_stat[j]);
    }
}

}  // namespace

hipError_t launch_get_resolve(const KeySpan &ks, const RouteTable &t, const GetTable &g,
                              const uint64_t *cand, size_t nw, int32_t *vals, int32_t *found,
                              uint64_t *stats, bool interpolate, hipStream_t stream) {
    if (nw == 0) return hipSuccess;
    const size_t lds = (size_t)t.total_fences * 4;
    // The grid is what fits on the chip at once, as for k_route: persistent
    // workgroups stage the fences once and walk many 64-key steps.
    const bool in_lds = lds <= kRouteLdsFenceBytesMax;
    const size_t per_block = (in_lds ? lds : 0) + 4096;
    int per_cu = (int)(kLdsBitmapBytes / per_block);
    per_cu = per_cu < 1 ? 1 : per_cu > 8 ? 8 : per_cu;  // 8 x 256 threads = 32 waves per CU
    const size_t blocks = (nw + kGetBlock / 64 - 1) / (kGetBlock / 64);
    const unsigned grid = (unsigned)std::min(blocks, (size_t)device_cu_count() * per_cu);
    unsigned long long *st = reinterpret_cast<unsigned long long *>(stats);
#define GET_LAUNCH(L, F, I) \
    k_get_resolve<L, F, I><<<grid, kGetBlock, F ? lds : 0, stream>>>(ks, t, g, cand, nw, vals, found, st)
#define GET_FORM(L, F) \
    do { if (interpolate) GET_LAUNCH(L, F, true); else GET_LAUNCH(L, F, false); } while (0)
    if (ks.layout == KEYS_PACKED) {
        if (in_lds) GET_FORM(KEYS_PACKED, true); else GET_FORM(KEYS_PACKED, false);
    } else {
        if (in_lds) GET_FORM(KEYS_STRIDED, true); else GET_FORM(KEYS_STRIDED, false);
    }
#undef GET_FORM
#undef GET_LAUNCH
    return hipGetLastError();
}

}  // namespace bloomhip
