// bloom_combine.h — the partitioned probes' last step: k_probe_combine, the
// page search of the GET routing (route_page) and the combine with the
// routing fused in (k_probe_combine_route).  Instantiated by bloom_probe.hip;
// route_page also by k_route (bloom_kernels.hip) and bloom_get.hip.
#pragma once

#include "bloom_prims.h"

namespace bloomhip {

namespace {

// Partitioned / stacked probe, last step (k_probe_combine): one workgroup per
// tile stages the tile's result bytes (sorted order) in LDS; thread t takes the
// 8 consecutive keys 8t .. 8t+7, reads their slots as one 16-B vector per hash
// (8-byte-per-lane loads of round 1 took the address unit 24 instructions per
// thread), ANDs each key's three bytes (bit j of the AND is filter j's is_set)
// and writes, per filter j, the byte of its 8 answers: key 8t + i at bit i of
// byte t of the tile's part of row rows.row[j] (the packed rows' bit order:
// bit i % 64 of word i / 64 is key i).  A wave's bytes are 64 contiguous bytes
// per row.  The bits of filter j are gathered out of the 8 AND bytes by two
// multiplies: with bytes b0..b3 (0/1 at bits 0, 8, 16, 24),
// (b * 0x01020408) >> 24 puts b_i at bit i and every other partial product
// below bit 24 or above bit 31 (no carries: those bits are distinct).
constexpr int kCombineKeys = 8;  // keys per thread (and pass: super-tiles take two)

// The passages the two combines share (their result-byte staging stays in
// each: as a function it changed the route kernels' spills,
// profiles/pass2_stages/README.md).
// Key i of a thread's 8: its three slots (u16 i of the slot vectors a, b, c)
// and the AND of their result bytes, bit j of which is member j's is_set; 0
// for a key past the live keys of a short last tile, whose slots are stale.
template <int TILE_KEYS>
__device__ __forceinline__ uint32_t combine_hit(const uint8_t *s_r, const uint32_t (&a)[4],
                                                const uint32_t (&b)[4], const uint32_t (&c)[4],
                                                int i, bool live) {
    constexpr int kTilePos = 3 * TILE_KEYS;
    const int sh = 16 * (i & 1);
    const uint32_t sa = (a[i / 2] >> sh) & 0xFFFFu, sb = (b[i / 2] >> sh) & 0xFFFFu,
                   sc = (c[i / 2] >> sh) & 0xFFFFu;
    return live ? (uint32_t)(s_r[min(sa, (uint32_t)kTilePos - 1)] &
                             s_r[min(sb, (uint32_t)kTilePos - 1)] &
                             s_r[min(sc, (uint32_t)kTilePos - 1)])
                : 0u;
}

// Bit j of the 8 keys' bytes (lo: keys 0-3, hi: keys 4-7) gathered by the
// two multiplies into one byte, stored at byte0 of row `row`.
__device__ __forceinline__ void combine_store_row(uint64_t *__restrict__ out, size_t row, size_t nw,
                                                  size_t byte0, uint32_t lo, uint32_t hi, int j) {
    const uint32_t bl = ((lo >> j) & 0x01010101u) * 0x01020408u;
    const uint32_t bh = ((hi >> j) & 0x01010101u) * 0x01020408u;
    const uint32_t byte = (bl >> 24) | ((bh >> 20) & 0xF0u);
    reinterpret_cast<uint8_t *>(out + row * nw)[byte0] = (uint8_t)byte;
}

template <int TILE_KEYS, int kCombineBlock>
__global__ void __launch_bounds__(kCombineBlock) k_probe_combine(
    const uint8_t *__restrict__ res, const uint16_t *__restrict__ slots, size_t n,
    uint64_t *__restrict__ out, size_t nw, StackTable rows) {
    constexpr int kTilePos = 3 * TILE_KEYS;
    constexpr int kPasses = TILE_KEYS / (kCombineBlock * kCombineKeys);
    static_assert(kPasses * kCombineBlock * kCombineKeys == TILE_KEYS, "8 keys per thread and pass");
    __shared__ __attribute__((aligned(16))) uint8_t s_r[kTilePos];
    const size_t tile = blockIdx.x;
    const size_t tile0 = tile * TILE_KEYS;
    const int tile_keys = (int)min((size_t)TILE_KEYS, n - tile0);
    uint4 va[kPasses], vb[kPasses], vc[kPasses];
#pragma unroll
    for (int ps = 0; ps < kPasses; ps++) {
        const int k0 = kCombineKeys * ((int)threadIdx.x + ps * kCombineBlock);
        const uint4 *sl = reinterpret_cast<const uint4 *>(slots + tile * 3 * TILE_KEYS + k0);
        va[ps] = sl[0];
        vb[ps] = sl[TILE_KEYS / 8];
        vc[ps] = sl[2 * (TILE_KEYS / 8)];
    }
    // the tile's result bytes: every load issued before any LDS store, at
    // clamped indices (no load under a branch; a load-store loop waited for
    // each load in turn)
    const uint4 *src = reinterpret_cast<const uint4 *>(res + tile * (size_t)kTilePos);
    constexpr int kResVec = kTilePos / 16, kResPer = (kResVec + kCombineBlock - 1) / kCombineBlock;
    uint4 rv[kResPer];
#pragma unroll
    for (int j = 0; j < kResPer; j++) rv[j] = src[min((int)threadIdx.x + j * kCombineBlock, kResVec - 1)];
#pragma unroll
    for (int j = 0; j < kResPer; j++)
        if ((int)threadIdx.x + j * kCombineBlock < kResVec)
            reinterpret_cast<uint4 *>(s_r)[threadIdx.x + j * kCombineBlock] = rv[j];
    __syncthreads();
#pragma unroll
    for (int ps = 0; ps < kPasses; ps++) {
        const int k0 = kCombineKeys * ((int)threadIdx.x + ps * kCombineBlock);  // this pass's first key
        // live keys of a short last tile; past them the slots are stale
        const uint32_t a[4] = {va[ps].x, va[ps].y, va[ps].z, va[ps].w},
                       b[4] = {vb[ps].x, vb[ps].y, vb[ps].z, vb[ps].w},
                       c[4] = {vc[ps].x, vc[ps].y, vc[ps].z, vc[ps].w};
        uint32_t hit[kCombineKeys];
#pragma unroll
        for (int i = 0; i < kCombineKeys; i++)
            hit[i] = combine_hit<TILE_KEYS>(s_r, a, b, c, i, k0 + i < tile_keys);
        // bytes of the tile's rows that hold keys: whole 64-key words, so the
        // last word of a short tile gets its zero bits too
        if (k0 >= ((tile_keys + 63) & ~63)) continue;
        const uint32_t lo = hit[0] | (hit[1] << 8) | (hit[2] << 16) | (hit[3] << 24);
        const uint32_t hi = hit[4] | (hit[5] << 8) | (hit[6] << 16) | (hit[7] << 24);
        const size_t byte0 = tile0 / 8 + threadIdx.x + ps * kCombineBlock;
#pragma unroll
        for (int j = 0; j < kMaxStack; j++) {
            if (j < rows.nf) combine_store_row(out, (size_t)rows.row[j], nw, byte0, lo, hi, j);
        }
    }
}

// The page of key k in a run (src/run.cpp:97-99): upper_bound over the run's
// n >= 1 fences (staged in LDS at fz) minus 1, for k >= fences[0] (the range
// check passed).  One interpolation guess from the run's first fence (f0) and
// fence spacing (scale = (n - 1) / (last - first)) places a window of
// kRouteWindow fences; two reads check that the answer is inside it, and 4
// branchless halving steps find it there; when the check fails, a binary
// search over the whole run does (exact either way, only slower).
constexpr int kRouteWindow = 15;  // fences; answers a .. a + 15: 4 halving steps
// A page guess is clamped to [0, 2^24] in float before it becomes an int
// (exact in float; a run has < 2^24 fences: n < 2^32 / kFenceStride).
constexpr float kGuessMax = 16777216.0f;

__device__ __forceinline__ int route_page(const int32_t *fz, int n, int32_t k, float f0, float scale) {
    int a = 0;
    bool ok = true;
    if (n > kRouteWindow) {
        const float gf = ((float)k - f0) * scale;
        // clamped in float first: a float-to-int conversion out of int range
        // is undefined (tight fences make the product huge); any guess past
        // the run's end is clamped to the last window below anyway
        const int g = (int)fminf(fmaxf(gf, 0.0f), kGuessMax);
        a = min(max(g - kRouteWindow / 2, 0), n - kRouteWindow);
        // the answer is in [a, a + 15] iff fences[a - 1] <= k and
        // fences[a + 15] > k (a window at either end passes that side)
        const int32_t fl = fz[max(a - 1, 0)], fh = fz[min(a + kRouteWindow, n - 1)];
        ok = (a == 0 || fl <= k) && (a + kRouteWindow >= n || fh > k);
    }
    int lo = a;
#pragma unroll
    for (int st = 8; st >= 1; st >>= 1) {  // fences at index >= n count as > k
        const int idx = lo + st - 1;
        if (idx < n && fz[min(idx, n - 1)] <= k) lo += st;
    }
    if (!ok) {  // the guess missed (rare): binary search the whole run
        int l = 1, h = n;
        while (l < h) {
            const int mid = (l + h) >> 1;
            if (fz[mid] <= k) l = mid + 1;
            else h = mid;
        }
        lo = l;
    }
    return lo - 1;
}

// Routing fused into the stacked probe's combine (§8f row 1, Run::get's test
// src/run.cpp:93-99 over the runs LSMTree::get visits, src/lsm_tree.cpp:
// 141-216), when every run of the call is a member of one stack: each key's
// member bits (the combine's AND byte) are range-checked against its runs'
// [first fence, max key] right here, the newest candidate run is the lowest
// set bit, its page comes from the fences staged in LDS, and the candidate
// rows leave range-checked -- the rows are not written by the combine and
// read back by k_route.  Persistent workgroups stage the runs' fences once.
// Member j is run rows.row[j]; the RouteTable is indexed by run.
// The fused page search's window: 7 fences and 3 halving steps (one
// dependent LDS read fewer than k_route's 15; the guess from the run's first
// and last fence lands within a fence or two for C3's keys).
constexpr int kFusedWindow = 7;

template <int TILE_KEYS, int BLOCK, int LAYOUT>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(8))) k_probe_combine_route(
    const uint8_t *__restrict__ res, const uint16_t *__restrict__ slots, KeySpan ks,
    uint64_t *__restrict__ out, size_t nw, StackTable rows, RouteTable rt,
    int32_t *__restrict__ first, int32_t *__restrict__ page, uint32_t *__restrict__ packed,
    size_t ntiles) {
    constexpr int kTilePos = 3 * TILE_KEYS;
    constexpr int kPasses = TILE_KEYS / (BLOCK * kCombineKeys);  // super-tiles: two
    static_assert(kPasses * BLOCK * kCombineKeys == TILE_KEYS, "8 keys per thread and pass");
    extern __shared__ int32_t s_fences[];
    __shared__ __attribute__((aligned(16))) uint8_t s_r[kTilePos];
    // per run: its fences' LDS offset and count, first fence and fence
    // spacing (one 16-B read per routed key); per member: its run's key
    // range as a window, k - lo <= span in u32 (one broadcast read per member
    // and pass of 8 keys)
    __shared__ __attribute__((aligned(16))) uint4 s_rec[kMaxStack];
    __shared__ __attribute__((aligned(8))) uint2 s_win[kMaxStack];
    __shared__ int s_run_of[kMaxStack];
    const int nf = rows.nf;
    for (int r = threadIdx.x; r < nf; r += BLOCK) {
        const uint32_t n = rt.nfences[r];
        const int32_t f0 = n ? rt.meta[r][1] : 0, fl = n ? rt.meta[r][n] : 0;
        const float scale = (n > 1 && fl > f0) ? (float)(n - 1) / ((float)fl - (float)f0) : 0.0f;
        s_rec[r] = make_uint4(rt.fence_off[r], n, __float_as_uint((float)f0), __float_as_uint(scale));
        s_run_of[r] = rows.row[r];
        const int rr = rows.row[r];  // member r's run: [first fence, max key]
        const uint32_t nr = rt.nfences[rr];
        const int32_t lo = nr ? rt.meta[rr][1] : 0, hi = nr ? rt.meta[rr][0] : 0;
        s_win[r] = make_uint2((uint32_t)lo, (uint32_t)hi - (uint32_t)lo);  // (a dead window: live below)
    }
    // members whose run has keys in range at all (no fences, or max key
    // below the first fence: never in range), and whether member j is run j
    uint32_t live = 0;
    bool ident = true;
#pragma unroll
    for (int j = 0; j < kMaxStack; j++) {
        if (j < nf) {
            const int r = rows.row[j];
            const uint32_t n = rt.nfences[r];
            if (n && rt.meta[r][0] >= rt.meta[r][1]) live |= 1u << j;
            ident &= r == j;
        }
    }
    const uint32_t live4 = live * 0x01010101u;
    {
        // every run's fences, contiguous in LDS (fence_off is the prefix of
        // the counts), 8 loads in flight per thread (a load-then-store loop
        // per run waited for each load: ~12 us before the first tile)
        constexpr int kBatch = 8;
        const uint32_t total = rt.total_fences;
        for (uint32_t b = 0; b < total; b += kBatch * BLOCK) {
            int32_t v[kBatch];
#pragma unroll
            for (int q = 0; q < kBatch; q++) {
                const uint32_t g = b + q * BLOCK + threadIdx.x;
                // g's run, by compile-time indices (a runtime index into the
                // kernel-argument arrays went through scratch memory)
                const int32_t *src = rt.meta[0] + 1;
                uint32_t off = 0;
#pragma unroll
                for (int rr = 1; rr < kMaxStack; rr++) {
                    if (rr < nf && rt.fence_off[rr] <= g) {
                        src = rt.meta[rr] + 1;
                        off = rt.fence_off[rr];
                    }
                }
                v[q] = g < total ? src[g - off] : 0;
            }
#pragma unroll
            for (int q = 0; q < kBatch; q++) {
                const uint32_t g = b + q * BLOCK + threadIdx.x;
                if (g < total) s_fences[g] = v[q];
            }
        }
    }
    const int kt = kCombineKeys * (int)threadIdx.x;  // this thread's first key in a tile's pass
    const bool vec_out = ((reinterpret_cast<uintptr_t>(first) | reinterpret_cast<uintptr_t>(page) |
                           reinterpret_cast<uintptr_t>(packed)) & 15) == 0;
    for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const size_t tile0 = tile * TILE_KEYS;
        const int tile_keys = (int)min((size_t)TILE_KEYS, ks.n - tile0);
        // pass ps's keys: 8 tid + 8 BLOCK ps .. + 7; their slots and the keys
        // (pass 0's loads in flight across the staging below)
        const uint4 *sl = reinterpret_cast<const uint4 *>(slots + tile * 3 * TILE_KEYS + kt);
        uint4 va = sl[0], vb = sl[TILE_KEYS / 8], vc = sl[2 * (TILE_KEYS / 8)];
        int32_t key[kCombineKeys];
        auto load_keys = [&](int k0) {
            if (LAYOUT == KEYS_PACKED && tile_keys == TILE_KEYS) {
                const int4 *kv = reinterpret_cast<const int4 *>(ks.base) + (tile0 + k0) / 4;
                const int4 x = kv[0], y = kv[1];
                key[0] = x.x; key[1] = x.y; key[2] = x.z; key[3] = x.w;
                key[4] = y.x; key[5] = y.y; key[6] = y.z; key[7] = y.w;
            } else {
#pragma unroll
                for (int i = 0; i < kCombineKeys; i++)
                    key[i] = k0 + i < tile_keys ? load_key<LAYOUT>(ks, tile0 + k0 + i) : 0;
            }
        };
        load_keys(kt);
        __syncthreads();  // the previous tile's result bytes are no longer read
        // the tile's result bytes: every load issued before any LDS store (a
        // load-store loop waited for each; loaded before the barrier, they
        // spilled under the 64-VGPR cap), clamped so no load sits under a branch
        constexpr int kResVec = kTilePos / 16, kResPer = (kResVec + BLOCK - 1) / BLOCK;
        const uint4 *src = reinterpret_cast<const uint4 *>(res + tile * (size_t)kTilePos);
        uint4 rv[kResPer];
#pragma unroll
        for (int j = 0; j < kResPer; j++) rv[j] = src[min((int)threadIdx.x + j * BLOCK, kResVec - 1)];
#pragma unroll
        for (int j = 0; j < kResPer; j++)
            if ((int)threadIdx.x + j * BLOCK < kResVec) reinterpret_cast<uint4 *>(s_r)[threadIdx.x + j * BLOCK] = rv[j];
        __syncthreads();
        // (unrolled: a loop over the two passes of a super-tile spilled 44
        // VGPRs; the 512-lane strided-key variant spills 2 either way)
#pragma unroll
        for (int ps = 0; ps < kPasses; ps++) {
        const int k0 = kt + ps * kCombineKeys * BLOCK;  // this pass's first key
        if (ps > 0) {
            const uint4 *sp = sl + ps * BLOCK;  // 8 u16 per thread: BLOCK vectors per pass
            va = sp[0];
            vb = sp[TILE_KEYS / 8];
            vc = sp[2 * (TILE_KEYS / 8)];
            load_keys(k0);
        }
        const uint32_t a[4] = {va.x, va.y, va.z, va.w}, b[4] = {vb.x, vb.y, vb.z, vb.w},
                       c[4] = {vc.x, vc.y, vc.z, vc.w};
        // byte i: key i's member bits, then its candidate runs (bit r: filter and range)
        uint32_t cand_lo = 0, cand_hi = 0, in_lo = 0, in_hi = 0;
        int32_t fr[kCombineKeys], pg[kCombineKeys];
#pragma unroll
        for (int i = 0; i < kCombineKeys; i++) {
            const uint32_t hit = combine_hit<TILE_KEYS>(s_r, a, b, c, i, k0 + i < tile_keys);
            if (i < 4) cand_lo |= hit << (8 * i);
            else cand_hi |= hit << (8 * (i - 4));
        }
        // the range checks, member by member over the 8 keys (k - lo <= span)
#pragma unroll
        for (int j = 0; j < kMaxStack; j++) {
            if (j < nf) {
                const uint2 w = s_win[j];
#pragma unroll
                for (int i = 0; i < kCombineKeys; i++) {
                    const uint32_t in = (uint32_t)key[i] - w.x <= w.y ? 1u << (8 * (i & 3) + j) : 0u;
                    if (i < 4) in_lo |= in;
                    else in_hi |= in;
                }
            }
        }
        cand_lo &= in_lo & live4;
        cand_hi &= in_hi & live4;
        if (!ident) {  // member j is run rows.row[j]: move its bits
            const uint32_t ml = cand_lo, mh = cand_hi;
            cand_lo = cand_hi = 0;
#pragma unroll
            for (int j = 0; j < kMaxStack; j++) {
                if (j < nf) {
                    const int sh = s_run_of[j] - j;
                    const uint32_t bl = ml & (0x01010101u << j), bh = mh & (0x01010101u << j);
                    cand_lo |= sh >= 0 ? bl << sh : bl >> -sh;
                    cand_hi |= sh >= 0 ? bh << sh : bh >> -sh;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < kCombineKeys; i++) {
            const uint32_t m = ((i < 4 ? cand_lo : cand_hi) >> (8 * (i & 3))) & 0xFFu;
            fr[i] = m ? __builtin_ctz(m) : -1;  // runs newest first: the lowest bit
        }
        // The pages of the lane's keys, two searched side by side (their LDS
        // reads independent; all 8 at once took 89 VGPRs, which left one
        // 1024-lane workgroup per CU, and 4 spilled under the 64-VGPR cap
        // that fits two): the window guess and its check, 4 halving steps,
        // and the whole-run binary search for the rare key whose guess missed.
        constexpr int kSide = 2;
#pragma unroll
        for (int h = 0; h < kCombineKeys; h += kSide) {
            int base_[kSide], n_[kSide], lo_[kSide];
            bool ok_[kSide];
#pragma unroll
            for (int u = 0; u < kSide; u++) {
                const int i = h + u;
                const uint4 rec = s_rec[max(fr[i], 0)];
                base_[u] = (int)rec.x;
                n_[u] = fr[i] >= 0 ? (int)rec.y : 0;
                int a = 0;
                ok_[u] = true;
                if (n_[u] > kFusedWindow) {
                    const int g = (int)fminf(fmaxf(((float)key[i] - __uint_as_float(rec.z)) * __uint_as_float(rec.w), 0.0f),
                                             kGuessMax);
                    a = min(max(g - kFusedWindow / 2, 0), n_[u] - kFusedWindow);
                    const int32_t fl = s_fences[base_[u] + max(a - 1, 0)];
                    const int32_t fh = s_fences[base_[u] + min(a + kFusedWindow, n_[u] - 1)];
                    ok_[u] = (a == 0 || fl <= key[i]) && (a + kFusedWindow >= n_[u] || fh > key[i]);
                }
                lo_[u] = a;
            }
#pragma unroll
            for (int st = (kFusedWindow + 1) / 2; st >= 1; st >>= 1) {
#pragma unroll
                for (int u = 0; u < kSide; u++) {
                    const int idx = lo_[u] + st - 1;
                    const int32_t f = s_fences[base_[u] + min(idx, max(n_[u] - 1, 0))];
                    if (idx < n_[u] && f <= key[h + u]) lo_[u] += st;
                }
            }
#pragma unroll
            for (int u = 0; u < kSide; u++) {
                const int i = h + u;
                if (!ok_[u]) {  // the guess missed (rare): binary search the whole run
                    const int32_t *fz = s_fences + base_[u];
                    int l = 1, hh = n_[u];
                    while (l < hh) {
                        const int mid = (l + hh) >> 1;
                        if (fz[mid] <= key[i]) l = mid + 1;
                        else hh = mid;
                    }
                    lo_[u] = l;
                }
                pg[i] = fr[i] >= 0 ? lo_[u] - 1 : -1;
            }
        }
        // first / page (or their packed form) of the live keys
        if (vec_out && tile_keys == TILE_KEYS) {
            int4 *f4 = reinterpret_cast<int4 *>(first + tile0 + k0);
            int4 *p4 = reinterpret_cast<int4 *>(page + tile0 + k0);
            if (first) {
                f4[0] = make_int4(fr[0], fr[1], fr[2], fr[3]);
                f4[1] = make_int4(fr[4], fr[5], fr[6], fr[7]);
            }
            if (page) {
                p4[0] = make_int4(pg[0], pg[1], pg[2], pg[3]);
                p4[1] = make_int4(pg[4], pg[5], pg[6], pg[7]);
            }
            if (packed) {
                uint4 *q4 = reinterpret_cast<uint4 *>(packed + tile0 + k0);
                q4[0] = make_uint4(route_pack(fr[0], pg[0]), route_pack(fr[1], pg[1]),
                                   route_pack(fr[2], pg[2]), route_pack(fr[3], pg[3]));
                q4[1] = make_uint4(route_pack(fr[4], pg[4]), route_pack(fr[5], pg[5]),
                                   route_pack(fr[6], pg[6]), route_pack(fr[7], pg[7]));
            }
        } else {
#pragma unroll
            for (int i = 0; i < kCombineKeys; i++) {
                if (k0 + i < tile_keys) {
                    if (first) first[tile0 + k0 + i] = fr[i];
                    if (page) page[tile0 + k0 + i] = pg[i];
                    if (packed) packed[tile0 + k0 + i] = route_pack(fr[i], pg[i]);
                }
            }
        }
        // candidate rows: bytes of the tile's rows that hold keys (whole
        // 64-key words), run r's byte = bit r of the 8 keys' masks
        if (k0 < ((tile_keys + 63) & ~63)) {
            const uint32_t lo = cand_lo, hi = cand_hi;
            const size_t byte0 = tile0 / 8 + threadIdx.x + ps * BLOCK;
#pragma unroll
            for (int r = 0; r < kMaxStack; r++) {
                if (r < nf) combine_store_row(out, (size_t)r, nw, byte0, lo, hi, r);
            }
        }
        }  // passes
    }
}

}  // namespace

// the combine (bloom_probe.hip)
hipError_t launch_combine(const PartitionWorkspace &ws, const uint8_t *res, const uint16_t *slots,
                          size_t n, uint64_t *out, size_t nw, const StackTable &rows,
                          hipStream_t stream);

}  // namespace bloomhip
