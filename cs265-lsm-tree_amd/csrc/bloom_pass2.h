// bloom_pass2.h — pass 2 of the partition path: k_part_apply (builds, the
// single probe, the segment stack, the ladder stack), the host choice of its
// walk (choose_apply_walk) and the launch templates that bloom_pass2.hip,
// bloom_probe.hip and bloom_probe_ladder.hip instantiate.
#pragma once

#include "bloom_prims.h"

namespace bloomhip {

namespace {

// ---------------------------------------------------------------------------
// partition pass 2 (k_part_apply): workgroup b ORs segment b's run of every
// tile into an LDS image of the segment (S bits), then writes the segment
// out with plain 16-B stores (OR-merged with the old bitmap when that may be
// non-zero).  Segments never overlap, so no atomics leave the CU.
// ---------------------------------------------------------------------------

constexpr int kApplyBlock = 1024;
// pass 2's prologue: loads per thread in flight while an LDS image is staged
constexpr int kStageBatch = 4;
constexpr int kApplyDepth = 2;  // lane-group loads per wave per batch
// a stamped build's u64 stamps per workgroup (k_part_apply's STAMP): its start,
// the image staged (past the barrier), the first entry vector arrived, the
// walk done (past its barrier), the write-out's stores complete
constexpr int kEdge2Start = 0, kEdge2Staged = 1, kEdge2FirstVec = 2, kEdge2Walked = 3, kEdge2End = 4;
constexpr int kEdgeStamps2 = 5;

// MODE kApplyBuild: OR every entry into the zeroed LDS image, write the
// segment.  kApplyProbe: the LDS image is the filter's segment; each entry's
// bit is written as one result byte at the entry's own index in the sorted
// tile (res[tile*kTilePos + index]), so the result stores follow the runs
// like the loads.  kApplyStack: LDS holds bits [b*w, (b+1)*w) mod m_j of
// every stack member j (StackTable), the result byte carries member j's bit
// at bit j.
//
// The walk: G consecutive lanes share one tile and read its run as 16-B
// vectors (two packed u64 = six entries), lane j of the group taking the
// vector that holds the run's first entry + j, so one load instruction
// covers 64/G tiles x 6G entries.  An entry is this segment's exactly when
// its index lies in [run start, run end) (the bounds are already in the
// lane's registers); its offset is (entry - b*S) mod 2^21.  Lanes of tiles
// past the end re-read the last tile, which ORs / writes the same values
// twice.  A wave owns batches of kApplyDepth load groups; the next batch's
// run bounds are loaded while the current one is applied, and the rare tile
// whose run outlasts the first step is finished by a wave-uniform loop.
constexpr int kApplyBuild = 0, kApplyProbe = 1, kApplyStack = 2, kApplyLadder = 3;
// kApplyBuildL: a build on plan_build's one-member ladder (bins = hash bits):
// the entry is the image offset itself, and the image's d blocks go to
// a << t | b << s (StackTable::lad's s, t[0], d).
constexpr int kApplyBuildL = 4;

// Lanes per tile for pass 2, from the average run length L = tile entries /
// nbins: a step reads 6G entries of a tile (G lanes x one 16-B vector);
// runs longer than a step finish in the wave-uniform tail loop.  Measured
// (tools/ubench.py part*, G x depth sweep): G = 4 wins from runs of 8 (C4)
// to 48 entries (C2, C5): C2 38 us vs 66 at G = 8 and 47 at G = 2.
inline int apply_lanes_per_tile(size_t nbins, size_t tile_pos = kPartTilePos) {
    const size_t L = tile_pos / (nbins ? nbins : 1);
    if (L < 96) return 4;
    if (L < 192) return 8;
    if (L < 384) return 16;
    return 32;
}

// The walk of one pass-2 launch: k_part_apply's G, CHAINS, VECS and REDIR.
struct ApplyWalk {
    int g;       // lanes per tile
    int chains;  // 0: the batch walk; 1 or 2: independent lane groups, chains per group
    int vecs;    // 16-B vectors per lane and step
    bool redir;  // a load past the run's end goes to the group's first vector
    bool lean;   // the build's one-vector group walk on 32-bit offsets (k_part_apply's LEAN)
};
inline bool operator==(const ApplyWalk &a, const ApplyWalk &b) {
    return a.g == b.g && a.chains == b.chains && a.vecs == b.vecs && a.redir == b.redir && a.lean == b.lean;
}

// Whether the lean loop can address a batch: a lane's tile is a signed 32-bit
// byte offset into the sorted tiles that steps one workgroup's worth of tiles
// (256 at G = 4) past either end, and its bounds a 32-bit byte offset into
// the segment's row of the run table.
inline bool apply_offsets_fit32(size_t tile_keys, size_t nbins, size_t ntiles) {
    const uint64_t tile_bytes = ((uint64_t)ntiles + 2 * 256) * tile_keys * 8;
    const uint64_t table_bytes = (uint64_t)ntiles * (nbins + 1) * 4;
    return tile_bytes < (1ull << 31) && table_bytes < (1ull << 31);
}

// The walk pass 2 takes for a batch of ntiles tiles of tile_keys keys sorted
// into nbins segments, by mode: every threshold of the choice, with what was
// measured for it.  launch_apply compiles exactly the walks this returns.
inline ApplyWalk choose_apply_walk(int mode, size_t tile_keys, size_t nbins, size_t ntiles) {
    const ApplyWalk batch8{8, 0, 1, false};
    // runs shorter than a group's step (4 lanes x 6 entries): loads past a
    // run's end are redirected (k_part_apply's vload)
    const bool short_runs = 3 * tile_keys / (nbins ? nbins : 1) < 24;
    // entries beyond the Infinity Cache are read from HBM
    const bool from_hbm = (uint64_t)ntiles * tile_keys * 8 > kInfinityCacheBytes;
    // the ladder stack: batch walk at G = 8 (C3, 5 levels at 96-entry runs:
    // 75.6 us against 84.2 for independent groups at G = 4 and 78.5 at G = 8)
    if (mode == kApplyLadder) return batch8;
    if (tile_keys == kSuperTileKeys) {
        // a segment stack on super-tiles (plan_stack: 1,024-4,095 segments,
        // runs of 12-48 entries): four lanes per tile, two vectors per lane
        if (mode == kApplyStack) return {4, 1, 2, true};
        // a build on super-tiles: >= kSuperMinBins segments, runs of at most
        // 48 entries on average: independent groups of 4 lanes.  Short runs:
        // two vectors per lane, on two interleaved chains per lane group (C4
        // pass 2 795 -> 764 us; three chains 875, four 916,
        // profiles/r06/c4_two_chains/)
        if (short_runs) return {4, 2, 2, true};
        return {4, 1, 1, false};
    }
    const int g = apply_lanes_per_tile(nbins, 3 * tile_keys);
    if (mode == kApplyStack) {
        // independent lane groups at G = 4 (C3, 5 levels: 108 -> 102 us; 4
        // levels: equal), else the batch walk at G = 8
        if (g > 4) return batch8;
        return {4, 1, 1, short_runs};
    }
    // single probes, and every longer run: the batch walk
    if (mode == kApplyProbe || g > 4) return {g, 0, 1, false};
    // builds: independent lane groups (C2 pass 2 39.5 -> 34.4 us, C4 1.39 ->
    // 1.36 ms)
    if (short_runs) return {4, 1, 1, true};
    // entries from HBM (C5: 512 MiB): two vectors per lane and step, so a
    // ~48-entry run is one step with twice the loads in flight (C5 pass 2
    // 192.5 -> 173.6 us, tools/ubench.py p2ab_c5; C2's 128 MiB equal either
    // way, so it keeps one vector)
    if (from_hbm) return {4, 1, 2, true};
    // tiles from the Infinity Cache, runs of a step or more (C2, the f = 10
    // build, the general remainder): the same walk on the lean loop
    // (k_part_apply's LEAN: 65-67 -> 49.5 VALU per step at C2).  The f = 10
    // build 0.1114 -> 0.1065 ms; C2 0.0773-0.0775 -> 0.0770-0.0771 ms, the
    // median below the parent's fastest run in both orders, its slowest not;
    // m = 100,000,007 equal; pass 2 alone, re-reading the same tiles, equal
    // (31.3 against 31.5 us): the walk is bound by its loads and LDS ORs more
    // than by its instructions (profiles/pass2_loop/README.md).  A batch the
    // loop's 32-bit offsets cannot address (none that fits the Infinity
    // Cache) keeps the loop below.
    if (apply_offsets_fit32(tile_keys, nbins, ntiles)) return {4, 1, 1, false, true};
    return {4, 1, 1, false};
}

// ---------------------------------------------------------------------------
// k_part_apply's per-entry results, one function per LDS image: what apply6
// does with one entry of a run once it has decoded the vector and the run
// mask.  The ladder's lookup, every staging and the write-out stay in the
// kernel's body: as functions they changed the kernels' walk loops or
// registers (profiles/pass2_stages/README.md).
// ---------------------------------------------------------------------------

// The build's OR of one entry at image offset d, entry k of a vector whose
// run mask is vm: an entry outside the run ORs 0.  The word's LDS byte
// address is (d mod 2^21) / 32 * 4 (the segment image starts at LDS address
// 0: the kernel has no static LDS, which launch_apply_g checks before the
// first launch; an address taken from seg's pointer costs a v_add of the
// image's relocated address, 0, per entry) and the bit index the low 5 bits
// of d, which the shift takes as they are.
__device__ __forceinline__ void build_or(uint32_t d, uint32_t vm, int k) {
    const uint32_t addr = (d >> 3) & ((kEntryMask >> 3) & ~3u);
    const uint32_t bit = __builtin_amdgcn_ubfe(vm, k, 1) << (d & 31);
    __attribute__((address_space(3))) uint32_t *w =
        (__attribute__((address_space(3))) uint32_t *)(size_t)addr;
    __hip_atomic_fetch_or(w, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The single probe's result: the bit at image offset o.
__device__ __forceinline__ uint32_t probe_bit(const uint32_t *seg, uint32_t o) {
    return (seg[o >> 5] >> (o & 31)) & 1u;
}

// The stack's result at image offset o: member j's bit at bit j, from the
// word-interleaved image (member j's word p at seg[p * nf + j]).
template <int NF>
__device__ __forceinline__ uint32_t stack_bits(const uint32_t *seg, uint32_t o,
                                                const StackTable &st) {
    const uint32_t sh = o & 31;
    uint32_t acc = 0;
    if constexpr (NF > 0) {  // straight-line: NF reads at immediate offsets
        const uint32_t *wp = seg + (o >> 5) * (uint32_t)NF;
#pragma unroll
        for (int j = 0; j < NF; j++) acc |= __builtin_amdgcn_ubfe(wp[j], sh, 1u) << j;
    } else {
        const uint32_t *wp = seg + __umul24(o >> 5, (uint32_t)st.nf);
#pragma unroll
        for (int j = 0; j < kMaxStack; j++)  // member j's word at immediate offset 4j
            if (j < st.nf) acc |= __builtin_amdgcn_ubfe(wp[j], sh, 1u) << j;
    }
    return acc;
}

template <int MODE, int G, int TILE_KEYS, int BLOCK = kApplyBlock, int DEPTH = kApplyDepth,
          int CHAINS = 0, int VECS = 1, bool REDIR = false, int NF = 0, int LK = 0, bool STAMP = false,
          bool LEAN = false>
__global__ void __launch_bounds__(BLOCK) k_part_apply(
    const uint64_t *__restrict__ pos, const uint32_t *__restrict__ run_starts, int ntiles,
    int nbins, uint32_t seg_bits, uint64_t m, uint32_t *__restrict__ words, uint64_t nw32,
    int merge_existing, uint8_t *__restrict__ res, StackTable st) {
    constexpr bool PROBE = MODE != kApplyBuild && MODE != kApplyBuildL;
    // A fresh filter's bitmap is stored write-through by the builds that were
    // measured with it: the group walk at one vector per lane without the
    // redirect, on 4096- and 8192-key tiles (choose_apply_walk: C2 with pass
    // 1's write-through tiles 0.0789-0.0797 -> 0.0776-0.0788 ms, the f = 10
    // build and the general remainder level or slightly faster).  Every other build
    // keeps the non-temporal store: C5 (two vectors per lane, entries from
    // HBM) measured 0.3854 -> 0.3896 written through, and the short-run and
    // super-tile builds (C4) were not measured (profiles/build_edges/README.md).
    constexpr bool kFreshWT =
        !PROBE && CHAINS == 1 && VECS == 1 && !REDIR && TILE_KEYS != (int)kSuperTileKeys;
    // STAMP (micro-benchmarks only, tools/ubench.py edges): a build's
    // workgroup b writes wall_clock64() at its kEdge2* stages into
    // res[b * kEdgeStamps2 ..] as u64 (a build has no result bytes), thread
    // 0 alone, with an ordinary store.
    static_assert(!STAMP || (!PROBE && CHAINS == 1 && VECS == 1), "stamps: the build's group walk");
    auto stamp = [&](int k) {
        if constexpr (STAMP) {
            if (threadIdx.x == 0)
                reinterpret_cast<uint64_t *>(res)[(size_t)blockIdx.x * kEdgeStamps2 + k] = wall_clock64();
        }
    };
    stamp(kEdge2Start);
    static_assert(G >= 1 && G <= 64 && (64 % G) == 0, "G lanes per tile");
    constexpr int kTilePos = 3 * TILE_KEYS;
    constexpr int kTPI = 64 / G;                 // tiles per load instruction
    constexpr int kBatchTiles = kTPI * DEPTH;   // tiles per wave batch
    constexpr uint32_t kLastVec = TILE_KEYS / 2 - 1;

    const uint32_t seg_words = seg_bits / 32;
    extern __shared__ __attribute__((aligned(16))) uint32_t seg[];
    // Neighbouring segments' runs share 128-B lines of every sorted tile and
    // of the run-start rows, so give consecutive segments to workgroups on one
    // XCD (blocks are dealt round-robin over the 8 XCDs): a bijection on
    // [0, nbins); placement only affects speed.
    // One segment b per workgroup, or (the stacked probe with a segment
    // stride S, StackTable::seg_stride; a compile-time 0 for every other
    // mode) segments c, c + S, c + 2S, ...: members whose windows repeat with
    // a period dividing S (StackTable::keep_mask) are staged for the first
    // of them only.  Only at G = 4 (short runs, many segments) and up to 7
    // compiled-in members: the loop took 64 -> 68 VGPRs at 8 members and
    // 62 -> 65 at G = 8 with 5, which leaves one 1024-lane workgroup per CU.
    constexpr bool kStrided = MODE == kApplyStack && NF < 8 && G == 4;
    const int seg_stride = kStrided ? st.seg_stride : 0;
    uint32_t stage_mask = ~0u;
    for (int b = (int)xcd_remap(blockIdx.x, seg_stride ? (unsigned)seg_stride : (unsigned)nbins);;) {
    {
    // the thread index laundered per segment in the strided loop, which
    // otherwise hoists thread-dependent addresses out of it (52 -> 61 VGPRs)
    uint32_t tix = threadIdx.x;
    if constexpr (kStrided) asm volatile("" : "+v"(tix));
    const uint64_t w0 = (uint64_t)b * seg_words;
    const int nseg = (int)(min(nw32, w0 + seg_words) - w0);  // last segment may be short
    const uint64_t base = (uint64_t)b * seg_bits;
    const uint32_t base21 = (uint32_t)base & kEntryMask;
    if constexpr (MODE == kApplyStack) {
        // member j's bits (b*w + o) mod m_j for o < w: the w bits from
        // (b*w) mod m_j on, wrapping at m_j (w <= m_j; w and m_j are
        // multiples of 128 bits, so no 16-B vector straddles the wrap)
        // Word-interleaved image: member j's word p at seg[p * nf + j], so an
        // entry's nf words sit together and one address (+ immediate offsets)
        // reaches all of them.
        const int nf = NF ? NF : st.nf;  // NF: the member count as a compile-time constant
        for (int j = 0; j < nf; j++) {
            if (!((stage_mask >> j) & 1u)) continue;  // its window is already in LDS
            const uint32_t mw = st.mwords[j];
            const uint32_t start = (uint32_t)(((uint64_t)b * seg_words) % mw);
            const uint4 *src = reinterpret_cast<const uint4 *>(st.words[j]);
            const int nvec = (int)seg_words / 4;
            // kStageBatch vectors per thread in flight before their LDS
            // stores; past the end a lane reloads its own first vector (no
            // load under a branch, and no one address every lane hits); a
            // load-store loop waited for each load in turn
            for (int i0 = tix; i0 < nvec; i0 += kStageBatch * BLOCK) {
                uint4 v[kStageBatch];
#pragma unroll
                for (int k = 0; k < kStageBatch; k++) {
                    const int ik = i0 + k * BLOCK;
                    uint32_t wi = start + 4u * (uint32_t)(ik < nvec ? ik : i0);
                    if (wi >= mw) wi -= mw;
                    v[k] = src[wi / 4];
                }
#pragma unroll
                for (int k = 0; k < kStageBatch; k++) {
                    const int i = i0 + k * BLOCK;
                    if (i < nvec) {
                        uint32_t *dst = seg + (size_t)(4 * i) * nf + j;
                        dst[0] = v[k].x;
                        dst[nf] = v[k].y;
                        dst[2 * nf] = v[k].z;
                        dst[3 * nf] = v[k].w;
                    }
                }
            }
        }
    } else if constexpr (MODE == kApplyLadder) {
        // bin b's blocks of the direct members (StackTable::lad), block q at
        // LDS word q << (s - 5); the table: row e (member 0's block, the
        // entry's bits above s) holds rs words, one 32-bit LDS byte address
        // each: the other direct members' blocks and the packed image's
        // tuple; the tuple map: per tuple, the first bit of each packed
        // member's block; then the packed image, bpp bits per position and
        // tuple.  With a computed tuple (LK = 0) there is no table, and the
        // tuple map lives in member 0's area until member 0 is staged.
        const LadderTable &L = st.lad;
        // direct members (L.k, compiled in); LK = 0: one, and the packed
        // tuple computed from the entry (LadderTable::ctup: no table)
        constexpr uint32_t K = LK == 0 ? 1 : LK;
        constexpr bool CT = LK == 0;
        constexpr uint32_t BPP = (uint32_t)NF - K <= 4 ? 4u : 8u;
        const uint32_t bv = L.s - 7;  // log2 of 16-B vectors per block
        const uint32_t bin = (uint32_t)b;
        // first bit of block i of member j for this bin
        auto first_bit = [&](uint32_t j, uint32_t i) -> uint32_t {
            const uint32_t tj = L.t[j];
            if (tj >= L.s + L.u) {
                const uint32_t hj = tj - L.s - L.u;
                return ((i >> hj) << tj) + ((i & ((1u << hj) - 1u)) << (L.s + L.u)) + (bin << L.s);
            }
            return (i << tj) + ((bin & ((1u << (tj - L.s)) - 1u)) << L.s);
        };
        // block of member j given a = (x >> t_j) % d and xs = hash bits [s, t)
        // for some t >= t_j (bits [s + u, t_j) of x are bits [u, t_j - s) of xs)
        auto block_of = [&](uint32_t j, uint32_t aj, uint32_t xs) -> uint32_t {
            const uint32_t tj = L.t[j];
            if (tj < L.s + L.u) return aj;
            const uint32_t hj = tj - L.s - L.u;
            return (aj << hj) | ((xs >> L.u) & ((1u << hj) - 1u));
        };
        // (one load per iteration: batching these loads, as the segment
        // stack's staging does, made C3's probe 0.170 -> 0.180 ms)
        auto stage_direct = [&]() {
            for (uint32_t j = 0; j < K; j++) {
                const uint4 *src = reinterpret_cast<const uint4 *>(st.words[j]);
                uint4 *dst = reinterpret_cast<uint4 *>(seg) + ((size_t)L.base[j] << bv);
                for (uint32_t q = tix; q < (L.nblk[j] << bv); q += BLOCK)
                    dst[q] = src[(first_bit(j, q >> bv) >> 7) + (q & ((1u << bv) - 1u))];
            }
        };
        if constexpr (!CT) stage_direct();
        uint32_t *tbl = seg + L.img_words;
        // the tuple map follows the table; with a computed tuple (no table,
        // the images fill the LDS) it sits where member 0's blocks go, which
        // are staged after the packed image is built from it
        uint32_t *tmap = CT ? seg : tbl + L.ne * L.rs;
        constexpr uint32_t kTupleShift = BPP == 4 ? 0u : 1u;  // tuple words = 2^(s-3+this)
        for (uint32_t e = CT ? L.ne : tix; e < L.ne; e += BLOCK) {
            const uint32_t amax = e >> L.hb;
            const uint32_t xs = ((e & ((1u << L.hb) - 1u)) << L.u) | bin;  // hash bits [s, t_max)
            for (uint32_t j = 1; j < (uint32_t)NF && j <= K; j++) {
                const uint32_t tj = L.t[j];
                const uint32_t aj = (amax * L.pmod[j] + (xs >> (tj - L.s)) % L.d) % L.d;
                const uint32_t ij = block_of(j, aj, xs);
                // direct member j: its block's LDS byte address; member K:
                // the packed tuple's
                tbl[e * L.rs + (j - 1)] = j < K ? (L.base[j] + ij) << (L.s - 3)
                                                : (L.pk_words + (ij << (L.s - 3 + kTupleShift))) << 2;
            }
        }
        if constexpr (K < (uint32_t)NF) {
            const uint32_t tk = L.t[K < (uint32_t)kMaxStack ? K : 0], ntup = L.nblk[K];
            for (uint32_t tp = tix; tp < ntup; tp += BLOCK) {
                // tuple tp = member K's block: a_K and hash bits [s, t_K)
                uint32_t ak, xs;
                if (tk >= L.s + L.u) {
                    const uint32_t hk = tk - L.s - L.u;
                    ak = tp >> hk;
                    xs = ((tp & ((1u << hk) - 1u)) << L.u) | bin;
                } else {
                    ak = tp;
                    xs = bin & ((1u << (tk - L.s)) - 1u);
                }
                for (uint32_t j = K; j < (uint32_t)NF; j++) {
                    const uint32_t aj = (ak * L.pmodk[j] + (xs >> (L.t[j] - L.s)) % L.d) % L.d;
                    tmap[8 * tp + (j - K)] = first_bit(j, block_of(j, aj, xs));
                }
            }
        }
        __syncthreads();
        if constexpr (K < (uint32_t)NF) {
            // packed image: thread task = (tuple, 32 positions): one 32-bit
            // read per packed member, spread to bpp-bit fields
            const uint32_t cps = 1u << (L.s - 5);  // 32-position chunks per tuple
            const uint32_t ntask = L.nblk[K] * cps;
            uint32_t *pk = seg + L.pk_words;
            for (uint32_t q = tix; q < ntask; q += BLOCK) {
                const uint32_t tp = q >> (L.s - 5), c = q & (cps - 1u);
                uint32_t w[NF];
#pragma unroll
                for (int j = 0; j < NF; j++)
                    w[j] = (uint32_t)j >= K ? st.words[j][(tmap[8 * tp + (j - K)] >> 5) + c] : 0u;
                uint32_t *dst = pk + q * BPP;
                if constexpr (BPP == 4) {
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        uint32_t o = 0;
#pragma unroll
                        for (int j = 0; j < NF; j++) {
                            if ((uint32_t)j < K) continue;
                            uint32_t x = (w[j] >> (8 * r)) & 0xFFu;  // positions 8r .. 8r+7
                            x = (x | (x << 12)) & 0x000F000Fu;
                            x = (x | (x << 6)) & 0x03030303u;
                            x = (x | (x << 3)) & 0x11111111u;  // bit i at 4i
                            o |= x << (j - K);
                        }
                        dst[r] = o;
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 8; r++) {
                        uint32_t o = 0;
#pragma unroll
                        for (int j = 0; j < NF; j++) {
                            if ((uint32_t)j < K) continue;
                            uint32_t x = (w[j] >> (4 * r)) & 0xFu;  // positions 4r .. 4r+3
                            x = (x | (x << 14)) & 0x00030003u;
                            x = (x | (x << 7)) & 0x01010101u;  // bit i at 8i
                            o |= x << (j - K);
                        }
                        dst[r] = o;
                    }
                }
            }
        }
        if constexpr (CT) {
            __syncthreads();  // the tuple map's last reads
            stage_direct();
        }
    } else if constexpr (MODE == kApplyProbe) {
        for (int i = tix; i < (int)seg_words; i += BLOCK)
            seg[i] = i < nseg ? words[w0 + i] : 0u;
    } else {
        for (int i = tix; i < (int)seg_words / 4; i += BLOCK)
            reinterpret_cast<uint4 *>(seg)[i] = make_uint4(0, 0, 0, 0);
    }
    __syncthreads();
    stamp(kEdge2Staged);

    const int lane = tix & 63;
    const int wave = tix >> 6;
    const uint32_t sub = (uint32_t)(lane % G);  // this lane's vector in its tile's step
    const int tl = lane / G;                    // this lane's tile in a load group
    const int nbatch = (ntiles + kBatchTiles - 1) / kBatchTiles;

    // Run bounds travel packed (start | end << 16) until they are used: a
    // decode right after the prefetching load makes the compiler wait for
    // it there, i.e. for every load issued before it, the entry-vector
    // prefetch included (that wait made the packed table slower than two
    // u32 columns: C2 pass 2 36 -> 41 us, C4 1.22 -> 1.56 ms).
    auto dec = [](uint32_t pk) { return make_uint2(pk & 0xFFFFu, pk >> 16); };
    // The walk visits tiles last to first (data tile rt(t) for walk step t):
    // pass 1 wrote them first to last, so the most recently written sorted
    // tiles -- the ones still in the Infinity Cache -- are read first (C5
    // pass 2 205 -> 197.5 us, C2 unchanged, profiles/r04/reverse_walk/).
    auto rt = [&](int t) -> int { return ntiles - 1 - t; };
    auto bounds = [&](int j, uint32_t (&r)[DEPTH]) {
#pragma unroll
        for (int d = 0; d < DEPTH; d++) {
            const int t = j * kBatchTiles + d * kTPI + tl;
            r[d] = t < ntiles ? run_starts[(size_t)b * ntiles + rt(t)] : 0u;
        }
    };
    // Vector vi of tile t; lanes past the tile's last vector load that one
    // but keep their own vi, so none of its entries counts for them (a
    // clamped index would make up to G-1 lanes OR the same words, and those
    // same-address LDS atomics serialise the segments at a tile's end).
    auto load = [&](int t, uint32_t vi) -> uint4 {
        return reinterpret_cast<const uint4 *>(pos + (size_t)rt(t) * TILE_KEYS)[min(vi, kLastVec)];
    };
    // The vector a lane loads for its step at vector vi of a run ending at
    // entry `end`, group base vector vb.  REDIR (short runs): a lane whose
    // vector lies past the run's end loads the group's first vector instead
    // -- a line the group reads anyway, so the wave instruction touches fewer
    // distinct lines (C4's ~10-entry runs span 2-3 of a group's 4 vectors:
    // pass 2 1190 -> 1158 us).  The lane keeps its own vi for the entry
    // mask, so none of what it loaded counts.  Longer runs keep the plain
    // load: there the vector past a run's end starts the neighbour
    // segment's run, which an XCD neighbour reads next from the same L2
    // (C2 pass 2 35.5 -> 39.5 us with the redirect, profiles/r05/redirect/).
    auto vload = [&](uint32_t vi, uint32_t vb, uint32_t end) -> uint32_t {
        if constexpr (REDIR) return 6 * vi < end ? vi : vb;
        return vi;
    };
    // The six entries of vector vi of tile t; run = [r.x, r.y).
    auto apply6 = [&](const uint4 &v, int t, uint32_t vi, const uint2 &r) {
        const uint32_t e[6] = {v.x & kEntryMask, __builtin_amdgcn_alignbit(v.y, v.x, 21) & kEntryMask,
                               v.y >> 10,        v.z & kEntryMask,
                               __builtin_amdgcn_alignbit(v.w, v.z, 21) & kEntryMask, v.w >> 10};
        // Branch-free: the run's entries among the six form the 6-bit mask
        // vm (round 6: once per vector instead of a compare and an OR per
        // entry); an entry outside the run ORs 0 or stores no result byte.
        const int s0 = (int)(6 * vi) - (int)r.x;          // entry 0's place in the run
        const int lo = max(-s0, 0), hi = min(max((int)r.y - (int)(6 * vi), 0), 6);
        const uint32_t vm = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
        if constexpr (!PROBE) {
            // The group walk: a lane whose vector holds none of the run's
            // entries (a redirected load past the run's end: about half of
            // them at C4's ~20-entry runs on super-tiles) issues no atomics,
            // so the segment image's banks serve only the lanes with bits to set
            if (CHAINS == 0 || vm != 0) {
#pragma unroll
                for (int k = 0; k < 6; k++)
                    build_or(MODE == kApplyBuildL ? e[k] : e[k] - base21, vm, k);
            }
        } else {
            uint32_t bits[6];
#pragma unroll
            for (int k = 0; k < 6; k++) {
                const uint32_t ok = __builtin_amdgcn_ubfe(vm, k, 1);
                if constexpr (MODE == kApplyLadder) {
                    // member 0's block is the entry's high part (its blocks
                    // come first at LDS 0, 2^(s-3) bytes each), so its word's
                    // byte address is (e >> 3) & ~3; the table row gives the
                    // other direct members' block addresses and the packed
                    // tuple's (block and tuple bases are aligned, so the
                    // offsets OR in).  Bit extracts take the entry itself
                    // as the shift: v_bfe_u32 uses its low 5 bits.
                    const LadderTable &L = st.lad;
                    constexpr int K = LK == 0 ? 1 : LK;  // direct members, compiled in
                    constexpr bool CT = LK == 0;          // packed tuple computed, no table
                    // An entry outside the run is another run's (or 0 past a
                    // short tile's end: k_part_bin writes zeros there), so
                    // its high part is a block this bin stages and its reads
                    // stay in the image; its result bits are not stored
                    // (round 6: the select cost a VALU per entry)
                    const uint32_t ee = e[k];
                    (void)ok;
                    const uint32_t a0 = (ee >> 3) & ~3u;
                    uint32_t acc = __builtin_amdgcn_ubfe(lds_word(a0), ee, 1u);
                    if constexpr (CT) {
                        // tuple = member 1's block = hi mod nblk[1] (LadderTable::ctup)
                        const uint32_t hi = ee >> L.s;
                        const uint32_t tup =
                            (uint32_t)((int)hi + __mul24((int)__umulhi(hi, L.tmagic), -(int)L.nblk[1]));
                        uint32_t pa, psh;
                        if constexpr (NF - 1 <= 4) {  // 8 positions per word, tuples of 2^(s-1) bytes
                            pa = ((ee >> 1) & ((1u << (L.s - 1)) - 4u)) | ((tup << (L.s - 1)) + 4 * L.pk_words);
                            psh = ee << 2;
                        } else {  // 4 positions per word, tuples of 2^s bytes
                            pa = (ee & ((1u << L.s) - 4u)) | ((tup << L.s) + 4 * L.pk_words);
                            psh = ee << 3;
                        }
                        acc |= __builtin_amdgcn_ubfe(lds_word(pa), psh, (uint32_t)(NF - 1)) << 1;
                    } else if constexpr (K > 1 || K < NF) {
                        constexpr int RW = (K - 1) + (K < NF ? 1 : 0);  // row words used
                        constexpr int RS = RW <= 1 ? 1 : RW <= 2 ? 2 : RW <= 4 ? 4 : 8;  // = L.rs
                        const uint32_t row = L.img_words * 4 + (ee >> L.s) * (4 * RS);  // byte address
                        uint32_t rw[RW];
                        if constexpr (RW == 1) {
                            rw[0] = lds_word(row);
                        } else if constexpr (RW == 2) {
                            const uint2 v2 = lds_word2(row);
                            rw[0] = v2.x;
                            rw[1] = v2.y;
                        } else {
#pragma unroll
                            for (int q = 0; q < RW; q += 4) {
                                const uint4 v4 = lds_word4(row + 4 * q);
                                const uint32_t vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
                                for (int r = 0; r < 4; r++)
                                    if (q + r < RW) rw[q + r] = vv[r];
                            }
                        }
                        const uint32_t wmask = (1u << (L.s - 3)) - 4u;  // word offset in a block
#pragma unroll
                        for (int j = 1; j < K; j++) {
                            const uint32_t wj = lds_word((a0 & wmask) | rw[j - 1]);
                            acc |= __builtin_amdgcn_ubfe(wj, ee, 1u) << j;
                        }
                        if constexpr (K < NF) {
                            uint32_t pa, psh;
                            if constexpr (NF - K <= 4) {  // 8 positions per word: (lo >> 3) words
                                pa = ((ee >> 1) & ((1u << (L.s - 1)) - 4u)) | rw[K - 1];
                                psh = ee << 2;
                            } else {  // 4 positions per word: (lo >> 2) words
                                pa = (ee & ((1u << L.s) - 4u)) | rw[K - 1];
                                psh = ee << 3;
                            }
                            const uint32_t pw = lds_word(pa);
                            acc |= __builtin_amdgcn_ubfe(pw, psh, (uint32_t)(NF - K)) << K;
                        }
                    }
                    bits[k] = acc;
                    continue;
                }
                const uint32_t o = ok ? (e[k] - base21) & kEntryMask : 0u;  // reads stay in the image
                if constexpr (MODE == kApplyStack) bits[k] = stack_bits<NF>(seg, o, st);
                else bits[k] = probe_bit(seg, o);
            }
            // six result bytes at 6*vi (2-byte aligned): whole pairs as
            // 2-byte stores, a run's edge byte by byte
            uint8_t *p = res + (size_t)rt(t) * kTilePos + 6 * vi;
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const uint32_t mq = (vm >> (2 * q)) & 3u;
                if (mq == 3u) {
                    *reinterpret_cast<uint16_t *>(p + 2 * q) =
                        (uint16_t)(bits[2 * q] | (bits[2 * q + 1] << 8));
                } else if (mq == 1u) {
                    p[2 * q] = (uint8_t)bits[2 * q];
                } else if (mq == 2u) {
                    p[2 * q + 1] = (uint8_t)bits[2 * q + 1];
                }
            }
        }
    };

    static_assert(VECS == 1 || VECS == 2, "vectors per lane and step");
    if constexpr (LEAN) {
        // The one-vector group walk below with the per-step bookkeeping cut
        // down (choose_apply_walk: builds whose tiles and run table are
        // addressed by 32-bit byte offsets; profiles/pass2_loop/README.md):
        //  - a lane's tile is the byte offset tb of data tile rt(t) in pos
        //    (negative once t >= ntiles), its vector the offset tb | vi << 4
        //    from the uniform base, its bounds at tb >> (kTileShift - 2) in
        //    the segment's row: no 64-bit address is built per step;
        //  - the lane's first entry 6 vi is one 24-bit multiply, the run mask
        //    two saturating subtracts, a min, a shift and a bit-field
        //    extract, and the group is done with its run when the entries
        //    left from the lane's first, n, are at most those of the group's
        //    step from this lane on (c = 6 (G - sub));
        //  - the mask is taken before the state moves on, so the step keeps
        //    no copy of the old state, and the body is written twice with
        //    the two vector registers swapped: the next vector lands where
        //    the next half reads it, and no step waits for a load it issued
        //    itself (the ORs wait for the vector of the step before, the
        //    tile change for the bounds of the step before).
        // Lanes past the last tile (tb < 0) stay where they are, re-read
        // tile 0 and apply nothing.
        static_assert(!PROBE && CHAINS == 1 && VECS == 1 && !REDIR && !STAMP, "the build's one-vector group walk");
        static_assert(TILE_KEYS == 4096 || TILE_KEYS == 8192, "tiles of 2^15 or 2^16 bytes");
        constexpr int kGroupsPerWave = 64 / G;
        constexpr int kTileShift = TILE_KEYS == 4096 ? 15 : 16;  // log2 of a tile's bytes
        constexpr int32_t kQB = (kGroupsPerWave * (BLOCK / 64)) << kTileShift;  // Q tiles, in bytes
        const char *tiles = reinterpret_cast<const char *>(pos);
        const char *row = reinterpret_cast<const char *>(run_starts + (size_t)b * ntiles);
        // packed bounds of the tile at byte offset x (a tile past the end: tile 0's, never applied)
        auto bnd_off = [&](int32_t x) -> uint32_t { return (uint32_t)(max(x, 0) >> (kTileShift - 2)); };
        auto bnd = [&](int32_t x) -> uint32_t { return *reinterpret_cast<const uint32_t *>(row + bnd_off(x)); };
        auto ldv = [&](int32_t x, uint32_t vi) -> uint4 {
            return *reinterpret_cast<const uint4 *>(tiles + ((uint32_t)max(x, 0) + (min(vi, kLastVec) << 4)));
        };
        auto first_vec = [&](uint32_t pk) -> uint32_t { return (pk & 0xFFFFu) / 6u + sub; };
        auto or6 = [&](const uint4 &v, uint32_t vm) {
            const uint32_t e[6] = {v.x & kEntryMask, __builtin_amdgcn_alignbit(v.y, v.x, 21) & kEntryMask,
                                   v.y >> 10,        v.z & kEntryMask,
                                   __builtin_amdgcn_alignbit(v.w, v.z, 21) & kEntryMask, v.w >> 10};
#pragma unroll
            for (int k = 0; k < 6; k++) build_or(MODE == kApplyBuildL ? e[k] : e[k] - base21, vm, k);
        };
        const uint32_t c = 6u * ((uint32_t)G - sub);
        int32_t tb = (ntiles - 1 - (wave * kGroupsPerWave + tl)) * (1 << kTileShift);
        uint32_t r = bnd(tb), rn = bnd(tb - kQB);
        uint32_t vi = first_vec(r);
        uint4 va = ldv(tb, vi), vb;
        // one step: the vector in cur is applied, the next one loaded into nxt
        auto step = [&](const uint4 &cur, uint4 &nxt) {
            const bool alive = tb >= 0;
            const uint32_t e = __umul24(vi, 6u);
            const uint32_t lo = __builtin_elementwise_sub_sat(r & 0xFFFFu, e);
            const uint32_t n = __builtin_elementwise_sub_sat(r >> 16, e);
            uint32_t vm = __builtin_amdgcn_ubfe(63u << lo, 0u, min(n, 6u));
            // (the mask is final before the bounds change: scheduled after the
            // next load it kept a copy of the old bounds alive, two moves a step)
            asm volatile("" : "+v"(vm), "+v"(r));
            vi += G;
            if (alive && n <= c) {
                tb -= kQB;
                // r = rn, made before the lookahead's register takes its load
                // (hoisted above the copy, the load went to a second register
                // and the two swapped with a move a step)
                asm volatile("v_mov_b32 %0, %1" : "=v"(r), "+v"(rn));
                vi = first_vec(r);
            }
            // The lookahead's bounds are loaded by every lane, a lane that
            // stays on its tile re-reading the ones it has: under the tile
            // change's branch the load may or may not have been issued, and
            // the wait for the current vector then had to be the one that
            // leaves a single load in flight, i.e. it waited for the bounds
            // just asked for, a memory round trip per step.  Two loads per
            // step, always: that wait leaves both in flight.  (The offset is
            // laundered: the compiler otherwise proves the re-read redundant
            // and moves the load back under the branch.)
            uint32_t on = bnd_off(tb - kQB);
            asm volatile("" : "+v"(on));
            rn = *reinterpret_cast<const uint32_t *>(row + on);
            nxt = ldv(tb, vi);
            if (alive && vm != 0) or6(cur, vm);
        };
        // The wave leaves when none of its lanes has a tile, tested once per
        // two steps: the second step of a pair that was not needed applies
        // nothing (no lane is alive).  One exit also keeps the loop's only
        // waits the ones for a vector about to be used: with an exit after
        // either step the compiler waited for every load at the loop's head.
        while (__ballot(tb >= 0) != 0) {
            step(va, vb);
            step(vb, va);
        }
    } else if constexpr (CHAINS == 1 && VECS == 1) {
        // Independent lane groups: group q (G lanes) walks tiles q, q + Q,
        // q + 2Q, ... one step (G vectors) per iteration, moving to its next
        // tile as soon as its run ends, so no group waits for the longest run
        // of a batch.  The next step's vector is loaded before the current
        // one is applied, and the next tile's run bounds one tile ahead.
        constexpr int kGroupsPerWave = 64 / G;
        const int Q = kGroupsPerWave * (BLOCK / 64);
        auto bnd = [&](int tt) -> uint32_t {  // packed; 0 = empty past the end
            return tt < ntiles ? run_starts[(size_t)b * ntiles + rt(tt)] : 0u;
        };
        // the current and the next tile's bounds both stay packed (a decode
        // of the next one as it becomes current would sit between its load
        // and its register: a copy, hence a wait)
        int t = wave * kGroupsPerWave + tl;
        uint32_t r = bnd(t), rn = bnd(t + Q);
        uint32_t vb = (r & 0xFFFFu) / 6u;  // the group's step base (vector index)
        uint4 v = load(min(t, ntiles - 1), vload(vb + sub, vb, r >> 16));
        if constexpr (STAMP) {  // the first vector has arrived
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            stamp(kEdge2FirstVec);
        }
        while (__ballot(t < ntiles) != 0) {
            // state after this step: advance within the run or to the next
            // tile.  On a tile change the new lookahead bounds are loaded
            // straight into their loop register, before the next step's
            // vector, so the wait before the apply (vmcnt 1) leaves only that
            // vector in flight
            int t2 = t;
            uint32_t r2 = r, vb2 = vb + G;
            const bool adv = 6 * vb2 >= (r >> 16);
            if (adv) {
                t2 += Q;
                r2 = rn;
                vb2 = (r2 & 0xFFFFu) / 6u;
            }
            uint32_t rn2 = rn;
            if (adv) rn2 = bnd(t2 + Q);
            const uint4 v2 = load(min(t2, ntiles - 1), vload(vb2 + sub, vb2, r2 >> 16));
            if (t < ntiles && 6 * vb < (r >> 16)) apply6(v, t, vb + sub, dec(r));
            t = t2; r = r2; rn = rn2; vb = vb2; v = v2;
        }
    } else if constexpr (CHAINS == 2) {
        // The same walk on two interleaved chains per lane group (round 6):
        // chain c walks the group's tiles q + c Q, q + (2 + c) Q, ..., both
        // chains' next vectors in flight together, so at two vectors per lane
        // a lane holds four 16-B loads and two run-bound loads in flight
        // instead of two and one (C4's entries come from HBM, not the
        // Infinity Cache: its pass 2 waits on load latency, one (tile,
        // segment) pair per group step).
        constexpr int kGroupsPerWave = 64 / G;
        const int Q = kGroupsPerWave * (BLOCK / 64);
        constexpr int NC = CHAINS;  // chains per lane group
        constexpr int NV = VECS;    // vectors per lane and step
        auto bnd = [&](int tt) -> uint32_t {
            return tt < ntiles ? run_starts[(size_t)b * ntiles + rt(tt)] : 0u;
        };
        int t[NC];
        uint32_t r[NC], rn[NC], vb[NC];
        uint4 v[NC][NV];
#pragma unroll
        for (int c = 0; c < NC; c++) {
            t[c] = wave * kGroupsPerWave + tl + c * Q;
            r[c] = bnd(t[c]);
            rn[c] = bnd(t[c] + NC * Q);
            vb[c] = (r[c] & 0xFFFFu) / 6u;
#pragma unroll
            for (int k = 0; k < NV; k++)
                v[c][k] = load(min(t[c], ntiles - 1), vload(vb[c] + k * G + sub, vb[c], r[c] >> 16));
        }
        auto live = [&]() {
            bool any = false;
#pragma unroll
            for (int c = 0; c < NC; c++) any |= t[c] < ntiles;
            return any;
        };
        while (__ballot(live()) != 0) {
            int t2[NC];
            uint32_t r2[NC], rn2[NC], vb2[NC];
            uint4 v2[NC][NV];
#pragma unroll
            for (int c = 0; c < NC; c++) {
                t2[c] = t[c];
                r2[c] = r[c];
                vb2[c] = vb[c] + NV * G;
                const bool adv = 6 * vb2[c] >= (r[c] >> 16);
                if (adv) {
                    t2[c] += NC * Q;
                    r2[c] = rn[c];
                    vb2[c] = (r2[c] & 0xFFFFu) / 6u;
                }
                rn2[c] = rn[c];
                if (adv) rn2[c] = bnd(t2[c] + NC * Q);
            }
#pragma unroll
            for (int c = 0; c < NC; c++)
#pragma unroll
                for (int k = 0; k < NV; k++)
                    v2[c][k] = load(min(t2[c], ntiles - 1), vload(vb2[c] + k * G + sub, vb2[c], r2[c] >> 16));
#pragma unroll
            for (int c = 0; c < NC; c++) {
                if (t[c] < ntiles && 6 * vb[c] < (r[c] >> 16)) {
#pragma unroll
                    for (int k = 0; k < NV; k++) apply6(v[c][k], t[c], vb[c] + k * G + sub, dec(r[c]));
                }
            }
#pragma unroll
            for (int c = 0; c < NC; c++) {
                t[c] = t2[c]; r[c] = r2[c]; rn[c] = rn2[c]; vb[c] = vb2[c];
#pragma unroll
                for (int k = 0; k < NV; k++) v[c][k] = v2[c][k];
            }
        }
    } else if constexpr (CHAINS == 1 && VECS == 2) {
        // The same walk with two vectors per lane per step (vectors vb + sub
        // and vb + G + sub: a step covers 12G entries), loads past a run's
        // end redirected (vload): runs a little longer than one G-vector
        // step (super-tiles: ~20 entries, 4-5 vectors) take one step.
        constexpr int kGroupsPerWave = 64 / G;
        const int Q = kGroupsPerWave * (BLOCK / 64);
        auto bnd = [&](int tt) -> uint32_t {
            return tt < ntiles ? run_starts[(size_t)b * ntiles + rt(tt)] : 0u;
        };
        int t = wave * kGroupsPerWave + tl;
        uint32_t r = bnd(t), rn = bnd(t + Q);
        uint32_t vb = (r & 0xFFFFu) / 6u;
        uint4 v = load(min(t, ntiles - 1), vload(vb + sub, vb, r >> 16));
        uint4 w = load(min(t, ntiles - 1), vload(vb + G + sub, vb, r >> 16));
        while (__ballot(t < ntiles) != 0) {
            int t2 = t;
            uint32_t r2 = r, vb2 = vb + 2 * G;
            const bool adv = 6 * vb2 >= (r >> 16);
            if (adv) {
                t2 += Q;
                r2 = rn;
                vb2 = (r2 & 0xFFFFu) / 6u;
            }
            uint32_t rn2 = rn;
            if (adv) rn2 = bnd(t2 + Q);
            const uint4 v2 = load(min(t2, ntiles - 1), vload(vb2 + sub, vb2, r2 >> 16));
            const uint4 w2 = load(min(t2, ntiles - 1), vload(vb2 + G + sub, vb2, r2 >> 16));
            if (t < ntiles && 6 * vb < (r >> 16)) {
                apply6(v, t, vb + sub, dec(r));
                apply6(w, t, vb + G + sub, dec(r));
            }
            t = t2; r = r2; rn = rn2; vb = vb2; v = v2; w = w2;
        }
    } else {
    static_assert(CHAINS == 0 && VECS == 1 && !REDIR, "the batch walk");
    uint32_t rp[DEPTH];  // this batch's bounds, packed
    if (wave < nbatch) bounds(wave, rp);
    for (int j = wave; j < nbatch; j += (BLOCK / 64)) {
        int t[DEPTH];
        uint32_t vi[DEPTH];
        uint4 v[DEPTH];
        uint2 r[DEPTH];
#pragma unroll
        for (int d = 0; d < DEPTH; d++) {
            r[d] = dec(rp[d]);
            t[d] = min(j * kBatchTiles + d * kTPI + tl, ntiles - 1);
            vi[d] = r[d].x / 6u + sub;
            v[d] = load(t[d], vload(vi[d], vi[d] - sub, r[d].y));
        }
        uint32_t rn[DEPTH];
        const int jn = j + (BLOCK / 64);
        if (jn < nbatch) bounds(jn, rn);
#pragma unroll
        for (int d = 0; d < DEPTH; d++) apply6(v[d], t[d], vi[d], r[d]);
#pragma unroll
        for (int d = 0; d < DEPTH; d++) {
            for (uint32_t vn = r[d].x / 6u + sub + G; __ballot(6 * vn < r[d].y) != 0; vn += G)
                apply6(load(t[d], vload(vn, vn - sub, r[d].y)), t[d], vn, r[d]);
        }
#pragma unroll
        for (int d = 0; d < DEPTH; d++) rp[d] = rn[d];
    }
    }
    if constexpr (PROBE) {
        if constexpr (kStrided) goto segment_done;
        return;
    }
    __syncthreads();
    stamp(kEdge2Walked);
    // (stamped: the write-out's stores have left the wave)
    auto stamp_end = [&]() {
        if constexpr (STAMP) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            stamp(kEdge2End);
        }
    };

    if constexpr (MODE == kApplyBuildL) {
        // block a of the image (2^s bits) is the bitmap's bits a << t | b << s;
        // with the relabelled pass 1 (LadderTable::rinv != 0) image block a'
        // is the bitmap's block ladder0_block(a', b)
        const uint32_t ls = st.lad.s, lt = st.lad.t[0];
        const uint32_t vpb = 1u << (ls - 7);  // 16-B vectors per block
        const uint4 *seg4 = reinterpret_cast<const uint4 *>(seg);
        uint4 *w4 = reinterpret_cast<uint4 *>(words);
        auto block = [&](uint32_t q) -> uint4 * {
            uint32_t a = q >> (ls - 7);
            const uint32_t i = q & (vpb - 1u);
            if (st.lad.rinv) a = ladder0_block(a, (uint32_t)b, ls, st.lad.d, st.lad.rinv);
            return w4 + (((size_t)a << (lt - 7)) + ((size_t)b << (ls - 7)) + i);
        };
        // (two loops: one loop with both stores under a branch had its
        // stores merged into one plain store; the segments' note below)
        if (merge_existing) {
            for (uint32_t q = tix; q < st.lad.d * vpb; q += BLOCK) {
                uint4 *dq = block(q);
                uint4 v = seg4[q];
                const uint4 o = *dq;
                v.x |= o.x; v.y |= o.y; v.z |= o.z; v.w |= o.w;
                *dq = v;
            }
        } else {
            // (the segments' note below; block(q) as a byte offset from this
            // bin's first block: the ladder is a build of m < 2^32 bits)
            if constexpr (kFreshWT) {
                uint4 *b0 = w4 + ((size_t)b << (ls - 7));
                for (uint32_t q = tix; q < st.lad.d * vpb; q += BLOCK)
                    wt_store16(b0, (uint32_t)((const char *)block(q) - (const char *)b0), seg4[q]);
            } else {
                for (uint32_t q = tix; q < st.lad.d * vpb; q += BLOCK) nt_store16(block(q), seg4[q]);
            }
        }
        stamp_end();
        return;
    }

    uint32_t *dst = words + w0;
    if (nseg == (int)seg_words) {  // seg_words % 4 == 0 and w0 is 16-B aligned
        uint4 *dst4 = reinterpret_cast<uint4 *>(dst);
        const uint4 *seg4 = reinterpret_cast<const uint4 *>(seg);
        if (merge_existing) {
            for (int q = tix; q < (int)seg_words / 4; q += BLOCK) {
                uint4 v = seg4[q];
                const uint4 o = dst4[q];
                v.x |= o.x; v.y |= o.y; v.z |= o.z; v.w |= o.w;
                dst4[q] = v;
            }
        } else {
            // a fresh filter's finished segment: stored non-temporal, for
            // later probes, not this build (the L2 and Infinity Cache keep the
            // keys and sorted tiles: C2 188.6 -> 191.3, C4 129.1 -> 130.3
            // Gkeys/s in the bench A/B); a merge stores plainly what it has
            // just read (re-reading a non-temporal bitmap in repeated merges
            // cost C2 0.0909 -> 0.0917 ms)
            // kFreshWT: written through instead, so that pass 2 ends with
            // none of the bitmap dirty in the L2s
            if constexpr (kFreshWT) {
                for (int q = tix; q < (int)seg_words / 4; q += BLOCK)
                    wt_store16(dst4, 16u * (uint32_t)q, seg4[q]);
            } else {
                for (int q = tix; q < (int)seg_words / 4; q += BLOCK) nt_store16(dst4 + q, seg4[q]);
            }
        }
    } else {
        for (int i = tix; i < nseg; i += BLOCK) {
            uint32_t v = seg[i];
            if (merge_existing) v |= dst[i];
            dst[i] = v;
        }
    }
    stamp_end();
    }
    segment_done:
        if (!seg_stride) return;
        b += seg_stride;
        if (b >= nbins) return;
        stage_mask = ~st.keep_mask;
        __syncthreads();  // the walk's last image reads, before the next staging
    }
}

}  // namespace

// pass 2 of the probes (bloom_probe.hip, bloom_probe_ladder.hip)
hipError_t launch_apply_stack(const PartitionWorkspace &ws, uint64_t m, uint8_t *res,
                              const StackTable &st, hipStream_t stream);
hipError_t launch_apply_ladder(const PartitionWorkspace &ws, uint64_t m, uint8_t *res,
                               const StackTable &st, hipStream_t stream);

namespace {

// The segment stack's pass 2 on persistent workgroups (round 5): member j's
// window of segment b starts at word (b * sw) mod mw_j, periodic in b with
// period P_j = mw_j / gcd(sw, mw_j) (the f = 10 tree at w = 409,600 bits:
// 25 for level 0, 125 for level 1, every segment for level 2).  With S
// resident workgroups, S a multiple of the periods of a set of members,
// workgroup c takes segments c, c + S, c + 2S, ... and stages those members'
// windows once (the f = 10 tree: 150 KiB staged per segment -> 50 KiB for
// four of a workgroup's five).  Sets st.seg_stride = 0 when no member
// repeats within the resident workgroups or each segment has its own anyway.
inline void stack_stride(size_t nbins, uint32_t seg_words, size_t lds, StackTable &st) {
    st.seg_stride = 0;
    st.keep_mask = 0;
    const size_t per_cu = std::max<size_t>(1, std::min<size_t>(2048 / kApplyBlock, kLdsBitmapBytes / std::max<size_t>(lds, 1)));
    const uint64_t cap = (uint64_t)device_cu_count() * per_cu;
    if (nbins <= cap || st.nf < 1 || st.nf > kMaxStack) return;
    uint64_t P[kMaxStack];
    int ord[kMaxStack];
    for (int j = 0; j < st.nf; j++) {
        P[j] = st.mwords[j] / std::gcd<uint64_t>(seg_words, st.mwords[j]);
        ord[j] = j;
    }
    std::sort(ord, ord + st.nf, [&](int a, int c) { return P[a] < P[c]; });
    uint64_t L = 1;
    uint32_t mask = 0;
    for (int q = 0; q < st.nf; q++) {
        const int j = ord[q];
        if (P[j] >= nbins) continue;  // no repeat among the segments
        const uint64_t l2 = std::lcm<uint64_t>(L, P[j]);
        if (l2 > cap) continue;
        L = l2;
        mask |= 1u << j;
    }
    if (!mask) return;
    const uint64_t S = L * (cap / L);
    if (S >= nbins) return;
    st.seg_stride = (int)S;
    st.keep_mask = mask;
}

// Launches pass 2 (build or probe) with S/8 bytes of dynamic LDS (> 64 KiB
// must be opted into per kernel).
template <int MODE, int G, int TK, int DEPTH = kApplyDepth, int CHAINS = 0, int VECS = 1,
          bool REDIR = false, int NF = 0, int LK = 0, bool STAMP = false, bool LEAN = false>
hipError_t launch_apply_g(const PartitionWorkspace &ws, uint64_t m, uint32_t *words,
                          uint64_t nw32, int merge, uint8_t *res, const StackTable &st,
                          hipStream_t stream) {
    if (NF && st.nf != NF) return hipErrorInvalidValue;
    // The build's walk addresses the segment image by absolute LDS byte
    // address, which is right only while the dynamic image starts at LDS
    // address 0, i.e. while the kernel has no static LDS: checked once per
    // instantiation from the code object, and the launch refused otherwise.
    static const bool lds_ok = [] {
        const void *fn = reinterpret_cast<const void *>(
            &k_part_apply<MODE, G, TK, kApplyBlock, DEPTH, CHAINS, VECS, REDIR, NF, LK, STAMP, LEAN>);
        (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(kStackMaxBits / 8));
        hipFuncAttributes fa{};
        return hipFuncGetAttributes(&fa, fn) == hipSuccess && fa.sharedSizeBytes == 0;
    }();
    if (!lds_ok) return hipErrorInvalidDeviceFunction;
    const size_t lds = MODE == kApplyLadder ? ladder_lds_bytes(st.lad)
                                            : (size_t)ws.seg_bits / 8 * (MODE == kApplyStack ? st.nf : 1);
    if (lds > kStackMaxBits / 8) return hipErrorInvalidValue;
    StackTable sk = st;
    sk.seg_stride = 0;
    sk.keep_mask = 0;
    if (MODE == kApplyStack && NF < 8 && G == 4) stack_stride(ws.nbins, ws.seg_bits / 32, lds, sk);
    const unsigned grid = sk.seg_stride ? (unsigned)sk.seg_stride : (unsigned)ws.nbins;
    k_part_apply<MODE, G, TK, kApplyBlock, DEPTH, CHAINS, VECS, REDIR, NF, LK, STAMP, LEAN>
        <<<grid, kApplyBlock, lds, stream>>>(ws.pos, ws.run_starts, (int)ws.ntiles, (int)ws.nbins,
                                             ws.seg_bits, m, words, nw32, merge, res, sk);
    return hipGetLastError();
}

// The stacked pass 2 with the member count compiled in (straight-line member
// reads instead of a guarded loop over up to kMaxStack), G lanes per tile.
template <int G, int TK, int CHAINS, int VECS, bool REDIR>
hipError_t launch_stack_nf(const PartitionWorkspace &ws, uint64_t m, uint8_t *res,
                           const StackTable &st, hipStream_t stream) {
    switch (st.nf) {
#define STACK_NF(N)                                                                              \
    case N:                                                                                      \
        return launch_apply_g<kApplyStack, G, TK, kApplyDepth, CHAINS, VECS, REDIR, N>(ws, m, nullptr, 0, 0, \
                                                                                       res, st, stream);
        STACK_NF(2) STACK_NF(3) STACK_NF(4) STACK_NF(5) STACK_NF(6) STACK_NF(7) STACK_NF(8)
#undef STACK_NF
        default:
            return launch_apply_g<kApplyStack, G, TK, kApplyDepth, CHAINS, VECS, REDIR>(ws, m, nullptr, 0, 0,
                                                                                        res, st, stream);
    }
}

// The ladder's pass 2 (batch walk) with the member count and the direct
// members (plan_ladder: 1, 2, 3 or all of them) compiled in.
template <int G, int TK, int N, int LK>
hipError_t launch_ladder_g(const PartitionWorkspace &ws, uint64_t m, uint8_t *res,
                           const StackTable &st, hipStream_t stream) {
    return launch_apply_g<kApplyLadder, G, TK, kApplyDepth, 0, 1, false, N, LK>(ws, m, nullptr, 0, 0, res,
                                                                                st, stream);
}

template <int G, int TK, int N>
hipError_t launch_ladder_k(const PartitionWorkspace &ws, uint64_t m, uint8_t *res,
                           const StackTable &st, hipStream_t stream) {
    switch (st.lad.k) {
        case 1:
            if (st.lad.ctup)  // the packed tuple computed (LadderTable::ctup)
                return launch_ladder_g<G, TK, N, 0>(ws, m, res, st, stream);
            return launch_ladder_g<G, TK, N, 1>(ws, m, res, st, stream);
        case 2: return launch_ladder_g<G, TK, N, 2>(ws, m, res, st, stream);
        case 3:
            if constexpr (N >= 3)
                return launch_ladder_g<G, TK, N, 3>(ws, m, res, st, stream);
            else
                return hipErrorInvalidValue;
        default:
            if (st.lad.k != (uint32_t)N) return hipErrorInvalidValue;
            return launch_ladder_g<G, TK, N, N>(ws, m, res, st, stream);
    }
}

template <int G, int TK>
hipError_t launch_ladder_nf(const PartitionWorkspace &ws, uint64_t m, uint8_t *res,
                            const StackTable &st, hipStream_t stream) {
    switch (st.nf) {
        case 2: return launch_ladder_k<G, TK, 2>(ws, m, res, st, stream);
        case 3: return launch_ladder_k<G, TK, 3>(ws, m, res, st, stream);
        case 4: return launch_ladder_k<G, TK, 4>(ws, m, res, st, stream);
        case 5: return launch_ladder_k<G, TK, 5>(ws, m, res, st, stream);
        case 6: return launch_ladder_k<G, TK, 6>(ws, m, res, st, stream);
        case 7: return launch_ladder_k<G, TK, 7>(ws, m, res, st, stream);
        case 8: return launch_ladder_k<G, TK, 8>(ws, m, res, st, stream);
        default: return hipErrorInvalidValue;
    }
}

// Pass 2 of mode MODE over TK-key tiles on the walk choose_apply_walk gives.
// Each (MODE, TK) lists the walks the choice can return for it, so the
// library holds exactly the kernels it launches.
template <int MODE, int TK>
hipError_t launch_apply_tk(const PartitionWorkspace &ws, uint64_t m, uint32_t *words,
                           uint64_t nw32, int merge, uint8_t *res, const StackTable &st,
                           hipStream_t stream) {
    constexpr bool kSuper = TK == (int)kSuperTileKeys;
    const ApplyWalk w = choose_apply_walk(MODE, TK, ws.nbins, ws.ntiles);
    // (a build's group walks at one load group per batch, DEPTH 1: they have no batches)
#define APPLY_ON(G, C, V, R)                                                                       \
    if (w == ApplyWalk{G, C, V, R}) {                                                              \
        if constexpr (MODE == kApplyLadder)                                                        \
            return launch_ladder_nf<G, TK>(ws, m, res, st, stream);                                \
        else if constexpr (MODE == kApplyStack)                                                    \
            return launch_stack_nf<G, TK, C, V, R>(ws, m, res, st, stream);                        \
        else                                                                                       \
            return launch_apply_g<MODE, G, TK, C ? 1 : kApplyDepth, C, V, R>(ws, m, words, nw32, merge, res, \
                                                                             st, stream);          \
    }
    if constexpr (MODE == kApplyLadder) {
        APPLY_ON(8, 0, 1, false)
    } else if constexpr (kSuper && MODE == kApplyStack) {
        APPLY_ON(4, 1, 2, true)
    } else if constexpr (kSuper) {
        APPLY_ON(4, 2, 2, true) APPLY_ON(4, 1, 1, false)
    } else if constexpr (MODE == kApplyStack) {
        APPLY_ON(4, 1, 1, true) APPLY_ON(4, 1, 1, false) APPLY_ON(8, 0, 1, false)
    } else if constexpr (MODE == kApplyProbe) {
        APPLY_ON(4, 0, 1, false) APPLY_ON(8, 0, 1, false) APPLY_ON(16, 0, 1, false) APPLY_ON(32, 0, 1, false)
    } else {
        if (w == ApplyWalk{4, 1, 1, false, true})  // the lean loop
            return launch_apply_g<MODE, 4, TK, 1, 1, 1, false, 0, 0, false, true>(ws, m, words, nw32, merge,
                                                                                  res, st, stream);
        APPLY_ON(4, 1, 1, true) APPLY_ON(4, 1, 2, true) APPLY_ON(4, 1, 1, false)
        APPLY_ON(8, 0, 1, false) APPLY_ON(16, 0, 1, false) APPLY_ON(32, 0, 1, false)
    }
#undef APPLY_ON
    return hipErrorInvalidValue;
}

template <int MODE>
hipError_t launch_apply(const PartitionWorkspace &ws, uint64_t m, uint32_t *words, uint64_t nw32,
                        int merge, uint8_t *res, const StackTable &st, hipStream_t stream) {
    const size_t tk = tile_keys_of(ws);
    if (tk == kSuperTileKeys) {  // plan_build's segments and plan_stack only
        if constexpr (MODE == kApplyBuild || MODE == kApplyStack)
            return launch_apply_tk<MODE, (int)kSuperTileKeys>(ws, m, words, nw32, merge, res, st, stream);
        else
            return hipErrorInvalidValue;
    }
    return tk == 2 * kPartTileKeys
               ? launch_apply_tk<MODE, 2 * (int)kPartTileKeys>(ws, m, words, nw32, merge, res, st, stream)
               : launch_apply_tk<MODE, (int)kPartTileKeys>(ws, m, words, nw32, merge, res, st, stream);
}

}  // namespace

}  // namespace bloomhip
