// bloom_pass1.h — pass 1 of the partition path: the tile kernels k_part_bin
// and k_part_bin2, the host rules that choose one (choose_pass1_kernel) and
// the launch templates the bloom_pass1_*.hip units instantiate.  Each product
// instantiation lives in exactly one translation unit (the exported wrappers
// declared below), so the units compile in parallel.
#pragma once

#include "bloom_prims.h"

namespace bloomhip {

namespace {

// ---------------------------------------------------------------------------
// partition pass 1 (k_part_bin): persistent workgroups of TB threads walk
// tiles of TB * kPartKPT keys.  Each thread hashes kPartKPT keys; the tile's
// 3 positions per key are counting-sorted by segment in LDS (an LDS atomic
// gives each its rank in its segment, a scan gives the segment offsets) and
// the sorted tile goes out packed: the low kEntryBits bits of each position,
// three per u64, 8 B per key-hash triple instead of 12.
// Column `tile` of the segment-major run table gets each segment's run of
// the tile, [start, end) in entries packed start | end << 16 (one u32 per
// (tile, segment): pass 2 reads the table once).  No global atomics.
//
// The next tile's keys are loaded while the current tile is sorted, and the
// workgroup barriers wait only for LDS (lgkmcnt), so the sorted tile's
// stores drain under the next tile's hashing.
//
// MK (how a position is reduced mod m): kModFast, the general remainder for
// m < 2^32 kept scaled by 2^l; kModWide, m >= 2^32 (64-bit positions,
// mod_wide; the entries are the same); kModP2, m = d << t with d | 255 and
// t >= kEntryBits (bloom_math.h mod_p2_hi): the entry is the key hash's own
// low 21 bits and p >> shift = (x >> t) % d << (t - shift) | bits shift..t-1
// of x, so only the 5-instruction (x >> t) % d is left of the remainder.
// SLOTS (partitioned probe): also write, per key and hash, the index its
// position got in the sorted tile: slots[(tile*3 + h)*tile_keys + key].
// PRIO: the issue priority (s_setprio) of the tile's phases, set inside the
// phase barriers (below, lds_barrier_prio); 0 = none.
// PIPE: the software-pipelined tile loop: a tile is scattered inside the hash
// phase of the workgroup's next tile, key by key, on two histograms (at the
// loop, below).
// ---------------------------------------------------------------------------

// k_part_bin's issue-priority policy PRIO = level | mode << 2, 0 = none
// (every wave at priority 0 throughout).  The level (1-3) is held
//   kPrioSort:    from the post-rank barrier (scan, run table, the next
//                 tile's key loads, scatter, packing and stores) to the
//                 hist-init barrier that opens the next tile's hash phase;
//   kPrioScatter: from the second scan barrier (key loads, scatter, packing
//                 and stores) to the hist-init barrier;
//   kPrioHash:    the inverse of kPrioSort: from the hist-init barrier (the
//                 hashing and its rank atomics) to the post-rank barrier;
//   kPrioYoung:   by waves TB/128 .. TB/64 - 1 of each workgroup for the whole
//                 kernel, set once, no flips.
// pass1_prio chooses; only kPrioHash measured faster anywhere.
// a stamped pipelined build's u64 stamps per workgroup (k_part_bin's STAMP)
constexpr int kEdge1Start = 0, kEdge1End = 1, kEdge1Tile0 = 2, kEdgeStamps1 = 32;
constexpr int kPrioSort = 0, kPrioScatter = 1, kPrioHash = 2, kPrioYoung = 3;
constexpr int pass1_prio_of(int mode, int level) { return level | mode << 2; }

// The keys of thread tid in a pass-1 tile: the kPartKPT consecutive keys
// tile0 + kPartKPT * tid + j, so a whole tile is read as 16-B vectors (two per
// thread for packed keys, four for entry_t runs); a short last tile by guarded
// scalar loads.  Which thread hashes which key does not matter to the sort,
// and the probe's slots are indexed by the key's place in the tile.
template <int LAYOUT, int TB>
__device__ __forceinline__ void load_tile_keys(const KeySpan &ks, size_t tile, int tid,
                                               int32_t (&k)[kPartKPT]) {
    static_assert(kPartKPT == 8, "two int4 / four entry pairs per thread");
    const size_t i0 = tile * (size_t)(TB * kPartKPT) + (size_t)kPartKPT * tid;
    const bool full = (tile + 1) * (size_t)(TB * kPartKPT) <= ks.n;  // uniform per workgroup
    if constexpr (LAYOUT == KEYS_PACKED) {
        if (full) {
            const int4 *v = reinterpret_cast<const int4 *>(ks.base) + i0 / 4;
            const int4 a = v[0], b = v[1];
            k[0] = a.x; k[1] = a.y; k[2] = a.z; k[3] = a.w;
            k[4] = b.x; k[5] = b.y; k[6] = b.z; k[7] = b.w;
            return;
        }
    } else if constexpr (LAYOUT == KEYS_ENTRY) {  // 16-B aligned entry_t run
        if (full) {
            const int4 *v = reinterpret_cast<const int4 *>(ks.base) + i0 / 2;
            const int4 a = v[0], b = v[1], c = v[2], d = v[3];
            k[0] = a.x; k[1] = a.z; k[2] = b.x; k[3] = b.z;
            k[4] = c.x; k[5] = c.z; k[6] = d.x; k[7] = d.z;
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < kPartKPT; j++) {
        const size_t i = i0 + j;
        k[j] = i < ks.n ? load_key<LAYOUT>(ks, i) : 0;
    }
}

// Pass-1 tile of persistent block x in round k: each round covers the next
// gridDim.x tiles, dealt so that every XCD takes a contiguous range of them
// (segment-major run-start stores then fill whole lines in one L2).  ntiles
// when the block has no tile in that round.
__device__ __forceinline__ size_t part_tile(size_t k, size_t ntiles) {
    const size_t base = k * gridDim.x;
    if (base >= ntiles) return ntiles;
    const size_t nr = min((size_t)gridDim.x, ntiles - base);
    return blockIdx.x < nr ? base + xcd_remap(blockIdx.x, (unsigned)nr) : ntiles;
}

// The segment of position p (SegMap: a shift, then an exact multiply-high
// division, checked on the host for every shifted value): two instructions,
// no branch.
template <typename P>
__device__ __forceinline__ uint32_t seg_of(P p, const SegMap &sm) {
    return __umulhi((uint32_t)(p >> sm.shift), sm.magic);
}

// A pass-1 histogram bin b starts at b << kBinShift and counts in steps of 4,
// so the rank atomic returns (b << kBinShift) + 4 * rank: (that >> 17) is the
// byte address 4b of the bin's offset (4 * rank < 4 * 3 * 8192 < 2^17), and
// no VALU touches the atomic's result before the scatter (its wait sits at the
// barrier).  After the scan bin b holds its BYTE offset into the sorted image
// minus b << kBinShift, so bin + rank value is the entry's byte slot.
constexpr uint32_t kBinShift = 19;  // 8192 segments << 19 < 2^32

// Outputs: pos_out[tile * kTileKeys ..] (u64), the tile's entries sorted by
// segment, packed three per u64; segment b's run of the tile (start | end
// << 16, b = 0..nbins-1): COLS = true: straight into the segment-major table
// runs[b * ntiles + tile]; COLS = false: into the tile-major
// runs[tile * nbins + b], for k_runs_transpose (large tables).
// How k_part_bin stores its sorted tiles (ST): plain, non-temporal
// (pass1_may_nt) or write-through (pass1_wt).
constexpr int kStorePlain = 0, kStoreNT = 1, kStoreWT = 2;
constexpr int kModFast = 0, kModWide = 1, kModP2 = 2, kModLadder = 3, kModLadder0 = 4;
// plan_build's one-member ladder with the block relabelled to (x >> 24) % d
// (bloom_math.h mod_p2_hi24; ladder0_relabel): C2 and C5
constexpr int kModLadder0R = 5;

// The bin (segment) of one raw hash and its pass-1 entry (the position's low
// kEntryBits bits, or the ladder's packed form), by reduction MK: pass 1's
// whole per-position arithmetic after the hash (tools/ubench.py prices it
// alone as the compute ceiling of pass 1).
template <int MK, int MINW>
__device__ __forceinline__ void bin_entry(uint64_t raw, const ModParams &mp, const SegMap &sm,
                                          uint32_t &b, uint32_t &ent) {
    if constexpr (MK == kModWide) {
        const uint64_t p = mod_wide(raw, mp);
        b = seg_of(p, sm);
        ent = (uint32_t)p & kEntryMask;
    } else if constexpr (MK == kModLadder) {
        // ladder stack (StackTable::lad): bin = hash bits
        // [s, s+u), entry = (a_max << hb | bits [s+u, t_max))
        // << s | bits [0, s) with a_max = (x >> t_max) % d
        const uint32_t xl = (uint32_t)raw;
        const uint32_t a = mod_p2_hi(raw, mp);
        b = __builtin_amdgcn_ubfe(xl, sm.shift, sm.lad_u);
        const uint32_t ehi =
            (a << sm.lad_hb) + __builtin_amdgcn_ubfe(xl, sm.scaled_shift, sm.lad_hb);
        ent = (ehi << sm.shift) | __builtin_amdgcn_ubfe(xl, 0, sm.shift);
    } else if constexpr (MK == kModLadder0) {
        // one-member ladder (plan_build): bin = hash bits
        // [s, t), entry = a << s | bits [0, s)
        const uint32_t xl = (uint32_t)raw;
        if constexpr (MINW >= 6) {
            // at the 80-VGPR cap of three workgroups per CU
            // the plain form spilled 50 VGPRs
            const uint32_t lo = __builtin_amdgcn_ubfe(xl, 0, sm.shift);
            b = __builtin_amdgcn_ubfe(xl, sm.shift, sm.lad_u);
            ent = lshl_or_s(mod_p2_hi(raw, mp), sm.shift, lo);
        } else {
            // (C5's pass 1: 229 us, against 256 for the pinned
            // form above and for segments)
            const uint32_t a = mod_p2_hi(raw, mp);
            b = __builtin_amdgcn_ubfe(xl, sm.shift, sm.lad_u);
            ent = (a << sm.shift) | __builtin_amdgcn_ubfe(xl, 0, sm.shift);
        }
    } else if constexpr (MK == kModLadder0R) {
        // as kModLadder0 with a' = (x >> 24) % d for a = (x >> t) % d: one
        // shift and one v_sad_u8 instead of an alignbit, a shift and the sad
        // (pass 2 maps image block a' back to a, ladder0_block)
        const uint32_t xl = (uint32_t)raw;
        if constexpr (MINW >= 6) {
            const uint32_t lo = __builtin_amdgcn_ubfe(xl, 0, sm.shift);
            b = __builtin_amdgcn_ubfe(xl, sm.shift, sm.lad_u);
            ent = lshl_or_s(mod_p2_hi24(raw, mp), sm.shift, lo);
        } else {
            const uint32_t a = mod_p2_hi24(raw, mp);
            b = __builtin_amdgcn_ubfe(xl, sm.shift, sm.lad_u);
            ent = (a << sm.shift) | __builtin_amdgcn_ubfe(xl, 0, sm.shift);
        }
    } else if constexpr (MK == kModP2) {
        const uint32_t xl = (uint32_t)raw;
        const uint32_t r = mod_p2_hi(raw, mp);
        const uint32_t q = (r << sm.p2_hi_shift) |
                           __builtin_amdgcn_ubfe(xl, sm.shift, sm.p2_hi_shift);
        b = __umulhi(q, sm.magic);
        ent = xl & kEntryMask;
    } else {
        // the remainder still scaled by 2^l: the entry is a
        // bit-field of it, and one shift reaches the segment
        const uint32_t ru = mod_fast_scaled(raw, mp);
        b = __umulhi(ru >> sm.scaled_shift, sm.magic);
        ent = __builtin_amdgcn_ubfe(ru, mp.l, kEntryBits);
    }
}

// ABL (micro-benchmarks only, tools/ubench.py p1abl: the pass's cost by
// stage): 0 the whole tile; 1 hash + bin and entry only; 2 + the rank
// atomics; 3 + the scan and the run table; 4 + the scatter (each thread reads
// one word of the image, or the compiler drops the stage); 5 + the packing,
// without the sorted tile's stores.  A stage's unconsumed results go to one
// store that only an impossible value takes.  The same numbers cut the PIPE
// loop: there stage 3 is the scan without any scatter and stage 4 adds the
// scatter interleaved with the hashing (it needs the scan's offsets to stay
// inside the image, so it cannot be priced before the scan).
template <int LAYOUT, bool SLOTS, bool COLS, int TB, int MK, int MAXB = 0, int MINW = 4,
          int ABL = 0, int ST = kStorePlain, bool DEFER = false, int PRIO = 0, int PIPE = 0, bool STAMP = false>
__global__ void __launch_bounds__(TB, MINW) k_part_bin(KeySpan ks, ModParams mp,
                                                       uint64_t *__restrict__ pos_out,
                                                       uint32_t *__restrict__ runs, SegMap sm,
                                                       size_t ntiles, uint16_t *__restrict__ slots) {
    constexpr int kTileKeys = TB * kPartKPT;
    constexpr int kTilePos = 3 * kTileKeys;
    constexpr int kMaxB = MAXB ? MAXB : TB >= 1024 ? (int)kPartMaxBinsBig : (int)kPartMaxBins;
    constexpr int kScanPer = (kMaxB + 1 + TB - 1) / TB;  // scan entries per thread, at most
    static_assert(4 * kTilePos <= (1 << 17) && kTilePos < (1 << 16) &&
                      ((uint64_t)(kMaxB - 1) << kBinShift) < (1ull << 32),
                  "packed rank fields (bin nbins, never incremented, may wrap to 0)");
    // PRIO: the priority each phase barrier leaves the wave at (-1: the plain
    // barrier, no s_setprio: every barrier of PRIO = 0)
    constexpr int kPrioLevel = PRIO & 3, kPrioMode = PRIO >> 2;
    static_assert(PRIO == 0 || (kPrioLevel > 0 && kPrioMode <= kPrioYoung), "PRIO = level | mode << 2");
    constexpr bool kFlips = PRIO != 0 && kPrioMode != kPrioYoung;
    constexpr int kPrioAtHist = !kFlips ? -1 : kPrioMode == kPrioHash ? kPrioLevel : 0;
    constexpr int kPrioAtRank = !kFlips || kPrioMode == kPrioScatter ? -1 : kPrioMode == kPrioSort ? kPrioLevel : 0;
    constexpr int kPrioAtScan = kFlips && kPrioMode == kPrioScatter ? kPrioLevel : -1;
    // static LDS even for the 96 KiB of an 8192-key tile (gfx950 takes it);
    // dynamic LDS or a pointer to it made the compiler spill registers here
    __shared__ __attribute__((aligned(16))) uint32_t s_sorted[kTilePos];
    // (PIPE: two histograms, H[1] at word offset kMaxB + 1)
    __shared__ uint32_t s_hist[(PIPE ? 2 : 1) * (kMaxB + 1)];
    __shared__ uint32_t s_wsum[TB / 64];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int nb = (int)sm.nbins;
    const int per = (nb + 1 + TB - 1) / TB;  // this launch's scan entries per thread
    int32_t kcur[kPartKPT], knext[kPartKPT];

    // Write-out of a sorted tile (its LDS image complete: after the tile's
    // post-scatter barrier), one 16-B vector per call: the image goes out
    // packed, three entries per u64; thread t packs entries 6v .. 6v+5 of
    // vector v = r * TB + t.  In a short tile the entries past its end are
    // stale, masked so they cannot spill into a neighbour field (pass 2 never
    // uses them).
    constexpr int kVecs = kTileKeys / 2;  // 16-B vectors per tile
    constexpr int kStores = kVecs / TB;
    static_assert(kStores * TB == kVecs && kStores * 2 == kPartKPT, "whole vectors per thread");
    auto pack_store = [&](auto full_c, int r, size_t tile, int tile_keys) {
        constexpr bool FULL = decltype(full_c)::value;
        uint4 *dst = reinterpret_cast<uint4 *>(pos_out + tile * (size_t)kTileKeys) + r * TB + tid;
        const uint2 *src = reinterpret_cast<const uint2 *>(s_sorted + 6 * (r * TB + tid));
        const uint2 a = src[0], b = src[1], c = src[2];
        uint32_t e[6] = {a.x, a.y, b.x, b.y, c.x, c.y};
        if constexpr (!FULL) {
            // past the tile's positions: 0, not stale (the ladder probe's
            // pass 2 reads with every entry of a vector, its run's or not)
#pragma unroll
            for (int q = 0; q < 6; q++) e[q] = 6 * (r * TB + tid) + q < 3 * tile_keys ? e[q] & kEntryMask : 0u;
        }
        const uint4 v = pack_entries6(e);
        if constexpr (ABL == 0) {
            // kStoreNT: sorted tiles beyond the Infinity Cache (C5: 512 MiB)
            // are stored non-temporal, so they do not evict what pass 2 can
            // use there (C5 build 0.419 -> 0.406 ms; below it, C2's 128 MiB,
            // pass 2 reads them from the cache: 35 us, 48 from HBM; a
            // runtime choice in the kernel spilled 3-4 VGPRs).
            // kStoreWT: written through (pass1_wt), so the kernel ends
            // with no dirty tile lines in the L2s for the boundary to flush;
            // pass 2 still reads them from the Infinity Cache.
            if constexpr (ST == kStoreNT) nt_store16(dst, v);
            else if constexpr (ST == kStoreWT)
                wt_store16(pos_out + tile * (size_t)kTileKeys, 16u * (uint32_t)(r * TB + tid), v);
            else *dst = v;
        } else {
            // keep the packing: a store only when an impossible value shows
            if (v.x == 0xFFFFFFFFu && v.y == 0xFFFFFFFFu) *dst = v;
        }
    };
    constexpr bool kPacks = ABL == 0 || ABL == 5;  // the stages that write tiles out

    // Exclusive scan of a histogram's nbins+1 counts (the extra slot is 0 and
    // receives the tile total), in two halves around a workgroup barrier of
    // the caller's; thread t owns [t*per, t*per + per).  Waves that own no
    // bin (C2: waves 5-7 of 8) skip it: nobody reads their wave sums, which
    // come after every live bin.  hoff: the histogram's word offset in s_hist
    // (0 but in the PIPE loop), part of its bins' bias.
    // first half: the thread's counts (4 * count of bin b) and the wave sums
    auto scan_counts = [&](uint32_t hoff, uint32_t (&local)[kScanPer], uint32_t &tsum, uint32_t &incl) {
        const bool scan_wave = wave * 64 * per <= nb;  // uniform per wave
        tsum = incl = 0;
        if (scan_wave) {
#pragma unroll
            for (int q = 0; q < kScanPer; q++) {
                const int b = tid * per + q;
                local[q] = (q < per && b <= nb) ? s_hist[hoff + b] - ((hoff + b) << kBinShift) : 0u;
                tsum += local[q];
            }
            incl = wave_incl_scan(tsum);
            if (lane == 63) s_wsum[wave] = incl;
        }
    };
    // second half: the bins' offsets into the histogram, the run table's column
    auto scan_offsets = [&](uint32_t hoff, size_t tile, const uint32_t (&local)[kScanPer], uint32_t tsum,
                            uint32_t incl) {
        if (wave * 64 * per <= nb) {
            uint32_t run = incl - tsum;
            for (int w = 0; w < wave; w++) run += s_wsum[w];
#pragma unroll
            for (int q = 0; q < kScanPer; q++) {
                const int b = tid * per + q;
                if (q < per && b <= nb) {
                    // biased by -(b << kBinShift): bin + rank value = byte slot
                    s_hist[hoff + b] = run - ((hoff + b) << kBinShift);
                    // segment b's run of this tile, [start, end) in entries,
                    // packed start | end << 16 (both < 3 * 8192), straight
                    // from the scan's registers: segment-major column or
                    // tile-major row
                    const uint32_t pk = (run >> 2) | (((run + local[q]) >> 2) << 16);
                    if (b < nb) {
                        if constexpr (COLS) runs[(size_t)b * ntiles + tile] = pk;
                        else runs[tile * (size_t)nb + b] = pk;
                    }
                    run += local[q];
                }
            }
        }
    };

    // One tile.  FULL (every tile but a short last one) makes the key count a
    // constant: no per-key guards, and a fixed number of vector-memory ops
    // after the next tile's key loads, so the wait for those keys at the top
    // of the next tile is vmcnt(#stores) instead of a drain of every store.
    // Those loads are issued after the run-start stores for that reason.
    //
    // DEFER (the 1024-thread builds, where a CU holds one workgroup and every
    // barrier phase idles the whole CU): a tile's write-out does not follow
    // its scatter, where the VALU has nothing else to do; it runs inside the
    // hash phase of the workgroup's next tile, one vector after every second
    // key (PREV: this tile carries the write-out of tile `prev`, always a
    // FULL one, since only a block's last tile can be short), and after the
    // block's last tile in an epilogue.  That is safe because s_sorted holds
    // tile t from the post-scatter barrier of iteration t; it is next written
    // by the scatter of t+1, which lies behind the hist-init, post-rank and
    // two scan barriers of iteration t+1; and the rank atomics between the
    // first two of those touch s_hist only.
    auto do_tile = [&](auto full_c, auto prev_c, size_t tile, size_t next, size_t prev) {
        constexpr bool FULL = decltype(full_c)::value;
        constexpr bool PREV = decltype(prev_c)::value && kPacks;
        const size_t tile0 = tile * kTileKeys;
        const int tile_keys = FULL ? (int)kTileKeys : (int)min((size_t)kTileKeys, ks.n - tile0);
        auto live = [&](int j) { return FULL || kPartKPT * tid + j < tile_keys; };
#pragma clang loop unroll(disable) vectorize(disable)
        for (int b = tid; b <= nb; b += TB) s_hist[b] = (uint32_t)b << kBinShift;
        lds_barrier_prio<kPrioAtHist>();  // also (!DEFER): the previous tile's s_sorted reads are done

        // 1. positions -> (segment, rank in segment) and the entry; the ranks
        //    are not consumed before the barrier, so all 24 LDS atomics of a
        //    thread stay in flight behind the hashing.  (PREV) the previous
        //    tile's vectors go out here, one after every second key: all
        //    four at the head spilled 3 VGPRs at 1024 threads.
        uint32_t br[kPartKPT * 3];   // (segment << kBinShift) + 4 * rank
        uint32_t ent[kPartKPT * 3];  // low kEntryBits bits of the position
#pragma unroll
        for (int j = 0; j < kPartKPT; j++) {
            if constexpr (PREV) {
                if (j & 1) pack_store(BoolC<true>{}, j / 2, prev, kTileKeys);
            }
            if (live(j)) {
                const int32_t k = kcur[j];
#pragma unroll
                for (int h = 0; h < 3; h++) {
                    const uint64_t raw = h == 0 ? raw_hash1(k) : h == 1 ? raw_hash2(k) : raw_hash3(k);
                    uint32_t b, e;
                    bin_entry<MK, MINW>(raw, mp, sm, b, e);
                    ent[3 * j + h] = e;
                    if constexpr (ABL == 1) br[3 * j + h] = b;
                    else br[3 * j + h] = atomicAdd(&s_hist[b], 4u);
                }
            } else {
#pragma unroll
                for (int h = 0; h < 3; h++) br[3 * j + h] = ent[3 * j + h] = 0;
            }
        }
        lds_barrier_prio<kPrioAtRank>();
        // (ablation: the stage's results consumed by one impossible store)
        auto consume = [&]() {
            uint32_t x = 0;
#pragma unroll
            for (int q = 0; q < 3 * kPartKPT; q++) x ^= br[q] + ent[q];
            if (x == 0x9E3779B9u) reinterpret_cast<uint32_t *>(pos_out)[tile * kTileKeys + tid] = x;
        };
        if constexpr (ABL == 1 || ABL == 2) {
            if (next < ntiles) load_tile_keys<LAYOUT, TB>(ks, next, tid, knext);
            consume();
            return;
        }

        // 2. exclusive scan of the nbins+1 counts, the run table's column
        uint32_t local[kScanPer];  // 4 * count of bin b
        uint32_t tsum, incl;
        scan_counts(0u, local, tsum, incl);
        lds_barrier();
        scan_offsets(0u, tile, local, tsum, incl);
        lds_barrier_prio<kPrioAtScan>();
        if (next < ntiles) load_tile_keys<LAYOUT, TB>(ks, next, tid, knext);
        if constexpr (ABL == 3) {
            consume();
            return;
        }

        // 3. scatter into the LDS image sorted by segment, one hash at a time:
        //    its kPartKPT offset reads first (one wait), then the writes.
        //    Byte addresses throughout (the histogram holds byte offsets).
        const char *hist_b = reinterpret_cast<const char *>(s_hist);
        char *sorted_b = reinterpret_cast<char *>(s_sorted);
#pragma unroll
        for (int h = 0; h < 3; h++) {
            uint32_t slot[kPartKPT];  // byte offset in the sorted image
#pragma unroll
            for (int j = 0; j < kPartKPT; j++)
                slot[j] = *reinterpret_cast<const uint32_t *>(hist_b + (br[3 * j + h] >> 17)) +
                          br[3 * j + h];
#pragma unroll
            for (int j = 0; j < kPartKPT; j++)
                if (live(j)) *reinterpret_cast<uint32_t *>(sorted_b + slot[j]) = ent[3 * j + h];
            if constexpr (SLOTS) {
                // key kPartKPT*tid + j's sorted index, one 16-B store per hash
                uint16_t *sl = slots + (tile * 3 + h) * kTileKeys + kPartKPT * tid;
                if (FULL) {
                    uint32_t w[kPartKPT / 2];
#pragma unroll
                    for (int q = 0; q < kPartKPT / 2; q++)  // slots are byte offsets: 4 | slot
                        w[q] = lshl_or(slot[2 * q + 1], 14, slot[2 * q] >> 2);
                    // non-temporal: the slots are read once, by the combine
                    // after pass 2, and kept out of the caches they leave the
                    // sorted entries pass 2 is about to read (C3 pass 1
                    // 108 -> 96 us, the whole probe 283 -> 262 us)
                    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
                    const v4u wv = {w[0], w[1], w[2], w[3]};
                    __builtin_nontemporal_store(wv, reinterpret_cast<v4u *>(sl));
                } else {
#pragma unroll
                    for (int j = 0; j < kPartKPT; j++)
                        if (live(j)) sl[j] = (uint16_t)(slot[j] >> 2);
                }
            }
        }
        lds_barrier();
        if constexpr (ABL == 4) {
            // (ablation: the scattered image consumed, one read per thread
            // into the impossible store; unread, the compiler dropped the
            // whole scatter)
            if ((s_sorted[tid] ^ br[0]) == 0x9E3779B9u)
                reinterpret_cast<uint32_t *>(pos_out)[tile * kTileKeys + tid] = br[0];
            return;
        }
        // 4. (not deferred) the sorted tile goes out at once
        if constexpr (!DEFER) {
#pragma unroll
            for (int r = 0; r < kStores; r++) pack_store(full_c, r, tile, tile_keys);
        }
    };
    // The block's last tile has no next tile to go out under.
    auto write_out = [&](auto full_c, size_t tile) {
        if constexpr (DEFER && kPacks) {
            const int tile_keys = (int)min((size_t)kTileKeys, ks.n - tile * kTileKeys);
#pragma unroll
            for (int r = 0; r < kStores; r++) pack_store(full_c, r, tile, tile_keys);
        }
    };

    // Full tiles in the loop; the short last tile (index ntiles - 1, always
    // in a block's final round) after it, so the loop sees only FULL.  With
    // DEFER the block's first tile is peeled off: it carries no write-out,
    // and a test of the round inside the loop kept both bodies' addresses
    // live across it (20 spilled VGPRs).
    const size_t nfull = ks.n / kTileKeys;
    size_t tile = part_tile(0, ntiles);
    if (tile >= ntiles) return;
    // STAMP (micro-benchmarks only, tools/ubench.py edges): the pipelined
    // build's workgroup x writes wall_clock64() into slots[x * kEdgeStamps1 ..]
    // as u64 (a build has no slot plane), thread 0 alone, with an ordinary
    // store: its start, its end (every store complete), then one stamp after
    // each iteration of the tile loop and after the epilogue.
    static_assert(!STAMP || (PIPE != 0 && !SLOTS), "stamps: the pipelined build");
    int nstamp = kEdge1Tile0;
    auto stamp = [&](int k) {
        if constexpr (STAMP) {
            if (tid == 0 && k < kEdgeStamps1)
                reinterpret_cast<uint64_t *>(slots)[(size_t)blockIdx.x * kEdgeStamps1 + k] = wall_clock64();
        }
    };
    auto stamp_end = [&]() {
        if constexpr (STAMP) {
            stamp(nstamp++);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            stamp(kEdge1End);
        }
    };
    stamp(kEdge1Start);
    if constexpr (PRIO != 0 && kPrioMode == kPrioYoung) {
        // the workgroup's later-dispatched half; the wave index from an SGPR,
        // so the branch is scalar (s_setprio ignores EXEC)
        if (__builtin_amdgcn_readfirstlane(threadIdx.x) >= TB / 2) __builtin_amdgcn_s_setprio(kPrioLevel);
    }
    load_tile_keys<LAYOUT, TB>(ks, tile, tid, kcur);
    if constexpr (PIPE != 0) {
        // The software-pipelined loop.  The scatter is LDS work with almost
        // no VALU work and the hashing the reverse, so a tile is not
        // scattered between barriers of its own: tile i-1 is scattered inside
        // the hash phase of tile i, key slot by key slot.  Two histograms
        // alternate, H[0] at word 0 of s_hist and H[1] at word kHist: tile i
        // ranks into H[i & 1].
        //   phase A (the hash phase's priority), per key slot j: tile i-1's
        //     three positions of slot j to the image (offsets from
        //     H[(i-1) & 1]), then tile i's key j hashed, its rank atomics on
        //     H[i & 1], their results into the same six registers;
        //   barrier 1: tile i-1's image and tile i's counts are complete;
        //   phase B (priority 0): scan of H[i & 1] and the run table (with
        //     its wave-sum barrier), H[(i+1) & 1] biased for tile i+1, the
        //     next keys loaded, tile i-1 packed and stored;
        //   final barrier.
        // Three barriers per tile instead of five.  The block's first tile is
        // peeled (nothing to scatter), and its last is scattered and written
        // out in an epilogue.  Only a block's last tile can be short, so a
        // scatter inside phase A is always of a FULL tile.
        // One loop body serves both histograms: bin b of the histogram at
        // word hoff is biased by (hoff + b) << kBinShift, so a rank value
        // >> 17 is the byte address of its bin's offset in either (the
        // scatter needs no parity), and the rank atomic's address is one
        // v_lshl_add of the uniform hoff.  (Two bodies with compile-time
        // addresses spilled every rank and entry of one of them.)
        // Ordering:
        //   - H[(i-1) & 1] is read by the scatters of phase A until barrier 1
        //     of iteration i and biased again only after that barrier;
        //     H[i & 1] gets its offsets in phase B, before the final barrier,
        //     and is read from the next phase A on;
        //   - s_sorted is written only in phase A (and the epilogue's
        //     scatter) and read only in phase B (and the epilogue's
        //     write-out); the final barrier waits for lgkmcnt(0), so the
        //     packing's reads are done before the next phase A writes.
        static_assert(!DEFER && !SLOTS && (PRIO == 0 || kPrioMode == kPrioHash),
                      "PIPE: a build's loop; phase A holds the hash phase's priority");
        constexpr uint32_t kHist = kMaxB + 1;  // H[1]'s word offset
        static_assert(((uint64_t)(2 * kHist - 1) << kBinShift) < (1ull << 32), "both histograms' bins in the rank field");
        uint32_t br[kPartKPT * 3];   // (hoff + segment << kBinShift) + 4 * rank
        uint32_t ent[kPartKPT * 3];  // low kEntryBits bits of the position
        constexpr bool kScatters = ABL == 0 || ABL >= 4;
        // key slot j's three positions into the image
        auto scatter_key = [&](int j, bool alive) {
            const char *hist_b = reinterpret_cast<const char *>(s_hist);
            char *sorted_b = reinterpret_cast<char *>(s_sorted);
            uint32_t slot[3];  // byte offset in the sorted image
#pragma unroll
            for (int h = 0; h < 3; h++)
                slot[h] = *reinterpret_cast<const uint32_t *>(hist_b + (br[3 * j + h] >> 17)) + br[3 * j + h];
            if (alive) {
#pragma unroll
                for (int h = 0; h < 3; h++) *reinterpret_cast<uint32_t *>(sorted_b + slot[h]) = ent[3 * j + h];
            }
        };
        // (ablation: a stage's results consumed by one impossible store)
        auto consume = [&](size_t tile) {
            uint32_t x = 0;
#pragma unroll
            for (int q = 0; q < 3 * kPartKPT; q++) x ^= br[q] + ent[q];
            if (x == 0x9E3779B9u) reinterpret_cast<uint32_t *>(pos_out)[tile * kTileKeys + tid] = x;
        };
        auto consume_image = [&](size_t tile) {
            if ((s_sorted[tid] ^ br[0]) == 0x9E3779B9u)
                reinterpret_cast<uint32_t *>(pos_out)[tile * kTileKeys + tid] = br[0];
        };
        // Iteration `tile` (ranks into the histogram at word hoff) carrying
        // the scatter and the write-out of tile `prev` (PREV; always FULL).
        auto pipe_tile = [&](auto full_c, auto prev_c, size_t tile, size_t next, size_t prev, uint32_t hoff) {
            constexpr bool FULL = decltype(full_c)::value, PREV = decltype(prev_c)::value;
            const int tile_keys = FULL ? (int)kTileKeys : (int)min((size_t)kTileKeys, ks.n - tile * kTileKeys);
            auto live = [&](int j) { return FULL || kPartKPT * tid + j < tile_keys; };
            // phase A
#pragma unroll
            for (int j = 0; j < kPartKPT; j++) {
                if constexpr (PREV && kScatters) scatter_key(j, true);
                if (live(j)) {
                    const int32_t k = kcur[j];
#pragma unroll
                    for (int h = 0; h < 3; h++) {
                        const uint64_t raw = h == 0 ? raw_hash1(k) : h == 1 ? raw_hash2(k) : raw_hash3(k);
                        uint32_t b, e;
                        bin_entry<MK, MINW>(raw, mp, sm, b, e);
                        ent[3 * j + h] = e;
                        if constexpr (ABL == 1) br[3 * j + h] = b;
                        else br[3 * j + h] = atomicAdd(&s_hist[hoff + b], 4u);
                    }
                } else {
#pragma unroll
                    for (int h = 0; h < 3; h++) br[3 * j + h] = ent[3 * j + h] = 0;
                }
            }
            lds_barrier_prio<kPrioAtRank>();  // barrier 1
            // phase B
            uint32_t local[kScanPer];  // 4 * count of bin b
            uint32_t tsum, incl;
            if constexpr (ABL == 0 || ABL >= 3) scan_counts(hoff, local, tsum, incl);
            // the other histogram's last readers were phase A's scatters
            const uint32_t other = kHist - hoff;
#pragma clang loop unroll(disable) vectorize(disable)
            for (int b = tid; b <= nb; b += TB) s_hist[other + b] = (other + b) << kBinShift;
            if constexpr (ABL == 0 || ABL >= 3) {
                lds_barrier();
                scan_offsets(hoff, tile, local, tsum, incl);
            }
            // after the run-start stores, before the tile's: do_tile's order
            if (next < ntiles) load_tile_keys<LAYOUT, TB>(ks, next, tid, kcur);
            if constexpr (ABL >= 1 && ABL <= 3) consume(tile);
            if constexpr (PREV) {
                if constexpr (ABL == 4) consume_image(prev);
                if constexpr (kPacks) {
#pragma unroll
                    for (int r = 0; r < kStores; r++) pack_store(BoolC<true>{}, r, prev, kTileKeys);
                }
            }
            lds_barrier_prio<kPrioAtHist>();  // final barrier
        };
        // Epilogue: the block's last tile scattered, then written out.
        auto pipe_last = [&](auto full_c, size_t tile) {
            constexpr bool FULL = decltype(full_c)::value;
            const int tile_keys = FULL ? (int)kTileKeys : (int)min((size_t)kTileKeys, ks.n - tile * kTileKeys);
            if constexpr (kScatters) {
#pragma unroll
                for (int j = 0; j < kPartKPT; j++) scatter_key(j, FULL || kPartKPT * tid + j < tile_keys);
                lds_barrier_prio<kPrioAtRank>();
                if constexpr (ABL == 4) consume_image(tile);
            }
            if constexpr (kPacks) {
#pragma unroll
                for (int r = 0; r < kStores; r++) pack_store(full_c, r, tile, tile_keys);
            }
        };

#pragma clang loop unroll(disable) vectorize(disable)
        for (int b = tid; b <= nb; b += TB) s_hist[b] = (uint32_t)b << kBinShift;
        lds_barrier_prio<kPrioAtHist>();
        if (tile >= nfull) {  // the block's only tile is the short one
            pipe_tile(BoolC<false>{}, BoolC<false>{}, tile, ntiles, tile, 0u);
            stamp(nstamp++);
            pipe_last(BoolC<false>{}, tile);
            stamp_end();
            return;
        }
        size_t prev = tile, next = part_tile(1, ntiles);
        pipe_tile(BoolC<true>{}, BoolC<false>{}, tile, next, tile, 0u);
        stamp(nstamp++);
        tile = next;
        uint32_t hoff = kHist;
        for (size_t round = 2; tile < nfull; round++) {
            next = part_tile(round, ntiles);
            pipe_tile(BoolC<true>{}, BoolC<true>{}, tile, next, prev, hoff);
            stamp(nstamp++);
            prev = tile;
            tile = next;
            hoff = kHist - hoff;
        }
        if (tile < ntiles) {
            pipe_tile(BoolC<false>{}, BoolC<true>{}, tile, ntiles, prev, hoff);
            stamp(nstamp++);
            pipe_last(BoolC<false>{}, tile);
        } else {
            pipe_last(BoolC<true>{}, prev);
        }
        stamp_end();
    } else if constexpr (!DEFER) {
        for (size_t round = 0; tile < nfull; round++) {
            const size_t next = part_tile(round + 1, ntiles);
            do_tile(BoolC<true>{}, BoolC<false>{}, tile, next, tile);
#pragma unroll
            for (int j = 0; j < kPartKPT; j++) kcur[j] = knext[j];
            tile = next;
        }
        if (tile < ntiles) do_tile(BoolC<false>{}, BoolC<false>{}, tile, ntiles, tile);
    } else if (tile >= nfull) {  // the block's only tile is the short one
        do_tile(BoolC<false>{}, BoolC<false>{}, tile, ntiles, tile);
        write_out(BoolC<false>{}, tile);
    } else {
        size_t prev = tile;
        {
            const size_t next = part_tile(1, ntiles);
            do_tile(BoolC<true>{}, BoolC<false>{}, tile, next, tile);
#pragma unroll
            for (int j = 0; j < kPartKPT; j++) kcur[j] = knext[j];
            tile = next;
        }
        for (size_t round = 1; tile < nfull; round++) {
            const size_t next = part_tile(round + 1, ntiles);
            do_tile(BoolC<true>{}, BoolC<true>{}, tile, next, prev);
#pragma unroll
            for (int j = 0; j < kPartKPT; j++) kcur[j] = knext[j];
            prev = tile;
            tile = next;
        }
        if (tile < ntiles) {
            do_tile(BoolC<false>{}, BoolC<true>{}, tile, ntiles, prev);
            write_out(BoolC<false>{}, tile);
        } else {
            write_out(BoolC<true>{}, prev);
        }
    }
}

// ---------------------------------------------------------------------------
// pass 1 on super-tiles (k_part_bin2, builds with many short runs: C4): one
// 1024-thread workgroup sorts a tile of kSuperTileKeys = 16,384 keys, two
// halves of 8,192 (A, B), so each segment's run of a tile is twice as long
// as k_part_bin's (C4: ~20 entries against ~10) and there are half as many
// (tile, segment) pairs for pass 2 to walk and half the run table.  Neither
// the sorted tile (49,152 entries, 192 KiB as u32) nor every position's
// entry and rank in registers fit (96 live values per thread spilled ~100
// VGPRs at the 128 of 4 waves per SIMD), so:
//   1. A's positions: bin + entry (bin_entry), rank in the JOINT histogram
//      (the rank atomic's return stays in a register), the key's three
//      entries packed into one u64 of an LDS stash (64 KiB, the thread's own
//      column: conflict-free);
//   2. B's positions: the same, entries kept in registers;
//   3. one scan of the joint counts: segment b's run of the super-tile is
//      [off(b), off(b + 1)), written to the run table;
//   4. every entry's index in the sorted super-tile, f = off(b) + rank (one
//      LDS read);
//   5. two phases of 24,576 sorted entries each: the entries whose f falls
//      in the phase (A's taken from the stash) are written to the 96 KiB LDS
//      image at f - phase base, which goes out packed as k_part_bin's.
// The histogram and the scan's wave sums live in the image's space (both
// are dead before the first phase writes): stash + image = all 160 KiB.
// Ranks reach 49,151, so the rank field is 18 bits: bins at << 20 (at most
// 4,095 bins), the bin's byte address is (rank value) >> 18.
// ---------------------------------------------------------------------------
constexpr uint32_t kBinShift2 = 20;
constexpr int kSuperBlock = 1024;

template <int LAYOUT>
__device__ __forceinline__ void load_half_keys(const KeySpan &ks, size_t tile, int half, int tid,
                                               int32_t (&k)[kPartKPT]) {
    constexpr size_t kHalf = (size_t)kSuperBlock * kPartKPT;
    const size_t i0 = tile * kSuperTileKeys + half * kHalf + (size_t)kPartKPT * tid;
    const bool full = tile * kSuperTileKeys + (half + 1) * kHalf <= ks.n;  // uniform per workgroup
    if constexpr (LAYOUT == KEYS_PACKED) {
        if (full) {
            const int4 *v = reinterpret_cast<const int4 *>(ks.base) + i0 / 4;
            const int4 a = v[0], b = v[1];
            k[0] = a.x; k[1] = a.y; k[2] = a.z; k[3] = a.w;
            k[4] = b.x; k[5] = b.y; k[6] = b.z; k[7] = b.w;
            return;
        }
    } else if constexpr (LAYOUT == KEYS_ENTRY) {
        if (full) {
            const int4 *v = reinterpret_cast<const int4 *>(ks.base) + i0 / 2;
            const int4 a = v[0], b = v[1], c = v[2], d = v[3];
            k[0] = a.x; k[1] = a.z; k[2] = b.x; k[3] = b.z;
            k[4] = c.x; k[5] = c.z; k[6] = d.x; k[7] = d.z;
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < kPartKPT; j++) {
        const size_t i = i0 + j;
        k[j] = i < ks.n ? load_key<LAYOUT>(ks, i) : 0;
    }
}

// SLOTS (the stacked probe's pass 1 on super-tiles): also each key's sorted
// index per hash, u16 (< 49,152), in the slot plane [tile][hash][key] the
// combine reads.
template <int LAYOUT, bool COLS, int MK, int MAXB, bool SLOTS = false>
__global__ void __launch_bounds__(kSuperBlock, 4) k_part_bin2(KeySpan ks, ModParams mp,
                                                              uint64_t *__restrict__ pos_out,
                                                              uint32_t *__restrict__ runs, SegMap sm,
                                                              size_t ntiles, uint16_t *__restrict__ slots) {
    constexpr int TB = kSuperBlock;
    constexpr int kHalfKeys = TB * kPartKPT;          // 8192
    constexpr int kTileKeys = 2 * kHalfKeys;          // 16384
    constexpr int kTilePos = 3 * kTileKeys;           // 49152
    constexpr int kPhasePos = kTilePos / 2;           // 24576 entries: 96 KiB
    constexpr uint32_t kPhaseBytes = 4u * kPhasePos;
    constexpr int kScanPer = (MAXB + 1 + TB - 1) / TB;
    constexpr int kPer = 3 * kPartKPT;                // positions per thread and half
    constexpr int kStashWords = 2 * kHalfKeys;        // one u64 per key of half A
    static_assert(4 * kTilePos <= (1 << 18) && kTilePos < (1 << 16) &&
                      ((uint64_t)MAXB << kBinShift2) < (1ull << 32),
                  "rank fields (the bin nbins, never incremented, included)");
    static_assert(kSuperTileKeys == (size_t)kTileKeys, "super-tile size");
    static_assert(MAXB + 1 + TB / 64 <= kPhasePos, "histogram and wave sums inside the image");
    // [image: kPhasePos][stash: kStashWords], histogram + wave sums at the
    // image's start until the phases.  The image first: an entry's slot is
    // then its LDS byte address (no add per write), and the stash is reached
    // through the offset field
    __shared__ __attribute__((aligned(16))) uint32_t s_pool[kPhasePos + kStashWords];
    uint32_t *img = s_pool;
    uint2 *stash = reinterpret_cast<uint2 *>(s_pool + kPhasePos);
    uint32_t *s_hist = img;
    uint32_t *s_wsum = img + MAXB + 1;
    char *img_b = reinterpret_cast<char *>(img);
    const char *hist_b = reinterpret_cast<const char *>(s_hist);

    const int nb = (int)sm.nbins;
    const int per = (nb + 1 + TB - 1) / TB;
    int32_t kA[kPartKPT], kB[kPartKPT];

    auto do_tile = [&](auto full_c, size_t tile, size_t next) {
        constexpr bool FULL = decltype(full_c)::value;
        // The thread index, opaque per tile: what derives from it (the scan's
        // bins and run-table pointers, stash and image addresses) is formed
        // in the tile, not hoisted out of the tile loop into ~30 registers
        // that the 128-VGPR cap then spilled.
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        const int lane = tid & 63, wave = tid >> 6;
        const size_t tile0 = tile * kTileKeys;
        const int tile_keys = FULL ? kTileKeys : (int)min((size_t)kTileKeys, ks.n - tile0);
        auto live = [&](int half, int j) { return FULL || half * kHalfKeys + kPartKPT * tid + j < tile_keys; };
        // B's keys load under A's hashing (needed only after it)
        load_half_keys<LAYOUT>(ks, tile, 1, tid, kB);
        lds_barrier();  // the previous tile's image and stash reads are done
#pragma clang loop unroll(disable) vectorize(disable)
        for (int b = tid; b <= nb; b += TB) s_hist[b] = (uint32_t)b << kBinShift2;
        lds_barrier();

        // 1. A: rank in the joint histogram, the key's entries to the stash
        uint32_t brA[kPer], brB[kPer], eB[2 * kPartKPT];
#pragma unroll
        for (int j = 0; j < kPartKPT; j++) {
            uint32_t e[3];
#pragma unroll
            for (int h = 0; h < 3; h++) {
                const int q = 3 * j + h;
                e[h] = 0;
                if (live(0, j)) {
                    const uint64_t raw = h == 0 ? raw_hash1(kA[j]) : h == 1 ? raw_hash2(kA[j]) : raw_hash3(kA[j]);
                    uint32_t b;
                    bin_entry<MK, 4>(raw, mp, sm, b, e[h]);
                    brA[q] = atomicAdd(&s_hist[b], 4u);
                } else {
                    brA[q] = 0;
                }
            }
            stash[j * TB + tid] = pack_entries3(e[0], e[1], e[2]);
            __builtin_amdgcn_sched_barrier(0);
        }
        // 2. B: the same, the key's entries kept packed (two registers for
        //    three entries: the unpacked 24 spilled)
#pragma unroll
        for (int j = 0; j < kPartKPT; j++) {
            uint32_t e[3];
#pragma unroll
            for (int h = 0; h < 3; h++) {
                const int q = 3 * j + h;
                e[h] = 0;
                if (live(1, j)) {
                    const uint64_t raw = h == 0 ? raw_hash1(kB[j]) : h == 1 ? raw_hash2(kB[j]) : raw_hash3(kB[j]);
                    uint32_t b;
                    bin_entry<MK, 4>(raw, mp, sm, b, e[h]);
                    brB[q] = atomicAdd(&s_hist[b], 4u);
                } else {
                    brB[q] = 0;
                }
            }
            const uint2 pk = pack_entries3(e[0], e[1], e[2]);
            eB[2 * j] = pk.x;
            eB[2 * j + 1] = pk.y;
            __builtin_amdgcn_sched_barrier(0);
        }
        lds_barrier();

        // 3. exclusive scan of the joint counts (k_part_bin step 2)
        const bool scan_wave = wave * 64 * per <= nb;
        uint32_t local[kScanPer];
        uint32_t tsum = 0, incl = 0;
        if (scan_wave) {
#pragma unroll
            for (int q = 0; q < kScanPer; q++) {
                const int b = tid * per + q;
                local[q] = (q < per && b <= nb) ? s_hist[b] - ((uint32_t)b << kBinShift2) : 0u;
                tsum += local[q];
            }
            incl = wave_incl_scan(tsum);
            if (lane == 63) s_wsum[wave] = incl;
        }
        lds_barrier();
        if (scan_wave) {
            uint32_t run = incl - tsum;
            for (int w = 0; w < wave; w++) run += s_wsum[w];
#pragma unroll
            for (int q = 0; q < kScanPer; q++) {
                const int b = tid * per + q;
                if (q < per && b <= nb) {
                    s_hist[b] = run - ((uint32_t)b << kBinShift2);
                    const uint32_t pk = (run >> 2) | (((run + local[q]) >> 2) << 16);
                    if (b < nb) {
                        if constexpr (COLS) runs[(size_t)b * ntiles + tile] = pk;
                        else runs[tile * (size_t)nb + b] = pk;
                    }
                    run += local[q];
                }
            }
        }
        lds_barrier();
        if (next < ntiles) load_half_keys<LAYOUT>(ks, next, 0, tid, kA);

        // 4. every entry's byte slot in the sorted super-tile (dead: ~0, in
        //    no phase); in groups of 6 (the scheduler would otherwise issue
        //    all 48 reads first, into 48 more registers)
#pragma unroll
        for (int q = 0; q < kPer; q++) {
            const uint32_t fa = *reinterpret_cast<const uint32_t *>(hist_b + (brA[q] >> 18)) + brA[q];
            const uint32_t fb = *reinterpret_cast<const uint32_t *>(hist_b + (brB[q] >> 18)) + brB[q];
            brA[q] = live(0, q / 3) ? fa : ~0u;
            brB[q] = live(1, q / 3) ? fb : ~0u;
            // formed here: the compiler otherwise defers the add into both
            // phases and keeps the read offset and the rank value apart
            // (two registers per entry instead of one)
            asm volatile("" : "+v"(brA[q]), "+v"(brB[q]));
            if (q % 6 == 5) __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (SLOTS) {
            // key 8 tid + j of half A and 8192 + 8 tid + j of half B: their
            // sorted index per hash, one non-temporal 16-B store per half and
            // hash (read once, by the combine, after pass 2)
            uint16_t *sl = slots + tile * 3 * (size_t)kTileKeys + kPartKPT * tid;
            if constexpr (FULL) {
                typedef uint32_t v4u __attribute__((ext_vector_type(4)));
#pragma unroll
                for (int h = 0; h < 3; h++) {
                    // byte slots: 4 | slot, so (odd << 14) | (even >> 2)
                    const v4u wa = {lshl_or(brA[3 + h], 14, brA[h] >> 2), lshl_or(brA[9 + h], 14, brA[6 + h] >> 2),
                                    lshl_or(brA[15 + h], 14, brA[12 + h] >> 2),
                                    lshl_or(brA[21 + h], 14, brA[18 + h] >> 2)};
                    const v4u wb = {lshl_or(brB[3 + h], 14, brB[h] >> 2), lshl_or(brB[9 + h], 14, brB[6 + h] >> 2),
                                    lshl_or(brB[15 + h], 14, brB[12 + h] >> 2),
                                    lshl_or(brB[21 + h], 14, brB[18 + h] >> 2)};
                    __builtin_nontemporal_store(wa, reinterpret_cast<v4u *>(sl + h * kTileKeys));
                    __builtin_nontemporal_store(wb, reinterpret_cast<v4u *>(sl + h * kTileKeys + kHalfKeys));
                }
            } else {
#pragma unroll
                for (int j = 0; j < kPartKPT; j++) {
#pragma unroll
                    for (int h = 0; h < 3; h++) {
                        if (live(0, j)) sl[h * kTileKeys + j] = (uint16_t)(brA[3 * j + h] >> 2);
                        if (live(1, j)) sl[h * kTileKeys + kHalfKeys + j] = (uint16_t)(brB[3 * j + h] >> 2);
                    }
                }
            }
        }
        lds_barrier();  // the histogram is read: the image is free

        // 5. two phases of kPhasePos sorted entries through the LDS image
        uint4 *dst = reinterpret_cast<uint4 *>(pos_out + tile * (size_t)kTileKeys);
        constexpr int kVecs = kPhasePos / 6;  // 16-B vectors per phase
        constexpr int kStores = kVecs / TB;
        static_assert(kStores * TB == kVecs, "whole vectors per thread");
#pragma unroll
        for (int ph = 0; ph < 2; ph++) {
            const uint32_t base = ph * kPhaseBytes;
            // the stash words of all 8 keys first (one wait), then the
            // conditional writes: a read inside each branch waited for the
            // LDS round trip once per entry
            uint2 w[kPartKPT];
#pragma unroll
            for (int j = 0; j < kPartKPT; j++) w[j] = stash[j * TB + tid];
#pragma unroll
            for (int j = 0; j < kPartKPT; j++) {
#pragma unroll
                for (int h = 0; h < 3; h++) {
                    const uint32_t la = brA[3 * j + h] - base;
                    if (la < kPhaseBytes) {
                        const uint32_t e = h == 0 ? w[j].x & kEntryMask
                                         : h == 1 ? __builtin_amdgcn_alignbit(w[j].y, w[j].x, 21) & kEntryMask
                                                  : w[j].y >> 10;
                        *reinterpret_cast<uint32_t *>(img_b + la) = e;
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < kPartKPT; j++) {
#pragma unroll
                for (int h = 0; h < 3; h++) {
                    const uint32_t lb = brB[3 * j + h] - base;
                    if (lb < kPhaseBytes) {
                        const uint32_t lo = eB[2 * j], hi = eB[2 * j + 1];
                        const uint32_t e = h == 0 ? lo & kEntryMask
                                         : h == 1 ? __builtin_amdgcn_alignbit(hi, lo, 21) & kEntryMask
                                                  : hi >> 10;
                        *reinterpret_cast<uint32_t *>(img_b + lb) = e;
                    }
                }
            }
            lds_barrier();
#pragma unroll
            for (int r = 0; r < kStores; r++) {
                const uint2 *src = reinterpret_cast<const uint2 *>(img + 6 * (r * TB + tid));
                const uint2 a = src[0], b = src[1], c = src[2];
                uint32_t e[6] = {a.x, a.y, b.x, b.y, c.x, c.y};
                if constexpr (!FULL) {
#pragma unroll
                    for (int z = 0; z < 6; z++) e[z] &= kEntryMask;
                }
                // (plain stores: non-temporal ones, as k_part_bin's at C5, made
                // C4's pass 1 slower, 1.299 -> 1.317 ms, more than pass 2 gained)
                dst[ph * kVecs + r * TB + tid] = pack_entries6(e);
            }
            if (ph == 0) lds_barrier();  // phase 0's image is read before phase 1 writes
        }
    };

    const size_t nfull = ks.n / kTileKeys;
    size_t tile = part_tile(0, ntiles);
    if (tile < ntiles) load_half_keys<LAYOUT>(ks, tile, 0, (int)threadIdx.x, kA);
    size_t round = 0;
    for (; tile < nfull; round++) {
        const size_t next = part_tile(round + 1, ntiles);
        do_tile(BoolC<true>{}, tile, next);
        tile = next;
    }
    if (tile < ntiles) do_tile(BoolC<false>{}, tile, ntiles);
}

// ---------------------------------------------------------------------------
// run-table transpose: pass 1 writes one row of nbins packed runs per tile
// (contiguous, cheap); pass 2 wants, per segment, its run bounds of all tiles
// contiguous.  A 64 x 64 LDS-tiled transpose: 256-B coalesced reads and
// writes, the LDS tile padded one word per row against bank conflicts.
// Small tables are written straight from pass 1 as columns (COLS): at C2
// (4 MiB) that costs ~2 us against ~6 us for a transpose launch.  Large ones
// go through the transpose: at C4 (805 MB) the column stores cost ~2.1 ms
// (partial-line write-backs), the transpose 0.39 ms (tools/ubench.py part*).
// The environment variable BLOOMHIP_RUN_TABLE = rows | cols forces one layout
// at any size (runs_as_columns reads it on every call; unset or any other
// value keeps the threshold).  Both are right at any size: partition_buffers
// allocates both tables and launch_bin transposes whenever the table went out
// as rows.  tests/test_gpu_run_table.py runs the rows kernels and the
// transpose at small shapes with it.
// ---------------------------------------------------------------------------
constexpr size_t kColumnTableMaxBytes = 16u << 20;  // larger run tables: rows + transpose
constexpr int kTransposeTile = 64;
constexpr int kTransposeBlock = 256;

}  // namespace

// Exported by the kernel translation units (one instantiation family each).
hipError_t launch_runs_transpose(const PartitionWorkspace &ws, hipStream_t stream);  // bloom_kernels.hip
bool runs_as_columns(const PartitionWorkspace &ws);                                  // bloom_kernels.hip

// Everything one pass-1 launch is compiled and launched with, as
// choose_pass1_kernel returns it (template parameter of k_part_bin /
// k_part_bin2 in capitals).
struct Pass1Kernel {
    bool super;      // k_part_bin2 on super-tiles, else k_part_bin
    int threads;     // TB: 512 (4096-key tiles) or 1024 (8192-key tiles, super-tiles)
    int layout;      // LAYOUT: KEYS_PACKED / KEYS_ENTRY (16-B aligned base only) / KEYS_STRIDED
    bool slots;      // SLOTS: a probe, with the slot plane
    bool cols;       // COLS: runs straight into the segment-major table, else rows + transpose
    int mk;          // MK: the reduction kind, kMod*
    int maxb;        // MAXB: histogram capacity
    int wgs_per_cu;  // resident workgroups per CU: MINW = pass1_min_waves(threads, wgs_per_cu)
    bool nt;         // ST = kStoreNT: the sorted tiles stored non-temporal
    bool wt;         // ST = kStoreWT: the sorted tiles stored write-through
    bool defer;      // DEFER: a tile's write-out inside the next tile's hash phase
    unsigned grid;   // persistent workgroups
    int prio;        // PRIO: the phases' issue priority (pass1_prio_of), 0 = none
    int pipe;        // PIPE: a tile scattered inside the next tile's hash phase, 0 = the plain loop
};
// pass 1: the unit of each family launches the kernel p names; false when it
// holds no such kernel.  Build / probe (slots) at 512 or 1024 threads
// (bloom_pass1_*.hip), a build / probe on super-tiles (bloom_pass1_super*.hip).
using Pass1Launch = bool(const Pass1Kernel &p, const KeySpan &ks, const ModParams &mp,
                         const PartitionWorkspace &ws, const SegMap &sm, uint16_t *slots,
                         hipStream_t stream);
// (six function declarations, one signature: each unit defines its own)
Pass1Launch launch_bin_build512, launch_bin_build1024, launch_bin_probe512, launch_bin_probe1024,
    launch_bin_super, launch_bin_super_probe;

namespace {

// The most segments a family's histogram and rank fields hold.
constexpr int pass1_max_bins(bool super, int threads) {
    return super ? (int)kSuperMaxBins : threads >= 1024 ? (int)kPartMaxBinsBig : (int)kPartMaxBins;
}

// The reduction kinds a family takes: the one-member ladder is a build's;
// super-tiles sort segments of m < 2^32.
constexpr bool pass1_takes_kind(bool super, bool slots, int mk) {
    if (super) return mk == kModP2 || mk == kModFast;
    return mk >= 0 && !(slots && (mk == kModLadder0 || mk == kModLadder0R));
}

// One pass-1 launch: MAXB is the histogram capacity the kernel is compiled
// for (its scan loop and registers follow it, so a small capacity is cheaper:
// C2's 256 segments at MAXB 511 run pass 1 in 74.5 us against 87 at 4096,
// tools/ubench.py part with UB_P1).  Only the packed / entry_t fast paths get
// the small capacities; strided keys and m >= 2^32 use the largest.
constexpr int pass1_capacity(int threads, int layout, int mk, size_t nbins) {
    const int cap = pass1_max_bins(false, threads);
    if (layout == KEYS_STRIDED || mk == kModWide) return cap;
    if (threads >= 1024) return nbins <= 1023 ? 1023 : nbins <= 2047 ? 2047 : nbins <= 4095 ? 4095 : cap;
    return nbins <= 511 ? 511 : cap;
}

// Workgroups of pass 1 resident per CU: the 4096-key build tile with a
// histogram of <= 511 bins takes 50 KiB of LDS, so three fit a CU when the
// registers are capped for 6 waves per SIMD (80 VGPRs, 2 spilled): C2 pass 1
// 59.5 -> 58.1 us (tools/ubench.py p1ab, variant 5003).  Everything else:
// two 512-thread or one 1024-thread workgroup per CU.
constexpr int pass1_wgs_per_cu(int threads, bool slots, int maxb) {
    return threads >= 1024 ? 1 : (!slots && maxb > 0 && maxb <= 511) ? 3 : 2;
}
// waves per SIMD the registers must allow (MINW) for wgs workgroups per CU
constexpr int pass1_min_waves(int threads, int wgs) { return wgs * threads / 256; }
// persistent workgroups: every resident slot of the device, at most one per tile
inline unsigned pass1_grid(size_t ntiles, int ncu, int wgs) {
    const size_t g = (size_t)ncu * wgs;
    return (unsigned)(ntiles < g ? ntiles : g);
}

// The write-out is deferred into the next tile's hash phase (k_part_bin's
// DEFER) where that measured faster: the 1024-thread builds (C5 0.394 ->
// 0.385 ms).  With the slot plane (C3's probe) it is level, and on 512
// threads at three workgroups per CU (C2) slower, 54.7 -> 56.0 us.
constexpr bool pass1_defer(int threads, bool slots) { return threads >= 1024 && !slots; }

// The phases' issue priority (k_part_bin's PRIO, pass1_prio_of(mode, level)).
// It matters only where workgroups in different phases share a CU.  The
// 512-thread builds on three workgroups per CU (C2) hash at priority 1 and
// sort at 0: pass 1 55.1 -> 49.8 us, the C2 build 0.0887 -> 0.0841 ms
// (0.0888 -> 0.0836 with the parent first), the median below the parent's
// fastest run in both orders; levels 2 and 3 measure as 1.  Raising the sort
// phases, or only scatter + packing, costs 0.5 us at any level; one static
// level for waves 4-7 gained 0.8 us in one run and nothing in the next; the
// static form on one 1024-thread workgroup per CU is level (C5 216.3 / 216.4
// us, the f = 10 build 71.0 / 71.3).  Not measured, so 0: 512 threads on two
// workgroups per CU (strided keys, m >= 2^32, the probe with its slot plane).
// (profiles/pass1_priority/README.md; tools/ubench.py p1ab, p1abl.)
constexpr int pass1_prio(int threads, bool slots, int wgs_per_cu) {
    return threads == 512 && !slots && wgs_per_cu == 3 ? pass1_prio_of(kPrioHash, 1) : 0;
}

// The software-pipelined tile loop (k_part_bin's PIPE), in the family that got
// the hash-phase priority, the 512-thread builds on three workgroups per CU
// (packed and entry_t keys): on the one-member ladder (kModLadder0,
// kModLadder0R), whose pipelined kernels keep to 80 VGPRs with 0-6 spilled.
// C2's pass 1 49.1 -> 46.5 us, the C2 build 0.0818 -> 0.0786 ms in both
// orders, every run of it below the parent's fastest; from entry_t keys the
// build is level (0.4226 / 0.4225 ms, 0.4214 / 0.4232).  Not on the general
// and p2 remainders: their longer hashing spills 22-26 VGPRs around the 48
// ranks and entries the loop keeps live through every phase, and the general
// build (m = 100,000,007) measured 0.379 -> 0.418 ms; the p2 form, with the
// same spills, was not measured.  Not built for the slot-plane kernels, the
// two-workgroup 512-thread kernels (strided keys, m >= 2^32) and the
// 1024-thread builds.  (profiles/pass1_scatter_overlap/README.md;
// tools/ubench.py p1ab_pipe, p1abl pipe; tools/build_ab.py c2, c2e, gen.)
constexpr int pass1_pipe(int threads, bool slots, int wgs_per_cu, int mk) {
    return threads == 512 && !slots && wgs_per_cu == 3 && (mk == kModLadder0 || mk == kModLadder0R) ? 1 : 0;
}

// builds whose sorted tiles exceed the Infinity Cache (C5): stored
// non-temporal (k_part_bin's kStoreNT); compiled for the 1024-thread builds at
// MAXB 1023 alone
constexpr bool pass1_may_nt(int threads, bool slots, int maxb) {
    return !slots && threads >= 1024 && maxb == 1023;
}

// builds from packed keys in the family of the pipelined loop (C2), while the
// sorted tiles fit the Infinity Cache (choose_pass1_kernel checks the size):
// stored write-through (k_part_bin's kStoreWT).  With plain stores pass 1
// ends with the L2s full of dirty tile lines, which are flushed at the kernel
// boundary while nothing runs.  Measured in this family alone, so entry_t
// keys (at the edge of their spread written through), every other family
// and batches beyond the Infinity Cache keep their stores
// (profiles/build_edges/README.md).
constexpr bool pass1_wt(int pipe, int layout) { return pipe != 0 && layout == KEYS_PACKED; }

// Whether pass 1 may take the p2 reduction (kModP2) for this geometry: the
// entry must be the hash's low kEntryBits bits (t >= 21) and p >> shift must
// reach bit t (shift <= t).
inline bool p2_pass1(const ModParams &mp, const SegMap &sm) {
    return mp.fast && mp.p2 && mp.p2t >= kEntryBits && sm.shift <= mp.p2t && mp.p2t - sm.shift < 32;
}

// Pass 1's reduction kind (kMod*) and segment map for a batch on geometry
// ws, as k_part_bin is launched with them; -1 when the geometry is not one
// pass 1 takes.  (tools/ubench.py prices bin_entry with these alone.)
inline int pass1_plan(const ModParams &mp, const PartitionWorkspace &ws, bool slots, SegMap *out) {
    SegMap sm = seg_map_of(ws);
    const bool wide = !mp.fast;
    if (!wide) {  // the fast path shifts the remainder scaled by 2^l
        sm.scaled_shift = sm.shift + mp.l;
        if (sm.scaled_shift > 31) {  // m < 2^(32-l) <= 2^shift: every p is in segment 0
            sm.scaled_shift = 0;
            sm.magic = 0;
        }
    }
    int mk;
    if (ws.lad_u) {  // ladder stack: bins are hash bits [s, s + u) (plan_ladder)
        if (!mp.fast || !mp.p2 || sm.shift + sm.lad_u + sm.lad_hb != mp.p2t) return -1;
        sm.scaled_shift = sm.shift + sm.lad_u;
        // plan_build's one-member ladder, relabelled where 24 lies in [s, t]
        mk = sm.lad_hb == 0 && !slots ? (ladder0_relabel(mp, ws) ? kModLadder0R : kModLadder0) : kModLadder;
    } else if (wide) {
        mk = kModWide;
    } else if (p2_pass1(mp, sm)) {
        sm.p2_hi_shift = mp.p2t - sm.shift;
        mk = kModP2;
    } else {
        mk = kModFast;
    }
    *out = sm;
    return mk;
}

// The pass-1 kernel of a build (slots = false) or a probe (slots = true) of
// batch ks on geometry ws, on a device of ncu CUs, and the segment map it is
// launched with: every rule of the choice, each with what was measured for
// it above.  False for a geometry pass 1 does not take.  No device call.
inline bool choose_pass1_kernel(const KeySpan &ks, const ModParams &mp, const PartitionWorkspace &ws,
                                bool slots, int ncu, Pass1Kernel *out, SegMap *sm) {
    Pass1Kernel p{};
    // Pass 1 on super-tiles (k_part_bin2): builds whose geometry plan_build gave
    // kSuperTileKeys (segments of m < 2^32, more than kSuperMinBins of them),
    // and plan_stack's probes on as many.  Else k_part_bin: 1024 threads for
    // the 8192-key tile (choose_tile_keys), 512 for the 4096-key one.
    p.super = tile_keys_of(ws) == kSuperTileKeys;
    p.threads = p.super ? kSuperBlock : tile_keys_of(ws) == 2 * kPartTileKeys ? 1024 : 512;
    p.slots = slots;
    if (ws.nbins > (size_t)pass1_max_bins(p.super, p.threads)) return false;
    p.mk = pass1_plan(mp, ws, slots, sm);
    if (p.mk < 0 || !pass1_takes_kind(p.super, slots, p.mk)) return false;
    // entry_t runs are read as 16-B vectors: from a 16-B aligned base only
    p.layout = ks.layout == KEYS_PACKED ? KEYS_PACKED
               : ks.layout == KEYS_ENTRY && (reinterpret_cast<uintptr_t>(ks.base) & 15) == 0 ? KEYS_ENTRY
                                                                                               : KEYS_STRIDED;
    p.maxb = p.super ? (int)kSuperMaxBins : pass1_capacity(p.threads, p.layout, p.mk, ws.nbins);
    p.wgs_per_cu = p.super ? 1 : pass1_wgs_per_cu(p.threads, slots, p.maxb);
    p.defer = !p.super && pass1_defer(p.threads, slots);
    p.nt = !p.super && pass1_may_nt(p.threads, slots, p.maxb) &&
           ws.ntiles * (uint64_t)(p.threads * kPartKPT) * 8 > kInfinityCacheBytes;
    p.prio = p.super ? 0 : pass1_prio(p.threads, slots, p.wgs_per_cu);
    p.pipe = p.super ? 0 : pass1_pipe(p.threads, slots, p.wgs_per_cu, p.mk);
    p.wt = !p.nt && pass1_wt(p.pipe, p.layout) &&
           ws.ntiles * (uint64_t)(p.threads * kPartKPT) * 8 <= kInfinityCacheBytes;
    p.cols = runs_as_columns(ws);
    p.grid = pass1_grid(ws.ntiles, ncu, p.wgs_per_cu);
    *out = p;
    return true;
}

// Launches the k_part_bin that p names, of the family <SLOTS, TB>.  The
// family holds exactly the kernels choose_pass1_kernel can return for it: a
// reduction kind the family takes, at a capacity pass1_capacity gives for
// the layout and kind (one it maps to itself).
template <bool SLOTS, int TB>
bool launch_pass1_tile(const Pass1Kernel &p, const KeySpan &ks, const ModParams &mp,
                       const PartitionWorkspace &ws, const SegMap &sm, uint16_t *slots,
                       hipStream_t stream) {
    constexpr bool kDefer = pass1_defer(TB, SLOTS);
    if (p.super || p.threads != TB || p.slots != SLOTS || p.defer != kDefer) return false;
    uint32_t *runs = p.cols ? ws.run_starts : ws.run_rows;
    return on_value<kModFast, kModWide, kModP2, kModLadder, kModLadder0, kModLadder0R>(p.mk, [&](auto mk_c) {
        return on_value<KEYS_PACKED, KEYS_ENTRY, KEYS_STRIDED>(p.layout, [&](auto layout_c) {
            return on_value<511, 1023, 2047, 4095, pass1_max_bins(false, TB)>(p.maxb, [&](auto maxb_c) {
                constexpr int MK = decltype(mk_c)::value, L = decltype(layout_c)::value;
                constexpr int MAXB = decltype(maxb_c)::value;
                constexpr bool kHeld = pass1_takes_kind(false, SLOTS, MK) && pass1_capacity(TB, L, MK, MAXB) == MAXB;
                if constexpr (kHeld) {
                    constexpr int kWgs = pass1_wgs_per_cu(TB, SLOTS, MAXB);
                    constexpr int kMinW = pass1_min_waves(TB, kWgs);
                    constexpr bool kMayNT = pass1_may_nt(TB, SLOTS, MAXB);
                    constexpr int kPrio = pass1_prio(TB, SLOTS, kWgs);
                    constexpr int kPipe = pass1_pipe(TB, SLOTS, kWgs, MK);
                    constexpr bool kMayWT = pass1_wt(kPipe, L);
                    if (p.wgs_per_cu != kWgs || (p.nt && !kMayNT) || p.prio != kPrio || p.pipe != kPipe ||
                        (p.wt && !kMayWT) || (p.nt && p.wt))
                        return false;
                    auto go = [&](auto cols_c, auto st_c) {
                        k_part_bin<L, SLOTS, decltype(cols_c)::value, TB, MK, MAXB, kMinW, 0, decltype(st_c)::value,
                                   kDefer, kPrio, kPipe>
                            <<<p.grid, TB, 0, stream>>>(ks, mp, ws.pos, runs, sm, ws.ntiles, slots);
                    };
                    using StNT = std::integral_constant<int, kStoreNT>;
                    using StWT = std::integral_constant<int, kStoreWT>;
                    using StPlain = std::integral_constant<int, kStorePlain>;
                    if constexpr (kMayNT) {
                        if (p.nt) {
                            p.cols ? go(BoolC<true>{}, StNT{}) : go(BoolC<false>{}, StNT{});
                            return true;
                        }
                    }
                    if constexpr (kMayWT) {
                        if (p.wt) {
                            p.cols ? go(BoolC<true>{}, StWT{}) : go(BoolC<false>{}, StWT{});
                            return true;
                        }
                    }
                    p.cols ? go(BoolC<true>{}, StPlain{}) : go(BoolC<false>{}, StPlain{});
                    return true;
                } else {
                    return false;
                }
            });
        });
    });
}

// The same for k_part_bin2, of the family <SLOTS>: the kinds
// pass1_takes_kind lists for super-tiles, every layout, one capacity.
template <bool SLOTS>
bool launch_pass1_super(const Pass1Kernel &p, const KeySpan &ks, const ModParams &mp,
                        const PartitionWorkspace &ws, const SegMap &sm, uint16_t *slots,
                        hipStream_t stream) {
    if (!p.super || p.slots != SLOTS) return false;
    uint32_t *runs = p.cols ? ws.run_starts : ws.run_rows;
    return on_value<kModP2, kModFast>(p.mk, [&](auto mk_c) {
        return on_value<KEYS_PACKED, KEYS_ENTRY, KEYS_STRIDED>(p.layout, [&](auto layout_c) {
            auto go = [&](auto cols_c) {
                k_part_bin2<decltype(layout_c)::value, decltype(cols_c)::value, decltype(mk_c)::value,
                            (int)kSuperMaxBins, SLOTS>
                    <<<p.grid, kSuperBlock, 0, stream>>>(ks, mp, ws.pos, runs, sm, ws.ntiles, slots);
            };
            p.cols ? go(BoolC<true>{}) : go(BoolC<false>{});
            return true;
        });
    });
}

// Pass 1 for a build (SLOTS = false) or a probe (SLOTS = true): the kernel
// choose_pass1_kernel gives, from the unit that holds its family, then the
// run-start transpose when the table is large.
template <bool SLOTS>
hipError_t launch_bin(const KeySpan &ks, const ModParams &mp, const PartitionWorkspace &ws,
                      uint16_t *slots, hipStream_t stream) {
    Pass1Kernel p{};
    SegMap sm{};
    if ((SLOTS && !slots) || !choose_pass1_kernel(ks, mp, ws, SLOTS, device_cu_count(), &p, &sm))
        return hipErrorInvalidValue;
    Pass1Launch *unit;
    if constexpr (SLOTS)
        unit = p.super ? launch_bin_super_probe : p.threads >= 1024 ? launch_bin_probe1024 : launch_bin_probe512;
    else
        unit = p.super ? launch_bin_super : p.threads >= 1024 ? launch_bin_build1024 : launch_bin_build512;
    if (!unit(p, ks, mp, ws, sm, SLOTS ? slots : nullptr, stream)) return hipErrorInvalidValue;
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || p.cols) return e;
    return launch_runs_transpose(ws, stream);
}

}  // namespace

}  // namespace bloomhip
