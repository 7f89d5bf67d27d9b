// bloom_flush.hip — the batched PUT: a batch of puts and deletes, in arrival
// order, sorted into a run on the device (bloomhip_flush_batch).
//
// Reference: LSMTree::put (src/lsm_tree.cpp:104-139) inserts into Buffer, a
// std::set<entry_t> ordered by key in which a second put of a key replaces the
// first (src/buffer.cpp:37-58); del is a put of VAL_TOMBSTONE
// (src/lsm_tree.cpp:292-294), load a put per record (:296-309); a flush walks
// the set in key order into a new run (:124-131).
//
// On the GPU: a stable least-significant-digit radix sort of the 8-byte
// records on the key (sign bit flipped, so unsigned digit order is signed key
// order), 8-bit digits.  The first pass reads the ops back to front, so
// stability leaves the ops of one key newest first and the compaction's dedup
// (bloom_merge.hip launch_dedup: first entry of every key) keeps the last
// writer.
//
// Tiled path, per digit pass: k_flush_count (digit counts per tile of
// kFlushTile records, laid out [digit][tile]), k_flush_scan twice (an exclusive
// scan of that table: chunks of kFlushScanChunk, then the chunk totals), and
// k_flush_scatter: the tile is ranked stably (tile_positions), reordered by
// digit in LDS, and every digit's segment leaves with consecutive lanes on
// consecutive addresses.  Workgroups synchronise at kernel boundaries only.
// One-workgroup path (k_flush_block): up to kFlushBlockCap ops, every pass
// and the dedup in one launch, with the same ranking code.
//
// Ranking: wave w of a tile owns records [w * 64 * kFlushIpt, ..) in
// kFlushIpt rounds of 64 consecutive records.  Per round the lanes holding one
// digit are found with 8 ballots; a lane's rank among them is mbcnt of that
// mask, and the wave's running count of the digit (LDS, touched by this wave
// only, rounds in program order) places the round after the earlier ones: no
// atomics, so the order is the record order.  Offsets come only from these
// counts; a key is never an address, and every store index is clamped.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "bloom_flush.h"

namespace bloomhip {
namespace {

constexpr int32_t kTombstone = INT32_MIN;  // VAL_TOMBSTONE, src/types.h:12
constexpr uint32_t kSignFlip = 0x80000000u;
constexpr int kHistWords = kFlushPasses * kFlushBins;
constexpr int kScanBlock = 1024;
constexpr int kScanIpt = kFlushScanChunk / kScanBlock;

template <int WAVES>
struct TileLds {
    uint32_t cnt[WAVES][kFlushBins];  // per-wave digit counts, then the wave's base in the digit
    uint32_t start[kFlushBins];       // the digit's first slot in the tile
    uint32_t s_w[WAVES];
};

__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

template <int WAVES>
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t *s_w, uint32_t *total) {
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
    for (int w = 0; w < WAVES; w++) {
        const uint32_t t = s_w[w];
        if (w < wave) base += t;
        all += t;
    }
    __syncthreads();
    if (total) *total = all;
    return base + incl - v;
}

// The record a lane holds in round j of its wave, as an index in the tile,
// when every wave owns `rounds` rounds (kFlushIpt in a full tile; fewer when a
// small batch is spread over all waves of its workgroup).  Rounds at or past
// `rounds` hold nothing: their index is past every tile.
__device__ __forceinline__ uint32_t tile_index(int j, uint32_t rounds = kFlushIpt) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    return (uint32_t)j < rounds ? wave * (64u * rounds) + (uint32_t)j * 64u + lane : ~0u;
}

// pos[j] = the slot of record tile_index(j, rounds) (key ukey[j], sign already
// flipped) in the tile stably sorted on digit (ukey >> shift) & 255; records
// at tile_index >= tile_n do not take part.  L.start[d] is left holding digit
// d's first slot.  Every lane of the workgroup calls this.
template <int WAVES>
__device__ __forceinline__ void tile_positions(const uint32_t (&ukey)[kFlushIpt], uint32_t tile_n,
                                               uint32_t shift, TileLds<WAVES> &L,
                                               uint32_t (&pos)[kFlushIpt],
                                               uint32_t rounds = kFlushIpt) {
    static_assert(WAVES * 64 >= kFlushBins, "one lane per digit in the tile scan");
    const uint32_t wave = threadIdx.x >> 6;
    for (uint32_t i = threadIdx.x; i < WAVES * kFlushBins; i += WAVES * 64) (&L.cnt[0][0])[i] = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kFlushIpt; j++) {
        if ((uint32_t)j < rounds) {  // uniform
            const bool valid = tile_index(j, rounds) < tile_n;
            const uint32_t d = (ukey[j] >> shift) & (kFlushBins - 1);
            uint64_t same = __ballot(valid);
#pragma unroll
            for (int b = 0; b < kFlushDigitBits; b++) {
                const bool bit = (d >> b) & 1;
                const uint64_t m = __ballot(bit);
                same &= bit ? m : ~m;
            }
            // the wave's count of d before this round; its lowest lane adds
            // the round's.  One wave, program order: the read is done before
            // the write, and the next round's read sees it.
            const uint32_t before = L.cnt[wave][d];
            __builtin_amdgcn_wave_barrier();
            const uint32_t r = lanes_below(same);
            if (valid && r == 0) L.cnt[wave][d] = before + (uint32_t)__popcll(same);
            __builtin_amdgcn_wave_barrier();
            pos[j] = before + r;
        }
    }
    __syncthreads();
    uint32_t c = 0;
    if (threadIdx.x < kFlushBins) {
#pragma unroll
        for (int w = 0; w < WAVES; w++) {
            const uint32_t t = L.cnt[w][threadIdx.x];
            L.cnt[w][threadIdx.x] = c;
            c += t;
        }
    }
    const uint32_t ex = block_exclusive_scan<WAVES>(c, L.s_w, nullptr);
    if (threadIdx.x < kFlushBins) L.start[threadIdx.x] = ex;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kFlushIpt; j++) {
        const uint32_t d = (ukey[j] >> shift) & (kFlushBins - 1);
        pos[j] += L.start[d] + L.cnt[wave][d];
    }
}

// Element i of the pass's input: in[i], or in[n - 1 - i] when reverse.
__device__ __forceinline__ uint2 load_op(const uint2 *__restrict__ in, uint64_t n, uint64_t i,
                                         int reverse) {
    return in[reverse ? n - 1 - i : i];
}

__global__ void __launch_bounds__(256) k_flush_hist(const uint2 *__restrict__ in, uint64_t n,
                                                    uint32_t *__restrict__ hist) {
    __shared__ uint32_t s_h[kHistWords];
    for (int i = threadIdx.x; i < kHistWords; i += 256) s_h[i] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint32_t u = in[i].x ^ kSignFlip;
#pragma unroll
        for (int p = 0; p < kFlushPasses; p++)
            atomicAdd(&s_h[p * kFlushBins + ((u >> (p * kFlushDigitBits)) & (kFlushBins - 1))], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kHistWords; i += 256)
        if (s_h[i]) atomicAdd(&hist[i], s_h[i]);
}

// counts[d * ntiles + tile] = the tile's records with digit d.
__global__ void __launch_bounds__(256) k_flush_count(const uint2 *__restrict__ in, uint64_t n,
                                                     int reverse, uint32_t shift, uint32_t ntiles,
                                                     uint32_t *__restrict__ counts) {
    __shared__ uint32_t s_h[kFlushBins];
    s_h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kFlushTile;
#pragma unroll
    for (int j = 0; j < kFlushIpt; j++) {
        const uint64_t i = base + (uint32_t)j * 256u + threadIdx.x;
        if (i < n) {
            const uint32_t u = load_op(in, n, i, reverse).x ^ kSignFlip;
            atomicAdd(&s_h[(u >> shift) & (kFlushBins - 1)], 1u);
        }
    }
    __syncthreads();
    counts[(uint64_t)threadIdx.x * ntiles + blockIdx.x] = s_h[threadIdx.x];
}

// Exclusive scan of a[0..len) in place, kFlushScanChunk per workgroup; the
// chunk's total goes to totals[blockIdx.x].
__global__ void __launch_bounds__(kScanBlock) k_flush_scan(uint32_t *__restrict__ a, uint32_t len,
                                                           uint32_t *__restrict__ totals) {
    __shared__ uint32_t s_w[kScanBlock / 64];
    const uint64_t i0 = (uint64_t)blockIdx.x * kFlushScanChunk + (uint64_t)threadIdx.x * kScanIpt;
    uint32_t v[kScanIpt];
    uint32_t sum = 0;
#pragma unroll
    for (int j = 0; j < kScanIpt; j++) {
        v[j] = i0 + j < len ? a[i0 + j] : 0u;
        sum += v[j];
    }
    uint32_t total;
    uint32_t run = block_exclusive_scan<kScanBlock / 64>(sum, s_w, &total);
#pragma unroll
    for (int j = 0; j < kScanIpt; j++) {
        if (i0 + j < len) a[i0 + j] = run;
        run += v[j];
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

// One tile of one digit pass: offs (the scanned counts, chunk-relative) and
// chunk_base give where the tile's share of every digit starts in out.
__global__ void __launch_bounds__(64 * kFlushTileWaves) k_flush_scatter(
    const uint2 *__restrict__ in, uint64_t n, int reverse, uint32_t shift, uint32_t ntiles,
    const uint32_t *__restrict__ offs, const uint32_t *__restrict__ chunk_base,
    uint2 *__restrict__ out) {
    __shared__ TileLds<kFlushTileWaves> L;
    __shared__ uint2 s_ent[kFlushTile];
    __shared__ uint32_t s_goff[kFlushBins];
    const uint64_t base = (uint64_t)blockIdx.x * kFlushTile;
    const uint32_t tile_n = (uint32_t)(n - base < kFlushTile ? n - base : kFlushTile);
    uint32_t ukey[kFlushIpt], val[kFlushIpt], pos[kFlushIpt];
#pragma unroll
    for (int j = 0; j < kFlushIpt; j++) {  // every load issued before any is used
        const uint32_t t = tile_index(j);
        uint2 e = make_uint2(kSignFlip, 0u);
        if (t < tile_n) e = load_op(in, n, base + t, reverse);
        ukey[j] = e.x ^ kSignFlip;
        val[j] = e.y;
    }
    if (threadIdx.x < kFlushBins) {
        const uint64_t ci = (uint64_t)threadIdx.x * ntiles + blockIdx.x;
        s_goff[threadIdx.x] = offs[ci] + chunk_base[ci / kFlushScanChunk];
    }
    tile_positions<kFlushTileWaves>(ukey, tile_n, shift, L, pos);
#pragma unroll
    for (int j = 0; j < kFlushIpt; j++)
        if (tile_index(j) < tile_n)
            s_ent[pos[j] < kFlushTile ? pos[j] : kFlushTile - 1] = make_uint2(ukey[j] ^ kSignFlip, val[j]);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < tile_n; i += 64 * kFlushTileWaves) {
        const uint2 e = s_ent[i];
        const uint32_t d = ((e.x ^ kSignFlip) >> shift) & (kFlushBins - 1);
        const uint64_t g = (uint64_t)s_goff[d] + (i - L.start[d]);
        if (g < n) out[g] = e;
    }
}

// The whole batch in one workgroup: s_ent holds it (logical order: newest op
// first), every digit pass that moves anything permutes it in place through
// the lanes' registers, then the first entry of every key is kept.
__global__ void __launch_bounds__(64 * kFlushBlockWaves) k_flush_block(
    const uint2 *__restrict__ ops, uint32_t n, int drop, uint2 *__restrict__ out,
    int32_t *__restrict__ keys_out, uint32_t *__restrict__ count_out) {
    extern __shared__ __attribute__((aligned(16))) uint2 s_ent[];  // kFlushBlockCap records
    __shared__ TileLds<kFlushBlockWaves> L;
    __shared__ uint32_t s_or[kFlushBlockWaves], s_and[kFlushBlockWaves];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t ukey[kFlushIpt], val[kFlushIpt], pos[kFlushIpt];
    uint32_t k_or = 0, k_and = ~0u;
    // a small batch is spread over all waves: fewer rounds each
    const uint32_t rounds = (n + 64 * kFlushBlockWaves - 1) / (64 * kFlushBlockWaves);
#pragma unroll
    for (int j = 0; j < kFlushIpt; j++) {
        const uint32_t t = tile_index(j, rounds);
        uint2 e = make_uint2(kSignFlip, 0u);
        if (t < n) {
            e = load_op(ops, n, t, 1);
            k_or |= e.x;
            k_and &= e.x;
        }
        ukey[j] = e.x ^ kSignFlip;
        val[j] = e.y;
        if (t < n) s_ent[t] = make_uint2(ukey[j], val[j]);
    }
    // a digit on which all keys agree moves nothing: its pass is skipped
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        k_or |= __shfl_xor(k_or, off, 64);
        k_and &= __shfl_xor(k_and, off, 64);
    }
    if (lane == 0) {
        s_or[wave] = k_or;
        s_and[wave] = k_and;
    }
    __syncthreads();
    uint32_t differ = 0;
    {
        uint32_t o = 0, a = ~0u;
#pragma unroll
        for (int w = 0; w < kFlushBlockWaves; w++) {
            o |= s_or[w];
            a &= s_and[w];
        }
        differ = o ^ a;
    }
    for (int p = 0; p < kFlushPasses; p++) {
        const uint32_t shift = p * kFlushDigitBits;
        if (((differ >> shift) & (kFlushBins - 1)) == 0) continue;  // uniform
        tile_positions<kFlushBlockWaves>(ukey, n, shift, L, pos, rounds);
#pragma unroll
        for (int j = 0; j < kFlushIpt; j++)
            if (tile_index(j, rounds) < n)
                s_ent[pos[j] < kFlushBlockCap ? pos[j] : kFlushBlockCap - 1] = make_uint2(ukey[j], val[j]);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kFlushIpt; j++) {
            const uint32_t t = tile_index(j, rounds);
            if (t < n) {
                const uint2 e = s_ent[t];
                ukey[j] = e.x;
                val[j] = e.y;
            }
        }
        __syncthreads();
    }
    // keep the first (newest) entry of every key; output order is the record
    // order (wave, round, lane), so a round's kept entries are placed by a
    // ballot and the rounds and waves by running counts
    uint32_t keep[kFlushIpt];
    uint32_t mine = 0;
#pragma unroll
    for (int j = 0; j < kFlushIpt; j++) {
        const uint32_t t = tile_index(j, rounds);
        const uint32_t prev = t > 0 && t < n ? s_ent[t - 1].x : 0u;
        const bool k = t < n && (t == 0 || prev != ukey[j]) &&
                       !(drop && (int32_t)val[j] == kTombstone);
        const uint64_t m = __ballot(k);
        keep[j] = k ? mine + lanes_below(m) : ~0u;
        mine += (uint32_t)__popcll(m);  // the wave's kept count so far (uniform)
    }
    if (lane == 0) L.s_w[wave] = mine;
    __syncthreads();
    uint32_t wbase = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kFlushBlockWaves; w++) {
        const uint32_t t = L.s_w[w];
        if ((uint32_t)w < wave) wbase += t;
        total += t;
    }
#pragma unroll
    for (int j = 0; j < kFlushIpt; j++) {
        if (keep[j] == ~0u) continue;
        const uint32_t o = wbase + keep[j];
        if (o >= n) continue;  // kept <= n by construction
        out[o] = make_uint2(ukey[j] ^ kSignFlip, val[j]);
        if (keys_out) keys_out[o] = (int32_t)(ukey[j] ^ kSignFlip);
    }
    if (threadIdx.x == 0) *count_out = total;
}

uint64_t flush_tiles(uint64_t n) { return (n + kFlushTile - 1) / kFlushTile; }

}  // namespace

uint64_t flush_workspace_words(uint64_t n) {
    const uint64_t len = flush_tiles(n) * kFlushBins;
    const uint64_t nchunks = (len + kFlushScanChunk - 1) / kFlushScanChunk;
    return kHistWords + len + nchunks + 2;
}

hipError_t launch_flush_hist(const void *in, uint64_t n, uint32_t *ws, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(ws, 0, kHistWords * 4, stream);
    if (e != hipSuccess || n == 0) return e;
    const uint64_t blocks = std::min<uint64_t>((n + 255) / 256, 2048);
    k_flush_hist<<<(unsigned)blocks, 256, 0, stream>>>(reinterpret_cast<const uint2 *>(in), n, ws);
    return hipGetLastError();
}

uint32_t flush_pass_mask(const uint32_t *hist_host, uint64_t n) {
    uint32_t mask = 0;
    for (int p = 0; p < kFlushPasses; p++) {
        bool one_bin = false;
        for (int d = 0; d < kFlushBins; d++) one_bin |= hist_host[p * kFlushBins + d] == n;
        if (!one_bin) mask |= 1u << p;
    }
    return mask;
}

hipError_t launch_flush_pass(const void *in, uint64_t n, bool reverse, int pass, void *out,
                             uint32_t *ws, hipStream_t stream) {
    if (n == 0 || n >= 0xFFFFFFFFull || pass < 0 || pass >= kFlushPasses || in == out)
        return hipErrorInvalidValue;
    const uint64_t ntiles = flush_tiles(n);
    const uint64_t len = ntiles * kFlushBins;
    const uint64_t nchunks = (len + kFlushScanChunk - 1) / kFlushScanChunk;
    if (nchunks > kFlushScanChunk) return hipErrorInvalidValue;  // one top-level workgroup
    uint32_t *counts = ws + kHistWords;
    uint32_t *chunk_tot = counts + len;
    const uint2 *src = reinterpret_cast<const uint2 *>(in);
    const uint32_t shift = (uint32_t)pass * kFlushDigitBits;
    k_flush_count<<<(unsigned)ntiles, 256, 0, stream>>>(src, n, reverse, shift, (uint32_t)ntiles, counts);
    k_flush_scan<<<(unsigned)nchunks, kScanBlock, 0, stream>>>(counts, (uint32_t)len, chunk_tot);
    k_flush_scan<<<1, kScanBlock, 0, stream>>>(chunk_tot, (uint32_t)nchunks, chunk_tot + nchunks);
    k_flush_scatter<<<(unsigned)ntiles, 64 * kFlushTileWaves, 0, stream>>>(
        src, n, reverse, shift, (uint32_t)ntiles, counts, chunk_tot, reinterpret_cast<uint2 *>(out));
    return hipGetLastError();
}

hipError_t launch_flush_block(const void *ops, uint64_t n, int drop_tombstones, void *out,
                              int32_t *keys_out, uint32_t *count_out, hipStream_t stream) {
    if (n == 0 || n > kFlushBlockCap) return hipErrorInvalidValue;
    constexpr int kLds = kFlushBlockCap * 8;
    // the batch's image is 64 KiB, above the default dynamic LDS limit
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_flush_block),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, kLds);
    if (e != hipSuccess) return e;
    k_flush_block<<<1, 64 * kFlushBlockWaves, kLds, stream>>>(
        reinterpret_cast<const uint2 *>(ops), (uint32_t)n, drop_tombstones,
        reinterpret_cast<uint2 *>(out), keys_out, count_out);
    return hipGetLastError();
}

}  // namespace bloomhip
