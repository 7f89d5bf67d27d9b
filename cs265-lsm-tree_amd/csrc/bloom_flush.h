// bloom_flush.h — the batched PUT (bloomhip_flush_batch); see bloom_flush.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bloomhip {

// A stable LSD radix sort of entry_t records on the key, 8-bit digits, 4
// passes.  A tile is ranked by one workgroup of kFlushTileWaves waves, every
// lane holding kFlushIpt records; a batch of at most kFlushBlockCap ops is
// sorted and de-duplicated whole by one workgroup of kFlushBlockWaves waves
// (one entry_t image of the batch in LDS, the records in flight in registers).
// bloomhip.FLUSH_TILE / FLUSH_BLOCK_CAP / FLUSH_SCAN_CHUNK mirror the three.
constexpr int kFlushDigitBits = 8;
constexpr int kFlushBins = 1 << kFlushDigitBits;
constexpr int kFlushPasses = 32 / kFlushDigitBits;
constexpr int kFlushIpt = 16;
constexpr int kFlushTileWaves = 4;
constexpr int kFlushBlockWaves = 8;
constexpr uint32_t kFlushTile = 4096;
constexpr uint32_t kFlushBlockCap = 8192;
static_assert(kFlushTile == 64u * kFlushIpt * kFlushTileWaves &&
                  kFlushBlockCap == 64u * kFlushIpt * kFlushBlockWaves,
              "a tile / the cap is its workgroup's lanes times kFlushIpt");
// The tile counts [digit][tile] are scanned in chunks of kFlushScanChunk by
// one workgroup each, then the chunk totals by a single workgroup: at most
// kFlushScanChunk chunks, which n < 2^32 - 1 keeps true (2^20 tiles, 2^28
// counts, 2^14 chunks).
constexpr uint32_t kFlushScanChunk = 16384;
static_assert(((1ull << 32) / kFlushTile) * kFlushBins / kFlushScanChunk <= kFlushScanChunk,
              "the chunk totals of the largest batch fit the top-level scan");

// u32 words of workspace a tiled sort of n ops needs (histograms, tile
// counts, chunk totals), and of the one-workgroup path (its kept count).
uint64_t flush_workspace_words(uint64_t n);

// All kFlushPasses digit histograms of the keys of in[0..n) in one pass:
// hist[p * kFlushBins + d], zeroed by the launch.
hipError_t launch_flush_hist(const void *in, uint64_t n, uint32_t *ws, hipStream_t stream);
// Bit p set: pass p moves something (no bin of its histogram holds all n).
uint32_t flush_pass_mask(const uint32_t *hist_host, uint64_t n);
// One digit pass: in[0..n) (read back to front when reverse: element i is
// in[n - 1 - i]) stably sorted on digit `pass` of the sign-flipped key into
// out (8-B aligned, not in).  ws as above.
hipError_t launch_flush_pass(const void *in, uint64_t n, bool reverse, int pass, void *out,
                             uint32_t *ws, hipStream_t stream);
// n <= kFlushBlockCap ops, whole, in one launch: the last op of every key,
// keys ascending (tombstones dropped on request), packed into out, the kept
// keys again into keys_out when non-null, the kept count into *count_out.
hipError_t launch_flush_block(const void *ops, uint64_t n, int drop_tombstones, void *out,
                              int32_t *keys_out, uint32_t *count_out, hipStream_t stream);

}  // namespace bloomhip
