// bloom_pass1_probe1024.hip — pass 1 of the partition probe (with the probe's slots) at
// 1024 threads per workgroup (8192-key tiles): every key layout and
// remainder kind of k_part_bin (bloom_pass1.h), in one translation unit.
#include "bloom_pass1.h"

namespace bloomhip {

bool launch_bin_probe1024(const Pass1Kernel &p, const KeySpan &ks, const ModParams &mp,
                          const PartitionWorkspace &ws, const SegMap &sm, uint16_t *slots,
                          hipStream_t stream) {
    return launch_pass1_tile<true, 1024>(p, ks, mp, ws, sm, slots, stream);
}

}  // namespace bloomhip
