// bloom_pass1_super.hip — pass 1 of the partition build on super-tiles of
// 16,384 keys (k_part_bin2, bloom_pass1.h): builds with many short runs.
#include "bloom_pass1.h"

namespace bloomhip {

bool launch_bin_super(const Pass1Kernel &p, const KeySpan &ks, const ModParams &mp,
                      const PartitionWorkspace &ws, const SegMap &sm, uint16_t *slots,
                      hipStream_t stream) {
    return launch_pass1_super<false>(p, ks, mp, ws, sm, slots, stream);
}

}  // namespace bloomhip
