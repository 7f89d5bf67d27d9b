// bloom_pass1_build512.hip — pass 1 of the partition build (no slots) at
// 512 threads per workgroup (4096-key tiles): every key layout and
// remainder kind of k_part_bin (bloom_pass1.h), in one translation unit.
#include "bloom_pass1.h"

namespace bloomhip {

bool launch_bin_build512(const Pass1Kernel &p, const KeySpan &ks, const ModParams &mp,
                         const PartitionWorkspace &ws, const SegMap &sm, uint16_t *slots,
                         hipStream_t stream) {
    return launch_pass1_tile<false, 512>(p, ks, mp, ws, sm, slots, stream);
}

}  // namespace bloomhip
