// bloom_pass1_super_probe.hip — pass 1 of the stacked probe on super-tiles
// of 16,384 keys (k_part_bin2 with the slot plane, bloom_pass1.h): segment
// stacks with many short runs (the f = 10 tree's 1,250 segments).
#include "bloom_pass1.h"

namespace bloomhip {

bool launch_bin_super_probe(const Pass1Kernel &p, const KeySpan &ks, const ModParams &mp,
                            const PartitionWorkspace &ws, const SegMap &sm, uint16_t *slots,
                            hipStream_t stream) {
    return launch_pass1_super<true>(p, ks, mp, ws, sm, slots, stream);
}

}  // namespace bloomhip
