// ubench.hip — micro-benchmarks that price the primitives the Bloom kernels
// are built from on gfx950: random 4-B global atomicOr (agent vs workgroup
// scope), random 4-B gathers, random LDS ds_or, and the exact hash+mod
// arithmetic alone.  Not part of the product path; used by
// tools/ubench.py to pick build strategies.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <numeric>
#include <vector>

// the product kernels and launch templates, for ablation builds
#include "bloom_combine.h"
#include "bloom_pass1.h"
#include "bloom_pass2.h"
#include "bloom_merge.h"

using namespace bloomhip;

namespace {

__device__ __forceinline__ uint32_t xorshift(uint32_t &s) {
    s ^= s << 13;
    s ^= s >> 17;
    s ^= s << 5;
    return s;
}

template <int SCOPE>
__global__ void ub_atomic_or(uint32_t *words, uint32_t nwords, int iters) {
    uint32_t s = 0x9E3779B9u ^ (blockIdx.x * blockDim.x + threadIdx.x) * 2654435761u;
    for (int i = 0; i < iters; i++) {
        const uint32_t r = xorshift(s);
        const uint32_t w = (uint32_t)(((uint64_t)r * nwords) >> 32);
        __hip_atomic_fetch_or(words + w, 1u << (r & 31), __ATOMIC_RELAXED, SCOPE);
    }
}

__global__ void ub_gather(const uint32_t *words, uint32_t nwords, int iters, uint32_t *sink) {
    uint32_t s = 0x9E3779B9u ^ (blockIdx.x * blockDim.x + threadIdx.x) * 2654435761u;
    uint32_t acc = 0;
    for (int i = 0; i < iters; i++) {
        const uint32_t r = xorshift(s);
        const uint32_t w = (uint32_t)(((uint64_t)r * nwords) >> 32);
        acc += words[w];
    }
    if (acc == 0x12345678u) sink[0] = acc;
}

__global__ void ub_lds_or(int iters, uint32_t *sink) {
    extern __shared__ uint32_t seg[];
    for (int i = threadIdx.x; i < 16384; i += blockDim.x) seg[i] = 0;
    __syncthreads();
    uint32_t s = 0x9E3779B9u ^ (blockIdx.x * blockDim.x + threadIdx.x) * 2654435761u;
    for (int i = 0; i < iters; i++) {
        const uint32_t r = xorshift(s);
        atomicOr(&seg[r >> 18], 1u << (r & 31));
    }
    __syncthreads();
    if (seg[threadIdx.x] == 0x12345678u) sink[0] = 1;
}

// Random ds_or with half the lanes idle in five ways (round 6: what pass 2's
// out-of-run entries cost the LDS): 0 every lane a random word; 1 odd lanes
// OR 0 into one word shared by the group; 2 odd lanes masked off; 3 odd lanes
// OR 0 into a private word each; 4 odd lanes OR 0 into a random word (pass
// 2's branch-free masking).
template <int MODE>
__global__ void __launch_bounds__(1024) ub_lds_or_idle(int iters, uint32_t *sink) {
    extern __shared__ uint32_t seg[];
    for (int i = threadIdx.x; i < 16384 + 64; i += blockDim.x) seg[i] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    const bool idle = MODE != 0 && (lane & 1);
    uint32_t s = 0x9E3779B9u ^ (blockIdx.x * blockDim.x + threadIdx.x) * 2654435761u;
    for (int i = 0; i < iters; i++) {
        const uint32_t r = xorshift(s);
        uint32_t w = r >> 18, v = 1u << (r & 31);
        if (idle) {
            v = 0;
            if constexpr (MODE == 1) w = 16384;
            if constexpr (MODE == 3) w = 16384 + lane;
        }
        if constexpr (MODE == 2) {
            if (!idle) atomicOr(&seg[w], v);
        } else {
            atomicOr(&seg[w], v);
        }
    }
    __syncthreads();
    if (seg[threadIdx.x] == 0x12345678u) sink[0] = 1;
}

__global__ void ub_hash(ModParams mp, int iters, uint32_t *sink) {
    uint32_t acc = 0;
    int32_t k = (int32_t)((blockIdx.x * blockDim.x + threadIdx.x) * 2654435761u);
    for (int i = 0; i < iters; i++) {
        acc ^= mod_fast(raw_hash1(k), mp) + mod_fast(raw_hash2(k), mp) + mod_fast(raw_hash3(k), mp);
        k += 0x9E3779B9;
    }
    if (acc == 0x12345678u) sink[0] = acc;
}

// hash3 + the p2 remainder (m = d << t, d | 255: bloom_math.h mod_p2), the
// remainder the C2-C5 filters take
__global__ void ub_hash_p2(ModParams mp, int iters, uint32_t *sink) {
    uint32_t acc = 0;
    int32_t k = (int32_t)((blockIdx.x * blockDim.x + threadIdx.x) * 2654435761u);
    for (int i = 0; i < iters; i++) {
        acc ^= mod_p2(raw_hash1(k), mp) + mod_p2(raw_hash2(k), mp) + mod_p2(raw_hash3(k), mp);
        k += 0x9E3779B9;
    }
    if (acc == 0x12345678u) sink[0] = acc;
}

// Pass 1's whole per-key arithmetic, without its loads, sort or stores: the
// three hashes and, per hash, the bin and entry exactly as k_part_bin forms
// them (bin_entry with the product's reduction MK and segment map for the
// batch's geometry): the VALU ceiling of a build's or probe's pass 1.
template <int MK>
__global__ void ub_pass1_arith(ModParams mp, SegMap sm, int iters, uint32_t *sink) {
    uint32_t acc = 0;
    int32_t k = (int32_t)((blockIdx.x * blockDim.x + threadIdx.x) * 2654435761u);
    for (int i = 0; i < iters; i++) {
        uint32_t b0, e0, b1, e1, b2, e2;
        bin_entry<MK, 4>(raw_hash1(k), mp, sm, b0, e0);
        bin_entry<MK, 4>(raw_hash2(k), mp, sm, b1, e1);
        bin_entry<MK, 4>(raw_hash3(k), mp, sm, b2, e2);
        acc ^= (b0 + e0) ^ (b1 + e1) ^ (b2 + e2);
        k += 0x9E3779B9;
    }
    if (acc == 0x12345678u) sink[0] = acc;
}

__global__ void ub_rawhash(int iters, uint32_t *sink) {
    uint64_t acc = 0;
    int32_t k = (int32_t)((blockIdx.x * blockDim.x + threadIdx.x) * 2654435761u);
    for (int i = 0; i < iters; i++) {
        acc ^= raw_hash1(k) + raw_hash2(k) + raw_hash3(k);
        k += 0x9E3779B9;
    }
    if (acc == 0x12345678u) sink[0] = (uint32_t)acc;
}

// VALU / LDS overlap probe: waves of the first `valu_waves` of each 16-wave
// workgroup run the hash+mod loop, the others random LDS ds_add_rtn (mode 0:
// both, 1: hash waves only (others exit), 2: LDS waves only).
// prio: the issue priority (s_setprio 0-3) of the LDS waves in bits 0-1 and of
// the hash waves in bits 2-3, set once after the barrier.  The wave's kind
// comes from an SGPR there, so the choice is a scalar branch: s_setprio
// ignores EXEC, and under a divergent `if` every wave would run it.
__device__ __forceinline__ void ub_set_prio(int p) {
    if (p == 1) __builtin_amdgcn_s_setprio(1);
    else if (p == 2) __builtin_amdgcn_s_setprio(2);
    else if (p == 3) __builtin_amdgcn_s_setprio(3);
}
template <int OP>  // LDS op of the non-hashing waves: 0 ds_add_rtn, 1 ds_write, 2 ds_read
__global__ void __launch_bounds__(1024) ub_mixed(ModParams mp, int valu_waves, int mode,
                                                 int hash_iters, int lds_iters, uint32_t *sink,
                                                 int prio) {
    extern __shared__ uint32_t seg[];
    for (int i = threadIdx.x; i < 16384; i += blockDim.x) seg[i] = 0;
    __syncthreads();
    if (prio) {
        const bool hashes = (__builtin_amdgcn_readfirstlane(threadIdx.x) >> 6) < valu_waves;
        ub_set_prio(hashes ? (prio >> 2) & 3 : prio & 3);
    }
    const int wave = threadIdx.x >> 6;
    if (wave < valu_waves) {
        if (mode == 2) return;
        uint32_t acc = 0;
        int32_t k = (int32_t)((blockIdx.x * blockDim.x + threadIdx.x) * 2654435761u);
        for (int i = 0; i < hash_iters; i++) {
            acc ^= mod_fast(raw_hash1(k), mp) + mod_fast(raw_hash2(k), mp) + mod_fast(raw_hash3(k), mp);
            k += 0x9E3779B9;
        }
        if (acc == 0x12345678u) sink[0] = acc;
    } else {
        if (mode == 1) return;
        uint32_t s = 0x9E3779B9u ^ (blockIdx.x * blockDim.x + threadIdx.x) * 2654435761u;
        uint32_t acc = 0;
        for (int i = 0; i < lds_iters; i++) {
            s += 0x9E3779B9u;  // 1 VALU per op (a Weyl sequence), so the LDS waves stay LDS-bound
            const uint32_t r = s;
            if constexpr (OP == 0) acc += atomicAdd(&seg[r >> 18], 1u);  // pass 1's ranks
            else if constexpr (OP == 1) seg[r >> 18] = r;                  // the scatter
            else acc += seg[r >> 18];                                      // offset reads
        }
        if (acc == 0x12345678u) sink[0] = acc;
    }
}

__global__ void ub_stream(const uint4 *buf, size_t n16, uint32_t *sink) {
    uint32_t acc = 0;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n16;
         i += (size_t)gridDim.x * blockDim.x) {
        const uint4 v = buf[i];
        acc ^= v.x ^ v.y ^ v.z ^ v.w;
    }
    if (acc == 0x12345678u) sink[0] = acc;
}

}  // namespace

extern "C" int ubench_run(int which, void *dbuf, size_t bytes, uint64_t m, int grid, int block,
                          int iters, void *stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint32_t *w = reinterpret_cast<uint32_t *>(dbuf);
    const uint32_t nwords = (uint32_t)(bytes / 4 - 1);  // last word is the sink
    uint32_t *sink = w + nwords;
    switch (which) {
        case 0: ub_atomic_or<__HIP_MEMORY_SCOPE_AGENT><<<grid, block, 0, s>>>(w, nwords, iters); break;
        case 1: ub_atomic_or<__HIP_MEMORY_SCOPE_WORKGROUP><<<grid, block, 0, s>>>(w, nwords, iters); break;
        case 2: ub_gather<<<grid, block, 0, s>>>(w, nwords, iters, sink); break;
        case 3: ub_lds_or<<<grid, block, 65536, s>>>(iters, sink); break;
        case 4: ub_hash<<<grid, block, 0, s>>>(make_mod_params(m), iters, sink); break;
        case 5: ub_rawhash<<<grid, block, 0, s>>>(iters, sink); break;
        case 7: {
            const ModParams mp = make_mod_params(m);
            if (!mp.p2) return -22;
            ub_hash_p2<<<grid, block, 0, s>>>(mp, iters, sink);
            break;
        }
        case 6: ub_stream<<<grid, block, 0, s>>>(reinterpret_cast<const uint4 *>(dbuf), bytes / 16 - 1, sink); break;
        case 40: ub_lds_or_idle<0><<<grid, 1024, 66 * 1024, s>>>(iters, sink); break;
        case 41: ub_lds_or_idle<1><<<grid, 1024, 66 * 1024, s>>>(iters, sink); break;
        case 42: ub_lds_or_idle<2><<<grid, 1024, 66 * 1024, s>>>(iters, sink); break;
        case 43: ub_lds_or_idle<3><<<grid, 1024, 66 * 1024, s>>>(iters, sink); break;
        case 44: ub_lds_or_idle<4><<<grid, 1024, 66 * 1024, s>>>(iters, sink); break;
        // block = waves doing VALU (of 16), iters = hash iters; m (no filter
        // here) = the priorities: LDS waves' in bits 0-1, hash waves' in 2-3
        case 10: case 11: case 12:
            ub_mixed<0><<<grid, 1024, 65536, s>>>(make_mod_params(167772160), block, which - 10,
                                                  iters, iters * 6, sink, (int)(m & 15));
            break;
        case 20: case 21: case 22:
            ub_mixed<1><<<grid, 1024, 65536, s>>>(make_mod_params(167772160), block, which - 20,
                                                  iters, iters * 6, sink, (int)(m & 15));
            break;
        case 30: case 31: case 32:
            ub_mixed<2><<<grid, 1024, 65536, s>>>(make_mod_params(167772160), block, which - 30,
                                                  iters, iters * 6, sink, (int)(m & 15));
            break;
        default: return -22;
    }
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

// Pass 1's per-key arithmetic (ub_pass1_arith) for the product's geometry:
// a build of a filter of ms[0] bits (nf = 1, plan_build), or a stacked probe
// of nf members (plan_ladder, else plan_stack).  *mk_out: the reduction kind.
extern "C" int ubench_pass1_arith(int nf, const uint64_t *ms, int grid, int block, int iters,
                                  void *dbuf, void *stream, int *mk_out) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint32_t *sink = reinterpret_cast<uint32_t *>(dbuf);
    PartitionWorkspace ws{};
    StackTable st{};
    uint64_t mmax = 0, g = 0, mmin = ~0ull;
    for (int j = 0; j < nf; j++) {
        mmax = std::max(mmax, ms[j]);
        mmin = std::min(mmin, ms[j]);
        g = g == 0 ? ms[j] : std::gcd(g, ms[j]);
    }
    const int ncu = device_cu_count();
    if (nf == 1) {
        if (!plan_build(mmax, ncu, &ws)) return -34;
    } else if (!plan_ladder(ms, nf, ncu, &st, &ws) && !plan_stack(mmax, g, mmin, nf, ncu, &ws)) {
        return -34;
    }
    const ModParams mp = make_mod_params(mmax);
    SegMap sm{};
    const int mk = pass1_plan(mp, ws, nf > 1, &sm);
    *mk_out = mk;
    switch (mk) {
        case kModFast: ub_pass1_arith<kModFast><<<grid, block, 0, s>>>(mp, sm, iters, sink); break;
        case kModWide: ub_pass1_arith<kModWide><<<grid, block, 0, s>>>(mp, sm, iters, sink); break;
        case kModP2: ub_pass1_arith<kModP2><<<grid, block, 0, s>>>(mp, sm, iters, sink); break;
        case kModLadder: ub_pass1_arith<kModLadder><<<grid, block, 0, s>>>(mp, sm, iters, sink); break;
        case kModLadder0: ub_pass1_arith<kModLadder0><<<grid, block, 0, s>>>(mp, sm, iters, sink); break;
        case kModLadder0R: ub_pass1_arith<kModLadder0R><<<grid, block, 0, s>>>(mp, sm, iters, sink); break;
        default: return -22;
    }
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

// Geometry of the product's partition build of n keys into m bits
// (tools/ubench.py sizes its buffers from it): segments, segment bits, tile
// keys and tiles.
// out4: segments, segment bits, tile keys, tiles.
// out4: the larger of plan_build's and plan_segments' segment counts, the
// product's segment bits, the smallest tile of the two plans and the tiles
// at that size: buffers sized from these hold every variant of ubench_part.
extern "C" int ubench_part_geometry(size_t n, uint64_t m, uint64_t *out4) {
    PartitionWorkspace ws{}, sg{};
    if (!plan_build(m, device_cu_count(), &ws) || !plan_segments(m, device_cu_count(), &sg)) return -34;
    const size_t tk = std::min<size_t>(ws.tile_keys ? ws.tile_keys : choose_tile_keys(ws.nbins),
                                       choose_tile_keys(sg.nbins));
    out4[0] = std::max(ws.nbins, sg.nbins);
    out4[1] = ws.seg_bits;
    out4[2] = tk;
    out4[3] = (n + tk - 1) / tk;
    return 0;
}

namespace {
// plan_build's one-member ladder as pass 2 takes it (launch_part_apply's table)
StackTable ladder0_table(const ModParams &mp, const PartitionWorkspace &ws) {
    StackTable st{};
    st.lad.s = ws.lad_s;
    st.lad.u = ws.lad_u;
    st.lad.d = mp.p2d;
    st.lad.t[0] = mp.p2t;
    st.lad.rinv = ladder0_relabel(mp, ws) ? ladder0_inv(mp) : 0u;
    return st;
}

// The product's build geometry of n keys into m bits on a device of ncu CUs
// (plan_build, tiles as partition_buffers sizes them); *mode: the build's
// pass-2 mode.
bool build_plan(size_t n, uint64_t m, int ncu, PartitionWorkspace *ws, int *mode) {
    if (!plan_build(m, ncu, ws)) return false;
    if (!ws->tile_keys) ws->tile_keys = choose_tile_keys(ws->nbins);  // plan_build's super-tiles kept
    ws->ntiles = (n + ws->tile_keys - 1) / ws->tile_keys;
    *mode = ws->lad_u ? kApplyBuildL : kApplyBuild;
    return true;
}

// The product's geometry of a stacked probe of n keys against nf > 1 filters
// of ms[] bits (largest first for a ladder) on a device of ncu CUs, as
// probe_stacks plans it: plan_ladder, else plan_stack, tiles as
// partition_buffers sizes them.  *mmax: the largest member; *mode: the
// probe's pass-2 mode.
bool stack_plan(size_t n, int nf, const uint64_t *ms, int ncu, PartitionWorkspace *ws,
                uint64_t *mmax, int *mode) {
    StackTable st{};
    uint64_t g = 0, mmin = ~0ull;
    *mmax = 0;
    for (int j = 0; j < nf; j++) {
        *mmax = std::max(*mmax, ms[j]);
        mmin = std::min(mmin, ms[j]);
        g = std::gcd(g, ms[j]);
    }
    const bool ladder = plan_ladder(ms, nf, ncu, &st, ws);
    if (!ladder && !plan_stack(*mmax, g, mmin, nf, ncu, ws)) return false;
    if (!ws->tile_keys) ws->tile_keys = choose_tile_keys(ws->nbins);
    ws->ntiles = (n + ws->tile_keys - 1) / ws->tile_keys;
    *mode = ladder ? kApplyLadder : kApplyStack;
    return true;
}
}  // namespace

// The pass-2 walk the product chooses (choose_apply_walk) on a device of
// cu_count CUs, with no device call: for nf = 1 a build of n keys into ms[0]
// bits, for nf > 1 a stacked probe of n keys against filters of ms[] bits
// (plan_ladder, else plan_stack, as probe_stacks plans it).
// out7: mode (kApply*), tile keys, segments, G, CHAINS, VECS, REDIR.
extern "C" int ubench_walk_choice(size_t n, int nf, const uint64_t *ms, int cu_count, int *out7) {
    PartitionWorkspace ws{};
    int mode = 0;
    if (nf == 1) {
        if (!build_plan(n, ms[0], cu_count, &ws, &mode)) return -34;
    } else {
        uint64_t mmax = 0;
        if (!stack_plan(n, nf, ms, cu_count, &ws, &mmax, &mode)) return -34;
    }
    const ApplyWalk w = choose_apply_walk(mode, ws.tile_keys, ws.nbins, ws.ntiles);
    const int out[7] = {mode, (int)ws.tile_keys, (int)ws.nbins, w.g, w.chains, w.vecs, (int)w.redir};
    std::copy(out, out + 7, out7);
    return 0;
}

// The same for a one-filter partitioned probe (launch_probe_partitioned) of n
// keys against a filter of m bits: plan_segments' geometry, tiles as
// partition_buffers sizes them, choose_apply_walk(kApplyProbe).  No device
// call.  out7 as above (tests/test_gpu_probe_walks.py asserts G from it).
extern "C" int ubench_probe_walk_choice(size_t n, uint64_t m, int cu_count, int *out7) {
    PartitionWorkspace ws{};
    if (!plan_segments(m, cu_count, &ws)) return -34;
    ws.tile_keys = choose_tile_keys(ws.nbins);
    ws.ntiles = (n + ws.tile_keys - 1) / ws.tile_keys;
    const ApplyWalk w = choose_apply_walk(kApplyProbe, ws.tile_keys, ws.nbins, ws.ntiles);
    const int out[7] = {kApplyProbe, (int)ws.tile_keys, (int)ws.nbins, w.g, w.chains, w.vecs, (int)w.redir};
    std::copy(out, out + 7, out7);
    return 0;
}

// The pass-1 kernel the product chooses (choose_pass1_kernel) on a device of
// cu_count CUs, with no device call, for n keys at `stride` bytes (4: packed,
// 8: entry_t, both from a 16-B aligned base; else strided) and m bits:
// slots = 0 a build (plan_build), slots = 1 a one-filter partitioned probe
// (plan_segments).  -34: no geometry; -22: one pass 1 does not take.
namespace {
int pass1_choice_of(size_t n, uint64_t m, int slots, size_t stride, int cu_count, Pass1Kernel *out) {
    PartitionWorkspace ws{};
    int mode = 0;
    if (slots) {
        if (!plan_segments(m, cu_count, &ws)) return -34;
        ws.tile_keys = choose_tile_keys(ws.nbins);
        ws.ntiles = (n + ws.tile_keys - 1) / ws.tile_keys;
    } else if (!build_plan(n, m, cu_count, &ws, &mode)) {
        return -34;
    }
    const KeySpan ks{nullptr, n, stride, stride == 4 ? KEYS_PACKED : stride == 8 ? KEYS_ENTRY : KEYS_STRIDED};
    SegMap sm{};
    if (!choose_pass1_kernel(ks, make_mod_params(m), ws, slots != 0, cu_count, out, &sm)) return -22;
    return 0;
}
}  // namespace

// out11: Pass1Kernel's fields in order: super, threads, layout, slots, cols,
// mk, maxb, wgs_per_cu, nt, defer, grid.
extern "C" int ubench_pass1_choice(size_t n, uint64_t m, int slots, size_t stride, int cu_count,
                                   int *out11) {
    Pass1Kernel p{};
    const int rc = pass1_choice_of(n, m, slots, stride, cu_count, &p);
    if (rc) return rc;
    const int out[11] = {p.super, p.threads, p.layout, p.slots, p.cols, p.mk, p.maxb, p.wgs_per_cu,
                         p.nt, p.defer, (int)p.grid};
    std::copy(out, out + 11, out11);
    return 0;
}

// The same for pass 1 of a stacked probe (slots) of n keys against nf > 1
// filters of ms[] bits, planned as ubench_walk_choice plans it; no device
// call.  out11 as above.
extern "C" int ubench_stack_pass1_choice(size_t n, int nf, const uint64_t *ms, size_t stride,
                                         int cu_count, int *out11) {
    if (nf < 2) return -22;
    PartitionWorkspace ws{};
    uint64_t mmax = 0;
    int mode = 0;
    if (!stack_plan(n, nf, ms, cu_count, &ws, &mmax, &mode)) return -34;
    const KeySpan ks{nullptr, n, stride, stride == 4 ? KEYS_PACKED : stride == 8 ? KEYS_ENTRY : KEYS_STRIDED};
    Pass1Kernel p{};
    SegMap sm{};
    if (!choose_pass1_kernel(ks, make_mod_params(mmax), ws, true, cu_count, &p, &sm)) return -22;
    const int out[11] = {p.super, p.threads, p.layout, p.slots, p.cols, p.mk, p.maxb, p.wgs_per_cu,
                         p.nt, p.defer, (int)p.grid};
    std::copy(out, out + 11, out11);
    return 0;
}

// The product's run-table transpose (launch_runs_transpose, k_runs_transpose)
// on the caller's device buffers: rows [ntiles][width] -> cols [width][ntiles]
// (tests/test_gpu_run_table.py checks it against numpy's transpose).
extern "C" int ubench_runs_transpose(const void *rows, void *cols, size_t ntiles, int width,
                                     void *stream) {
    if (!rows || !cols || ntiles == 0 || width <= 0) return -22;
    PartitionWorkspace ws{};
    ws.run_rows = const_cast<uint32_t *>(reinterpret_cast<const uint32_t *>(rows));
    ws.run_starts = reinterpret_cast<uint32_t *>(cols);
    ws.ntiles = ntiles;
    ws.nbins = (size_t)width;
    return launch_runs_transpose(ws, reinterpret_cast<hipStream_t>(stream)) == hipSuccess ? 0 : -5;
}

// The issue priority of that kernel's phases (Pass1Kernel::prio,
// pass1_prio_of(mode, level); 0 = none), same arguments and status.
extern "C" int ubench_pass1_prio(size_t n, uint64_t m, int slots, size_t stride, int cu_count,
                                 int *prio_out) {
    Pass1Kernel p{};
    const int rc = pass1_choice_of(n, m, slots, stride, cu_count, &p);
    if (rc) return rc;
    *prio_out = p.prio;
    return 0;
}

// Whether that kernel runs the software-pipelined tile loop
// (Pass1Kernel::pipe; 0 = the plain loop), same arguments and status.
extern "C" int ubench_pass1_pipe(size_t n, uint64_t m, int slots, size_t stride, int cu_count,
                                 int *pipe_out) {
    Pass1Kernel p{};
    const int rc = pass1_choice_of(n, m, slots, stride, cu_count, &p);
    if (rc) return rc;
    *pipe_out = p.pipe;
    return 0;
}

// The product's pass 1, then pass 2 on a forced group walk (CHAINS, VECS,
// REDIR) at G = 4, in the geometry's own mode and tile size: the four group
// walks are right at any run length, only their speed differs
// (tests/test_gpu_pass2_walks.py).  Buffers as for ubench_part.
extern "C" int ubench_part_walk(int chains, int vecs, int redir, const void *keys, size_t n,
                                uint64_t m, uint64_t *pos, uint32_t *runs, uint32_t *words,
                                void *stream, size_t pos_cap, size_t runs_cap) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const KeySpan ks{reinterpret_cast<const char *>(keys), n, 4, KEYS_PACKED};
    const ModParams mp = make_mod_params(m);
    PartitionWorkspace ws{};
    int mode = 0;
    if (n == 0) return -22;
    if (!build_plan(n, m, device_cu_count(), &ws, &mode)) return -34;
    if (ws.ntiles * ws.tile_keys > pos_cap || 2 * ws.ntiles * (ws.nbins + 1) > runs_cap) return -28;
    ws.pos = pos;
    ws.run_rows = runs;
    ws.run_starts = runs + ws.ntiles * (ws.nbins + 1);
    hipError_t e = launch_part_bin(ks, mp, ws, s);
    if (e != hipSuccess) {
        fprintf(stderr, "ubench_part_walk: pass 1: %s\n", hipGetErrorString(e));
        return -5;
    }
    const StackTable st = mode == kApplyBuildL ? ladder0_table(mp, ws) : StackTable{};
    const uint64_t nw32 = ((mp.m + 63) / 64) * 2;
    const ApplyWalk w{4, chains, vecs, redir != 0};
    e = hipErrorInvalidValue;  // no such walk
#define UB_ON(MODE, TK, C, V, R)                                                                  \
    if (mode == MODE && ws.tile_keys == TK && w == ApplyWalk{4, C, V, R})                         \
        e = launch_apply_g<MODE, 4, TK, 1, C, V, R>(ws, mp.m, words, nw32, 0, nullptr, st, s);
#define UB_WALKS(MODE, TK) \
    UB_ON(MODE, TK, 1, 1, false) UB_ON(MODE, TK, 1, 1, true) UB_ON(MODE, TK, 1, 2, true) UB_ON(MODE, TK, 2, 2, true)
    UB_WALKS(kApplyBuildL, 4096) UB_WALKS(kApplyBuildL, 8192)
    UB_WALKS(kApplyBuild, 4096) UB_WALKS(kApplyBuild, 8192) UB_WALKS(kApplyBuild, 16384)
#undef UB_WALKS
#undef UB_ON
    if (e != hipSuccess) fprintf(stderr, "ubench_part_walk: pass 2: %s\n", hipGetErrorString(e));
    return e == hipSuccess ? 0 : e == hipErrorInvalidValue ? -22 : -5;
}

// The product's pass 1, then pass 2 on the one-vector group walk (G = 4, no
// redirect) with either of its loops forced: lean = 0 the plain loop, 1 the
// lean loop on 32-bit offsets (k_part_apply's LEAN), in the geometry's own
// mode on 4096- or 8192-key tiles; merge: OR into the bitmap in words
// (tests/test_gpu_pass2_build_loop.py, tools/ubench.py p2ab).  -22: not such
// a geometry, or a batch the lean loop's offsets cannot address.  Buffers as
// for ubench_part.
extern "C" int ubench_part_loop(int lean, int merge, const void *keys, size_t n, uint64_t m,
                                uint64_t *pos, uint32_t *runs, uint32_t *words, void *stream,
                                size_t pos_cap, size_t runs_cap) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const KeySpan ks{reinterpret_cast<const char *>(keys), n, 4, KEYS_PACKED};
    const ModParams mp = make_mod_params(m);
    PartitionWorkspace ws{};
    int mode = 0;
    if (n == 0) return -22;
    if (!build_plan(n, m, device_cu_count(), &ws, &mode)) return -34;
    if (ws.ntiles * ws.tile_keys > pos_cap || 2 * ws.ntiles * (ws.nbins + 1) > runs_cap) return -28;
    if (lean && !apply_offsets_fit32(ws.tile_keys, ws.nbins, ws.ntiles)) return -22;
    ws.pos = pos;
    ws.run_rows = runs;
    ws.run_starts = runs + ws.ntiles * (ws.nbins + 1);
    hipError_t e = launch_part_bin(ks, mp, ws, s);
    if (e != hipSuccess) {
        fprintf(stderr, "ubench_part_loop: pass 1: %s\n", hipGetErrorString(e));
        return -5;
    }
    const StackTable st = mode == kApplyBuildL ? ladder0_table(mp, ws) : StackTable{};
    const uint64_t nw32 = ((mp.m + 63) / 64) * 2;
    e = hipErrorInvalidValue;  // no such geometry
#define UB_ON(MODE, TK)                                                                           \
    if (mode == MODE && ws.tile_keys == TK)                                                       \
        e = lean ? launch_apply_g<MODE, 4, TK, 1, 1, 1, false, 0, 0, false, true>(ws, mp.m, words, nw32, merge, nullptr, st, s) \
                 : launch_apply_g<MODE, 4, TK, 1, 1, 1, false>(ws, mp.m, words, nw32, merge, nullptr, st, s);
    UB_ON(kApplyBuildL, 4096) UB_ON(kApplyBuildL, 8192) UB_ON(kApplyBuild, 4096) UB_ON(kApplyBuild, 8192)
#undef UB_ON
    if (e != hipSuccess) fprintf(stderr, "ubench_part_loop: pass 2: %s\n", hipGetErrorString(e));
    return e == hipSuccess ? 0 : e == hipErrorInvalidValue ? -22 : -5;
}

// choose_apply_walk itself, with no device call: out6 = G, CHAINS, VECS,
// REDIR, LEAN for a pass 2 of `mode` (kApply*) over ntiles tiles of tile_keys
// keys sorted into nbins segments, then whether the lean loop's 32-bit
// offsets can address that batch (apply_offsets_fit32)
// (tests/test_host_pass2_loop.py).
extern "C" void ubench_apply_walk(int mode, size_t tile_keys, size_t nbins, size_t ntiles, int *out6) {
    const ApplyWalk w = choose_apply_walk(mode, tile_keys, nbins, ntiles);
    const int out[6] = {w.g, w.chains, w.vecs, (int)w.redir, (int)w.lean,
                        (int)apply_offsets_fit32(tile_keys, nbins, ntiles)};
    std::copy(out, out + 6, out6);
}

// The product's build on a forced pass-1 grid: the kernel choose_pass1_kernel
// gives (store policy included), launched on min(grid, tiles) persistent
// workgroups, then the product's pass 2.  A small grid runs the tile loop of
// the persistent kernels (peeled first tile, steady state, partial last round,
// ragged last tile, epilogue) at batches of a few tiles
// (tests/test_gpu_build_edges.py).  entry_keys: the keys are entry_t records
// (stride 8).  ubench_part_walk's signature; buffers as for ubench_part.
extern "C" int ubench_part_grid(int grid, int entry_keys, int merge, const void *keys, size_t n,
                                uint64_t m, uint64_t *pos, uint32_t *runs, uint32_t *words,
                                void *stream, size_t pos_cap, size_t runs_cap) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const KeySpan ks{reinterpret_cast<const char *>(keys), n, entry_keys ? (size_t)8 : (size_t)4,
                     entry_keys ? KEYS_ENTRY : KEYS_PACKED};
    const ModParams mp = make_mod_params(m);
    PartitionWorkspace ws{};
    int mode = 0;
    if (n == 0 || grid < 1) return -22;
    if (!build_plan(n, m, device_cu_count(), &ws, &mode)) return -34;
    if (ws.ntiles * ws.tile_keys > pos_cap || 2 * ws.ntiles * (ws.nbins + 1) > runs_cap) return -28;
    ws.pos = pos;
    ws.run_rows = runs;
    ws.run_starts = runs + ws.ntiles * (ws.nbins + 1);
    Pass1Kernel p{};
    SegMap sm{};
    if (!choose_pass1_kernel(ks, mp, ws, false, device_cu_count(), &p, &sm)) return -22;
    p.grid = (unsigned)std::min<size_t>((size_t)grid, ws.ntiles);
    Pass1Launch *unit = p.super ? launch_bin_super : p.threads >= 1024 ? launch_bin_build1024 : launch_bin_build512;
    if (!unit(p, ks, mp, ws, sm, nullptr, s)) return -22;
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && !p.cols) e = launch_runs_transpose(ws, s);
    if (e == hipSuccess) e = launch_part_apply(mp, words, ws, merge, s);
    if (e != hipSuccess) fprintf(stderr, "ubench_part_grid: %s\n", hipGetErrorString(e));
    // the pass-1 kernel's store policy and loop, for the caller to check what ran
    return e == hipSuccess ? (p.wt ? 2 : p.nt ? 1 : 0) | (p.pipe ? 4 : 0) : -5;
}

// The stamps' layout: u64 stamps per workgroup of pass 1 and of pass 2.
extern "C" void ubench_edge_layout(int *out2) {
    out2[0] = kEdgeStamps1;
    out2[1] = kEdgeStamps2;
}

// The C2 build's two kernels stamped (k_part_bin's and k_part_apply's STAMP),
// one after the other in one stream (tools/ubench.py edges): pass 1's
// workgroup x stamps at stamps[x * kEdgeStamps1 ..], pass 2's workgroup b at
// stamps[grid1 * kEdgeStamps1 + b * kEdgeStamps2 ..].  out4: pass 1's grid,
// pass 2's, pass 1's rounds, the stamps' clock in kHz.  Buffers as for
// ubench_part; only the geometry of UB_PIPE (plan_build's relabelled
// one-member ladder on 4096-key tiles).
extern "C" int ubench_edges(const void *keys, size_t n, uint64_t m, uint64_t *pos, uint32_t *runs,
                            uint32_t *words, void *stream, size_t pos_cap, size_t runs_cap,
                            uint64_t *stamps, size_t stamps_cap, int *out4) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const KeySpan ks{reinterpret_cast<const char *>(keys), n, 4, KEYS_PACKED};
    const ModParams mp = make_mod_params(m);
    PartitionWorkspace ws{};
    if (n == 0 || !plan_build(m, device_cu_count(), &ws)) return -34;
    if (!ws.tile_keys) ws.tile_keys = choose_tile_keys(ws.nbins);
    ws.ntiles = (n + ws.tile_keys - 1) / ws.tile_keys;
    if (ws.ntiles * ws.tile_keys > pos_cap || 2 * ws.ntiles * (ws.nbins + 1) > runs_cap) return -28;
    ws.pos = pos;
    ws.run_rows = runs;
    ws.run_starts = runs + ws.ntiles * (ws.nbins + 1);
    SegMap sm{};
    if (pass1_plan(mp, ws, false, &sm) != kModLadder0R || ws.tile_keys != 4096 || ws.nbins > 511 ||
        !runs_as_columns(ws) || !ws.lad_u || ws.lad_hb != 0 || !mp.p2 ||
        // (the store policies compiled in below are the product's only while
        // the tiles fit the Infinity Cache, choose_pass1_kernel)
        ws.ntiles * (uint64_t)4096 * 8 > kInfinityCacheBytes)
        return -22;
    constexpr int kWgs = pass1_wgs_per_cu(512, false, 511);
    const unsigned grid1 = pass1_grid(ws.ntiles, device_cu_count(), kWgs);
    const size_t rounds = (ws.ntiles + grid1 - 1) / grid1;
    // a stamp per loop iteration and one for the epilogue
    if (rounds + 1 > (size_t)(kEdgeStamps1 - kEdge1Tile0)) return -22;
    if ((size_t)grid1 * kEdgeStamps1 + ws.nbins * kEdgeStamps2 > stamps_cap) return -28;
    int dev = 0, khz = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess)
        return -5;
    k_part_bin<KEYS_PACKED, false, true, 512, kModLadder0R, 511, pass1_min_waves(512, kWgs), 0,
               pass1_wt(1, KEYS_PACKED) ? kStoreWT : kStorePlain, false, pass1_prio_of(kPrioHash, 1), 1, true>
        <<<grid1, 512, 0, s>>>(ks, mp, ws.pos, ws.run_starts, sm, ws.ntiles, reinterpret_cast<uint16_t *>(stamps));
    if (hipGetLastError() != hipSuccess) return -5;
    const StackTable st = ladder0_table(mp, ws);
    const uint64_t nw32 = ((mp.m + 63) / 64) * 2;
    const hipError_t e = launch_apply_g<kApplyBuildL, 4, 4096, 1, 1, 1, false, 0, 0, true>(
        ws, mp.m, words, nw32, 0, reinterpret_cast<uint8_t *>(stamps + (size_t)grid1 * kEdgeStamps1), st, s);
    out4[0] = (int)grid1;
    out4[1] = (int)ws.nbins;
    out4[2] = (int)rounds;
    out4[3] = khz;
    return e == hipSuccess ? 0 : -5;
}

// Phases of the product's partition build (tools/ubench.py part, p1ab):
// 0 = pass 1 as the product launches it, 1 = pass 2 as the product launches
// it over variant 0's output; 5001 / 5003 = pass-1 shapes (MINW waves per
// SIMD, NWG workgroups per CU).  runs: both table layouts.
extern "C" int ubench_part(int variant, const void *keys, size_t n, uint64_t m, uint64_t *pos,
                           uint32_t *runs, uint32_t *words, void *stream, size_t pos_cap,
                           size_t runs_cap) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const KeySpan ks{reinterpret_cast<const char *>(keys), n, 4, KEYS_PACKED};
    const ModParams mp = make_mod_params(m);
    PartitionWorkspace ws{};
    // 20 / 21: pass 1 / pass 2 on plan_segments' segments (the round-2
    // geometry); everything else on the product's plan_build
    const bool seg = variant == 20 || variant == 21;
    if (!(seg ? plan_segments(m, device_cu_count(), &ws) : plan_build(m, device_cu_count(), &ws)))
        return -34;
    if (!ws.tile_keys) ws.tile_keys = choose_tile_keys(ws.nbins);  // plan_build's super-tiles kept
    ws.ntiles = (n + ws.tile_keys - 1) / ws.tile_keys;
    // the caller's buffers must hold this plan's tiles (pos, in u64) and
    // both run-table layouts (runs, in u32): refused, not overrun
    if (ws.ntiles * ws.tile_keys > pos_cap || 2 * ws.ntiles * (ws.nbins + 1) > runs_cap) return -28;
    ws.pos = pos;
    ws.run_rows = runs;
    ws.run_starts = runs + ws.ntiles * (ws.nbins + 1);
    hipError_t e = hipSuccess;
    switch (variant) {
        case 0: case 20: e = launch_part_bin(ks, mp, ws, s); break;
        case 1: case 21: e = launch_part_apply(mp, words, ws, 0, s); break;
        // pass-1 shapes with the p2 remainder at NWG workgroups per CU: two,
        // and the product's (pass1_wgs_per_cu: three)
#define UB_P2(V, TB, MAXB, NWG)                                                                   \
    case V: {                                                                                    \
        if (ws.nbins > MAXB || ws.tile_keys != TB * kPartKPT || !mp.p2) return -22;             \
        SegMap sm = seg_map_of(ws);                                                              \
        sm.p2_hi_shift = mp.p2t - sm.shift;                                                      \
        k_part_bin<KEYS_PACKED, false, true, TB, kModP2, MAXB, pass1_min_waves(TB, NWG)>         \
            <<<pass1_grid(ws.ntiles, device_cu_count(), NWG), TB, 0, s>>>(                       \
                ks, mp, ws.pos, ws.run_starts, sm, ws.ntiles, nullptr);                          \
        e = hipGetLastError();                                                                   \
        break;                                                                                   \
    }
        UB_P2(5001, 512, 511, 2) UB_P2(5003, 512, 511, pass1_wgs_per_cu(512, false, 511))
#undef UB_P2
        // Pass 2 of a super-tile build (C4) over variant 0's output, by
        // k_part_apply's (G, CHAINS, VECS, REDIR): 2503 (4, 1, 2, redirected),
        // 2507 the product's (4, 2, 2, redirected), 2522 (4, 1, 1,
        // redirected), 2523 two lanes per tile (24 entries a step for C4's
        // ~20-entry runs) at (2, 1, 2, redirected)
        case 2503: case 2507: case 2522: case 2523: {
            if (ws.lad_u || tile_keys_of(ws) != kSuperTileKeys) return -22;
            const uint64_t nw32 = ((mp.m + 63) / 64) * 2;
            constexpr int TK = (int)kSuperTileKeys;
#define UB_WALK(V, G, C, NV, R)                                                                   \
    if (variant == V)                                                                             \
        e = launch_apply_g<kApplyBuild, G, TK, 1, C, NV, R>(ws, mp.m, words, nw32, 0, nullptr, StackTable{}, s);
            UB_WALK(2503, 4, 1, 2, true) UB_WALK(2507, 4, 2, 2, true) UB_WALK(2522, 4, 1, 1, true)
            UB_WALK(2523, 2, 1, 2, true)
#undef UB_WALK
            break;
        }
        // Pass 2 of plan_build's one-member ladder (C2, C5) over variant 0's
        // output at G = 4: 2401 the C2 walk (1, 1, plain) on the plain loop, 2413
        // the product's C5 walk (1, 2, redirected), 2417 that on two chains
        case 2401: case 2413: case 2417: case 2420: {
            if (!ws.lad_u || ws.lad_hb != 0 || !mp.p2) return -22;
            const StackTable st = ladder0_table(mp, ws);
            const uint64_t nw32 = ((mp.m + 63) / 64) * 2;
            const size_t tk = tile_keys_of(ws);
            if (tk != 4096 && tk != 8192) return -22;
#define UB_WALK(V, C, NV, R)                                                                      \
    if (variant == V)                                                                             \
        e = tk == 4096 ? launch_apply_g<kApplyBuildL, 4, 4096, 1, C, NV, R>(ws, mp.m, words, nw32, 0, nullptr, st, s) \
                       : launch_apply_g<kApplyBuildL, 4, 8192, 1, C, NV, R>(ws, mp.m, words, nw32, 0, nullptr, st, s);
            UB_WALK(2401, 1, 1, false) UB_WALK(2413, 1, 2, true) UB_WALK(2417, 2, 2, true)
#undef UB_WALK
            // 2420: 2401's walk on the lean loop (the product's at C2)
            if (variant == 2420 && apply_offsets_fit32(tk, ws.nbins, ws.ntiles))
                e = tk == 4096 ? launch_apply_g<kApplyBuildL, 4, 4096, 1, 1, 1, false, 0, 0, false, true>(ws, mp.m, words, nw32, 0, nullptr, st, s)
                               : launch_apply_g<kApplyBuildL, 4, 8192, 1, 1, 1, false, 0, 0, false, true>(ws, mp.m, words, nw32, 0, nullptr, st, s);
            else if (variant == 2420)
                return -22;
            break;
        }
        // 5100 + ABL: the product's C2 pass 1 (plan_build's one-member
        // ladder, 4096-key tiles, three workgroups per CU) cut after a
        // stage (k_part_bin's ABL): the ablation ladder of tools/ubench.py p1abl
        // + 20: the tile's write-out deferred into the next tile's hash
        // phase (k_part_bin's DEFER, the 1024-thread builds' form) instead
        // of after its own scatter (5100, the product's form at C2)
#define UB_ABL(A, D)                                                                              \
    case 5100 + 20 * D + A: {                                                                    \
        SegMap sm{};                                                                             \
        if (pass1_plan(mp, ws, false, &sm) != kModLadder0R || ws.tile_keys != 4096 ||           \
            ws.nbins > 511 || !runs_as_columns(ws))                                              \
            return -22;                                                                          \
        constexpr int kWgs = pass1_wgs_per_cu(512, false, 511);                                  \
        k_part_bin<KEYS_PACKED, false, true, 512, kModLadder0R, 511, pass1_min_waves(512, kWgs), A, false, D != 0> \
            <<<pass1_grid(ws.ntiles, device_cu_count(), kWgs), 512, 0, s>>>(                     \
                ks, mp, ws.pos, ws.run_starts, sm, ws.ntiles, nullptr);                          \
        e = hipGetLastError();                                                                   \
        break;                                                                                   \
    }
        UB_ABL(0, 0) UB_ABL(1, 0) UB_ABL(2, 0) UB_ABL(3, 0) UB_ABL(4, 0) UB_ABL(5, 0)
        // (stages 1-4 write no tile out: the same with and without DEFER)
        UB_ABL(0, 1) UB_ABL(5, 1)
#undef UB_ABL
        // 5200 + 10 * PRIO + ABL: 5100 + ABL with the phases at an issue
        // priority (k_part_bin's PRIO = level | mode << 2): the sort phases
        // at level 1, 2, 3 (PRIO 1, 2, 3), only scatter + packing at 1
        // (PRIO 5), the inverse, the hash phase at 1, 2, 3 (PRIO 9, 10, 11),
        // and waves 4-7 of each workgroup at a static 1 (PRIO 13).  The
        // ladders start at stage 3: stages 1 and 2 end at the post-rank
        // barrier, where a tile's first flip is.
#define UB_PRIO(P, A)                                                                             \
    case 5200 + 10 * P + A: {                                                                    \
        SegMap sm{};                                                                             \
        if (pass1_plan(mp, ws, false, &sm) != kModLadder0R || ws.tile_keys != 4096 ||           \
            ws.nbins > 511 || !runs_as_columns(ws))                                              \
            return -22;                                                                          \
        constexpr int kWgs = pass1_wgs_per_cu(512, false, 511);                                  \
        k_part_bin<KEYS_PACKED, false, true, 512, kModLadder0R, 511, pass1_min_waves(512, kWgs), A, false, false, P> \
            <<<pass1_grid(ws.ntiles, device_cu_count(), kWgs), 512, 0, s>>>(                     \
                ks, mp, ws.pos, ws.run_starts, sm, ws.ntiles, nullptr);                          \
        e = hipGetLastError();                                                                   \
        break;                                                                                   \
    }
#define UB_PRIO_LADDER(P) UB_PRIO(P, 0) UB_PRIO(P, 3) UB_PRIO(P, 4) UB_PRIO(P, 5)
        UB_PRIO_LADDER(pass1_prio_of(kPrioSort, 1)) UB_PRIO_LADDER(pass1_prio_of(kPrioSort, 2))
        UB_PRIO_LADDER(pass1_prio_of(kPrioSort, 3)) UB_PRIO_LADDER(pass1_prio_of(kPrioScatter, 1))
        UB_PRIO_LADDER(pass1_prio_of(kPrioHash, 1)) UB_PRIO(pass1_prio_of(kPrioHash, 2), 0)
        UB_PRIO(pass1_prio_of(kPrioHash, 3), 0) UB_PRIO(pass1_prio_of(kPrioYoung, 1), 0)
#undef UB_PRIO_LADDER
#undef UB_PRIO
        // 5500 + ABL: C2's pass 1 on the software-pipelined tile loop
        // (k_part_bin's PIPE, the hash phase at priority 1) cut after a
        // stage; the plain loop's ladder beside it is 5101, 5102, then
        // 5290 + ABL (PRIO 9)
#define UB_PIPE(A)                                                                                \
    case 5500 + A: {                                                                             \
        SegMap sm{};                                                                             \
        /* (tiles within the Infinity Cache: the store policy compiled in here is the */         \
        /* product's only there, choose_pass1_kernel) */                                         \
        if (pass1_plan(mp, ws, false, &sm) != kModLadder0R || ws.tile_keys != 4096 ||           \
            ws.nbins > 511 || !runs_as_columns(ws) ||                                            \
            ws.ntiles * (uint64_t)4096 * 8 > kInfinityCacheBytes)                                \
            return -22;                                                                          \
        constexpr int kWgs = pass1_wgs_per_cu(512, false, 511);                                  \
        k_part_bin<KEYS_PACKED, false, true, 512, kModLadder0R, 511, pass1_min_waves(512, kWgs), A,           \
                   pass1_wt(1, KEYS_PACKED) ? kStoreWT : kStorePlain, false, pass1_prio_of(kPrioHash, 1), 1>  \
            <<<pass1_grid(ws.ntiles, device_cu_count(), kWgs), 512, 0, s>>>(                     \
                ks, mp, ws.pos, ws.run_starts, sm, ws.ntiles, nullptr);                          \
        e = hipGetLastError();                                                                   \
        break;                                                                                   \
    }
        UB_PIPE(0) UB_PIPE(1) UB_PIPE(2) UB_PIPE(3) UB_PIPE(4) UB_PIPE(5)
#undef UB_PIPE
        // 5413: the 1024-thread builds' pass 1 (one workgroup per CU, write-out
        // deferred) with waves 8-15 at a static priority 1: C5 (one-member
        // ladder, 512 bins, non-temporal tiles) and the f = 10 tree's level-2
        // build (the general remainder, 505 segments)
        case 5413: {
            SegMap sm{};
            const int mk = pass1_plan(mp, ws, false, &sm);
            constexpr int kP = pass1_prio_of(kPrioYoung, 1);
            if (ws.tile_keys != 8192 || ws.nbins > 1023 || !runs_as_columns(ws)) return -22;
            const unsigned grid = pass1_grid(ws.ntiles, device_cu_count(), 1);
            const bool nt = ws.ntiles * (uint64_t)8192 * 8 > kInfinityCacheBytes;
            if (mk == kModLadder0R && nt)
                k_part_bin<KEYS_PACKED, false, true, 1024, kModLadder0R, 1023, 4, 0, true, true, kP>
                    <<<grid, 1024, 0, s>>>(ks, mp, ws.pos, ws.run_starts, sm, ws.ntiles, nullptr);
            else if (mk == kModFast && !nt)
                k_part_bin<KEYS_PACKED, false, true, 1024, kModFast, 1023, 4, 0, false, true, kP>
                    <<<grid, 1024, 0, s>>>(ks, mp, ws.pos, ws.run_starts, sm, ws.ntiles, nullptr);
            else
                return -22;
            e = hipGetLastError();
            break;
        }
        default: return -22;
    }
    return e == hipSuccess ? 0 : -5;
}

// The stacked probe (C3 by default) by phase: 0 = the product's three
// launches, 1 = pass 1 (with slots), 2 = pass 2, 5 = the combine; 100 + G =
// pass 2 with G lanes per tile.  Buffers sized by the caller for plan_stack's
// geometry (ubench_stack_geometry; runs: both layouts).  Members must divide
// the largest, so their gcd is the smallest.
namespace {
bool ub_stack_plan(int nf, const uint64_t *ms, uint64_t *mmax, PartitionWorkspace *ws) {
    uint64_t g = 0;
    *mmax = 0;
    for (int j = 0; j < nf; j++) {
        *mmax = ms[j] > *mmax ? ms[j] : *mmax;
        g = g == 0 || ms[j] < g ? ms[j] : g;
    }
    return plan_stack(*mmax, g, g, nf, device_cu_count(), ws);
}
}  // namespace

extern "C" int ubench_stack_geometry(int nf, const uint64_t *ms, uint64_t *nbins_out,
                                     uint64_t *seg_bits_out) {
    uint64_t mmax = 0;
    PartitionWorkspace ws{};
    if (!ub_stack_plan(nf, ms, &mmax, &ws)) return -34;
    *nbins_out = ws.nbins;
    *seg_bits_out = ws.seg_bits;
    return 0;
}

extern "C" int ubench_stack(int variant, const void *keys, size_t n, int nf, const uint64_t *ms,
                            void *const *words, uint64_t *pos, uint32_t *runs, uint8_t *res,
                            uint16_t *slots, uint64_t *out, void *stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const KeySpan ks{reinterpret_cast<const char *>(keys), n, 4, KEYS_PACKED};
    uint64_t mmax = 0;
    PartitionWorkspace ws{};
    if (!ub_stack_plan(nf, ms, &mmax, &ws)) return -34;
    ws.tile_keys = choose_tile_keys(ws.nbins);
    ws.ntiles = (n + ws.tile_keys - 1) / ws.tile_keys;
    ws.pos = pos;
    ws.run_rows = runs;
    ws.run_starts = runs + ws.ntiles * (ws.nbins + 1);
    StackTable st{};
    st.nf = nf;
    for (int j = 0; j < nf; j++) {
        st.words[j] = reinterpret_cast<const uint32_t *>(words[j]);
        st.mwords[j] = (uint32_t)(ms[j] / 32);
        st.row[j] = j;
    }
    const ModParams mp = make_mod_params(mmax);
    const size_t nw = (n + 63) / 64;
    hipError_t e = hipSuccess;
    switch (variant) {
        case 0: e = launch_probe_stacked(ks, mp, st, ws, res, slots, out, nw, s); break;
        case 1: e = launch_bin<true>(ks, mp, ws, slots, s); break;
        case 2: e = launch_apply_stack(ws, mmax, res, st, s); break;
        case 5: e = launch_combine(ws, res, slots, n, out, nw, st, s); break;
        default: return -22;
    }
    return e == hipSuccess ? 0 : -5;
}

// Ladder stack (plan_ladder) on the product kernels, tile_keys 4096 or 8192:
// 0 the whole probe, 1 pass 1, 2 pass 2 (product walk), 5 combine, 11 / 12
// pass 1 without the slot stores / without slot and sorted-tile stores;
// 100 + v: variant v on the table planner.
extern "C" int ubench_ladder(int variant, int tile_keys, const void *keys, size_t n, int nf,
                             const uint64_t *ms, void *const *words, uint64_t *pos,
                             uint32_t *runs, uint8_t *res, uint16_t *slots, uint64_t *out,
                             void *stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const KeySpan ks{reinterpret_cast<const char *>(keys), n, 4, KEYS_PACKED};
    PartitionWorkspace ws{};
    StackTable st{};
    // variants >= 100: the same phase (variant - 100) on the table planner
    // (no computed tuple, LadderTable::ctup = 0), for A/B
    const bool table = variant >= 100 && variant < 200;
    if (table) variant -= 100;
    if (!plan_ladder(ms, nf, device_cu_count(), &st, &ws, !table)) return -34;
    if (tile_keys) ws.tile_keys = (uint32_t)tile_keys;
    ws.ntiles = (n + ws.tile_keys - 1) / ws.tile_keys;
    ws.pos = pos;
    ws.run_rows = runs;
    ws.run_starts = runs + ws.ntiles * (ws.nbins + 1);
    st.nf = nf;
    for (int j = 0; j < nf; j++) {
        st.words[j] = reinterpret_cast<const uint32_t *>(words[j]);
        st.mwords[j] = (uint32_t)(ms[j] / 32);
        st.row[j] = j;
    }
    const ModParams mp = make_mod_params(ms[0]);
    const size_t nw = (n + 63) / 64;
    hipError_t e = hipSuccess;
    switch (variant) {
        case 0: e = launch_probe_stacked(ks, mp, st, ws, res, slots, out, nw, s); break;
        case 1: e = launch_bin<true>(ks, mp, ws, slots, s); break;
        case 2: e = launch_apply_ladder(ws, ms[0], res, st, s); break;
        case 5: e = launch_combine(ws, res, slots, n, out, nw, st, s); break;
        case 11: case 12: {
            // pass 1 of the product's geometry WITHOUT the slot stores (11:
            // the sorted tile and runs as the product writes them; 12: also
            // no sorted-tile stores): what the slot plane and the tile's
            // write-out cost C3's pass 1
            SegMap sm{};
            if (pass1_plan(mp, ws, true, &sm) != kModLadder || ws.tile_keys != 8192) return -22;
            const bool cols = runs_as_columns(ws);
            uint32_t *rt = cols ? ws.run_starts : ws.run_rows;
            constexpr int kMinW = pass1_min_waves(1024, pass1_wgs_per_cu(1024, false, 1023));
            const unsigned g = pass1_grid(ws.ntiles, device_cu_count(), pass1_wgs_per_cu(1024, false, 1023));
            if (variant == 11) {
                if (cols) k_part_bin<KEYS_PACKED, false, true, 1024, kModLadder, 1023, kMinW><<<g, 1024, 0, s>>>(ks, mp, ws.pos, rt, sm, ws.ntiles, nullptr);
                else k_part_bin<KEYS_PACKED, false, false, 1024, kModLadder, 1023, kMinW><<<g, 1024, 0, s>>>(ks, mp, ws.pos, rt, sm, ws.ntiles, nullptr);
            } else {
                if (cols) k_part_bin<KEYS_PACKED, false, true, 1024, kModLadder, 1023, kMinW, 5><<<g, 1024, 0, s>>>(ks, mp, ws.pos, rt, sm, ws.ntiles, nullptr);
                else k_part_bin<KEYS_PACKED, false, false, 1024, kModLadder, 1023, kMinW, 5><<<g, 1024, 0, s>>>(ks, mp, ws.pos, rt, sm, ws.ntiles, nullptr);
            }
            e = hipGetLastError();
            if (e == hipSuccess && !cols) e = launch_runs_transpose(ws, s);
            break;
        }
        default: return -22;
    }
    return e == hipSuccess ? 0 : -5;
}

extern "C" int ubench_ladder_geometry(int nf, const uint64_t *ms, uint64_t *out6) {
    PartitionWorkspace ws{};
    StackTable st{};
    if (!plan_ladder(ms, nf, device_cu_count(), &st, &ws)) return -34;
    out6[0] = ws.nbins;
    out6[1] = st.lad.s;
    out6[2] = st.lad.hb;
    out6[3] = ladder_lds_bytes(st.lad);
    out6[4] = st.lad.k;
    out6[5] = st.lad.bpp;
    return 0;
}

// ---- rocprofv3 counter calibration (tools/ubench.py cal) --------------------
// Kernels that request a known number of bytes in the access shapes the
// product issues, so FETCH_SIZE / WRITE_SIZE can be read against them
// (MI355X_MICROARCH.md calibrates FETCH_SIZE only for wide coalesced reads).
// Reads (each requested byte once):
//   0  coalesced 16-B vectors, a wave's 64 vectors contiguous (1 KiB)
//   1  the first 64 B of every 128-B line, coalesced over lines
//   2  one 16-B vector of every 128-B line
//   3  pass 2's walk: the buffer as tiles x nseg runs of R vectors; block b
//      reads segment b's run of every tile, 4 lanes per run (lane i the
//      run's vectors i, i + 4, ...), each group of 4 its own tiles
// Writes (each byte once):
//   10 coalesced 16-B vector stores
//   11 2-byte stores, three per lane at 6i, 6i + 2, 6i + 4 (the probe's
//      result bytes along sorted runs)
//   12 one 4-B store per 128-B line, column-major into a row-major table
//      (pass 1's segment-major run-table columns)
__global__ void __launch_bounds__(1024) ub_cal(uint4 *buf, size_t nv, int shape, int R, int nseg,
                                               uint32_t *sink) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nth = (size_t)gridDim.x * blockDim.x;
    uint32_t acc = 0;
    if (shape == 0) {
        for (size_t i = tid; i < nv; i += nth) {
            const uint4 v = buf[i];
            acc ^= v.x ^ v.y ^ v.z ^ v.w;
        }
    } else if (shape == 1) {
        for (size_t i = tid; i < nv / 2; i += nth) {  // vector i of the half lines
            const uint4 v = buf[(i / 4) * 8 + (i % 4)];
            acc ^= v.x ^ v.y ^ v.z ^ v.w;
        }
    } else if (shape == 2) {
        for (size_t i = tid; i < nv / 8; i += nth) {
            const uint4 v = buf[i * 8];
            acc ^= v.x ^ v.y ^ v.z ^ v.w;
        }
    } else if (shape == 3) {
        const size_t ntiles = nv / ((size_t)nseg * R);
        const int g = threadIdx.x / 4, gl = threadIdx.x % 4, ng = blockDim.x / 4;
        for (int b = blockIdx.x; b < nseg; b += gridDim.x)
            for (size_t t = g; t < ntiles; t += ng) {
                const uint4 *run = buf + (t * nseg + b) * R;
                for (int i = gl; i < R; i += 4) {
                    const uint4 v = run[i];
                    acc ^= v.x ^ v.y ^ v.z ^ v.w;
                }
            }
    } else if (shape == 10) {
        for (size_t i = tid; i < nv; i += nth) buf[i] = make_uint4((uint32_t)i, 1, 2, 3);
    } else if (shape == 11) {
        uint16_t *b16 = reinterpret_cast<uint16_t *>(buf);
        for (size_t i = tid; i < nv * 16 / 6; i += nth) {
            b16[3 * i] = (uint16_t)i;
            b16[3 * i + 1] = (uint16_t)(i >> 1);
            b16[3 * i + 2] = (uint16_t)(i >> 2);
        }
    } else if (shape == 12) {
        uint32_t *b32 = reinterpret_cast<uint32_t *>(buf);
        const size_t rows = nv * 4 / 32, cols = 32;  // 128-B rows of 32 words
        for (size_t i = tid; i < rows * cols; i += nth) b32[(i % rows) * cols + i / rows] = (uint32_t)i;
    }
    if (acc == 0x12345678u) sink[0] = acc;
}

// Bytes each calibration shape requests from a buffer of nv vectors.
extern "C" uint64_t ubench_cal_bytes(int shape, size_t nv, int R, int nseg) {
    switch (shape) {
        case 0: case 10: return (uint64_t)nv * 16;
        case 1: return (uint64_t)nv * 8;
        case 2: return (uint64_t)nv * 2;
        case 3: return (uint64_t)(nv / ((size_t)nseg * R)) * nseg * R * 16;
        case 11: return (uint64_t)(nv * 16 / 6) * 6;
        case 12: return (uint64_t)nv * 16;
        default: return 0;
    }
}

extern "C" int ubench_cal(int shape, void *buf, size_t nv, int R, int nseg, void *stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint32_t *sink = reinterpret_cast<uint32_t *>(buf);  // never written for these inputs
    const unsigned grid = shape == 3 ? (unsigned)nseg : (unsigned)(device_cu_count() * 2);
    ub_cal<<<grid, 1024, 0, s>>>(reinterpret_cast<uint4 *>(buf), nv, shape, R, nseg, sink);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

// The run-table transpose with a configurable column stride (>= ntiles):
// rows [ntiles][width] -> cols[b * cstride + tile].  VEC = 1: the product's
// 64 x 64 LDS tile, 4-B accesses; VEC = 4: rows read as 16-B vectors when
// width % 4 == 0.  (tools/ubench.py transpose: does the 64 KiB column stride
// of C4's 16,384 super-tiles cost the write side?)
namespace {
__global__ void __launch_bounds__(256) ub_transpose(const uint32_t *__restrict__ rows,
                                                    uint32_t *__restrict__ cols, size_t ntiles,
                                                    int width, size_t cstride) {
    __shared__ uint32_t t[64][65];
    const int b0 = blockIdx.x * 64;
    const size_t t0 = (size_t)blockIdx.y * 64;
    const int x = threadIdx.x & 63, y0 = threadIdx.x >> 6;
    for (int y = y0; y < 64; y += 4) {
        const size_t tile = t0 + y;
        if (tile < ntiles && b0 + x < width) t[y][x] = rows[tile * width + b0 + x];
    }
    __syncthreads();
    for (int y = y0; y < 64; y += 4) {
        const size_t tile = t0 + x;
        if (tile < ntiles && b0 + y < width) cols[(size_t)(b0 + y) * cstride + tile] = t[x][y];
    }
}
}  // namespace

// variant 2: every load of the tile issued before any LDS store (clamped
// addresses, no load under a branch), the stores likewise; TR tile rows.
template <int TR>
__global__ void __launch_bounds__(256) ub_transpose2(const uint32_t *__restrict__ rows,
                                                     uint32_t *__restrict__ cols, size_t ntiles,
                                                     int width, size_t cstride) {
    __shared__ uint32_t t[TR][65];
    constexpr int kPer = TR / 4;
    const int b0 = blockIdx.x * 64;
    const size_t t0 = (size_t)blockIdx.y * TR;
    const int x = threadIdx.x & 63, y0 = threadIdx.x >> 6;
    uint32_t v[kPer];
    const int bx = min(b0 + x, width - 1);
#pragma unroll
    for (int i = 0; i < kPer; i++) {
        const size_t tile = min(t0 + y0 + 4 * i, ntiles - 1);
        v[i] = rows[tile * width + bx];
    }
#pragma unroll
    for (int i = 0; i < kPer; i++) t[y0 + 4 * i][x] = v[i];
    __syncthreads();
    // writes: lane x takes tile t0 + x (+ 64 per half for TR = 128), row b0 + y
#pragma unroll
    for (int h = 0; h < TR / 64; h++) {
        const size_t tile = t0 + h * 64 + x;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int y = y0 + 4 * i;
            if (tile < ntiles && b0 + y < width) cols[(size_t)(b0 + y) * cstride + tile] = t[h * 64 + x][y];
        }
    }
}

extern "C" int ubench_transpose(const void *rows, void *cols, size_t ntiles, int width,
                                size_t cstride, void *stream) {
    if (cstride < ntiles) return -22;
    const dim3 grid((unsigned)((width + 63) / 64), (unsigned)((ntiles + 63) / 64));
    ub_transpose<<<grid, 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(
        reinterpret_cast<const uint32_t *>(rows), reinterpret_cast<uint32_t *>(cols), ntiles, width,
        cstride);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int ubench_transpose2(int tr, const void *rows, void *cols, size_t ntiles, int width,
                                 size_t cstride, void *stream) {
    if (cstride < ntiles || (tr != 64 && tr != 128)) return -22;
    const dim3 grid((unsigned)((width + 63) / 64), (unsigned)((ntiles + tr - 1) / tr));
    auto r = reinterpret_cast<const uint32_t *>(rows);
    auto c = reinterpret_cast<uint32_t *>(cols);
    auto s = reinterpret_cast<hipStream_t>(stream);
    if (tr == 64) ub_transpose2<64><<<grid, 256, 0, s>>>(r, c, ntiles, width, cstride);
    else ub_transpose2<128><<<grid, 256, 0, s>>>(r, c, ntiles, width, cstride);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

// ---------------------------------------------------------------------------
// The compaction's launches, forced one at a time on the caller's device
// buffers (tests/test_gpu_compact_edges.py): each allocates and frees its own
// workspace, runs on the null stream, synchronises it before returning and
// returns the HIP error as an int (0 = hipSuccess).  runs / a / b / out and the
// length arrays are host arrays of device pointers and of entry counts.
// ---------------------------------------------------------------------------
namespace {
// a call's workspace, freed on every way out
struct UbScratch {
    void *p = nullptr;
    hipError_t alloc(uint64_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }
    ~UbScratch() {
        if (p) (void)hipFree(p);
    }
};
}  // namespace

// launch_compact_kway (k_kway_samples, k_kway_split, k_kway_merge) of k runs,
// newest first.  out: sum(n) entries; keys_out (optional): sum(n) int32.
// Host results: bounds_out = the partition bounds, (*nparts_out + 1) rows of
// kKwayMaxRuns u32 as launch_compact_kway leaves them in its workspace
// (kway_bounds_offset; columns k and up unwritten), sized by the caller for
// at least sum(ceil(n[r] / 256)) + 1 rows; *count_out = the kept count.
extern "C" int ubench_kway_compact(const void *const *runs, const uint64_t *n, int k, int drop,
                                   void *out, int32_t *keys_out, uint32_t *bounds_out,
                                   uint64_t *nparts_out, uint32_t *count_out) {
    if (k < 1 || k > kKwayMaxRuns) return (int)hipErrorInvalidValue;
    const uint64_t np = kway_parts(n, k);
    const uint64_t wbytes = (kway_workspace_bytes(n, k) + 15) & ~15ull;
    UbScratch ws;
    hipError_t e = ws.alloc(wbytes + 16);  // + the kept count
    if (e != hipSuccess) return (int)e;
    char *w = static_cast<char *>(ws.p);
    uint32_t *dcount = reinterpret_cast<uint32_t *>(w + wbytes);
    e = launch_compact_kway(runs, n, k, drop, out, keys_out, w, dcount, nullptr);
    if (e != hipSuccess) return (int)e;
    e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) return (int)e;
    e = hipMemcpy(bounds_out, w + kway_bounds_offset(n, k), (np + 1) * kKwayMaxRuns * 4,
                  hipMemcpyDeviceToHost);
    if (e != hipSuccess) return (int)e;
    *nparts_out = np;
    return (int)hipMemcpy(count_out, dcount, 4, hipMemcpyDeviceToHost);
}

// launch_merge_round (k_merge_split, k_merge_tile) of np pairs: out[p] = the
// stable merge of a[p] (na[p] entries, wins ties) and b[p]; a, b 8-B aligned,
// out 16-B aligned, na[p] + nb[p] entries.
extern "C" int ubench_merge_round(const void *const *a, const uint64_t *na, const void *const *b,
                                  const uint64_t *nb, void *const *out, int np) {
    std::vector<MergePairArgs> pairs;
    uint64_t total = 0;
    for (int p = 0; p < np; p++) {
        pairs.push_back({a[p], na[p], b[p], nb[p], out[p]});
        total += na[p] + nb[p];
    }
    UbScratch ws;
    hipError_t e = ws.alloc(merge_split_words(total) * 8);
    if (e != hipSuccess) return (int)e;
    e = launch_merge_round(pairs.data(), np, static_cast<uint64_t *>(ws.p), nullptr);
    if (e != hipSuccess) return (int)e;
    return (int)hipStreamSynchronize(nullptr);
}

// launch_dedup (k_compact_count, k_scan_counts, k_compact_write) of n
// key-sorted entries at `in` (16-B aligned: the kernels read entry pairs as
// vectors).  out: n entries; keys_out (optional): n int32; *count_out (host)
// = the kept count.
extern "C" int ubench_dedup(const void *in, uint64_t n, int drop, void *out, int32_t *keys_out,
                            uint32_t *count_out) {
    if (reinterpret_cast<uintptr_t>(in) & 15) return (int)hipErrorInvalidValue;
    UbScratch ws;
    hipError_t e = ws.alloc(compact_count_words(n) * 4 + 4);
    if (e != hipSuccess) return (int)e;
    uint32_t *counts = static_cast<uint32_t *>(ws.p);
    e = launch_dedup(in, n, drop, out, counts, nullptr, keys_out);
    if (e != hipSuccess) return (int)e;
    e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) return (int)e;
    return (int)hipMemcpy(count_out, counts + compact_count_words(n) - 1, 4, hipMemcpyDeviceToHost);
}
