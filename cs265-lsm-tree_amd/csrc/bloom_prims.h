// bloom_prims.h — device primitives shared by the partition kernels (key
// loads, the wave scan, one-instruction shift-ors, the LDS barriers and
// absolute-address LDS reads, the sorted tiles' packing, the XCD map, the
// non-temporal and the write-through store) and the two compile-time helpers
// of their launchers.
//
// Bit-exact restatement of jackdent/cs265-lsm-tree src/bloom_filter.cpp:49-59
// over batches of int32 keys; the bitmap is dynamic_bitset<unsigned long>'s
// block layout (src/bloom_filter.h:7), addressed as 32-bit words.
#pragma once

#include <stdlib.h>

#include <algorithm>
#include <numeric>
#include <type_traits>

#include "bloom_kernels.h"

namespace bloomhip {

namespace {

// Key i of a span.  The layout is a template argument wherever the kernel
// has one, so entry_t runs (stride 8) address as base + 8i instead of a
// runtime 64-bit stride multiply.
template <int LAYOUT = KEYS_STRIDED>
__device__ __forceinline__ int32_t load_key(const KeySpan &ks, size_t i) {
    if constexpr (LAYOUT == KEYS_PACKED) return reinterpret_cast<const int32_t *>(ks.base)[i];
    else if constexpr (LAYOUT == KEYS_ENTRY) return reinterpret_cast<const int2 *>(ks.base)[i].x;
    else return *reinterpret_cast<const int32_t *>(ks.base + i * ks.stride);
}

// Inclusive prefix sum across the 64 lanes of a wave in DPP steps (no LDS):
// row_shr 1/2/4/8 inside each row of 16 lanes (a lane with no source keeps
// the old value 0), then row_bcast:15 (row r's last lane into row r + 1,
// rows 1 and 3) and row_bcast:31 (lane 31 into rows 2 and 3).
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);
    return v;
}

// (a << S) | b in one instruction.
template <typename S>
__device__ __forceinline__ uint32_t lshl_or(uint32_t a, S sh, uint32_t b) {
    uint32_t r;
    asm("v_lshl_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "i"(sh), "v"(b));
    return r;
}

// (a << s) | b in one instruction, s in an SGPR.
__device__ __forceinline__ uint32_t lshl_or_s(uint32_t a, uint32_t sh, uint32_t b) {
    uint32_t r;
    asm("v_lshl_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(sh), "v"(b));
    return r;
}

// Workgroup barrier that waits for this wave's LDS operations only.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
// The same, and from the barrier on the wave issues at priority P (0-3): the
// s_setprio sits in the barrier's own asm, so it is no scheduling boundary
// of its own.  P < 0: lds_barrier().
template <int P>
__device__ __forceinline__ void lds_barrier_prio() {
    static_assert(P <= 3, "s_setprio takes 0-3");
    if constexpr (P < 0) lds_barrier();
    else asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier\n\ts_setprio %0" ::"n"(P) : "memory");
}

// LDS word at an absolute byte address.  Pass 2 has no static LDS, so its
// dynamic image starts at LDS address 0 (launch_apply_g checks that once per
// kernel) and image offsets are addresses: a pointer formed from the image's
// generic pointer costs a v_add of its relocated address (0) per access.
__device__ __forceinline__ uint32_t lds_word(uint32_t byte_addr) {
    return *(const __attribute__((address_space(3))) uint32_t *)(size_t)byte_addr;
}
typedef uint32_t lds_v2u __attribute__((ext_vector_type(2)));
typedef uint32_t lds_v4u __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint2 lds_word2(uint32_t byte_addr) {
    const lds_v2u v = *(const __attribute__((address_space(3))) lds_v2u *)(size_t)byte_addr;
    return make_uint2(v.x, v.y);
}
__device__ __forceinline__ uint4 lds_word4(uint32_t byte_addr) {
    const lds_v4u v = *(const __attribute__((address_space(3))) lds_v4u *)(size_t)byte_addr;
    return make_uint4(v.x, v.y, v.z, v.w);
}

template <bool B>
struct BoolC {
    static constexpr bool value = B;
};

// The sorted tiles' format: three 21-bit entries in one u64 (bits 0-20,
// 21-41, 42-62), as its two words, and six in one 16-B vector.
// (a << s) | b is one v_lshl_or_b32; the compiler emitted a shift
// and an or for each (5 instead of 3 per u64)
__device__ __forceinline__ uint2 pack_entries3(uint32_t e0, uint32_t e1, uint32_t e2) {
    return make_uint2(lshl_or(e1, 21, e0), lshl_or(e2, 10, e1 >> 11));
}
__device__ __forceinline__ uint4 pack_entries6(const uint32_t (&e)[6]) {
    return make_uint4(lshl_or(e[1], 21, e[0]), lshl_or(e[2], 10, e[1] >> 11),
                      lshl_or(e[4], 21, e[3]), lshl_or(e[5], 10, e[4] >> 11));
}

// Bijective block -> work-unit map that gives each XCD a contiguous range of
// units (cdna_hip_programming.md §5.5 T1, bijective form for n % 8 != 0).
__device__ __forceinline__ unsigned xcd_remap(unsigned x, unsigned n) {
    constexpr unsigned kXcds = 8;
    const unsigned q = n / kXcds, r = n % kXcds;
    const unsigned xcd = x % kXcds, idx = x / kXcds;
    // XCD xcd owns units [start, start + q + (xcd < r)).
    const unsigned start = xcd * q + min(xcd, r);
    return start + idx;
}

// A 16-B non-temporal store (pass 1's sorted tiles beyond the Infinity Cache).
__device__ __forceinline__ void nt_store16(uint4 *p, const uint4 &v) {
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    const v4u x = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(x, reinterpret_cast<v4u *>(p));
}

// A 16-B write-through (sc1) store at byte offset off of a wave-uniform
// base: the line goes to memory as it is stored and leaves the writer's L2, so
// nothing of it is left to flush at the kernel's end.  A buffer store (the
// base in SGPRs, counted in vmcnt like any store); off < 4 GiB.
// The whole offset travels in the VGPR operand: with part of it in the SGPR
// offset operand pass 1 wrote wrong tiles (cause not found;
// profiles/build_edges/README.md section 4), so soffset stays 0 with this
// descriptor.
__device__ __forceinline__ void wt_store16(void *base, uint32_t off, const uint4 &v) {
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    const v4u x = {v.x, v.y, v.z, v.w};
    // raw buffer: stride 0, no bound (num_records ~0), 32-bit data format
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(base, 0, -1, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b128(x, rsrc, (int)off, 0, /*aux: sc1*/ 16);
}

// f(integral_constant<V>) for the V of Vs that equals v; false when none
// does, or f's own result.
template <int... Vs, typename F>
bool on_value(int v, F &&f) {
    return ((v == Vs && f(std::integral_constant<int, Vs>{})) || ...);
}

}  // namespace

}  // namespace bloomhip
