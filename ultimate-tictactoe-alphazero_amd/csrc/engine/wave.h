// engine/wave.h — lane and wave helpers for wave64: lane / wave indices, ballots below a lane, readlane of floats,
// the DPP arg-max (first index wins ties), the wave's memory fence and the system-scope stores the host reads.
#pragma once
#include "layout.h"

namespace uttt {

// ------------------------------------------------------------ wave helpers --
__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & (kWave - 1)); }
// This wave's global index (one wave per tree / slot / row), marked wave-uniform: what is derived from
// it (the tree's control words, its states, the rules applied to them) lives in scalar registers and
// runs on the scalar unit instead of as 64 identical vector lanes (round 4)
__device__ __forceinline__ int wave_index() {
    return __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)));
}

__device__ __forceinline__ uint64_t lanes_below() {
    const int l = lane_id();
    return l == 0 ? 0ull : (~0ull >> (64 - l));
}

// Wave-wide arg-max: larger value wins, equal values -> smaller index
// (the reference's strict '>' scan in child order, uttt_mcts.cpp:69-78).
__device__ __forceinline__ void wave_argmax_d(double &v, int &i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off);
        const int oi = __shfl_xor(i, off);
        if (ov > v || (ov == v && oi < i)) {
            v = ov;
            i = oi;
        }
    }
}

__device__ __forceinline__ float readlane_f(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// The same arg-max by DPP lane moves, no LDS round trips (k_select's per-level reduction): the wave's
// largest value by one reduction of one instruction pair per step, then the smallest index among the
// lanes holding it ("larger value, then smaller index": the reference's strict '>' scan in child order)
// from one ballot when the maximum is unique, else from per-group ballots. Values are never NaN here (the per-lane scan's strict '>' from -1e9 never takes one); -0 and
// +0 compare equal, so they tie on the index as in the scan. Each reduction runs within each row of 16
// lanes (quad swaps, half-row and row mirrors), then row 0 into row 1 and row 2 into row 3
// (row_bcast15), then row 1 into rows 2-3 (row_bcast31): the result is valid in lane 63.
// one reduction step as a single DPP-sourced VALU op (the two wait states a DPP read of a VGPR
// written by the previous VALU op needs are in the asm: the compiler does not see inside it)
#define UTTT_DPP_STEP(op, ctl)                                                                     \
    __device__ __forceinline__ void op##_##ctl(uint32_t &k) {                                      \
        asm volatile("s_nop 1\n\t" #op "_dpp %0, %0, %0 " UTTT_DPP_##ctl : "+v"(k));             \
    }
#define UTTT_DPP_q1 "quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf"
#define UTTT_DPP_q2 "quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf"
#define UTTT_DPP_hm "row_half_mirror row_mask:0xf bank_mask:0xf"
#define UTTT_DPP_rm "row_mirror row_mask:0xf bank_mask:0xf"
#define UTTT_DPP_b15 "row_bcast:15 row_mask:0xa bank_mask:0xf"
#define UTTT_DPP_b31 "row_bcast:31 row_mask:0xc bank_mask:0xf"
UTTT_DPP_STEP(v_max_u32, q1)
UTTT_DPP_STEP(v_max_u32, q2)
UTTT_DPP_STEP(v_max_u32, hm)
UTTT_DPP_STEP(v_max_u32, rm)
UTTT_DPP_STEP(v_max_u32, b15)
UTTT_DPP_STEP(v_max_u32, b31)
// wave-uniform result: the index of the largest v, the lowest index among equal maxima
// (cnt: the scanned child count; candidate indices are below it)
__device__ __forceinline__ int wave_argmax(float v, int i, int cnt) {
    // the value as an order-preserving unsigned (-0 canonicalised to +0 first), so each step of the max
    // is an integer max (no float canonicalisation)
    uint32_t b = __float_as_uint(v + 0.0f);
    b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    uint32_t m = b;
    v_max_u32_q1(m);   // quad_perm [1,0,3,2]
    v_max_u32_q2(m);   // quad_perm [2,3,0,1]
    v_max_u32_hm(m);   // row_half_mirror
    v_max_u32_rm(m);   // row_mirror
    v_max_u32_b15(m);  // row_bcast15 -> rows 1, 3
    v_max_u32_b31(m);  // row_bcast31 -> rows 2, 3
    asm volatile("s_nop 1");  // the asm's VALU write before the compiler's reads of m
    const uint32_t top = (uint32_t)__builtin_amdgcn_readlane((int)m, 63);
    // the usual case: one lane holds the maximum, and its index is the answer (no second pass)
    const uint64_t at = __ballot(b == top);
    if (__popcll(at) == 1) return __builtin_amdgcn_readlane(i, __builtin_ctzll(at));
    // ties (a node expanded by a flush of k copies holds k equal children per action until they are
    // visited): the smallest index among the lanes holding the maximum. Lane l's candidate is its own first
    // maximum, child l + 64 g of its scan group g (i & 63 == l), so the answer is the lowest such lane of
    // the lowest group present: one ballot per group from group 0 (round 5: in place of a second 6-step DPP
    // reduction and its wait states; usually group 0 or 1 answers). Every scan group of the node is
    // covered: a flush of k copies gives up to k x 81 children, more than 64 groups past batch 50.
    const int ngroups = (cnt + kWave - 1) / kWave;
    for (int g = 0; g < ngroups; ++g) {
        const uint64_t m = __ballot(b == top && (i >> 6) == g);
        if (m) return g * kWave + __builtin_ctzll(m);
    }
    return kNone;  // unreachable: some lane holds the maximum with a child index
}

// Orders this wave's global stores before its later global loads (other lanes
// read what one lane wrote; same CU, so workgroup scope suffices).
__device__ __forceinline__ void wave_memory_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }

// Stores to host-visible (fine-grained pinned) words: system-coherent (sc0 sc1) and relaxed. A hand-off to
// the host is these stores, one s_waitcnt vmcnt(0) (they are acknowledged), then the tag, also relaxed: no
// release fence, whose L2 write-back (buffer_wbl2 sc0 sc1) would flush every line the kernel dirtied in the
// XCD's L2 (tree records, rows) to HBM at each hand-off, when the host reads only these words (round 6)
__device__ __forceinline__ void st_host(int32_t *a, int32_t v) {
    __hip_atomic_store(a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void st_host(float *a, float v) {
    __hip_atomic_store(a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void host_stores_done() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

}  // namespace uttt
