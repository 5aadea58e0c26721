// engine/scan.h — between the descent and the evaluator: the 1,024-thread block scans, k_scan (pending flags ->
// dense slots in tree order, the round's counts) and k_encode (leaf -> NCHW (3,9,9) f32 row).
//
// A part of engine.hip's one translation unit, like its siblings in engine/. The order of the definitions here,
// and of this header among the others, is load-bearing for the code object: engine.hip's include list is the
// order of definition.
#pragma once
#include "layout.h"
#include "wave.h"
#include "uttt_bits.h"

namespace uttt {

// ------------------------------------------------------------------- scan --
// Exclusive prefix sum of one value per thread over a 1,024-thread block (16 waves): a wave scan
// by lane shifts, the 16 wave totals scanned by the first wave through LDS; two barriers where
// a Hillis-Steele scan over LDS takes twenty. Returns the exclusive prefix; *total gets the sum.
template <typename T>
__device__ __forceinline__ T block_scan_1024(T v, T *total, T *wsum /* __shared__ [16] */) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    T x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T t = __shfl_up(x, off);
        if (lane >= off) x += t;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    if (wave == 0) {
        T w = lane < 16 ? wsum[lane] : T(0);
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
            const T t = __shfl_up(w, off);
            if (lane >= off) w += t;
        }
        if (lane < 16) wsum[lane] = w;
    }
    __syncthreads();
    *total = wsum[15];
    return x - v + (wave > 0 ? wsum[wave - 1] : T(0));
}

// Two exclusive scans over the block in one pass (the barriers and the wave-0 step shared): k_finalize's
// finished lengths and its packed (free, finished) counts (round 6: two passes of block_scan_1024 before)
__device__ __forceinline__ void block_scan2_1024(unsigned long long &a, unsigned long long &c,
                                                 unsigned long long *a_tot, unsigned long long *c_tot,
                                                 unsigned long long *wsum /* __shared__ [32] */) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long x = a, y = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long tx = __shfl_up(x, off), ty = __shfl_up(y, off);
        if (lane >= off) {
            x += tx;
            y += ty;
        }
    }
    if (lane == 63) {
        wsum[wave] = x;
        wsum[16 + wave] = y;
    }
    __syncthreads();
    if (wave == 0) {
        unsigned long long w = lane < 32 ? wsum[lane] : 0ull;  // lanes 0-15: a's wave sums, 16-31: c's
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
            const unsigned long long t = __shfl_up(w, off);
            if ((lane & 15) >= off) w += t;
        }
        if (lane < 32) wsum[lane] = w;
    }
    __syncthreads();
    *a_tot = wsum[15];
    *c_tot = wsum[31];
    a = x - a + (wave > 0 ? wsum[wave - 1] : 0ull);
    c = y - c + (wave > 0 ? wsum[16 + wave - 1] : 0ull);
}

// One block: exclusive scan of pending flags -> tree_of[slot] in tree order.
// host_count (optional): the three counts are also stored to this host-visible (fine-grained pinned)
// word triple at system scope, so the host reads a round's counts when the round's event completes
// without a copy operation on the stream (round 4: one stream operation less per round). Round 5: word 3
// gets the round's tag after them (a system-scope release store), so a host that polls the tag needs no
// event either (uttt_round_hash_async).
__global__ __launch_bounds__(1024) void k_scan(Trees tr, unsigned long long *stats, int32_t *host_count, int32_t tag) {
    __shared__ unsigned long long wsum[16];
    const int tid = threadIdx.x;
    if (stats && tid < 64) {  // the select launch before this scan is complete: fold its slowest tree
        // (the max over the stripes, one per lane of the first wave)
        unsigned long long ml = 0ull, mt = 0ull;
        if (tid < kStripes) {
            unsigned long long *a = stats + kKSelMax * kRow + tid * kStripeStride;
            unsigned long long *b = stats + kKSelTripMax * kRow + tid * kStripeStride;
            ml = *a;
            mt = *b;
            *a = 0ull;
            *b = 0ull;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long ol = __shfl_xor(ml, off), ot = __shfl_xor(mt, off);
            ml = ol > ml ? ol : ml;
            mt = ot > mt ? ot : mt;
        }
        if (tid == 0) {
            stats[kKSelMaxSum * kRow] += ml;
            stats[kKSelTripMaxSum * kRow] += mt;
        }
    }
    const int per = (tr.n_trees + 1023) / 1024;
    const int b = tid * per, e = min(b + per, tr.n_trees);
    // up to kScanPer flags per thread (4,096 trees) are loaded together and kept for the second pass (round 5:
    // the two loops each waited for one load per tree in turn); more per thread are re-read there
    constexpr int kScanPer = 4;
    int held[kScanPer];
#pragma unroll
    for (int j = 0; j < kScanPer; ++j) held[j] = b + j < e ? tr.pending[b + j] : 0;
    unsigned long long local = 0, cap = 0, mo = 0;
    for (int i = b; i < e; ++i) {
        const int p = (i - b < kScanPer ? held[i - b] : tr.pending[i]) & 0xFF;
        local += p == 1 || p == 3;
        cap += p == 2;
        mo += p >= 2;
    }
    // the three counts in 21-bit fields of one scanned word (each total <= n_trees < 2^21)
    unsigned long long tot;
    const unsigned long long ex = block_scan_1024(local | (cap << 21) | (mo << 42), &tot, wsum);
    int slot = (int)(ex & 0x1FFFFFull);
    for (int i = b; i < e; ++i) {
        const int p = i - b < kScanPer ? held[i - b] : tr.pending[i];
        if ((p & 1) != 0) {  // 1 or 3
            tr.depth_of[slot] = p >> 8;
            tr.tree_of[slot++] = i;
        }
    }
    if (tid == 0) {
        const int c0 = (int)(tot & 0x1FFFFFull), c1 = (int)((tot >> 21) & 0x1FFFFFull);
        const int c2 = (int)(tot >> 42);  // trees with simulations left after this round (0: the search ends with it)
        tr.count[0] = c0;
        tr.count[1] = c1;
        tr.count[2] = c2;
        if (host_count) {
            __hip_atomic_store(host_count + 0, c0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(host_count + 1, c1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(host_count + 2, c2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            host_stores_done();
            st_host(host_count + 3, tag);
        }
    }
}

// ----------------------------------------------------------------- encode --
// The network input of each pending leaf (uttt_game.cpp:244-280 transposed to
// NCHW as pv_mcts_cpp.py:57-60 does): ch0 own stones, ch1 opponent, ch2 legal.
__global__ __launch_bounds__(256) void k_encode(Trees tr, float *__restrict__ x, int n) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n * 243) return;
    const int slot = g / 243, j = g % 243;
    const int ch = j / 81, pos = j % 81;
    const uttt_state_t s = tr.leaf[tr.tree_of[slot]];
    const int a = action_at(pos);
    uint32_t bit;
    if (ch == 0) bit = bit_of(s.own, a);
    else if (ch == 1) bit = bit_of(s.opp, a);
    else {
        uint32_t m[3];
        legal_mask(s, m);
        bit = bit_of(m, a);
    }
    x[g] = bit ? 1.0f : 0.0f;
}

}  // namespace uttt
