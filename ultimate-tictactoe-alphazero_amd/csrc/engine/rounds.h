// engine/rounds.h — the fused rounds, select_wave and apply_wave in one dispatch: k_flush1 (one flush of a one-tree
// search), the wave's input_words and hash_leaf_row (the hash evaluator on the leaf a wave just queued), k_round1
// (one tree-only round with its per-block counts) and k_apply_tree (the last round's evaluations, by tree).
//
// A part of engine.hip's one translation unit, like its siblings in engine/. The order of the definitions here,
// and of this header among the others, is load-bearing for the code object: engine.hip's include list is the
// order of definition.
#pragma once
#include "apply.h"
#include "cache.h"
#include "layout.h"
#include "select.h"
#include "wave.h"
#include "uttt_bits.h"

namespace uttt {

// One flush of a one-tree search in one launch (round 5, uttt_search_select_host / _apply_host): the previous
// flush's evaluation applied (k_apply's body, reading it from pinned host memory), then the next descent
// (k_select's body), which stores the round's result to pinned host memory behind its tag. One wave, one
// dispatch per flush where k_apply, k_select and k_scan took three.
template <bool PY>
__global__ __launch_bounds__(kWave) void k_flush1(Pool pool, Trees tr, EvalCache cache, EvalCache apply_cache,
                                                  const float *__restrict__ policy, int64_t pld,
                                                  const float *__restrict__ value, int64_t vld,
                                                  const int32_t *__restrict__ rowbase, int per_copy, int do_apply,
                                                  unsigned long long *stats, HostLeaf *host_leaf, int32_t tag) {
    __shared__ __attribute__((aligned(16))) float s_row[84];
    if (do_apply) {
        apply_wave(pool, tr, apply_cache, policy, pld, value, vld, rowbase, per_copy,
                   stats ? stats + kKApply * kRow : nullptr, 0, s_row);
        wave_memory_fence();  // the descent reads the records the apply wrote
    }
    select_wave<PY>(pool, tr, cache, stats, 0, s_row, host_leaf, tag);
}

// The hash evaluator's outputs for one state into row `row` (k_hash_leaves' and k_round1's): bit j = ch * 81 +
// R * 9 + C of the network input, as k_encode writes it, so the words and outputs are k_hash_eval's.
// The network input of state s (m: its legal mask) as four ballot words over its 243 bits
__device__ __forceinline__ void input_words(const uttt_state_t &s, const uint32_t (&m)[3], uint64_t (&w)[4]) {
    const int lane = lane_id();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = i * 64 + lane;
        bool on = false;
        if (j < 243) {
            const int ch = j / 81, a = action_at(j % 81);
            on = (ch == 0 ? bit_of(s.own, a) : (ch == 1 ? bit_of(s.opp, a) : bit_of(m, a))) != 0u;
        }
        w[i] = __ballot(on);
    }
}
__device__ __forceinline__ void hash_leaf_row(const uttt_state_t &s, float *__restrict__ policy, float *__restrict__ value,
                                              int row) {
    const int lane = lane_id();
    uint32_t m[3];
    legal_mask(s, m);
    uint64_t w[4];
    input_words(s, m, w);
    const uint64_t h = hash_words(w);
    policy[(size_t)row * 81 + lane] = hash_prior(h, lane);
    if (lane < 17) policy[(size_t)row * 81 + 64 + lane] = hash_prior(h, 64 + lane);
    if (lane == 0) value[row] = hash_value(h);
}

// The select's slowest tree folded into the sums (as k_scan folds it): the max over the stripes of rows rm and
// rt, one stripe per lane l of one wave, which clears them
__device__ __forceinline__ void fold_select_max(unsigned long long *stats, int rm, int rt, int l) {
    unsigned long long ml = 0ull, mt = 0ull;
    if (l < kStripes) {
        unsigned long long *a = stats + rm * kRow + l * kStripeStride;
        unsigned long long *bb = stats + rt * kRow + l * kStripeStride;
        ml = __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        mt = __hip_atomic_load(bb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(a, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(bb, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long ol = __shfl_xor(ml, off), ot = __shfl_xor(mt, off);
        ml = ol > ml ? ol : ml;
        mt = ot > mt ? ot : mt;
    }
    if (l == 0) {
        stats[kKSelMaxSum * kRow] += ml;
        stats[kKSelTripMaxSum * kRow] += mt;
    }
}

// One tree-only round in ONE dispatch (round 6; UTTT_FUSED_ROUNDS=0 keeps the public calls'
// k_select + k_scan + k_hash_leaves + k_apply). With the hash evaluator nothing needs the leaves in slot order,
// so the rows are indexed by TREE: wave t applies its tree's evaluation of the previous round from row t
// (apply != 0 and its pending word, still the previous round's, shows a queued leaf), runs the next descent
// (k_select's body), and evaluates the leaf it queued straight into row t. The round's counts, which k_scan
// produces for the other rounds, are summed per block into a partial (sc1 store) and the last block to arrive
// (striped arrival counters, then one top counter) adds the partials, publishes them (device counts, the host
// ring and its tag) and resets the counters for the next round. Every tree's work is k_apply's and k_select's
// in the same order, so every result is the unfused round's (the fused-rounds test runs both).
constexpr int kR1Stripes = 8;
// uttt_rounds_hash_move's per-block count words: n0 (queued leaves) bits 0-4, n1 (budget stops) 5-9, n2
// (trees with simulations left) 10-14, at most kWavesPerBlock = 16 each; the round's tag (17 bits) above
constexpr int kPartTagShift = 15;
constexpr uint32_t kPartTagMask = 0x1FFFFu;
constexpr uint32_t kPartLiveMask = 0x1Fu | (0x1Fu << 10);
static_assert(kWavesPerBlock <= 31, "k_round1's per-block count words hold 5-bit counts");
constexpr int kR1Partial = 64;  // rctl: [0..7] stripe arrivals, [32] top, [64 + block] partials
template <bool PY>
__global__ __launch_bounds__(kBlock, 4) void k_round1(Pool pool, Trees tr, EvalCache cache, const float *apply_policy,
                                                   const float *apply_value, float *__restrict__ policy,
                                                   float *__restrict__ value, int apply, unsigned long long *stats,
                                                   int32_t *host_count, int32_t tag, uint32_t *rctl,
                                                   uint32_t *part_host, uint32_t *part_dev, const uint32_t *part_prev,
                                                   int nb_prev, int stats_parity) {
    __shared__ __attribute__((aligned(16))) float s_row[kWavesPerBlock][84];
    __shared__ uint32_t s_cnt;
    __shared__ int s_last;
    // part_host (uttt_rounds_hash_move's rounds, no kernel timing): no last-block publish. Each block stores its
    // counts with the round's tag into its own word of a host array (and of a device array the next round's
    // empty-round check reads, part_prev), and the host sums the words once every block's has the tag: the
    // arrival atomics, the partials' reload and the last block's drain left each round's critical path (round 6)
    if (part_host) {
        if (stats && blockIdx.x == 0 && threadIdx.x < kWave) {
            // the previous round's slowest tree (the other parity's rows) into the sums; this round's waves
            // write this parity's rows meanwhile
            fold_select_max(stats, stats_parity ? kKSelMax : kKSelMaxB, stats_parity ? kKSelTripMax : kKSelTripMaxB,
                            (int)threadIdx.x);
        }
        const uint32_t t17 = ((uint32_t)tag & kPartTagMask) << kPartTagShift;
        bool empty = false;
        if (part_prev) {  // the previous round queued no leaf and left no tree with simulations
            bool busy = false;
            for (int i = threadIdx.x; i < nb_prev; i += kBlock) busy |= (part_prev[i] & kPartLiveMask) != 0u;
            empty = !__syncthreads_or(busy);
        }
        if (empty) {
            if (threadIdx.x == 0) {
                part_dev[blockIdx.x] = t17;
                __hip_atomic_store(part_host + blockIdx.x, t17, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            return;
        }
    }
    // a round behind one that queued no leaf and left no tree with simulations (the host's look-ahead rounds
    // past a move's end) has nothing to apply or select: every pending word is already 0 and the counts
    // stay 0, so block 0 publishes them and its tag, and every other block leaves at once (round 6: such a
    // round cost ~19 us of GPU time as a full pass over the trees; k_begin marks a new search non-empty)
    if (!part_host && tr.count[0] == 0 && tr.count[2] == 0) {
        if (blockIdx.x == 0 && threadIdx.x == 0 && host_count) {
            st_host(host_count + 0, 0);
            st_host(host_count + 1, 0);
            st_host(host_count + 2, 0);
            host_stores_done();
            st_host(host_count + 3, tag);
        }
        return;
    }
    const int t = wave_index();
    const int lane = lane_id();
    if (threadIdx.x == 0) s_cnt = 0u;
    __syncthreads();
    CachePublish held{-1, 0u};  // the apply's cache insert, published after this block's drain below
    if (t < tr.n_trees) {
        const int prev = __builtin_amdgcn_readfirstlane(tr.pending[t]);  // the previous round's, until the select
        if (apply && (prev & 1)) {
            apply_wave(pool, tr, cache, apply_policy, 81, apply_value, 1, nullptr, 0,
                       stats ? stats + kKApply * kRow : nullptr, t, s_row[threadIdx.x >> 6], t, prev >> 8, nullptr,
                       false, &held);
            wave_memory_fence();  // the descent reads the records the apply wrote
        }
        uttt_state_t leaf;
        const int p = select_wave<PY>(pool, tr, cache, stats, t, s_row[threadIdx.x >> 6], nullptr, 0,
                                      part_host ? stats_parity : 0, &leaf);
        if (p & 1) hash_leaf_row(leaf, policy, value, t);  // the queued leaf (its state from the descent)
        const int q = p & 0xFF;
        if (lane == 0)  // pending | stopped << 10 | left << 20 (at most kWavesPerBlock each)
            atomicAdd(&s_cnt, (uint32_t)((q == 1 || q == 3) ? 1 : 0) | ((q == 2 ? 1u : 0u) << 10) |
                                  ((q >= 2 ? 1u : 0u) << 20));
    }
    // every wave's stores (rows, records, stats atomics, a held cache record) complete before the block's
    // partial is published, and before the held record's flag
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    cache_publish(cache, held);
    __syncthreads();
    if (part_host) {  // the block's counts and the round's tag, one word (its stores drained above)
        if (threadIdx.x == 0) {
            const uint32_t w = (((uint32_t)tag & kPartTagMask) << kPartTagShift) | ((s_cnt >> 20) << 10) |
                               (((s_cnt >> 10) & 0x3FFu) << 5) | (s_cnt & 0x3FFu);
            part_dev[blockIdx.x] = w;
            __hip_atomic_store(part_host + blockIdx.x, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        return;
    }
    const int nb = (int)gridDim.x, b = (int)blockIdx.x;
    if (threadIdx.x == 0) {
        __hip_atomic_store(rctl + kR1Partial + b, s_cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int st = b & (kR1Stripes - 1);
        const uint32_t in_stripe = (uint32_t)((nb - st + kR1Stripes - 1) / kR1Stripes);
        const int stripes = nb < kR1Stripes ? nb : kR1Stripes;
        int last = 0;
        if (__hip_atomic_fetch_add(rctl + st, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == in_stripe - 1)
            last = __hip_atomic_fetch_add(rctl + 32, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
                   (uint32_t)(stripes - 1);
        s_last = last;
    }
    __syncthreads();
    if (!s_last) return;
    // the last block: every partial was published before its block's arrival (sc1 loads, no stale L1 copy)
    uint32_t c0 = 0u, c1 = 0u, c2 = 0u;
    for (int i = threadIdx.x; i < nb; i += kBlock) {
        const uint32_t v = __hip_atomic_load(rctl + kR1Partial + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        c0 += v & 0x3FFu;
        c1 += (v >> 10) & 0x3FFu;
        c2 += v >> 20;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        c0 += __shfl_xor(c0, off);
        c1 += __shfl_xor(c1, off);
        c2 += __shfl_xor(c2, off);
    }
    __shared__ uint32_t s_sum[3][kWavesPerBlock];
    if (lane == 0) {
        s_sum[0][threadIdx.x >> 6] = c0;
        s_sum[1][threadIdx.x >> 6] = c1;
        s_sum[2][threadIdx.x >> 6] = c2;
    }
    // the select's slowest tree (as k_scan folds it): the max over the stripes, one per lane of wave 1
    if (stats && threadIdx.x >= kWave && threadIdx.x < 2 * kWave)
        fold_select_max(stats, kKSelMax, kKSelTripMax, (int)threadIdx.x - kWave);
    __syncthreads();
    if (threadIdx.x == 0) {
        int n0 = 0, n1 = 0, n2 = 0;
        for (int w = 0; w < kWavesPerBlock; ++w) {
            n0 += (int)s_sum[0][w];
            n1 += (int)s_sum[1][w];
            n2 += (int)s_sum[2][w];
        }
        tr.count[0] = n0;
        tr.count[1] = n1;
        tr.count[2] = n2;
        for (int i = 0; i < kR1Stripes; ++i) rctl[i] = 0u;
        rctl[32] = 0u;
        if (host_count) {
            __hip_atomic_store(host_count + 0, n0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(host_count + 1, n1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(host_count + 2, n2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            host_stores_done();
            st_host(host_count + 3, tag);
        }
    }
}

// A one-dispatch round's staged evaluation applied by tree (flush before anything else reads the trees)
__global__ __launch_bounds__(kBlock) void k_apply_tree(Pool pool, Trees tr, EvalCache cache, const float *policy,
                                                       const float *value, unsigned long long *bytes_ctr) {
    __shared__ __attribute__((aligned(16))) float s_row[kWavesPerBlock][84];
    const int t = wave_index();
    if (t >= tr.n_trees) return;
    const int prev = __builtin_amdgcn_readfirstlane(tr.pending[t]);
    if (prev & 1)
        apply_wave(pool, tr, cache, policy, 81, value, 1, nullptr, 0, bytes_ctr, t, s_row[threadIdx.x >> 6], t,
                   prev >> 8);
}

}  // namespace uttt
