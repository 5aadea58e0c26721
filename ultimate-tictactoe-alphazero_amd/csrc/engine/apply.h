// engine/apply.h — an evaluation applied to its pending leaf: stop_tree, apply_wave (one wave per leaf: the rows
// checked, the priors normalised per copy, k child blocks appended, k back-ups along the path, the evaluation
// cache fed) and k_apply.
//
// A part of engine.hip's one translation unit, like its siblings in engine/. The order of the definitions here,
// and of this header among the others, is load-bearing for the code object: engine.hip's include list is the
// order of definition.
#pragma once
#include "cache.h"
#include "expand.h"
#include "layout.h"
#include "wave.h"
#include "uttt_bits.h"

namespace uttt {

// ------------------------------------------------------------------ apply --
// One wave per pending leaf (uttt_mcts.cpp:138-167 for each of its k copies):
// legal priors, sequential f32 sum in action order, divide (uniform 1/|legal|
// if sum <= 0), append the child block, back up the value along the path.
// per_copy: row rowbase[slot] + j holds copy j's result; else row = slot.

// An apply that cannot go on: the tree's status gets the error bit (its ctl is stored as the wave holds it) and
// the search's failure flag is raised; the host reports it at the move / search end
__device__ __forceinline__ void stop_tree(const Trees &tr, int t, TreeCtl &ctl, int32_t err_bit) {
    if (lane_id() != 0) return;
    ctl.status |= err_bit;
    tr.ctl[t] = ctl;
    flag_tree_error(tr);
}

__device__ __forceinline__ void apply_wave(Pool pool, Trees tr, EvalCache cache, const float *__restrict__ policy,
                                           int64_t pld, const float *__restrict__ value, int64_t vld,
                                           const int32_t *__restrict__ rowbase, int per_copy,
                                           unsigned long long *bytes_ctr, int slot, float *row /* LDS, 84 floats */,
                                           int by_tree = -1, int by_tree_depth = 0, float *copy_rows = nullptr,
                                           bool host_rows = false, CachePublish *defer = nullptr) {
    // copy_rows (LDS, 8 x 84 floats, 16-B aligned; optional): the per-copy prior sums of a chunk run in 8 lanes
    // at once instead of one copy after another. host_rows: the evaluation rows sit in fine-grained host
    // memory the host wrote behind a polled command; they are read with system-coherent (sc0 sc1) loads,
    // so no cache invalidation stands between the command and them (k_search1: one leaf, its rows from row 0,
    // at least 8 rows readable)
    auto ld_row = [host_rows](const float *a) -> float {
        return host_rows ? __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : *a;
    };
    const int lane = lane_id();
    // two dependent round trips before the work: the count with this slot's tree and leaf depth
    // (tree_of / depth_of hold n_trees entries, stale past the count), then the tree's records, the
    // path entries 0..depth (round 4: all 128 were loaded, 2.5 KB a leaf) and the slot's evaluation.
    // by_tree >= 0 (one-dispatch hash rounds, k_round1): the tree and its leaf's depth are given and its
    // evaluation is row `slot` == by_tree (rows by tree, no scan)
    int t, dq;
    if (by_tree >= 0) {
        t = by_tree;
        dq = by_tree_depth;
    } else {
        const int cnt = tr.count[0];
        t = tr.tree_of[slot < tr.n_trees ? slot : 0];
        dq = tr.depth_of[slot < tr.n_trees ? slot : 0];
        if (slot >= cnt) return;
    }
    // host_rows, per copy: the first 8 rows (the host block holds at least 16) are loaded before the tree's
    // records, whose round trip they then share; masked by legality and by k once those have arrived
    constexpr int kCopyChunk = 8;
    float h0[kCopyChunk], h1[kCopyChunk], hv[kCopyChunk];
    if (host_rows && per_copy) {
#pragma unroll
        for (int jj = 0; jj < kCopyChunk; ++jj) {
            const float *pol = policy + (int64_t)jj * pld;
            h0[jj] = ld_row(pol + lane);
            h1[jj] = ld_row(pol + 64 + (lane < 17 ? lane : 16));
            hv[jj] = ld_row(value + (int64_t)jj * vld);
        }
    }
    const LeafRec r = tr.rec[t];
    TreeCtl ctl = tr.ctl[t];
    const uttt_state_t s = tr.leaf[t];
    const size_t base = (size_t)t * pool.cap;
    const int32_t *gp = tr.path + (size_t)t * kMaxDepth;
    const uint4 *gr = tr.path_rec + (size_t)t * kMaxDepth;
    int g_lo = 0, g_hi = 0;
    uint4 pr_lo = {0u, 0u, 0u, 0u}, pr_hi = {0u, 0u, 0u, 0u};  // the path nodes' records as the select read them
    if (lane <= dq) {
        g_lo = gp[lane];
        pr_lo = gr[lane];
    }
    if (lane + 64 <= dq) {
        g_hi = gp[lane + 64];
        pr_hi = gr[lane + 64];
    }
    float raw0 = 0.0f, raw1 = 0.0f, rawv = 0.0f;
    if (!per_copy) {
        const float *pol = policy + (int64_t)slot * pld;
        raw0 = ld_row(pol + lane);
        raw1 = ld_row(pol + 64 + (lane < 17 ? lane : 16));
        rawv = ld_row(value + (int64_t)slot * vld);
    }
    const int depth = r.depth;
    const int k = r.k;
    const int pn_lo = lane <= depth ? g_lo : 0;
    const int pn_hi = lane + 64 <= depth ? g_hi : 0;
    int L = 0;
    bool inserted = false;
    const int nodes_before = ctl.node_count;
    if (!per_copy) {
        const float v = rawv;
        // SURVEY §5 failure detection: a NaN / Inf legal prior or value (uttt_mcts.cpp:144-166 would
        // expand and back it up silently) stops the tree with kErrNonFinite, which the host raises at
        // the move boundary (UTTT_ERR_NONFINITE); nothing of it is expanded or cached. A non-finite
        // entry of an illegal action is never read by the search (it is expanded as the reference
        // would), but such a row is not cached either: the table only ever holds finite rows.
        const bool fin0 = __builtin_isfinite(raw0), fin1 = __builtin_isfinite(raw1);
        {
            uint32_t m[3];
            legal_mask(s, m);
            const bool bad = (bit_of(m, lane) && !fin0) || (lane < 17 && bit_of(m, 64 + lane) && !fin1) ||
                             !__builtin_isfinite(v);
            if (__ballot(bad)) {
                stop_tree(tr, t, ctl, kErrNonFinite);
                return;
            }
        }
        const bool cacheable = __ballot(!fin0 || (lane < 17 && !fin1)) == 0ull;
        // the insert's flag loads go out before the expansion's work, which runs under their round trip
        const CacheProbe ipr = cache_probe_issue(cache, s);
        float psum = 0.0f;
        if (!expand_backup(pool, base, r.node, depth, pn_lo, pn_hi, pr_lo, pr_hi, k, s, raw0, lane < 17 ? raw1 : 0.0f,
                           v, ctl.node_count, tr.py != 0, row, false, 0.0f, &psum)) {
            stop_tree(tr, t, ctl, kErrCapacity);
            return;
        }
        inserted = cacheable && cache_insert(cache, ipr, s, raw0, raw1, v, tr.py == 0, psum, defer);
        L = (ctl.node_count - nodes_before) / k;
    } else {
        // the reference's exact call pattern: k results, one per queued copy, applied in order
        const Legal g = legal_of(s);
        const bool l0 = g.l0, l1 = g.l1;
        const uint64_t b0 = g.b0, b1 = g.b1;
        const int i0 = g.i0, i1 = g.i1;
        L = g.L;
        const int nb = ctl.node_count;
        if ((int64_t)nb + (int64_t)k * L > pool.cap || L == 0) {
            stop_tree(tr, t, ctl, kErrCapacity);
            return;
        }
        // the copies' rows in chunks of kCopyChunk whose loads are all issued before the first use: one
        // memory round trip per chunk instead of one per copy (the rows of a one-tree search sit in host
        // memory, a PCIe round trip each: round 6 measured 16 us of a flush's apply on 8 sequential rows)
        const int64_t rb = rowbase[slot];
        float c0[kCopyChunk], c1[kCopyChunk], cv[kCopyChunk];
        auto load_chunk = [&](int j0) {
            if (host_rows && j0 == 0) {  // the prefetched rows (row base 0)
#pragma unroll
                for (int jj = 0; jj < kCopyChunk; ++jj) {
                    const int q = jj < k ? jj : 0;
                    float x0 = h0[0], x1 = h1[0], xv = hv[0];
#pragma unroll
                    for (int i = 1; i < kCopyChunk; ++i) {
                        x0 = q == i ? h0[i] : x0;
                        x1 = q == i ? h1[i] : x1;
                        xv = q == i ? hv[i] : xv;
                    }
                    c0[jj] = l0 ? x0 : 0.0f;
                    c1[jj] = l1 ? x1 : 0.0f;
                    cv[jj] = xv;
                }
                return;
            }
#pragma unroll
            for (int jj = 0; jj < kCopyChunk; ++jj) {
                const int64_t row = rb + (j0 + jj < k ? j0 + jj : j0);
                const float *pol = policy + row * pld;
                c0[jj] = l0 ? ld_row(pol + lane) : 0.0f;
                c1[jj] = l1 ? ld_row(pol + 64 + lane) : 0.0f;
                cv[jj] = ld_row(value + row * vld);
            }
        };
        // copy_rows: lane jj's sum of the chunk's copy jj, its legal priors compacted in action order into an
        // LDS row (seq_sum_legal's order and zero padding, so the same f32 sum as the one-lane loop below)
        float csum = 0.0f;
        auto chunk_sums = [&]() {
#pragma unroll
            for (int jj = 0; jj < kCopyChunk; ++jj) store_ranked_row(copy_rows + jj * 84, c0[jj], c1[jj], g);
            csum = sum_row4(copy_rows + (lane & (kCopyChunk - 1)) * 84, L);
        };
        bool bad = false;  // any copy's legal prior or value non-finite: nothing is applied (as above)
        for (int j0 = 0; j0 < k; j0 += kCopyChunk) {
            load_chunk(j0);
#pragma unroll
            for (int jj = 0; jj < kCopyChunk; ++jj)
                bad |= !__builtin_isfinite(c0[jj]) || !__builtin_isfinite(c1[jj]) || !__builtin_isfinite(cv[jj]);
        }
        if (__ballot(bad)) {
            stop_tree(tr, t, ctl, kErrNonFinite);
            return;
        }
        uint4 r_lo = pr_lo, r_hi = pr_hi;
        float w_lo = __uint_as_float(r_lo.x), w_hi = __uint_as_float(r_hi.x);
        for (int j = 0; j < k; ++j) {
            const int jj = j & (kCopyChunk - 1);
            if (jj == 0 && k > kCopyChunk) load_chunk(j);  // k <= kCopyChunk: the check's chunk is still held
            if (jj == 0 && copy_rows) chunk_sums();
            float p0 = c0[0], p1 = c1[0], v = cv[0];
#pragma unroll
            for (int i = 1; i < kCopyChunk; ++i) {
                p0 = jj == i ? c0[i] : p0;
                p1 = jj == i ? c1[i] : p1;
                v = jj == i ? cv[i] : v;
            }
            float sum = 0.0f;
            if (copy_rows) {
                sum = readlane_f(csum, jj);
            } else {
                for (uint64_t bits = b0; bits; bits &= bits - 1ull) sum += readlane_f(p0, __builtin_ctzll(bits));
                for (uint64_t bits = b1; bits; bits &= bits - 1ull) sum += readlane_f(p1, __builtin_ctzll(bits));
            }
            const float un = 1.0f / (float)L;
            const float q0 = sum > 0 ? p0 / sum : un;
            const float q1 = sum > 0 ? p1 / sum : un;
            const size_t blk = base + nb + (size_t)j * L;
            if (l0) pool.rec[blk + i0] = new_child(q0, (uint32_t)lane);
            if (l1) pool.rec[blk + i1] = new_child(q1, (uint32_t)(64 + lane));
            if (lane <= depth) w_lo += ((depth - lane) & 1) ? -v : v;
            if (lane + 64 <= depth) w_hi += ((depth - lane - 64) & 1) ? -v : v;
        }
        // path nodes: w, N += k; the leaf (depth) also gets L and its link (first child, k blocks)
        auto put = [&](uint4 rr, float w, int pn, int d) {
            rr.x = __float_as_uint(w);
            rr.z += (uint32_t)k;
            if (d == depth) {
                rr.z = (rr.z & ~kMetaLMask) | ((uint32_t)L << 23);
                rr.w = make_link((uint32_t)nb, (uint32_t)k);
            }
            pool.rec[base + pn] = rr;
        };
        if (lane <= depth) put(r_lo, w_lo, pn_lo, lane);
        if (lane + 64 <= depth) put(r_hi, w_hi, pn_hi, lane + 64);
        ctl.node_count = nb + k * L;
    }
    if (lane == 0) {
        ctl.sims_done += k;
        tr.ctl[t] = ctl;
        if (bytes_ctr) {
            // algorithmic bytes of one leaf: the slot's tree, depth and count (12), its LeafRec, TreeCtl and
            // state (64), the path's indices and records (20 per level), the evaluation (328 per copy);
            // written: the k child blocks (16 per child), the path's records (16 per level), the TreeCtl
            // (16); with the evaluation cache: the probe's 8 flags (32) and a new record (368 + 4)
            const int copies = per_copy ? k : 1;
            const unsigned long long b = 12ull + 64ull + 36ull * (unsigned long long)(depth + 1) + 328ull * copies +
                                         16ull * (unsigned long long)(k * L) + 16ull + (cache.flag ? 32ull : 0ull) +
                                         (inserted ? 372ull : 0ull);
            atomicAdd(stripe_of(bytes_ctr), b);
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_apply(Pool pool, Trees tr, EvalCache cache, const float *__restrict__ policy,
                                                  int64_t pld, const float *__restrict__ value, int64_t vld,
                                                  const int32_t *__restrict__ rowbase, int per_copy,
                                                  unsigned long long *bytes_ctr) {
    __shared__ __attribute__((aligned(16))) float s_row[kWavesPerBlock][84];  // the prior sum's row, per wave
    apply_wave(pool, tr, cache, policy, pld, value, vld, rowbase, per_copy, bytes_ctr, wave_index(),
               s_row[threadIdx.x >> 6]);
}

}  // namespace uttt
