// engine/reroot.h — tree reuse: k_reroot builds a move's roots in place of k_begin. One wave per
// tree copies the subtree under the played move from the tree's pool (`from`) to the front of its other pool
// (`to`), in the canonical breadth-first order uttt_reroot.h's host mirror writes, bit for bit; the host then swaps
// the pools, and select, apply, scan and the move end go on as after k_begin. A part of engine.hip's one
// translation unit, included after every other header of engine/ so that their definitions keep their places.
//
// The copy is Cheney's: the destination pool is the queue. A copied record keeps its link into `from` until the
// scan reaches it; then its block is appended to the queue and its link re-based. The scan takes 64 records a
// step: their block sizes are prefix-summed over the wave, and the blocks are copied lane-parallel, entry e of the
// step's appended range by lane e mod 64, so a step is two dependent round trips however wide its nodes are (a
// node expanded by a flush of 8 copies has 648 children). No LDS, no atomics but the failure flag, no scratch.
#pragma once
#include "expand.h"
#include "layout.h"
#include "selfplay.h"
#include "wave.h"
#include "uttt_reroot.h"

namespace uttt {

static_assert(reroot::kNoAct == kNoAction, "uttt_reroot.h restates the node record's fields");

// Where the trees' played moves and new root states come from.
struct RerootSrc {
    const Slot *slot;          // self-play: the slots, their states already advanced by k_move_end (else null)
    const int32_t *live;       // self-play: the slots' live flags (SelfPlay::live)
    const int8_t *ply_action;  // self-play: [slot][kMaxPlies], the move made at each ply
    const int32_t *actions;    // a plain search (uttt_search_reroot): [tree], each a legal move of the tree's root
    int32_t fresh;             // 1: `from` holds no finished move of these games: every root is built fresh
};

// The wave's exclusive prefix of v, and its total.
__device__ __forceinline__ int wave_excl_sum(int v, int &total) {
    const int lane = lane_id();
    int incl = v;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const int u = __shfl_up(incl, o);
        if (lane >= o) incl += u;
    }
    total = __shfl(incl, kWave - 1);
    return incl - v;
}

// Lane l holds a block of `from` (first record sf, sz records; sz 0: none). The blocks are appended to D at
// `alloc`, one after another in lane order; my_first (optional): where this lane's block went. Returns the records
// appended (wave-uniform), or -1 without writing when they would pass the pool's end.
__device__ __forceinline__ int copy_blocks(const uint4 *__restrict__ S, uint4 *__restrict__ D, int cap, int sf, int sz,
                                           int alloc, int *my_first = nullptr) {
    const int lane = lane_id();
    int total;
    const int excl = wave_excl_sum(sz, total);
    const int incl = excl + sz;
    if (my_first) *my_first = alloc + excl;
    if (alloc + total > cap) return -1;
    const int delta = sf - excl;  // entry e of this lane's block is S[delta + e]
    constexpr int kU = 4;         // independent loads in flight per lane
    for (int e0 = 0; e0 < total; e0 += kU * kWave) {
        uint4 v[kU];
#pragma unroll
        for (int j = 0; j < kU; ++j) {
            const int e = e0 + j * kWave + lane;
            const int ec = min(e, total - 1);
            // the block holding entry ec: the first lane whose inclusive prefix is above it (every lane takes
            // part in the lane reads)
            int b = 0;
#pragma unroll
            for (int step = kWave / 2; step; step >>= 1)
                if (__shfl(incl, b + step - 1) <= ec) b += step;
            const int src = __shfl(delta, b) + ec;
            v[j] = S[min(max(src, 0), cap - 1)];  // (a lane past the range loads its last entry again: no branch)
        }
#pragma unroll
        for (int j = 0; j < kU; ++j) {
            const int e = e0 + j * kWave + lane;
            if (e < total) D[alloc + e] = v[j];
        }
    }
    return total;
}

__device__ __forceinline__ uint4 readlane4(uint4 v, int l) {
    return make_uint4((uint32_t)__builtin_amdgcn_readlane((int)v.x, l), (uint32_t)__builtin_amdgcn_readlane((int)v.y, l),
                      (uint32_t)__builtin_amdgcn_readlane((int)v.z, l), (uint32_t)__builtin_amdgcn_readlane((int)v.w, l));
}

// err and count[2]: as k_begin resets them, once per launch (count[3]: see below).
__global__ __launch_bounds__(kBlock) void k_reroot(Pool from, Pool to, Trees tr, RerootSrc src, unsigned long long *err) {
    const int lane = lane_id();
    const int t = wave_index();
    if (t == 0 && lane == 0) {
        if (err) *err = ~0ull;
        tr.count[2] = -1;
        // count[3], the search's failure flag, is zeroed by the host on the stream before this launch: a wave of
        // this kernel may raise it (the capacity guard), and a reset by wave 0 could come after that
    }
    if (t >= tr.n_trees) return;
    // the played move a (-1: none) and the new root's state s
    bool on = true;
    int a = -1;
    const uttt_state_t s0 = src.slot ? src.slot[t].state : tr.root[t];
    if (src.slot) {
        on = src.live[t] != 0;
        const int ply = src.slot[t].ply;
        if (on && ply > 0 && ply <= kMaxPlies && !src.fresh) a = src.ply_action[(size_t)t * kMaxPlies + ply - 1];
    } else {
        a = src.actions[t];
    }
    a = __builtin_amdgcn_readfirstlane(a);
    const uttt_state_t s = src.slot ? s0 : next_state(s0, a);
    const int cap = (int)from.cap;
    const uint4 *__restrict__ S = from.rec + (size_t)t * from.cap;
    uint4 *__restrict__ D = to.rec + (size_t)t * to.cap;
    // c: the old root's child with action a (the root's block is one record per move, ascending)
    uint4 c = make_uint4(0u, 0u, 0u, 0u);
    bool reuse = on && a >= 0 && a < 81;
    if (reuse) {
        const uint4 r0 = S[0];
        const int L0 = meta_L(r0.z), f0 = link_first(r0.w);
        const bool in0 = lane < L0, in1 = lane + kWave < L0;
        const uint4 x0 = S[min(f0 + lane, cap - 1)], x1 = S[min(f0 + kWave + lane, cap - 1)];
        const uint64_t m0 = __ballot(in0 && meta_action(x0.z) == a), m1 = __ballot(in1 && meta_action(x1.z) == a);
        if (m0) c = readlane4(x0, __builtin_ctzll(m0));
        else if (m1) c = readlane4(x1, __builtin_ctzll(m1));
        // a child that was never expanded, or a terminal one, has no subtree to keep
        reuse = (m0 || m1) && link_k(c.w) > 0 && meta_L(c.z) > 0;
    }
    if (!reuse) {
        init_root(to, tr, t, s, on, 0);
        return;
    }
    const int kc = link_k(c.w), Lp = meta_L(c.z), fc = link_first(c.w);
    const int carried = meta_n(c.z) - kc;  // the sum of c's children's visits
    bool ok = (int64_t)fc + (int64_t)kc * Lp <= (int64_t)cap;
    // level 1: lane r merges the kc duplicates of move rank r (and of rank 64 + r), as init_root lays lanes over
    // moves: N and k summed, W summed in copy order, P and the action of the first copy, L of an expanded copy
    uint4 m0, m1;  // the merged records, their link word holding k alone until the blocks' places are known
    int bsz0, bsz1;
    auto merge = [&](int r, uint4 &out, int &bsz) {
        uint32_t n = 0u, k = 0u, Lc = 0u, act = 0u, p = 0u;
        float w = 0.0f;
        if (ok && r < Lp) {
            for (int i = 0; i < kc; ++i) {
                const uint4 d = S[fc + i * Lp + r];
                if (i == 0) {
                    w = __uint_as_float(d.x);
                    p = d.y;
                    act = (uint32_t)meta_action(d.z);
                } else {
                    w = w + __uint_as_float(d.x);
                }
                n += (uint32_t)meta_n(d.z);
                k += (uint32_t)link_k(d.w);
                Lc = max(Lc, (uint32_t)meta_L(d.z));
            }
        }
        out = make_uint4(__float_as_uint(w), p, (n & 0xFFFFu) | make_meta(act, Lc), k);
        bsz = (int)(k * Lc);
    };
    merge(lane, m0, bsz0);
    merge(lane + kWave, m1, bsz1);
    int tot0, tot1;
    const int ex0 = wave_excl_sum(bsz0, tot0), ex1 = wave_excl_sum(bsz1, tot1);
    int alloc = 1 + Lp;
    ok = ok && alloc + tot0 + tot1 <= cap;
    if (ok) {
        if (lane < Lp) D[1 + lane] = make_uint4(m0.x, m0.y, m0.z, make_link(m0.w ? (uint32_t)(alloc + ex0) : 0u, m0.w));
        if (lane + kWave < Lp)
            D[1 + kWave + lane] = make_uint4(m1.x, m1.y, m1.z, make_link(m1.w ? (uint32_t)(alloc + tot0 + ex1) : 0u, m1.w));
        if (lane == 0) D[0] = make_uint4(c.x, 0u, (uint32_t)carried | make_meta(kNoAction, (uint32_t)Lp), make_link(1u, 1u));
        // level 2: the duplicates' child blocks, move by move and copy by copy (item j: move j / kc, copy j % kc)
        const int items = kc * Lp;
        for (int j0 = 0; j0 < items && ok; j0 += kWave) {
            const int j = j0 + lane;
            int sf = 0, sz = 0;
            if (j < items) {
                const int r = j / kc, i = j - r * kc;
                const uint4 d = S[fc + i * Lp + r];
                sf = link_first(d.w);
                sz = link_k(d.w) * meta_L(d.z);
            }
            const int got = copy_blocks(S, D, cap, sf, sz, alloc);
            ok = got >= 0;
            alloc += ok ? got : 0;
        }
        // the rest: 64 queued records a step; their blocks go to the queue's end and their links are re-based
        int q = 1 + Lp;
        while (ok && q < alloc) {
            wave_memory_fence();  // the records other lanes appended, before this lane reads them
            const int grp = min(kWave, alloc - q);
            uint4 rec = make_uint4(0u, 0u, 0u, 0u);
            if (lane < grp) rec = D[q + lane];
            const int sz = link_k(rec.w) * meta_L(rec.z);
            int nf;
            const int got = copy_blocks(S, D, cap, link_first(rec.w), sz, alloc, &nf);
            ok = got >= 0;
            if (ok && sz) reinterpret_cast<uint32_t *>(D + q + lane)[3] = make_link((uint32_t)nf, (uint32_t)link_k(rec.w));
            alloc += ok ? got : 0;
            q += grp;
        }
    }
    if (lane == 0) {
        tr.root[t] = s;
        TreeCtl ctl;
        ctl.sims_done = carried;
        ctl.node_count = ok ? alloc : 1;
        ctl.status = kLive | (ok ? 0 : kErrCapacity);  // unreachable for a search's tree: the guard
        ctl.pad = 0;
        tr.ctl[t] = ctl;
        if (!ok) flag_tree_error(tr);
    }
}

}  // namespace uttt
