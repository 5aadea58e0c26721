// engine/expand.h — a leaf's legal moves over the wave, the f32 prior sums in the reference's order, expand_backup
// (k child blocks appended, k back-ups along the path), and the root: init_root and k_begin.
#pragma once
#include "layout.h"
#include "wave.h"

namespace uttt {

// ---------------------------------------------------------- expand + backup --
// uttt_mcts.cpp:138-167 for k identical copies of one flushed leaf: priors =
// pol[a] for legal a, sequential f32 sum in action order, divide (uniform
// 1/|legal| if the sum is <= 0); append k child blocks (expand never clears,
// :38-43); back up v k times along path[0..depth] (:47-54, leaf first, sign
// flipping upward). Lane d holds path[d] in path_lo and path[64+d] in path_hi.
// Returns false without writing when the node pool would overflow.
// py (pv_mcts.py:46-56, :104-116): priors normalised by np.sum (float32 pairwise),
// all-zero -> float64 uniform (kMetaP64); ONE child block (expand replaces, and
// the k copies of a flush expand the same children); every node on the path
// gets a network value, so its w becomes float32 (kMetaWF32).

// A state's legal moves compacted over the wave: lane l holds action l (l0) and action 64 + l (l1, l < 17);
// b0 / b1 their ballots, L = |legal|, i0 / i1 this lane's actions' ranks in action order. on == false
// (k_begin's dead slots): no move counts as legal.
struct Legal {
    bool l0, l1;
    uint64_t b0, b1;
    int L, i0, i1;
};
__device__ __forceinline__ Legal legal_of(const uttt_state_t &s, bool on = true) {
    const int lane = lane_id();
    uint32_t m[3];
    legal_mask(s, m);
    Legal g;
    g.l0 = on && bit_of(m, lane) != 0u;
    g.l1 = on && lane < 17 && bit_of(m, 64 + lane) != 0u;
    g.b0 = __ballot(g.l0);
    g.b1 = __ballot(g.l1);
    g.L = __popcll(g.b0) + __popcll(g.b1);
    g.i0 = __popcll(g.b0 & lanes_below());
    g.i1 = __popcll(g.b0) + __popcll(g.b1 & lanes_below());
    return g;
}

__device__ float np_sum_f32_legal(float p0, float p1, uint64_t b0, uint64_t b1, int L) {
    // numpy pairwise_sum for float32, n <= 128: 8 strided accumulators, then the tail
    auto nth = [&](int idx) -> float {  // idx-th legal prior in action order (wave-uniform)
        const int c0 = __popcll(b0);
        uint64_t bits = idx < c0 ? b0 : b1;
        int r = idx < c0 ? idx : idx - c0;
        for (; r > 0; --r) bits &= bits - 1ull;
        const int l = __builtin_ctzll(bits);
        return idx < c0 ? readlane_f(p0, l) : readlane_f(p1, l);
    };
    if (L < 8) {
        float res = 0.0f;
        for (int i = 0; i < L; ++i) res += nth(i);
        return res;
    }
    float r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = nth(j);
    const int main_end = L - L % 8;
    for (int i = 8; i < main_end; i += 8)
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] += nth(i + j);
    float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (int i = main_end; i < L; ++i) res += nth(i);
    return res;
}

// raw0 / raw1: this lane's prior of action lane / 64 + lane (lane < 17), loaded by the caller
// The sequential f32 sum of the legal priors in action order (uttt_mcts.cpp:150-153): each legal
// prior is stored at its rank in the wave's LDS row (zeros pad the row to a multiple of 4; adding
// +0.0 to a sum that started at +0.0 changes nothing), then every lane reads the row back by
// broadcast 16-byte reads and adds it up in order: one dependent add per prior, instead of a scalar
// find-first-bit, a v_readlane and an add per prior.
__device__ __forceinline__ void store_ranked_row(float *row /* LDS, 16-B aligned, >= 84 floats */, float p0, float p1,
                                                 const Legal &g) {
    const int lane = lane_id();
    if (g.l0) row[g.i0] = p0;
    if (g.l1) row[g.i1] = p1;
    // lanes 0 .. L4 - L - 1 (at most three) pad ranks L .. L4 - 1 (<= 83): by offset from L, so that a row of
    // more than 64 legal moves is padded too (a lane index never reaches such a rank, and the row then kept
    // what an earlier, wider leaf or another user of the LDS left there)
    if (lane < ((g.L + 3) & ~3) - g.L) row[g.L + lane] = 0.0f;
}
__device__ __forceinline__ float sum_row4(const float *row, int L) {
    // the other lanes' stores before any lane's reads (LDS executes a wave's accesses in order; the
    // wait and the clobber keep the compiler from hoisting the reads above the stores)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    float sum = 0.0f;
    const float4 *r4 = reinterpret_cast<const float4 *>(row);
    for (int i = 0; i < ((L + 3) & ~3) / 4; ++i) {
        const float4 q = r4[i];
        sum += q.x;
        sum += q.y;
        sum += q.z;
        sum += q.w;
    }
    return sum;
}
__device__ __forceinline__ float seq_sum_legal(float *row, float p0, float p1, const Legal &g) {
    store_ranked_row(row, p0, p1, g);
    return sum_row4(row, g.L);
}

// rec_lo / rec_hi: this lane's path node's record (path[lane] / path[64 + lane]) as the select read it
__device__ bool expand_backup(const Pool &pool, size_t base, int node, int depth, int path_lo, int path_hi,
                              uint4 rec_lo, uint4 rec_hi, int k, const uttt_state_t &s, float raw0, float raw1, float v,
                              int &node_count, bool py = false, float *row = nullptr, bool has_sum = false,
                              float known_sum = 0.0f, float *sum_out = nullptr, uint4 *root_out = nullptr) {
    const int lane = lane_id();
    const Legal g = legal_of(s);
    const bool l0 = g.l0, l1 = g.l1;
    const uint64_t b0 = g.b0, b1 = g.b1;
    const int L = g.L, i0 = g.i0, i1 = g.i1;
    const int nb = node_count;
    const int blocks = py ? 1 : k;
    if ((int64_t)nb + (int64_t)blocks * L > pool.cap || L == 0) return false;
    const float p0 = l0 ? raw0 : 0.0f;
    const float p1 = l1 ? raw1 : 0.0f;
    float sum = 0.0f;
    if (py) {
        sum = np_sum_f32_legal(p0, p1, b0, b1, L);
    } else if (has_sum) {
        sum = known_sum;  // the cache record's (the same values added in the same order at insert)
    } else if (row) {
        sum = seq_sum_legal(row, p0, p1, g);
    } else {
        for (uint64_t bits = b0; bits; bits &= bits - 1ull) sum += readlane_f(p0, __builtin_ctzll(bits));
        for (uint64_t bits = b1; bits; bits &= bits - 1ull) sum += readlane_f(p1, __builtin_ctzll(bits));
    }
    if (sum_out) *sum_out = sum;
    const float un = 1.0f / (float)L;
    const bool p64 = py && !(sum > 0);  // np.ones(float) / L: float64 priors
    const float q0 = sum > 0 ? p0 / sum : un;
    const float q1 = sum > 0 ? p1 / sum : un;
    const uint4 c0 = new_child(q0, (uint32_t)lane), c1 = new_child(q1, (uint32_t)(64 + lane));
    for (int j = 0; j < blocks; ++j) {
        const size_t blk = base + nb + (size_t)j * L;
        if (l0) pool.rec[blk + i0] = c0;
        if (l1) pool.rec[blk + i1] = c1;
    }
    // the path, leaf (lane depth) to root: w += v k times with the sign flipping upwards, N += k; the
    // leaf also gets its children's block size L and its link (first child, k copies: cpp k blocks,
    // py one block); py: every node on the path now holds a float32 w (kMetaWF32), and the leaf's
    // children carry float64 priors when the policy summed to zero (kMetaP64)
    const uint32_t leaf_meta = (uint32_t)L << 23 | (py ? (kMetaWF32 | (p64 ? kMetaP64 : 0u)) : 0u);
    const uint32_t leaf_link = make_link((uint32_t)nb, (uint32_t)k);
    auto update = [&](uint4 r, int pn, int d) -> uint4 {  // path node pn at depth d, its record r
        float w = __uint_as_float(r.x);
        const float x = ((depth - d) & 1) ? -v : v;
        for (int j = 0; j < k; ++j) w += x;
        r.x = __float_as_uint(w);
        r.z += (uint32_t)k;
        if (py && d < depth) r.z |= kMetaWF32;
        if (d == depth) {
            r.z = (r.z & ~kMetaLMask) | leaf_meta;
            r.w = leaf_link;
        }
        pool.rec[base + pn] = r;
        return r;
    };
    uint4 new_lo = rec_lo;
    if (lane <= depth) new_lo = update(rec_lo, path_lo, lane);
    if (lane + 64 <= depth) update(rec_hi, path_hi, lane + 64);
    if (root_out)  // the root's record as just written (lane 0 holds path[0])
        *root_out = make_uint4((uint32_t)__builtin_amdgcn_readlane((int)new_lo.x, 0),
                               (uint32_t)__builtin_amdgcn_readlane((int)new_lo.y, 0),
                               (uint32_t)__builtin_amdgcn_readlane((int)new_lo.z, 0),
                               (uint32_t)__builtin_amdgcn_readlane((int)new_lo.w, 0));
    node_count = nb + blocks * L;
    return true;
}

// ----------------------------------------------------------- root (begin) --
// uttt_mcts.cpp:92-103: root expanded at once with uniform priors 1.0f/|legal|.
// Self-play passes `live` (slot flags) and the slots' states in place (src_stride = sizeof(Slot)),
// and err: the asynchronous move end's failure word, reset here (once per move, before this move's end,
// after the previous move end's read of it) instead of by a memset on the stream, as is the search's
// failure flag (Trees::count[3]);
// search passes nullptr (all live) and packed states.

// Tree t's root record, its uniform child block and its TreeCtl from the root state s (k_begin; k_search1 for
// tree 0). py (pv_mcts.py:134): the root is a plain unexpanded node, evaluated by the first flush. on == false
// (a self-play slot without a game): a root without children that is not live.
__device__ __forceinline__ void init_root(const Pool &pool, const Trees &tr, int t, const uttt_state_t &s, bool on, int py) {
    const int lane = lane_id();
    const size_t base = (size_t)t * pool.cap;
    const Legal g = legal_of(s, on || py);
    const int L = py ? 0 : g.L;  // the child block's size
    const float up = L ? 1.0f / (float)L : 0.0f;
    if (!py && g.l0) pool.rec[base + 1 + g.i0] = new_child(up, (uint32_t)lane);
    if (!py && g.l1) pool.rec[base + 1 + g.i1] = new_child(up, (uint32_t)(64 + lane));
    if (lane == 0) {
        pool.rec[base] = make_uint4(0u, 0u, make_meta(kNoAction, (uint32_t)L), make_link(L ? 1u : 0u, L ? 1u : 0u));
        tr.root[t] = s;
        TreeCtl c;
        c.sims_done = 0;
        c.node_count = 1 + L;
        c.status = (on && g.L > 0) ? kLive : 0;
        c.pad = 0;
        tr.ctl[t] = c;
    }
}

__global__ __launch_bounds__(kBlock) void k_begin(Pool pool, Trees tr, const char *src, int src_stride, const int32_t *live,
                                                  unsigned long long *err) {
    const int lane = lane_id();
    const int t = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (t == 0 && lane == 0) {
        if (err) *err = ~0ull;
        tr.count[2] = -1;  // a search starts: no round of it is known to be empty yet (k_round1's fast exit)
        tr.count[3] = 0;   // and no tree of it has failed
    }
    if (t >= tr.n_trees) return;
    const bool on = live ? (live[t] != 0) : true;
    const uttt_state_t s = *reinterpret_cast<const uttt_state_t *>(src + (size_t)t * src_stride);
    init_root(pool, tr, t, s, on, tr.py);
}

}  // namespace uttt
