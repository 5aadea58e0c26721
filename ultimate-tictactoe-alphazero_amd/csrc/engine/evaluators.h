// engine/evaluators.h — the device evaluators and the root's results: k_hash_eval and k_hash_leaves (the
// deterministic test evaluator), root_children / visits_of / root_scores, the random-playout kernels
// (uttt_playout.h), LdsStack and the two exact-solver kernels (uttt_solve.h), k_root_visits and k_root_scores.
//
// A part of engine.hip's one translation unit, like its siblings in engine/. The order of the definitions here,
// and of this header among the others, is load-bearing for the code object: engine.hip's include list is the
// order of definition, and the root-result helpers stand between the evaluators as they always did.
#pragma once
#include <cmath>

#include "layout.h"
#include "rounds.h"
#include "wave.h"
#include "uttt_bits.h"
#include "uttt_engine.h"
#include "uttt_playout.h"
#include "uttt_solve.h"

namespace uttt {

// -------------------------------------------------------------- hash eval --
// Deterministic test evaluator on the NCHW rows: one wave per row; the 4
// ballots of "x != 0" over the 243 floats are exactly the 4 hash words.
__global__ __launch_bounds__(kBlock) void k_hash_eval(const float *__restrict__ x, int n, float *__restrict__ policy,
                                                      float *__restrict__ value) {
    const int lane = lane_id();
    const int row = wave_index();
    if (row >= n) return;
    const float *xr = x + (size_t)row * 243;
    uint64_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = i * 64 + lane;
        w[i] = __ballot(j < 243 && xr[j] != 0.0f);
    }
    const uint64_t h = hash_words(w);
    policy[(size_t)row * 81 + lane] = hash_prior(h, lane);
    if (lane < 17) policy[(size_t)row * 81 + 64 + lane] = hash_prior(h, 64 + lane);
    if (lane == 0) value[row] = hash_value(h);
}

// ---------------------------------------------------------- root results --
__device__ __forceinline__ int root_children(const Pool &pool, size_t base, int &first) {
    const uint4 r = pool.rec[base];
    first = link_first(r.w);
    return meta_L(r.z);
}
__device__ __forceinline__ int visits_of(const Pool &pool, size_t i) { return meta_n(pool.rec[i].z); }

// pv_mcts_scores' return value (uttt_mcts.cpp:177-195): root child visits as
// f32 -> one-hot first max (t == 0) or boltzman (:199-216).
__device__ void root_scores(const Pool &pool, size_t base, float temperature, float *sc, int &L) {
    int first;
    L = root_children(pool, base, first);
    if (temperature == 0.0f) {
        int mi = 0;
        float mv = L ? (float)visits_of(pool, base + first) : 0.0f;
        for (int i = 1; i < L; ++i) {
            const float v = (float)visits_of(pool, base + first + i);
            if (v > mv) {
                mv = v;
                mi = i;
            }
        }
        for (int i = 0; i < L; ++i) sc[i] = (i == mi) ? 1.0f : 0.0f;
    } else {
        // glibc's powf (what the reference's std::pow(float, float) calls) evaluates in
        // double and rounds once; ocml's f32 powf is not correctly rounded (pow(19, 1)
        // came out 1 ulp low), so do the same: double pow of the f32 operands, one rounding.
        const double y = (double)(1.0f / temperature);
        float sum = 0.0f;
        for (int i = 0; i < L; ++i) {
            sc[i] = (float)pow((double)visits_of(pool, base + first + i), y);
            sum += sc[i];
        }
        if (sum > 0)
            for (int i = 0; i < L; ++i) sc[i] /= sum;
    }
}

// The same evaluator on this round's pending leaves straight from their states (the device-count
// rounds: no NCHW input is written): bit j = ch * 81 + R * 9 + C of the network input, as k_encode
// writes it, so the words and outputs are k_hash_eval's. One wave per slot; the count is read on the
// device (the grid covers every tree).
__global__ __launch_bounds__(kBlock) void k_hash_leaves(Trees tr, float *__restrict__ policy,
                                                        float *__restrict__ value) {
    const int row = wave_index();
    if (row >= tr.count[0]) return;
    const uttt_state_t s = tr.leaf[tr.tree_of[row]];
    hash_leaf_row(s, policy, value, row);
}

// ---------------------------------------------------------------- playouts --
// Random-playout evaluator (uttt_playout.h; game.py:277-287 `playout`, the evaluation of game.py:294-379's
// mcts_action): one wave per position, lane = playout, ceil(P / 64) passes. The position is wave-uniform; each
// lane plays its own game on a private copy of the 32-byte state in registers until it ends (at most 81 plies;
// the wave leaves the loop with its last lane), and a pass's wins and losses are two ballots' popcounts.
// No LDS, no atomics, no scratch.
__device__ __forceinline__ void playout_wave(const uttt_state_t &s, int P, uint64_t seed, int32_t &wins, int32_t &losses) {
    const int lane = lane_id();
    uint32_t m[3];
    legal_mask(s, m);
    uint64_t w[4];
    input_words(s, m, w);
    const uint64_t h = playout_key(w, seed);
    wins = losses = 0;
    for (int base = 0; base < P; base += kWave) {
        const int j = base + lane;
        int r = 0;
        if (j < P) r = playout(s, h, (uint32_t)j);
        wins += (int32_t)__popcll(__ballot(r > 0));
        losses += (int32_t)__popcll(__ballot(r < 0));
    }
}

// The round's evaluator, shaped like k_hash_leaves (one wave per slot, the count read on the device): the
// value is the mean playout result; the priors are 81 x 1, which k_apply's legal mask and sequential
// renormalisation turn into exactly 1 / |legal|.
__global__ __launch_bounds__(kBlock) void k_playout_leaves(Trees tr, int P, uint64_t seed, float *__restrict__ policy,
                                                           float *__restrict__ value) {
    const int row = wave_index();
    if (row >= tr.count[0]) return;
    const int lane = lane_id();
    const uttt_state_t s = tr.leaf[tr.tree_of[row]];
    int32_t wins, losses;
    playout_wave(s, P, seed, wins, losses);
    policy[(size_t)row * 81 + lane] = 1.0f;
    if (lane < 17) policy[(size_t)row * 81 + 64 + lane] = 1.0f;
    if (lane == 0) value[row] = playout_value(wins - losses, P);
}

// Flat Monte-Carlo on arbitrary positions, terminal ones included (a lost position: every playout a loss;
// a drawn one: neither): wins and losses of the side to move over P playouts, one wave per position.
__global__ __launch_bounds__(kBlock) void k_playout_states(const uttt_state_t *__restrict__ states, int n, int P,
                                                           uint64_t seed, int32_t *__restrict__ wins,
                                                           int32_t *__restrict__ losses) {
    const int row = wave_index();
    if (row >= n) return;
    const uttt_state_t s = states[row];
    int32_t nw, nl;
    playout_wave(s, P, seed, nw, nl);
    if (lane_id() == 0) {
        wins[row] = nw;
        losses[row] = nl;
    }
}

// ------------------------------------------------------------------ solver --
// Exact endgame values (uttt_solve.h; game.py:240-274 `alpha_beta` / `alpha_beta_action`): one wave per
// position, lane i searches the child of the i-th legal action. The position is wave-uniform; each lane keeps
// the node it is at in registers and its frames in LDS, frame d of lane l at word d * 64 + l of the wave's
// block: whatever depths the lanes are at, lane l reads and writes bank l % 64 only, so no step has a bank
// conflict (lane-contiguous stacks of 32 words put every second lane at one depth on one bank). One trip of the loop is
// one step of the machine for every live lane; the wave leaves with its last lane. No atomics, no scratch;
// each wave writes its own position's outputs only.
struct LdsStack {
    uint32_t *base;  // this lane's frame 0
    __device__ __forceinline__ uint32_t load(int d) const { return base[d * kWave]; }
    __device__ __forceinline__ void store(int d, uint32_t x) { base[d * kWave] = x; }
};
static_assert(sizeof(uint32_t) * kWavesPerBlock * kSolveMaxEmpty * kWave <= 65536,
              "k_solve_states, k_solve_leaves: LDS per workgroup");

__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// Legal actions below action j: the lane that searched j, when j is legal.
__device__ __forceinline__ int legal_rank(const uint32_t m[3], int j) {
    int r = 0;
#pragma unroll
    for (int w = 0; w < 3; ++w) {
        const int k = j - 27 * w;
        r += (int)popc32(k <= 0 ? 0u : (k >= 27 ? m[w] : m[w] & ((1u << k) - 1u)));
    }
    return r;
}

// The machine both solver kernels run on a searched position (solve_root said so): lane i < L searches the
// child of the i-th legal move on this wave's block of `frames`. av: this lane's action value
// (UTTT_SOLVE_UNKNOWN for a lane without a move or out of budget); total: the nodes of all lanes; best / every:
// solve_result's arguments. All but av are wave-uniform.
__device__ __forceinline__ void solve_wave(const uttt_state_t &s, const uint32_t m[3], int32_t max_nodes,
                                           uint32_t *frames, int &av, int &total, int &best, bool &every) {
    const int lane = lane_id();
    const int L = (int)(popc32(m[0]) + popc32(m[1]) + popc32(m[2]));  // <= empties(s) <= 64
    const bool mine = lane < L;
    SolveLane ln;
    solve_lane_begin(ln, next_state(s, mine ? nth_legal(m, (uint32_t)lane) : 0));
    ln.live = mine;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    LdsStack stack{frames + wave * (kSolveMaxEmpty * kWave) + lane};
    while (__ballot(ln.live != 0) != 0ull) {
        if (ln.live) solve_step(ln, stack, max_nodes);
    }
    const bool known = mine && ln.solved;
    av = known ? -ln.v : UTTT_SOLVE_UNKNOWN;
    total = wave_sum_i(mine ? ln.nodes : 0);  // <= 64 * 2^22
    best = wave_max_i(known ? av : -2);
    every = __ballot(mine && !ln.solved) == 0ull;
}

// The values of actions `lane` and 64 + lane (the latter for lane < 17) from the lanes that searched them:
// action j's value sits in lane legal_rank(j). Meaningful for legal actions only.
__device__ __forceinline__ void action_values_of(const uint32_t m[3], int av, int &v0, int &v1) {
    const int lane = lane_id(), j1 = 64 + lane;
    v0 = __shfl(av, legal_rank(m, lane) & (kWave - 1));
    v1 = __shfl(av, legal_rank(m, j1 < 81 ? j1 : 80) & (kWave - 1));
}

__global__ __launch_bounds__(kBlock) void k_solve_states(const uttt_state_t *__restrict__ states, int n,
                                                         int32_t max_nodes, int8_t *__restrict__ value,
                                                         int8_t *__restrict__ action, int8_t *__restrict__ status,
                                                         int64_t *__restrict__ nodes,
                                                         int8_t *__restrict__ action_values) {
    __shared__ uint32_t frames[kWavesPerBlock * kSolveMaxEmpty * kWave];
    const int row = wave_index();
    if (row >= n) return;
    const int lane = lane_id();
    const uttt_state_t s = states[row];
    uint32_t m[3];
    legal_mask(s, m);
    int8_t st, val;
    int act = -1, total = 0;
    int av = UTTT_SOLVE_UNKNOWN;  // this lane's action value
    if (!solve_root(s, m, st, val)) {
        int best;
        bool every;
        solve_wave(s, m, max_nodes, frames, av, total, best, every);
        if (solve_result(best, every, st, val))  // the lowest move that reaches the value (unknown lanes: -128)
            act = nth_legal(m, (uint32_t)(__ffsll((long long)__ballot(av == best)) - 1));
    }
    const int j1 = 64 + lane;
    int v0, v1;
    action_values_of(m, av, v0, v1);
    int8_t *out = action_values + (size_t)row * 81;
    out[lane] = (int8_t)(bit_of(m, lane) ? v0 : UTTT_SOLVE_UNKNOWN);
    if (j1 < 81) out[j1] = (int8_t)(bit_of(m, j1) ? v1 : UTTT_SOLVE_UNKNOWN);
    if (lane == 0) {
        value[row] = val;
        action[row] = (int8_t)act;
        status[row] = st;
        nodes[row] = (int64_t)total;
    }
}

// The overlay of uttt_solve.h on the round's pending leaves, shaped like k_playout_leaves (one wave per slot,
// the count read on the device) and run after an evaluator has filled the rows: a leaf with more than
// max_empties empties leaves at once (the test is wave-uniform: in the opening the kernel costs its launch
// and one state load per leaf); the others run k_solve_states' machine, and a SOLVED one overwrites its
// row's value and, with UTTT_PRIORS_OPTIMAL, its 81 priors. The same 32 KB of LDS per workgroup, no
// scratch, no atomics; each wave writes its own row only.
__global__ __launch_bounds__(kBlock) void k_solve_leaves(Trees tr, int32_t max_empties, int32_t max_nodes,
                                                         int32_t priors, float *__restrict__ policy,
                                                         int64_t policy_ld, float *__restrict__ value,
                                                         int64_t value_ld, int8_t *__restrict__ status) {
    __shared__ uint32_t frames[kWavesPerBlock * kSolveMaxEmpty * kWave];
    const int row = wave_index();
    if (row >= tr.count[0]) return;
    const int lane = lane_id();
    const uttt_state_t s = tr.leaf[tr.tree_of[row]];
    int8_t st = UTTT_OVERLAY_SKIPPED, val = 0;
    bool searched = false;
    int av = UTTT_SOLVE_UNKNOWN;
    uint32_t m[3] = {0u, 0u, 0u};
    if (!overlay_skips(s, max_empties)) {
        legal_mask(s, m);
        searched = !solve_root(s, m, st, val);
        if (searched) {
            int total, best;
            bool every;
            solve_wave(s, m, max_nodes, frames, av, total, best, every);
            solve_result(best, every, st, val);
        }
    }
    if (status && lane == 0) status[row] = st;
    if (st != UTTT_SOLVE_SOLVED) return;
    if (lane == 0) value[(size_t)row * value_ld] = (float)val;
    if (!searched || priors != UTTT_PRIORS_OPTIMAL) return;
    const int j1 = 64 + lane;
    int v0, v1;
    action_values_of(m, av, v0, v1);
    float *out = policy + (size_t)row * policy_ld;
    out[lane] = overlay_prior(bit_of(m, lane) != 0u, v0, val);
    if (j1 < 81) out[j1] = overlay_prior(bit_of(m, j1) != 0u, v1, val);
}

__global__ void k_root_visits(Pool pool, Trees tr, int32_t *visits, int32_t *n_legal) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= tr.n_trees * 81) return;
    const int t = g / 81, i = g % 81;
    const size_t base = (size_t)t * pool.cap;
    int first;
    const int L = root_children(pool, base, first);
    visits[g] = i < L ? visits_of(pool, base + first + i) : 0;
    if (i == 0) n_legal[t] = L;
}

__global__ void k_root_scores(Pool pool, Trees tr, float temperature, float *scores, int32_t *n_legal) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= tr.n_trees) return;
    float *sc = scores + (size_t)t * 81;  // the output row is the working buffer (no scratch)
    int L;
    root_scores(pool, (size_t)t * pool.cap, temperature, sc, L);
    for (int i = L; i < 81; ++i) sc[i] = 0.0f;
    n_legal[t] = L;
}

}  // namespace uttt
