// engine/symmetry.h — the round's pending leaves seen through a symmetry of the square, and an evaluator's rows
// mapped back (uttt_sym.h). A part of engine.hip's one translation unit, like its siblings in
// engine/. The hashed choice shares the wave's input_words (the hash evaluator's four ballots), which rounds.h
// defines further down and this header only declares.
//
// Both kernels are shaped like k_playout_leaves: one wave per slot, the count read on the device (the grid covers
// every tree), each wave writing its own row only. The leaf and its symmetry are wave-uniform, so the transform
// runs on the scalar unit. No LDS, no atomics, no scratch.
#pragma once
#include "layout.h"
#include "wave.h"
#include "uttt_sym.h"

namespace uttt {

__device__ __forceinline__ void input_words(const uttt_state_t &s, const uint32_t (&m)[3], uint64_t (&w)[4]);

// states_out[row] = T_g(leaf), sym_out[row] = g, and with nn_out the NCHW input of T_g(leaf) as k_encode writes a
// leaf's: g fixed, or the hashed choice of the leaf and the seed.
__global__ __launch_bounds__(kBlock) void k_sym_leaves(Trees tr, int32_t mode, uint64_t g_or_seed,
                                                       uttt_state_t *__restrict__ states_out,
                                                       int8_t *__restrict__ sym_out, float *__restrict__ nn_out) {
    const int row = wave_index();
    if (row >= tr.count[0]) return;
    const int lane = lane_id();
    const uttt_state_t s = tr.leaf[tr.tree_of[row]];
    int g = (int)(g_or_seed & 7u);
    if (mode == UTTT_SYM_HASHED) {
        uint32_t m[3];
        legal_mask(s, m);
        uint64_t w[4];
        input_words(s, m, w);
        g = sym_of_key(w, g_or_seed);
    }
    const uttt_state_t t = sym_state(s, g);
    if (lane == 0) {
        states_out[row] = t;
        sym_out[row] = (int8_t)g;
    }
    if (!nn_out) return;
    uint32_t tm[3];
    legal_mask(t, tm);
    float *xr = nn_out + (size_t)row * UTTT_INPUT_SIZE;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = i * kWave + lane;
        if (j < UTTT_INPUT_SIZE) {
            const int ch = j / 81, a = action_at(j % 81);
            const uint32_t on = ch == 0 ? bit_of(t.own, a) : (ch == 1 ? bit_of(t.opp, a) : bit_of(tm, a));
            xr[j] = on ? 1.0f : 0.0f;
        }
    }
}

// Row `row` of an evaluator's output for the transformed leaves, mapped back to the leaf's own actions:
// out[a] = p[pi_g(a)] (+ out[a] when accumulating) (* scale unless it is 1), and the same for the value. g is
// masked to 0..7, so every read stays inside the row whatever sym holds.
__global__ __launch_bounds__(kBlock) void k_sym_rows(Trees tr, const int8_t *__restrict__ sym,
                                                     const float *__restrict__ policy, int64_t policy_ld,
                                                     const float *__restrict__ value, int64_t value_ld,
                                                     float *__restrict__ out_policy, int64_t out_policy_ld,
                                                     float *__restrict__ out_value, int64_t out_value_ld,
                                                     int32_t accumulate, float scale) {
    const int row = wave_index();
    if (row >= tr.count[0]) return;
    const int lane = lane_id();
    const int g = __builtin_amdgcn_readfirstlane((int)sym[row]) & 7;
    const float *p = policy + (size_t)row * policy_ld;
    float *o = out_policy + (size_t)row * out_policy_ld;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int a = i * kWave + lane;
        if (a < 81) {
            float x = p[sym_action(g, a)];
            if (accumulate) x = o[a] + x;
            if (scale != 1.0f) x = x * scale;
            o[a] = x;
        }
    }
    if (lane == 0) {
        float x = value[(size_t)row * value_ld];
        if (accumulate) x = out_value[(size_t)row * out_value_ld] + x;
        if (scale != 1.0f) x = x * scale;
        out_value[(size_t)row * out_value_ld] = x;
    }
}

}  // namespace uttt
