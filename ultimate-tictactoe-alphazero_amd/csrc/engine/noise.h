// engine/noise.h — Dirichlet noise mixed into the roots' priors (uttt_noise.h), and the roots'
// priors read back. A part of engine.hip's one translation unit, like its siblings in engine/.
//
// k_root_noise is shaped like k_begin, which it follows on the stream: one wave per tree, each wave rewriting the
// P word of its own root's child block only. The round loop's kernels load a child's P from its record
// (puct_group), so nothing downstream knows the priors were uniform. One 84-float LDS row per wave, no atomics,
// no scratch.
#pragma once
#include "expand.h"
#include "layout.h"
#include "wave.h"
#include "uttt_noise.h"

namespace uttt {

// What keys a self-play root: the slot's global game id and ply (adjacent in Slot; engine.hip asserts it).
struct NoiseKey {
    int64_t stream;
    int32_t ply;
};

// keys (self-play): tree t's NoiseKey at keys + t * key_stride bytes; nullptr (a plain search): (t, 0).
__global__ __launch_bounds__(kBlock) void k_root_noise(Pool pool, Trees tr, const char *keys, int key_stride, float eps,
                                                       float alpha, uint64_t seed) {
    __shared__ __attribute__((aligned(16))) float s_row[kWavesPerBlock][84];  // the variates' sum's row, per wave
    const int t = wave_index();
    if (t >= tr.n_trees) return;
    if (!(tr.ctl[t].status & kLive)) return;  // a slot without a game, a root without a move
    const uttt_state_t s = tr.root[t];
    const Legal g = legal_of(s);
    if (g.L == 0) return;
    uint64_t stream = (uint64_t)t;
    uint32_t ply = 0u;
    if (keys) {
        const NoiseKey k = *reinterpret_cast<const NoiseKey *>(keys + (size_t)t * key_stride);
        stream = (uint64_t)k.stream;
        ply = (uint32_t)k.ply;
    }
    const uint64_t key = noise_key(seed, stream, ply);
    // lane l draws for action l and action 64 + l, at their ranks; the largest logarithm over the wave
    const float lg0 = g.l0 ? noise_log_gamma(alpha, key, (uint32_t)g.i0) : 0.0f;
    const float lg1 = g.l1 ? noise_log_gamma(alpha, key, (uint32_t)g.i1) : 0.0f;
    float m = g.l0 ? lg0 : -3.0e38f;  // below every logarithm (they are above -1e3): lanes without a move
    m = g.l1 ? noise_max(m, lg1) : m;
#pragma unroll
    for (int o = 32; o; o >>= 1) m = noise_max(m, __shfl_xor(m, o));
    const float g0 = g.l0 ? noise_scaled(lg0, m) : 0.0f;
    const float g1 = g.l1 ? noise_scaled(lg1, m) : 0.0f;
    const float S = seq_sum_legal(s_row[threadIdx.x >> 6], g0, g1, g);  // rank order: the host's loop
    uint32_t *const P = reinterpret_cast<uint32_t *>(pool.rec + (size_t)t * pool.cap + 1) + 1;  // record r's .y at P[4 r]
    if (g.l0) P[4 * g.i0] = __float_as_uint(noise_mix(eps, noise_eta(g0, S, g.L), __uint_as_float(P[4 * g.i0])));
    if (g.l1) P[4 * g.i1] = __float_as_uint(noise_mix(eps, noise_eta(g1, S, g.L), __uint_as_float(P[4 * g.i1])));
}

// The root children's P in legal order (row stride 81, zeros past L) and L, as k_root_visits reads the visits.
__global__ void k_root_priors(Pool pool, Trees tr, float *priors, int32_t *n_legal) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= tr.n_trees * 81) return;
    const int t = g / 81, i = g % 81;
    const size_t base = (size_t)t * pool.cap;
    const uint4 r = pool.rec[base];
    const int L = meta_L(r.z), first = link_first(r.w);
    priors[g] = i < L ? __uint_as_float(pool.rec[base + first + i].y) : 0.0f;
    if (i == 0) n_legal[t] = L;
}

}  // namespace uttt
