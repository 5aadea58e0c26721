// uttt_noise.h — Dirichlet noise on a root's priors, compiled for both the host (uttt_root_noise_host, the
// checker's counterpart) and gfx950 (k_root_noise). DESIGN.md §6f.
//
// A root with L legal moves in ascending action order (rank i = 0..L-1) gets eta ~ Dirichlet(alpha, ..., alpha)
// as L normalised Gamma(alpha, 1) variates and the mixed priors p'_i = eps * eta_i + (1 - eps) * p_i. The draws
// are counter-based: a pure function of (seed, stream, ply, rank), so the same on host and device, in any slot,
// lane, process or sharding. Self-play keys a root by (global game id, ply), a plain search by (tree index, 0).
//
// Bit equality between the host compiler and hipcc: only + - * / (correctly rounded on both sides; the device
// through -fhip-fp32-correctly-rounded-divide-sqrt), sqrt, explicit fmaf, integer <-> float conversions and the
// header's own log / exp (bit manipulation and a polynomial). No call into libm or the device math library
// beyond fmaf / sqrtf, and every multiply-add is an fmaf the source spells out (the builds also pass
// -ffp-contract=off).
#pragma once

#include "uttt_bits.h"

namespace uttt {

constexpr float kNoiseAlphaMin = 1.0f / 32.0f, kNoiseAlphaMax = 32.0f;
constexpr int kNoiseAttempts = 32;  // Cheng's GB accepts with probability >= 0.68: 0.32^32 < 2e-16 reach the bound

// epsilon in [0, 1] and alpha in [kNoiseAlphaMin, kNoiseAlphaMax], or UTTT_ERR_ARG with a message (rules_api.cpp)
int noise_check_args(const char *who, float epsilon, float alpha);

// fmaf as the compiler's builtin: one rounding on both sides (v_fma_f32 on the device)
UTTT_HD float noise_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

UTTT_HD uint32_t f32_bits(float x) {
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    return u;
}
UTTT_HD float bits_f32(uint32_t u) {
    float x;
    __builtin_memcpy(&x, &u, 4);
    return x;
}

// The key of a root: (seed, stream, ply) through mix64 / kGold.
UTTT_HD uint64_t noise_key(uint64_t seed, uint64_t stream, uint32_t ply) {
    uint64_t h = mix64(seed + kGold);
    h = mix64(h ^ stream);
    return mix64(h + ((uint64_t)ply + 1ull) * kGold);
}

// Draw j of rank i under key: 64 bits, a function of (key, i, j) alone (j < 64).
UTTT_HD uint64_t noise_bits(uint64_t key, uint32_t i, uint32_t j) {
    return mix64(key + (uint64_t)(i * 64u + j + 1u) * kGold);
}
// A uniform in (0, 1) from 23 bits: (2 k + 1) / 2^24, so u and 1 - u are both exact in f32 and never 0 or 1.
UTTT_HD float noise_unit(uint32_t k23) { return (float)(2u * k23 + 1u) * (1.0f / 16777216.0f); }

// ln x for a positive normal x: x = m 2^e with m in [sqrt(1/2), sqrt 2), ln m = 2 atanh(s), s = (m - 1) / (m + 1),
// |s| <= 0.1716; the series through s^9 leaves 2 s^11 / 11 < 1e-9. Absolute error about 1e-7 (+ 6e-8 |ln x|).
UTTT_HD float noise_log(float x) {
    const uint32_t b = f32_bits(x);
    int e = (int)(b >> 23) - 127;
    uint32_t mb = (b & 0x007FFFFFu) | 0x3F800000u;  // m in [1, 2)
    if (mb >= 0x3FB504F3u) {                        // m >= sqrt 2: halve it
        mb -= 0x00800000u;
        e += 1;
    }
    const float m = bits_f32(mb);
    const float s = (m - 1.0f) / (m + 1.0f);
    const float z = s * s;
    float p = 1.0f / 9.0f;
    p = noise_fma(p, z, 1.0f / 7.0f);
    p = noise_fma(p, z, 1.0f / 5.0f);
    p = noise_fma(p, z, 1.0f / 3.0f);
    p = noise_fma(p, z, 1.0f);
    const float lm = (s + s) * p;
    const float fe = (float)e;
    return noise_fma(fe, 0.693145751953125f, noise_fma(fe, 1.42860682030941723212e-6f, lm));  // ln 2 = hi + lo
}

// e^x: 0 below -87 (no subnormal results), x above 88 taken as 88. x = n ln 2 + r, |r| <= 0.35, the Taylor
// polynomial through r^6 leaves r^7 / 5040 < 1.3e-7 relative; 2^n by the exponent field.
UTTT_HD float noise_exp(float x) {
    if (!(x >= -87.0f)) return 0.0f;
    x = x > 88.0f ? 88.0f : x;
    const int n = (int)noise_fma(x, 1.44269504088896341f, x < 0.0f ? -0.5f : 0.5f);  // truncation: round to nearest
    const float fn = (float)n;
    float r = noise_fma(-fn, 0.693145751953125f, x);
    r = noise_fma(-fn, 1.42860682030941723212e-6f, r);
    float p = 1.0f / 720.0f;
    p = noise_fma(p, r, 1.0f / 120.0f);
    p = noise_fma(p, r, 1.0f / 24.0f);
    p = noise_fma(p, r, 1.0f / 6.0f);
    p = noise_fma(p, r, 0.5f);
    p = noise_fma(p, r, 1.0f);
    p = noise_fma(p, r, 1.0f);
    return p * bits_f32((uint32_t)(n + 127) << 23);  // n in -126 .. 127
}

// ln of a Gamma(alpha, 1) variate for (key, rank i), alpha in [1/32, 32].
//
// a >= 1: Cheng's GB (1977), a rejection from the log-logistic: with u1, u2 uniform, v = c1 ln(u1 / (1 - u1)),
// x = a e^v, z = u1^2 u2, r = (a - ln 4) + (a + 1 / c1) v - x; accept when r + 1 + ln 4.5 >= 4.5 z or r >= ln z,
// c1 = 1 / sqrt(2 a - 1). Attempt j uses noise_bits(key, i, j); after kNoiseAttempts the last proposal stands.
// The variate's logarithm is ln a + v: no exp of the result, so nothing under- or overflows.
// alpha < 1: G(alpha) = G(alpha + 1) U^(1 / alpha), in logarithms ln G(alpha + 1) + ln(U) / alpha with U from
// noise_bits(key, i, kNoiseAttempts). At alpha = 1/32 the second term reaches -532: the variate itself would
// underflow f32 in most lanes, its logarithm does not.
UTTT_HD float noise_log_gamma(float alpha, uint64_t key, uint32_t i) {
    const bool boost = alpha < 1.0f;
    const float a = boost ? alpha + 1.0f : alpha;
    const float c1 = 1.0f / __builtin_sqrtf(noise_fma(2.0f, a, -1.0f));
    const float c2 = a - 1.38629436111989062f;  // a - ln 4
    const float c3 = a + 1.0f / c1;
    float v = 0.0f;
    for (uint32_t j = 0u; j < (uint32_t)kNoiseAttempts; ++j) {
        const uint64_t bits = noise_bits(key, i, j);
        const float u1 = noise_unit((uint32_t)(bits >> 41)), u2 = noise_unit((uint32_t)(bits >> 18) & 0x7FFFFFu);
        v = c1 * noise_log(u1 / (1.0f - u1));
        const float x = a * noise_exp(v);
        const float z = (u1 * u1) * u2;
        const float r = noise_fma(c3, v, c2) - x;
        if (noise_fma(-4.5f, z, r + 2.50407739677627407f) >= 0.0f) break;  // 1 + ln 4.5
        if (r >= noise_log(z)) break;
    }
    float lg = noise_log(a) + v;
    if (boost) {
        const float u = noise_unit((uint32_t)(noise_bits(key, i, (uint32_t)kNoiseAttempts) >> 41));
        lg = lg + noise_log(u) / alpha;
    }
    return lg;
}

// g_i up to the root's common factor: e^(ln g_i - m), m the largest ln g of the root's ranks, so the largest is
// exactly 1 and the sum S is in [1, L] for every alpha. eta does not see the factor.
UTTT_HD float noise_scaled(float lg, float lg_max) { return noise_exp(lg - lg_max); }
// The larger of two logarithms by a compare and a select (max is order-free: a wave reduction and the host's
// loop agree).
UTTT_HD float noise_max(float a, float b) { return b > a ? b : a; }

UTTT_HD float noise_eta(float g, float S, int L) { return S > 0.0f ? g / S : 1.0f / (float)L; }

// The mixed prior, written once for both sides.
UTTT_HD float noise_mix(float eps, float eta, float p) { return noise_fma(eps, eta, (1.0f - eps) * p); }

// eta[0..L-1] of a root with L legal moves (the host's form; k_root_noise spreads the ranks over a wave): the
// draws, their maximum, the scaled variates and their sequential f32 sum in rank order, the divide.
UTTT_HD void noise_eta_row(float alpha, uint64_t key, int L, float *eta) {
    float m = 0.0f;
    for (int i = 0; i < L; ++i) {
        eta[i] = noise_log_gamma(alpha, key, (uint32_t)i);
        m = i == 0 ? eta[i] : noise_max(m, eta[i]);
    }
    float S = 0.0f;
    for (int i = 0; i < L; ++i) {
        eta[i] = noise_scaled(eta[i], m);
        S += eta[i];
    }
    for (int i = 0; i < L; ++i) eta[i] = noise_eta(eta[i], S, L);
}

}  // namespace uttt
