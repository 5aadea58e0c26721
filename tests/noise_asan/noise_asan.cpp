// Host sanitizer program for the root noise: uttt_root_noise_host (csrc/rules_api.cpp, csrc/uttt_noise.h) under
// AddressSanitizer + UBSan on roots of every width a game meets (the initial state's 81 moves, 9 after a move,
// free-move roots, late positions, terminal ones with none), alpha at both ends of its range and between, and
// 64-bit seeds and streams. Checks what needs no second implementation: rows are finite, non-negative and sum to
// one, nothing is written past a root's legal moves or past the buffers, the key decides the row, argument errors.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "uttt_engine.h"

static uint64_t rng_state = 0x2545F4914F6CDD1Dull;
static uint32_t rnd() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

int main() {
    std::vector<uttt_state_t> pos;
    int widest = 0, ended = 0;
    while (pos.size() < 300) {
        uttt_state_t s;
        uttt_state_initial(&s);
        for (int ply = 0;; ++ply) {
            int32_t legal[81];
            const int n = uttt_state_legal_actions(&s, legal);
            if (ply < 2 || n > 64 || rnd() % 6 == 0 || uttt_state_is_done(&s)) {
                pos.push_back(s);
                if (n > widest && ply > 0) widest = n;
                ended += uttt_state_is_done(&s) != 0;
            }
            if (uttt_state_is_done(&s)) break;
            uttt_state_t t;
            if (uttt_state_next(&s, legal[rnd() % (uint32_t)n], &t) != UTTT_OK) return 2;
            s = t;
        }
    }
    const int64_t n = (int64_t)pos.size();
    int failures = 0;
    long long entries = 0;
    // exact-size heap buffers: an out-of-range store is an AddressSanitizer report
    std::vector<int64_t> stream(n);
    std::vector<int32_t> ply(n);
    for (int64_t i = 0; i < n; ++i) {
        stream[i] = (i % 5 == 0) ? (int64_t)(0x7FFFFFFF00000000ll + i) : i;
        ply[i] = (int32_t)(i % 81);
    }
    const float alphas[] = {1.0f / 32.0f, 0.3f, 1.0f, 3.0f, 32.0f};
    const uint64_t seeds[] = {0ull, 7ull, ~0ull};
    for (float alpha : alphas) {
        for (uint64_t seed : seeds) {
            std::vector<float> eta((size_t)n * 81, -7.0f), pri((size_t)n * 81, -7.0f);
            if (uttt_root_noise_host(pos.data(), n, stream.data(), ply.data(), 0.25f, alpha, seed, eta.data(), pri.data()) !=
                UTTT_OK)
                ++failures;
            for (int64_t i = 0; i < n; ++i) {
                int32_t legal[81];
                const int L = uttt_state_legal_actions(&pos[i], legal);
                double se = 0.0, sp = 0.0;
                for (int j = 0; j < 81; ++j) {
                    const float e = eta[(size_t)i * 81 + j], p = pri[(size_t)i * 81 + j];
                    if (j >= L) {
                        if (e != -7.0f || p != -7.0f) ++failures;
                        continue;
                    }
                    if (!std::isfinite(e) || e < 0.0f || !std::isfinite(p) || p < 0.0f) ++failures;
                    se += e;
                    sp += p;
                    ++entries;
                }
                if (L > 0 && (std::fabs(se - 1.0) > L * 1.2e-7 || std::fabs(sp - 1.0) > L * 1.2e-7)) ++failures;
            }
        }
    }
    // the key decides the row: the same (seed, stream, ply, L) twice, and one output at a time
    {
        std::vector<float> a((size_t)n * 81, 0.0f), b((size_t)n * 81, 0.0f), c((size_t)n * 81, 0.0f);
        if (uttt_root_noise_host(pos.data(), n, stream.data(), ply.data(), 0.5f, 0.3f, 11, a.data(), b.data()) != UTTT_OK) ++failures;
        if (uttt_root_noise_host(pos.data(), n, stream.data(), ply.data(), 0.5f, 0.3f, 11, c.data(), nullptr) != UTTT_OK) ++failures;
        if (std::memcmp(a.data(), c.data(), a.size() * sizeof(float)) != 0) ++failures;
        std::fill(c.begin(), c.end(), 0.0f);
        if (uttt_root_noise_host(pos.data(), n, stream.data(), ply.data(), 0.5f, 0.3f, 11, nullptr, c.data()) != UTTT_OK) ++failures;
        if (std::memcmp(b.data(), c.data(), b.size() * sizeof(float)) != 0) ++failures;
        if (uttt_root_noise_host(pos.data(), n, stream.data(), ply.data(), 0.5f, 0.3f, 12, c.data(), nullptr) != UTTT_OK) ++failures;
        if (std::memcmp(a.data(), c.data(), a.size() * sizeof(float)) == 0) ++failures;
    }
    float one[81];
    if (uttt_root_noise_host(pos.data(), 1, stream.data(), ply.data(), -0.1f, 0.3f, 0, one, nullptr) != UTTT_ERR_ARG) ++failures;
    if (uttt_root_noise_host(pos.data(), 1, stream.data(), ply.data(), 1.1f, 0.3f, 0, one, nullptr) != UTTT_ERR_ARG) ++failures;
    if (uttt_root_noise_host(pos.data(), 1, stream.data(), ply.data(), 0.25f, 0.03f, 0, one, nullptr) != UTTT_ERR_ARG) ++failures;
    if (uttt_root_noise_host(pos.data(), 1, stream.data(), ply.data(), 0.25f, 33.0f, 0, one, nullptr) != UTTT_ERR_ARG) ++failures;
    if (uttt_root_noise_host(pos.data(), 1, stream.data(), ply.data(), NAN, 0.3f, 0, one, nullptr) != UTTT_ERR_ARG) ++failures;
    if (uttt_root_noise_host(pos.data(), 1, stream.data(), ply.data(), 0.25f, NAN, 0, one, nullptr) != UTTT_ERR_ARG) ++failures;
    if (uttt_root_noise_host(nullptr, 1, stream.data(), ply.data(), 0.25f, 0.3f, 0, one, nullptr) != UTTT_ERR_ARG) ++failures;
    if (uttt_root_noise_host(pos.data(), 1, nullptr, ply.data(), 0.25f, 0.3f, 0, one, nullptr) != UTTT_ERR_ARG) ++failures;
    if (uttt_root_noise_host(pos.data(), 1, stream.data(), nullptr, 0.25f, 0.3f, 0, one, nullptr) != UTTT_ERR_ARG) ++failures;
    if (uttt_root_noise_host(pos.data(), -1, stream.data(), ply.data(), 0.25f, 0.3f, 0, one, nullptr) != UTTT_ERR_ARG) ++failures;
    if (uttt_root_noise_host(nullptr, 0, nullptr, nullptr, 0.25f, 0.3f, 0, nullptr, nullptr) != UTTT_OK) ++failures;
    uttt_state_t bad = pos[0];
    bad.active = 40;
    if (uttt_root_noise_host(&bad, 1, stream.data(), ply.data(), 0.25f, 0.3f, 0, one, nullptr) != UTTT_ERR_ARG) ++failures;
    if (widest <= 64 || ended == 0) ++failures;  // the walk met a free-move root and a finished game
    std::printf("noise_asan: %lld positions (widest after the opening %d, %d finished), %lld entries, %d failures\n",
                (long long)n, widest, ended, entries, failures);
    return failures ? 1 : 0;
}
