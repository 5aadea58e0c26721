// Host sanitizer program for the random-playout evaluator: uttt_playout_host (csrc/rules_api.cpp,
// csrc/uttt_playout.h) under AddressSanitizer + UBSan on a few hundred positions along random games, their
// terminal positions included. Checks what needs no second implementation: counts within [0, P], the prefix
// property (playout j does not depend on P), terminal positions' fixed results, argument errors.
#include <cstdint>
#include <cstdio>
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
    while (pos.size() < 400) {
        uttt_state_t s;
        uttt_state_initial(&s);
        for (;;) {
            if (rnd() % 4 == 0 || uttt_state_is_done(&s)) pos.push_back(s);
            if (uttt_state_is_done(&s)) break;
            int32_t legal[81];
            const int n = uttt_state_legal_actions(&s, legal);
            uttt_state_t t;
            if (uttt_state_next(&s, legal[rnd() % (uint32_t)n], &t) != UTTT_OK) return 2;
            s = t;
        }
    }
    const int64_t n = (int64_t)pos.size();
    int failures = 0;
    // exact-size heap buffers: an out-of-range store is an AddressSanitizer report
    std::vector<int32_t> w1(n), l1(n), w64(n), l64(n), w65(n), l65(n), wmax(n), lmax(n);
    if (uttt_playout_host(pos.data(), n, 1, 3, w1.data(), l1.data()) != UTTT_OK) ++failures;
    if (uttt_playout_host(pos.data(), n, 64, 3, w64.data(), l64.data()) != UTTT_OK) ++failures;
    if (uttt_playout_host(pos.data(), n, 65, 3, w65.data(), l65.data()) != UTTT_OK) ++failures;
    if (uttt_playout_host(pos.data(), 8, 4096, ~0ull, wmax.data(), lmax.data()) != UTTT_OK) ++failures;
    long long decided = 0;
    for (int64_t i = 0; i < n; ++i) {
        const bool ok = w1[i] >= 0 && l1[i] >= 0 && w1[i] + l1[i] <= 1 && w64[i] >= w1[i] && l64[i] >= l1[i] &&
                        w64[i] + l64[i] <= 64 && w65[i] >= w64[i] && l65[i] >= l64[i] &&
                        (w65[i] - w64[i]) + (l65[i] - l64[i]) <= 1;
        if (!ok) ++failures;
        if (uttt_state_is_lose(&pos[i]) && !(w64[i] == 0 && l64[i] == 64)) ++failures;
        if (uttt_state_is_draw(&pos[i]) && !(w64[i] == 0 && l64[i] == 0)) ++failures;
        decided += w64[i] + l64[i];
    }
    for (int i = 0; i < 8; ++i)
        if (wmax[i] < 0 || lmax[i] < 0 || wmax[i] + lmax[i] > 4096) ++failures;
    if (decided == 0) ++failures;
    if (uttt_playout_host(pos.data(), n, 0, 0, w1.data(), l1.data()) != UTTT_ERR_ARG) ++failures;
    if (uttt_playout_host(pos.data(), n, 4097, 0, w1.data(), l1.data()) != UTTT_ERR_ARG) ++failures;
    if (uttt_playout_host(nullptr, 1, 8, 0, w1.data(), l1.data()) != UTTT_ERR_ARG) ++failures;
    if (uttt_playout_host(nullptr, 0, 8, 0, nullptr, nullptr) != UTTT_OK) ++failures;
    uttt_state_t bad = pos[0];
    bad.active = 40;
    if (uttt_playout_host(&bad, 1, 8, 0, w1.data(), l1.data()) != UTTT_ERR_ARG) ++failures;
    std::printf("playout_asan: %lld positions, %lld of %lld playouts decided, %d failures\n", (long long)n, decided,
                (long long)n * 64, failures);
    return failures ? 1 : 0;
}
