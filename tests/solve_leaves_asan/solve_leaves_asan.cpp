// Host sanitizer program for the solver overlay: uttt_solve_overlay_host (csrc/rules_api.cpp, csrc/uttt_solve.h)
// under AddressSanitizer + UBSan on late positions of random games, terminal ones and the opening included, over
// rows in exact-size heap buffers (contiguous and with a row stride of 96), both priors modes, a generous and a
// stopping budget, max_empties 0 / 10 / 32 and a NULL status. Checks what needs no second implementation: the
// statuses against uttt_solve_host's, untouched rows and the padding between rows bit for bit, the marks against
// the action values, argument errors.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "uttt_engine.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

static int failures = 0;
static void expect(bool ok, const char *what, long long i) {
    if (!ok) {
        ++failures;
        std::printf("FAILED: %s (row %lld)\n", what, i);
    }
}

static bool same_bits(const float *a, const float *b, size_t n) { return std::memcmp(a, b, n * sizeof(float)) == 0; }

int main() {
    std::vector<uttt_state_t> pos;
    while (pos.size() < 100) {  // the last plies of random games, the final position included
        uttt_state_t s;
        uttt_state_initial(&s);
        for (int ply = 0;; ++ply) {
            const bool done = uttt_state_is_done(&s) != 0;
            if (done || (ply >= 45 && rnd() % 3 == 0)) pos.push_back(s);
            if (done) break;
            int32_t legal[81];
            const int n = uttt_state_legal_actions(&s, legal);
            uttt_state_t t;
            if (uttt_state_next(&s, legal[rnd() % (uint32_t)n], &t) != UTTT_OK) return 2;
            s = t;
        }
    }
    uttt_state_t first;
    uttt_state_initial(&first);
    pos.push_back(first);
    const int64_t n = (int64_t)pos.size();
    long long solved = 0, stopped = 0, skipped = 0, marks = 0;
    for (const int32_t max_nodes : {4096, 16}) {
        std::vector<int8_t> sv(n), ss(n), sav(n * 81);
        if (uttt_solve_host(pos.data(), n, max_nodes, sv.data(), nullptr, ss.data(), nullptr, sav.data()) != UTTT_OK)
            ++failures;
        for (const int32_t max_empties : {0, 10, 32})
            for (const int32_t priors : {UTTT_PRIORS_KEEP, UTTT_PRIORS_OPTIMAL})
                for (const int64_t ld : {(int64_t)81, (int64_t)96}) {
                    // exact-size heap buffers: an out-of-range store is an AddressSanitizer report
                    std::vector<float> policy((n - 1) * ld + 81), value(n);
                    for (float &x : policy) x = (float)(rnd() % 1000) / 7.0f;
                    for (float &x : value) x = (float)(rnd() % 1000) / 7.0f;
                    const std::vector<float> policy0 = policy, value0 = value;
                    std::vector<int8_t> status(n, 77);
                    const bool with_status = ld == 81;
                    if (uttt_solve_overlay_host(pos.data(), n, max_empties, max_nodes, priors, policy.data(), ld,
                                                value.data(), 1, with_status ? status.data() : nullptr) != UTTT_OK)
                        ++failures;
                    for (int64_t i = 0; i < n; ++i) {
                        int32_t legal[81];
                        const int L = uttt_state_legal_actions(&pos[i], legal);
                        const bool over = ss[i] == UTTT_SOLVE_TOO_LARGE;  // more than 32 empties
                        const float *row = &policy[i * ld], *row0 = &policy0[i * ld];
                        if (i + 1 < n) expect(same_bits(row + 81, row0 + 81, (size_t)(ld - 81)), "padding touched", i);
                        const bool changed = !same_bits(row, row0, 81) || !same_bits(&value[i], &value0[i], 1);
                        if (with_status) {
                            const int8_t st = status[i];
                            expect(st == UTTT_OVERLAY_SKIPPED || st == UTTT_SOLVE_SOLVED || st == UTTT_SOLVE_BUDGET,
                                   "status out of range", i);
                            if (st != UTTT_OVERLAY_SKIPPED) expect(st == ss[i], "status differs from the solver's", i);
                            if (over || max_empties == 0)
                                expect(st == UTTT_OVERLAY_SKIPPED || uttt_state_is_done(&pos[i]), "searched", i);
                            if (st != UTTT_SOLVE_SOLVED) expect(!changed, "an unsolved row changed", i);
                            solved += st == UTTT_SOLVE_SOLVED;
                            stopped += st == UTTT_SOLVE_BUDGET;
                            skipped += st == UTTT_OVERLAY_SKIPPED;
                        }
                        if (!changed) continue;
                        expect(ss[i] == UTTT_SOLVE_SOLVED && value[i] == (float)sv[i], "value of a changed row", i);
                        if (priors == UTTT_PRIORS_KEEP || uttt_state_is_done(&pos[i])) {
                            expect(same_bits(row, row0, 81), "policy changed", i);
                            continue;
                        }
                        int count = 0;
                        for (int a = 0; a < 81; ++a) {
                            const bool mark = sav[i * 81 + a] == sv[i];
                            expect(row[a] == (mark ? 1.0f : 0.0f), "mark", i);
                            count += mark;
                        }
                        expect(count >= 1 && count <= L, "number of marks", i);
                        marks += count;
                    }
                }
    }
    expect(solved > 0 && stopped > 0 && skipped > 0 && marks > 0, "every outcome occurs", -1);
    std::vector<float> p(81), v(1);
    expect(uttt_solve_overlay_host(&first, 1, 33, 16, 0, p.data(), 81, v.data(), 1, nullptr) == UTTT_ERR_ARG, "E", -1);
    expect(uttt_solve_overlay_host(&first, 1, -1, 16, 0, p.data(), 81, v.data(), 1, nullptr) == UTTT_ERR_ARG, "E", -1);
    expect(uttt_solve_overlay_host(&first, 1, 10, 0, 0, p.data(), 81, v.data(), 1, nullptr) == UTTT_ERR_ARG, "M", -1);
    expect(uttt_solve_overlay_host(&first, 1, 10, 16, 2, p.data(), 81, v.data(), 1, nullptr) == UTTT_ERR_ARG, "priors",
           -1);
    expect(uttt_solve_overlay_host(&first, 1, 10, 16, 0, p.data(), 80, v.data(), 1, nullptr) == UTTT_ERR_ARG, "ld", -1);
    expect(uttt_solve_overlay_host(&first, 1, 10, 16, 0, nullptr, 81, v.data(), 1, nullptr) == UTTT_ERR_ARG, "null", -1);
    std::printf("solve_leaves_asan: %lld positions, %lld solved, %lld stopped, %lld skipped, %lld marks, "
                "%d failures\n", (long long)n, solved, stopped, skipped, marks, failures);
    return failures ? 1 : 0;
}
