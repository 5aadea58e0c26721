// Host sanitizer program for the exact endgame solver: uttt_solve_host (csrc/rules_api.cpp, csrc/uttt_solve.h)
// under AddressSanitizer + UBSan on late positions of random games, with a generous budget, a budget that stops
// lanes, and the deepest accepted position (32 empties: the stack's last frames). Checks what needs no second
// implementation: outputs in range, the value against the action values, a smaller budget never knows more,
// terminal and too-large positions' fixed results, argument errors.
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

// Boards 0, 1, 5, 6, 7 closed for both sides, one stone in each of boards 2, 3, 4, 8: 32 empties, a free move.
static uttt_state_t deepest() {
    int32_t p[81] = {0}, e[81] = {0};
    const int32_t closed[9] = {1, 1, 0, 0, 0, 1, 1, 1, 0};
    p[2 * 9] = p[4 * 9] = 1;
    e[3 * 9] = e[8 * 9] = 1;
    uttt_state_t s;
    if (uttt_state_from_arrays(p, e, closed, closed, -1, &s) != UTTT_OK) std::printf("deepest: bad arrays\n");
    return s;
}

struct Out {
    std::vector<int8_t> value, action, status, av;
    std::vector<int64_t> nodes;
    // exact-size heap buffers: an out-of-range store is an AddressSanitizer report
    explicit Out(int64_t n) : value(n), action(n), status(n), av(n * 81), nodes(n) {}
};

int main() {
    std::vector<uttt_state_t> pos;
    while (pos.size() < 120) {  // the last plies of random games, the final position included
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
    pos.push_back(deepest());
    const int64_t n = (int64_t)pos.size();
    int failures = 0;
    Out big(n), small(n);
    if (uttt_solve_host(pos.data(), n, 4096, big.value.data(), big.action.data(), big.status.data(), big.nodes.data(),
                        big.av.data()) != UTTT_OK)
        ++failures;
    if (uttt_solve_host(pos.data(), n, 16, small.value.data(), small.action.data(), small.status.data(),
                        small.nodes.data(), small.av.data()) != UTTT_OK)
        ++failures;
    long long solved = 0, stopped = 0;
    for (int64_t i = 0; i < n; ++i) {
        int32_t legal[81];
        const int L = uttt_state_legal_actions(&pos[i], legal);
        for (const Out *o : {&big, &small}) {
            const int8_t st = o->status[i], v = o->value[i], a = o->action[i];
            const int8_t *av = &o->av[i * 81];
            bool ok = st >= UTTT_SOLVE_SOLVED && st <= UTTT_SOLVE_TOO_LARGE && v >= -1 && v <= 1 && a >= -1 && a < 81 &&
                      o->nodes[i] >= 0 && o->nodes[i] <= (int64_t)(o == &big ? 4096 : 16) * L;
            int known = 0, best = -2;
            for (int j = 0; j < 81; ++j) {
                if (av[j] == UTTT_SOLVE_UNKNOWN) continue;
                ok = ok && av[j] >= -1 && av[j] <= 1;
                ++known;
                if (av[j] > best) best = av[j];
            }
            if (uttt_state_is_done(&pos[i]))
                ok = ok && st == UTTT_SOLVE_SOLVED && a == -1 && o->nodes[i] == 0 && known == 0 &&
                     v == (uttt_state_is_lose(&pos[i]) ? -1 : 0);
            else if (st == UTTT_SOLVE_SOLVED)
                ok = ok && a >= 0 && av[a] == v && v == best && (known == L || v == 1);
            else
                ok = ok && v == 0 && a == -1 && (st == UTTT_SOLVE_BUDGET ? known < L : known == 0 && o->nodes[i] == 0);
            if (!ok) ++failures;
        }
        for (int j = 0; j < 81; ++j)  // what 16 nodes settle, 4096 nodes settle the same way
            if (small.av[i * 81 + j] != UTTT_SOLVE_UNKNOWN && small.av[i * 81 + j] != big.av[i * 81 + j]) ++failures;
        solved += big.status[i] == UTTT_SOLVE_SOLVED;
        stopped += small.status[i] == UTTT_SOLVE_BUDGET;
    }
    if (big.status[n - 2] != UTTT_SOLVE_TOO_LARGE) ++failures;
    if (big.status[n - 1] != UTTT_SOLVE_BUDGET || big.nodes[n - 1] != 4096 * 32) ++failures;  // every lane cut short
    if (solved < 40 || stopped < 40) ++failures;  // the run covered both ends (of 122 positions)
    // NULL outputs, argument errors
    if (uttt_solve_host(pos.data(), n, 64, nullptr, nullptr, nullptr, nullptr, nullptr) != UTTT_OK) ++failures;
    if (uttt_solve_host(pos.data(), n, 64, nullptr, small.action.data(), nullptr, nullptr, nullptr) != UTTT_OK) ++failures;
    if (uttt_solve_host(pos.data(), n, 0, nullptr, nullptr, nullptr, nullptr, nullptr) != UTTT_ERR_ARG) ++failures;
    if (uttt_solve_host(pos.data(), n, (1 << 22) + 1, nullptr, nullptr, nullptr, nullptr, nullptr) != UTTT_ERR_ARG)
        ++failures;
    if (uttt_solve_host(pos.data(), -1, 64, nullptr, nullptr, nullptr, nullptr, nullptr) != UTTT_ERR_ARG) ++failures;
    if (uttt_solve_host(nullptr, 1, 64, nullptr, nullptr, nullptr, nullptr, nullptr) != UTTT_ERR_ARG) ++failures;
    if (uttt_solve_host(nullptr, 0, 64, nullptr, nullptr, nullptr, nullptr, nullptr) != UTTT_OK) ++failures;
    uttt_state_t bad = pos[0];
    bad.active = 40;
    if (uttt_solve_host(&bad, 1, 64, nullptr, nullptr, nullptr, nullptr, nullptr) != UTTT_ERR_ARG) ++failures;
    std::printf("solve_asan: %lld positions, %lld solved at 4096 nodes, %lld stopped at 16, %d failures\n", (long long)n,
                solved, stopped, failures);
    return failures ? 1 : 0;
}
