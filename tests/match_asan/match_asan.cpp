// Host sanitizer program for match play: uttt_match_move_host, uttt_match_draw_host and uttt_match_check_host
// (csrc/rules_api.cpp, csrc/uttt_match.h) under AddressSanitizer + UBSan. Whole games are played through the move
// rule from random visit rows in exact-size heap buffers: every root width a game meets (81 at the start, free-move
// roots above 64, single moves near the end), sampled and first-max plies, 64-bit seeds. Checks what needs no second
// implementation: the action is a legal move with a positive count whenever the row has one, the next state is
// uttt_state_next's, the result is live exactly until the game is done, and the argument errors.
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

int main() {
    int failures = 0, widest = 0, narrowest = 81, wins = 0, draws = 0;
    long long moves = 0;
    const uint64_t seeds[] = {0ull, 7ull, ~0ull, 0x8000000000000000ull};
    std::vector<uttt_state_t> finished;
    for (int game = 0; game < 400; ++game) {
        const uint64_t seed = seeds[game % 4];
        const int sample_plies = game % 3 == 0 ? 0 : (game % 3 == 1 ? 6 : 81);
        const int64_t id = game % 5 == 0 ? 0x7FFFFFFF00000000ll + game : game;
        uttt_state_t s;
        uttt_state_initial(&s);
        for (int ply = 0;; ++ply) {
            int32_t legal[81];
            const int L = uttt_state_legal_actions(&s, legal);
            if (L == 0) return 2;  // a live game has a move
            if (ply > 0 && L > widest) widest = L;
            if (L < narrowest) narrowest = L;
            std::vector<int32_t> N((size_t)L);  // exact size: a read past the row is a report
            const int mode = (int)(rnd() % 4u);
            for (int i = 0; i < L; ++i) N[i] = mode == 0 ? 0 : (mode == 1 ? 3 : (int32_t)(rnd() % 50u));
            uttt_state_t nx, ref;
            int32_t a = -1, res = -7;
            if (uttt_match_move_host(&s, N.data(), L, ply, id, seed, sample_plies, &nx, &a, &res) != UTTT_OK) {
                ++failures;
                break;
            }
            ++moves;
            int rank = -1;
            for (int i = 0; i < L; ++i)
                if (legal[i] == a) rank = i;
            if (rank < 0) {
                ++failures;
                break;
            }
            int32_t total = 0, top = 0;
            for (int i = 0; i < L; ++i) {
                total += N[i];
                if (N[i] > top) top = N[i];
            }
            if (total > 0 && N[rank] == 0) ++failures;                 // a sampled move has a visit
            if (ply >= sample_plies && N[rank] != top) ++failures;     // a late move is a most visited one
            if (total == 0 && rank != 0) ++failures;
            if (uttt_state_next(&s, a, &ref) != UTTT_OK || std::memcmp(&ref, &nx, sizeof(nx)) != 0) ++failures;
            const bool done = uttt_state_is_done(&nx) != 0, lost = uttt_state_is_lose(&nx) != 0;
            const int mover = (int)((id + ply) & 1);
            const int want = lost ? (mover == 0 ? 2 : 0) : (done ? 1 : -1);
            if (res != want) ++failures;
            s = nx;
            if (done) {
                wins += lost;
                draws += !lost;
                if (finished.size() < 8) finished.push_back(s);
                break;
            }
            if (ply >= 80) {
                ++failures;  // a game has at most 81 plies
                break;
            }
        }
    }
    // the draw: a function of the triple, each argument matters
    if (uttt_match_draw_host(3, 4, 5) != uttt_match_draw_host(3, 4, 5)) ++failures;
    if (uttt_match_draw_host(3, 4, 5) == uttt_match_draw_host(4, 4, 5)) ++failures;
    if (uttt_match_draw_host(3, 4, 5) == uttt_match_draw_host(3, 5, 5)) ++failures;
    if (uttt_match_draw_host(3, 4, 5) == uttt_match_draw_host(3, 4, 6)) ++failures;
    // argument errors
    uttt_state_t s0, nx;
    uttt_state_initial(&s0);
    std::vector<int32_t> row(81, 1);
    int32_t a, res;
    if (uttt_match_move_host(nullptr, row.data(), 81, 0, 0, 0, 0, &nx, &a, &res) != UTTT_ERR_ARG) ++failures;
    if (uttt_match_move_host(&s0, nullptr, 81, 0, 0, 0, 0, &nx, &a, &res) != UTTT_ERR_ARG) ++failures;
    if (uttt_match_move_host(&s0, row.data(), 80, 0, 0, 0, 0, &nx, &a, &res) != UTTT_ERR_ARG) ++failures;
    if (uttt_match_move_host(&s0, row.data(), 81, -1, 0, 0, 0, &nx, &a, &res) != UTTT_ERR_ARG) ++failures;
    if (uttt_match_move_host(&s0, row.data(), 81, 81, 0, 0, 0, &nx, &a, &res) != UTTT_ERR_ARG) ++failures;
    if (uttt_match_move_host(&s0, row.data(), 81, 0, -1, 0, 0, &nx, &a, &res) != UTTT_ERR_ARG) ++failures;
    if (uttt_match_move_host(&s0, row.data(), 81, 0, 0, 0, 0, nullptr, &a, &res) != UTTT_ERR_ARG) ++failures;
    row[80] = -1;
    if (uttt_match_move_host(&s0, row.data(), 81, 0, 0, 0, 0, &nx, &a, &res) != UTTT_ERR_ARG) ++failures;
    row[80] = 1;
    uttt_state_t bad = s0;
    bad.active = 40;
    if (uttt_match_move_host(&bad, row.data(), 81, 0, 0, 0, 0, &nx, &a, &res) != UTTT_ERR_ARG) ++failures;
    if (finished.empty()) ++failures;
    for (const uttt_state_t &f : finished)
        if (uttt_match_move_host(&f, row.data(), 1, 50, 0, 0, 0, &nx, &a, &res) != UTTT_ERR_ARG) ++failures;
    // uttt_match_begin's check: exact-size opening lists
    {
        std::vector<uttt_state_t> op(4, s0);
        if (uttt_match_check_host(op.data(), 4, 8, 8, 1) != UTTT_OK) ++failures;
        if (uttt_match_check_host(op.data(), 4, 4, 8, 0) != UTTT_OK) ++failures;
        if (uttt_match_check_host(op.data(), 4, 5, 8, 0) != UTTT_ERR_ARG) ++failures;
        if (uttt_match_check_host(op.data(), 4, 10, 16, 1) != UTTT_ERR_ARG) ++failures;
        if (uttt_match_check_host(op.data(), 4, 7, 8, 1) != UTTT_ERR_ARG) ++failures;
        if (uttt_match_check_host(op.data(), 4, 9, 8, 0) != UTTT_ERR_ARG) ++failures;
        if (uttt_match_check_host(op.data(), 4, 0, 8, 0) != UTTT_ERR_ARG) ++failures;
        if (uttt_match_check_host(nullptr, 4, 2, 8, 0) != UTTT_ERR_ARG) ++failures;
        if (!finished.empty()) {
            op[3] = finished[0];
            if (uttt_match_check_host(op.data(), 4, 8, 8, 1) != UTTT_ERR_ARG) ++failures;
            if (uttt_match_check_host(op.data(), 4, 6, 8, 1) != UTTT_OK) ++failures;  // opening 3 is not used
        }
        op[0].active = 9;
        if (uttt_match_check_host(op.data(), 4, 2, 8, 1) != UTTT_ERR_ARG) ++failures;
    }
    if (widest <= 64 || narrowest != 1 || wins == 0 || draws == 0) ++failures;  // the walk met every kind of root and end
    std::printf("match_asan: %lld moves (widest after the opening %d, narrowest %d, %d won, %d drawn), %d failures\n", moves,
                widest, narrowest, wins, draws, failures);
    return failures ? 1 : 0;
}
