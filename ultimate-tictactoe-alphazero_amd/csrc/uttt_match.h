// uttt_match.h — the rules of a match between two players, compiled for both the host (uttt_match_move_host,
// uttt_match_draw_host: the checker's counterpart and random_openings' draws) and gfx950 (k_match_move,
// k_match_lists; engine/match.h). DESIGN.md §6h.
//
// A match is G games (evaluate_network.py:78-92's loop over play(), :33-54, with every game resident on the device). Game g starts at
// openings[g / 2] when the match is paired and at openings[g] when it is not, and player g % 2 takes the side to
// move at the start position: games 2 i and 2 i + 1 are one opening with the colours swapped. The ply is counted
// from the start position, so the player to move at ply p of game g is (g + p) % 2.
//
// The move rule takes the root's L visit counts in legal (ascending action) order:
//   ply >= sample_plies  the first index of the largest count (what uttt_search_scores makes one-hot at
//                        temperature 0, and what np.random.choice then returns: evaluate_network.py:47-51's move);
//   ply <  sample_plies  an index drawn in proportion to the counts, in integers only: T = sum N, x = the high 64
//                        bits of draw * T with draw = match_draw(seed, game, ply), and the choice is the smallest
//                        i with N[0] + ... + N[i] > x. x < T, so the index exists; T == 0 falls back to the first
//                        maximum. No float is touched, so host and device cannot differ by rounding.
// The chosen action is the i-th legal move; the game ends when the new state is lost for its side to move (the
// mover wins) or done without a loss (a draw): evaluate_network.py:26-30's first_player_point.
#pragma once

#include "uttt_bits.h"
#include "uttt_playout.h"

namespace uttt {

constexpr int kMatchLive = -1;        // a game's result while it is played; else player 0's half-points 0 / 1 / 2
constexpr int kMatchMaxGames = (1 << 20) - 1;  // k_match_lists packs its counts into 21-bit fields (points <= 2 G)

// The draw of (seed, game, ply): 64 bits through mix64 / kGold, as noise_key and playout_key are built, under a
// constant of its own so that a match seeded like the noise does not walk the noise's stream.
UTTT_HD uint64_t match_draw(uint64_t seed, uint64_t game, uint32_t ply) {
    uint64_t h = mix64(seed ^ 0xA5A35C9B6D2F81E7ull);
    h = mix64(h ^ game);
    return mix64(h + ((uint64_t)ply + 1ull) * kGold);
}

// The high 64 bits of draw * T for T < 2^32 (T is at most the search's simulations): two 32 x 32 partial products,
// the same on every compiler (no 128-bit type).
UTTT_HD uint64_t match_scale(uint64_t draw, uint32_t T) {
    const uint64_t lo = (draw & 0xFFFFFFFFull) * (uint64_t)T, hi = (draw >> 32) * (uint64_t)T;
    return (hi + (lo >> 32)) >> 32;
}

UTTT_HD int match_opening_of(int game, int paired) { return paired ? game >> 1 : game; }
UTTT_HD int match_player_to_move(int game, int ply) { return (game + ply) & 1; }
UTTT_HD bool match_samples(int ply, int sample_plies) { return ply < sample_plies; }

// The first index of the largest of N[0..L-1] (0 for an empty row).
UTTT_HD int match_first_max(const int32_t *N, int L) {
    int mi = 0;
    for (int i = 1; i < L; ++i)
        if (N[i] > N[mi]) mi = i;
    return mi;
}

// The move rule's index (the host's form; k_match_move spreads the row over a wave). Counts are non-negative.
UTTT_HD int match_choose(const int32_t *N, int L, int ply, uint64_t game, uint64_t seed, int sample_plies) {
    if (!match_samples(ply, sample_plies)) return match_first_max(N, L);
    uint32_t T = 0u;
    for (int i = 0; i < L; ++i) T += (uint32_t)N[i];
    if (T == 0u) return match_first_max(N, L);
    const uint64_t x = match_scale(match_draw(seed, game, (uint32_t)ply), T);
    uint64_t acc = 0ull;
    for (int i = 0; i < L; ++i) {
        acc += (uint64_t)(uint32_t)N[i];
        if (acc > x) return i;
    }
    return L - 1;  // unreachable: x < T
}

// Player 0's half-points once `mover` has moved into state ns, or kMatchLive.
UTTT_HD int match_result_after(const uttt_state_t &ns, int mover) {
    if (is_lose(ns)) return mover == 0 ? 2 : 0;
    return is_done(ns) ? 1 : kMatchLive;
}

}  // namespace uttt
