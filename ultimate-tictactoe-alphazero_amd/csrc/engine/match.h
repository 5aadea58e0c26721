// engine/match.h — a match between two players on the device (uttt_match.h): k_match_move plays the
// move a finished search chose in every game of one player's list, k_match_lists rebuilds the two players' lists
// and root arrays and publishes the match's counters. A part of engine.hip's one translation unit, like its
// siblings in engine/, and the last of them: every kernel before it keeps its place in the code object.
#pragma once
#include "evaluators.h"
#include "layout.h"
#include "scan.h"
#include "selfplay.h"
#include "wave.h"
#include "uttt_match.h"

namespace uttt {

struct Match {
    uttt_state_t *state;  // [game] the current position
    int32_t *ply;         // [game] plies played from the start position
    int8_t *action;       // [game][kMaxPlies] the actions played, -1 past the ply
    int8_t *result;       // [game] kMatchLive, or player 0's half-points
    int32_t *list;        // [2][max_games] player p's live games to move, ascending
    uttt_state_t *roots;  // [2][max_games] their positions, in list order: the roots of player p's next search
    int32_t games;
    int32_t max_games;
    int32_t sample_plies;
    uint64_t seed;
};

// One wave per tree of player `player`'s finished search: tree t is game list[player][t]. Entry i of the root's
// visit row (k_root_visits' output) lives in lane i (n0) and lane i - 64 (n1), as in k_move_end; the largest
// count, the sum and the sampled index are wave reductions and one wave prefix sum, all on integers. Lane 0 stores
// the game's new state, action, ply and result. No LDS, no atomics, no scratch.
__global__ __launch_bounds__(kBlock) void k_match_move(Match m, int player, int n_trees,
                                                       const int32_t *__restrict__ visits,
                                                       const int32_t *__restrict__ n_legal) {
    const int lane = lane_id();
    const int t = wave_index();
    if (t >= n_trees) return;
    const int g = m.list[(size_t)player * m.max_games + t];
    if (g < 0 || g >= m.games) return;
    const uttt_state_t s = m.state[g];
    const int ply = m.ply[g];
    uint32_t lm[3];
    legal_mask(s, lm);
    // the search's root is this game's position, so its row has the position's legal count; a row that does not
    // (or a game already over) is left alone rather than played from
    const int L = n_legal[t];
    if (L <= 0 || L != (int)legal_count(s) || ply >= kMaxPlies || m.result[g] != kMatchLive) return;
    const bool h0 = lane < L, h1 = lane + 64 < L;
    const int n0 = h0 ? visits[(size_t)t * 81 + lane] : 0;
    const int n1 = h1 ? visits[(size_t)t * 81 + 64 + lane] : 0;
    // first maximum: the largest count, then the lowest index holding it (counts <= 4095 < 2^23)
    const int kk = wave_max_i(max(h0 ? (n0 << 8) | (255 - lane) : -1, h1 ? (n1 << 8) | (255 - 64 - lane) : -1));
    int idx = kk < 0 ? 0 : 255 - (kk & 0xFF);
    const uint32_t T = (uint32_t)wave_sum_i(n0 + n1);
    if (match_samples(ply, m.sample_plies) && T != 0u) {
        const uint64_t x = match_scale(match_draw(m.seed, (uint64_t)g, (uint32_t)ply), T);  // < T
        // inclusive prefix sums of the row: lanes' n0 first, then n1 behind their total
        int p0 = n0, p1 = n1;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int a = __shfl_up(p0, off), b = __shfl_up(p1, off);
            if (lane >= off) {
                p0 += a;
                p1 += b;
            }
        }
        p1 += __builtin_amdgcn_readlane(p0, 63);
        const uint32_t xs = (uint32_t)x;
        const uint64_t b0 = __ballot(h0 && (uint32_t)p0 > xs), b1 = __ballot(h1 && (uint32_t)p1 > xs);
        idx = b0 ? __builtin_ctzll(b0) : (b1 ? 64 + __builtin_ctzll(b1) : L - 1);
    }
    if (lane == 0) {
        const int a = nth_legal(lm, (uint32_t)idx);
        const uttt_state_t ns = next_state(s, a);
        m.state[g] = ns;
        m.action[(size_t)g * kMaxPlies + ply] = (int8_t)a;
        m.ply[g] = ply + 1;
        m.result[g] = (int8_t)match_result_after(ns, match_player_to_move(g, ply));
    }
}

// One block: the live games in which each player is to move, in ascending game id (a deterministic scan, as
// k_finalize's: thread i takes a contiguous range of games, the block scans the per-thread counts), their
// positions gathered into the players' root arrays, and the counters {list length 0, list length 1, games
// finished, player 0's half-points, games drawn} stored to host (fine-grained pinned) at system scope.
__global__ __launch_bounds__(1024) void k_match_lists(Match m, int64_t *host) {
    __shared__ unsigned long long wsum[32];
    const int tid = threadIdx.x;
    const int per = (m.games + 1023) / 1024;
    const int b = min(tid * per, m.games), e = min(b + per, m.games);
    unsigned long long c0 = 0, c1 = 0, fin = 0, pts = 0, drw = 0;
    for (int g = b; g < e; ++g) {
        const int r = m.result[g];
        if (r == kMatchLive) {
            if (match_player_to_move(g, m.ply[g])) ++c1;
            else ++c0;
        } else {
            ++fin;
            pts += (unsigned long long)r;
            drw += r == 1;
        }
    }
    // the two list positions in 32-bit halves of one scanned word, the three totals in 21-bit fields of the other
    unsigned long long lists = c0 | (c1 << 32), sums = fin | (pts << 21) | (drw << 42), lists_tot, sums_tot;
    block_scan2_1024(lists, sums, &lists_tot, &sums_tot, wsum);
    int at0 = (int)(lists & 0xFFFFFFFFull), at1 = (int)(lists >> 32);
    for (int g = b; g < e; ++g) {
        if (m.result[g] != kMatchLive) continue;
        const int p = match_player_to_move(g, m.ply[g]);
        const size_t at = (size_t)p * m.max_games + (p ? at1++ : at0++);
        m.list[at] = g;
        m.roots[at] = m.state[g];
    }
    if (tid == 0) {
        store_host_i64(host + 0, (int64_t)(lists_tot & 0xFFFFFFFFull));
        store_host_i64(host + 1, (int64_t)(lists_tot >> 32));
        store_host_i64(host + 2, (int64_t)(sums_tot & 0x1FFFFFull));
        store_host_i64(host + 3, (int64_t)((sums_tot >> 21) & 0x1FFFFFull));
        store_host_i64(host + 4, (int64_t)(sums_tot >> 42));
    }
}

}  // namespace uttt
