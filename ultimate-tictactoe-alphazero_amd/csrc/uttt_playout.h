// uttt_playout.h — uniformly random playouts (game.py:277-287 `playout`) on the packed bitboards,
// compiled for both the host (uttt_playout_host, the checker's counterpart) and gfx950 (k_playout_leaves,
// k_playout_states). Python's global `random` is replaced by a counter-based draw, so a playout is a pure
// function of (position, seed, playout index): the same on host and device, however playouts are laid over
// lanes, and exact under the evaluation cache (DESIGN.md "Playout evaluator").
//
// Key: h = hash_words(w) ^ mix64(seed), w the four words of the position's 243 network-input bits (own,
// opponent, legal; bit j = ch * 81 + R * 9 + C), the words k_hash_eval and hash_leaf_row form. Two states with
// the same stones and the same legal moves (active == -1 against active == b when only board b is open) have
// the same key and, since next_state never reads `active`, the same playouts.
#pragma once

#include "uttt_bits.h"

namespace uttt {

constexpr int kMaxPlayouts = 4096;  // per position and call (uttt_playout_host, uttt_playouts, uttt_eval_playout_dev)

// The input words of one state, bit by bit (the host's form; a wave forms them with four ballots).
UTTT_HD void input_words(const uttt_state_t &s, uint64_t w[4]) {
    uint32_t m[3];
    legal_mask(s, m);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint64_t x = 0ull;
        for (int l = 0; l < 64; ++l) {
            const int j = i * 64 + l;
            if (j >= 243) break;
            const int ch = j / 81, a = action_at(j % 81);
            const uint32_t on = ch == 0 ? bit_of(s.own, a) : (ch == 1 ? bit_of(s.opp, a) : bit_of(m, a));
            x |= (uint64_t)on << l;
        }
        w[i] = x;
    }
}

UTTT_HD uint64_t playout_key(const uint64_t w[4], uint64_t seed) { return hash_words(w) ^ mix64(seed); }

// Position of the k-th (from 0) set bit of a 27-bit word holding more than k: a binary search on popcounts.
UTTT_HD uint32_t nth_bit27(uint32_t x, uint32_t k) {
    uint32_t pos = 0u, c;
    c = popc32(x & 0xFFFFu);
    if (k >= c) { k -= c; x >>= 16; pos += 16u; }
    c = popc32(x & 0xFFu);
    if (k >= c) { k -= c; x >>= 8; pos += 8u; }
    c = popc32(x & 0xFu);
    if (k >= c) { k -= c; x >>= 4; pos += 4u; }
    c = popc32(x & 0x3u);
    if (k >= c) { k -= c; x >>= 2; pos += 2u; }
    if (k >= (x & 1u)) pos += 1u;
    return pos;
}

// The idx-th legal action in ascending action order (idx < |legal|): the word from the popcounts, chosen by
// selects, not a dynamic index into m (which puts it in scratch on the device; uttt_bits.h next_state, bit_of).
UTTT_HD int nth_legal(const uint32_t m[3], uint32_t idx) {
    const uint32_t c0 = popc32(m[0]), c1 = popc32(m[1]);
    const int w = idx < c0 ? 0 : (idx < c0 + c1 ? 1 : 2);
    const uint32_t x = w == 0 ? m[0] : (w == 1 ? m[1] : m[2]);
    const uint32_t k = idx - (w == 0 ? 0u : (w == 1 ? c0 : c0 + c1));
    return 27 * w + (int)nth_bit27(x, k);
}

// Playout j of the position with key h from state s (game.py:277-287: a lost state is -1 for its side to
// move, a drawn one 0, else minus the playout of a random legal move's successor; iterated here, the sign
// carried): +1 / 0 / -1 from the side to move in s. Every ply fills an empty cell, so the loop ends within 81
// plies (the bound is never reached) and ply + 1 < 128 keeps the draws of different playouts apart.
UTTT_HD int playout(uttt_state_t s, uint64_t h, uint32_t j) {
    int sign = 1;
    for (uint32_t ply = 0u; ply < 82u; ++ply) {
        if (is_lose(s)) return -sign;
        uint32_t m[3];
        legal_mask(s, m);
        const uint32_t L = popc32(m[0]) + popc32(m[1]) + popc32(m[2]);
        if (L == 0u) return 0;
        const uint64_t r = mix64(h + (uint64_t)(j * 128u + ply + 1u) * kGold);
        const uint32_t idx = (uint32_t)(((r >> 32) * L) >> 32);
        s = next_state(s, nth_legal(m, idx));
        sign = -sign;
    }
    return 0;
}

// A leaf's value from its P playouts' sum S (wins - losses): one correctly rounded divide.
UTTT_HD float playout_value(int32_t S, int32_t P) { return (float)S / (float)P; }

}  // namespace uttt
