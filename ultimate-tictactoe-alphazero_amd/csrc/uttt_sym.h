// uttt_sym.h — the eight symmetries of the square on the packed bitboards, compiled for both the host
// (uttt_states_transform_host, uttt_states_symmetry_host: the checker's counterparts) and gfx950 (k_sym_leaves,
// k_sym_rows). DESIGN.md §6e.
//
// Symmetry g = r + 4 f (r in 0..3 quarter turns, f in 0..1 a mirror first): on the 9x9 image it is
// np.rot90(np.fliplr(img) if f else img, k = r). One quarter turn takes the cell at (R, C) to (n - 1 - C, R),
// the mirror takes it to (R, n - 1 - C). An image row or column is 3 * (board coordinate) + (cell coordinate) and
// 8 - (3 B + c) = 3 (2 - B) + (2 - c), so the image transform acts on the board index and on the cell index by
// the same map beta_g of a 3x3 index 3 R + C, and action a = 9 b + c goes to pi_g(a) = 9 beta_g(b) + beta_g(c).
//
// The state transform T_g moves bit a of own / opp to bit pi_g(a), bit b of each half of mains to bit beta_g(b)
// and the active board to beta_g(active) (-1 stays). The rules commute with it: legal(T_g s) = pi_g(legal(s)),
// next(T_g s, pi_g(a)) = T_g(next(s, a)); win9 is invariant under beta_g.
//
// Everything is shifts and selects on values: no local array under a dynamic index (which the device compiler
// places in scratch; uttt_bits.h next_state, bit_of).
#pragma once

#include "uttt_bits.h"
#include "uttt_playout.h"

namespace uttt {

constexpr int kSymCount = 8;

// beta_g(i) for a 3x3 index i = 3 R + C.
UTTT_HD int sym_beta(int g, int i) {
    int R = div3(i), C = i - 3 * R;
    if (g & 4) C = 2 - C;
    const int r = g & 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int nR = 2 - C, nC = R;
        R = k < r ? nR : R;
        C = k < r ? nC : C;
    }
    return 3 * R + C;
}

// pi_g(a) for an action a = 9 b + c.
UTTT_HD int sym_action(int g, int a) {
    const int b = div9(a), c = a - 9 * b;
    return 9 * sym_beta(g, b) + sym_beta(g, c);
}

// Three 9-bit boards of a 27-bit word at once (a lone 9-bit mask is the word's low board): the mirror swaps
// columns 0 and 2; a quarter turn is the transpose (bits 1<->3, 2<->6, 5<->7) followed by the swap of rows 0
// and 2, since (R, C) -> (C, R) -> (2 - C, R).
constexpr uint32_t kRep3 = 1u | (1u << 9) | (1u << 18);
UTTT_HD uint32_t sym_mirror27(uint32_t m) {
    return ((m & (0x049u * kRep3)) << 2) | ((m & (0x124u * kRep3)) >> 2) | (m & (0x092u * kRep3));
}
UTTT_HD uint32_t sym_turn27(uint32_t m) {
    const uint32_t t = (m & (0x111u * kRep3)) | ((m & (0x022u * kRep3)) << 2) | ((m & (0x088u * kRep3)) >> 2) |
                       ((m & (0x004u * kRep3)) << 4) | ((m & (0x040u * kRep3)) >> 4);
    return ((t & (0x007u * kRep3)) << 6) | ((t & (0x1C0u * kRep3)) >> 6) | (t & (0x038u * kRep3));
}
// Bit beta_g(i) of the result is bit i of m, within each 9-bit board of the word.
UTTT_HD uint32_t sym_cells27(int g, uint32_t m) {
    m = (g & 4) ? sym_mirror27(m) : m;
    const int r = g & 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) m = k < r ? sym_turn27(m) : m;
    return m;
}

// The 81 bits of own or opp: the cells turn within every board, then board b's nine cells go to board beta_g(b).
UTTT_HD void sym_boards(int g, const uint32_t in[3], uint32_t out[3]) {
    uint32_t o0 = 0u, o1 = 0u, o2 = 0u;
#pragma unroll
    for (int w = 0; w < 3; ++w) {
        const uint32_t t = sym_cells27(g, in[w]);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int db = sym_beta(g, 3 * w + j), dw = div3(db);
            const uint32_t v = ((t >> (9 * j)) & kCells) << (9 * (db - 3 * dw));
            o0 |= dw == 0 ? v : 0u;
            o1 |= dw == 1 ? v : 0u;
            o2 |= dw == 2 ? v : 0u;
        }
    }
    out[0] = o0;
    out[1] = o1;
    out[2] = o2;
}

// T_g(s).
UTTT_HD uttt_state_t sym_state(const uttt_state_t &s, int g) {
    uttt_state_t t;
    sym_boards(g, s.own, t.own);
    sym_boards(g, s.opp, t.opp);
    t.mains = sym_cells27(g, main_own(s)) | (sym_cells27(g, main_opp(s)) << 16);
    t.active = s.active < 0 ? s.active : sym_beta(g, s.active);
    return t;
}

// The symmetry with T_k = T_g T_h (h first): pi_k = pi_g o pi_h. A symmetry is known by where it takes the
// 3x3 indices 0 and 1.
UTTT_HD int sym_compose(int g, int h) {
    const int i0 = sym_beta(g, sym_beta(h, 0)), i1 = sym_beta(g, sym_beta(h, 1));
    int k = 0;
#pragma unroll
    for (int c = 0; c < kSymCount; ++c) k = (sym_beta(c, 0) == i0 && sym_beta(c, 1) == i1) ? c : k;
    return k;
}
UTTT_HD int sym_inverse(int g) {
    int k = 0;
#pragma unroll
    for (int c = 0; c < kSymCount; ++c) k = sym_compose(c, g) == 0 ? c : k;
    return k;
}

// The hashed choice: the top three bits of the playout key of the position's 243 input bits (w) and the seed, so
// a function of the stones, the legal moves and the seed alone.
UTTT_HD int sym_of_key(const uint64_t w[4], uint64_t seed) { return (int)(playout_key(w, seed) >> 61); }

}  // namespace uttt
