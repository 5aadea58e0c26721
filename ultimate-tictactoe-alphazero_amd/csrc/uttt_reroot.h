// uttt_reroot.h — tree reuse on the host: the plain C++ mirror of k_reroot (engine/reroot.h). One
// tree's records in, the re-rooted tree's records out, in the canonical breadth-first layout the kernel writes,
// bit for bit. Host only (rules_api.cpp, uttt_reroot_host): it states the record's bit fields itself, since
// engine/layout.h belongs to the device's translation unit; engine/reroot.h asserts that the two agree.
#pragma once
#include <cstdint>
#include <cstring>

#include "uttt_bits.h"
#include "uttt_engine.h"

namespace uttt {
namespace reroot {

// a record is four words: W (f32 bits), P (f32 bits), meta = N (0-15) | action (16-22) | L (23-29) | 2 flags,
// link = first child (0-19) | k (20-31)
constexpr uint32_t kNoAct = 0x7Fu;
inline int rec_n(uint32_t meta) { return (int)(meta & 0xFFFFu); }
inline int rec_action(uint32_t meta) { return (int)((meta >> 16) & 0x7Fu); }
inline int rec_L(uint32_t meta) { return (int)((meta >> 23) & 0x7Fu); }
inline int rec_first(uint32_t link) { return (int)(link & 0xFFFFFu); }
inline int rec_k(uint32_t link) { return (int)(link >> 20); }
inline uint32_t pack_meta(uint32_t n, uint32_t action, uint32_t L) { return (n & 0xFFFFu) | ((action & 0x7Fu) << 16) | ((L & 0x7Fu) << 23); }
inline uint32_t pack_link(uint32_t first, uint32_t k) { return (first & 0xFFFFFu) | (k << 20); }

inline float as_f32(uint32_t b) {
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}
inline uint32_t as_u32(float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}

// A fresh root of state s (init_root): uniform priors 1.0f / L over the legal moves in ascending order.
inline int fresh_root(const uttt_state_t &s, uint32_t *out) {
    uint32_t m[3];
    legal_mask(s, m);
    const int L = (int)legal_count(s);
    const float up = L ? 1.0f / (float)L : 0.0f;
    out[0] = 0u;
    out[1] = 0u;
    out[2] = pack_meta(0u, kNoAct, (uint32_t)L);
    out[3] = pack_link(L ? 1u : 0u, L ? 1u : 0u);
    int r = 0;
    for (int a = 0; a < 81; ++a) {
        if (!bit_of(m, a)) continue;
        uint32_t *o = out + 4 * (size_t)(1 + r++);
        o[0] = 0u;
        o[1] = as_u32(up);
        o[2] = pack_meta(0u, (uint32_t)a, 0u);
        o[3] = 0u;
    }
    return 1 + L;
}

// rec: node_count records of a C++-semantics tree whose root's state is `state`; out: room for
// max(node_count, 82) records. Returns the new tree's node count, or -1 for an action that is not a move of the
// root, or a tree whose indices do not fit node_count (nothing a search produces).
inline int reroot_tree(const uint32_t *rec, int node_count, const uttt_state_t &state, int action, uint32_t *out) {
    const int out_cap = node_count > 82 ? node_count : 82;
    if (node_count < 1 || action < 0 || action > 80) return -1;
    const int L0 = rec_L(rec[2]), f0 = rec_first(rec[3]);
    if (f0 + L0 > node_count) return -1;
    int ci = -1;
    for (int i = 0; i < L0; ++i)
        if (rec_action(rec[4 * (size_t)(f0 + i) + 2]) == action) {
            ci = f0 + i;
            break;
        }
    if (ci < 0) return -1;
    const uint32_t *c = rec + 4 * (size_t)ci;
    const uttt_state_t ns = next_state(state, action);
    const int kc = rec_k(c[3]), Lp = rec_L(c[2]), fc = rec_first(c[3]);
    if (kc == 0 || Lp == 0) return fresh_root(ns, out);  // never expanded, or terminal
    if ((int)legal_count(ns) != Lp || (int64_t)fc + (int64_t)kc * Lp > node_count) return -1;
    // the new root: c's visits less the k_c its own expansion counted, which is the sum of its children's
    out[0] = c[0];  // W as c's: nothing reads a root's W
    out[1] = 0u;
    out[2] = pack_meta((uint32_t)(rec_n(c[2]) - kc), kNoAct, (uint32_t)Lp);
    out[3] = pack_link(1u, 1u);
    // level 1: the k_c duplicates of each move merged into one child, whose blocks follow level 1 move by move
    int alloc = 1 + Lp;
    for (int r = 0; r < Lp; ++r) {
        uint32_t n = 0u, ks = 0u, Lc = 0u, w = 0u, p = 0u, act = 0u;
        for (int i = 0; i < kc; ++i) {
            const uint32_t *d = rec + 4 * (size_t)(fc + i * Lp + r);
            if (i == 0) {
                w = d[0];
                p = d[1];
                act = (uint32_t)rec_action(d[2]);
            } else {
                w = as_u32(as_f32(w) + as_f32(d[0]));
            }
            n += (uint32_t)rec_n(d[2]);
            ks += (uint32_t)rec_k(d[3]);
            if ((uint32_t)rec_L(d[2]) > Lc) Lc = (uint32_t)rec_L(d[2]);
        }
        uint32_t *o = out + 4 * (size_t)(1 + r);
        o[0] = w;
        o[1] = p;
        o[2] = pack_meta(n, act, Lc);
        o[3] = pack_link(ks ? (uint32_t)alloc : 0u, ks);
        alloc += (int)(ks * Lc);
        if (alloc > out_cap) return -1;
    }
    // level 2: the duplicates' child blocks, move by move and copy by copy; the copied records keep their link
    // into `rec` until the scan below reaches them
    int at = 1 + Lp;
    for (int r = 0; r < Lp; ++r)
        for (int i = 0; i < kc; ++i) {
            const uint32_t *d = rec + 4 * (size_t)(fc + i * Lp + r);
            const int cnt = rec_k(d[3]) * rec_L(d[2]), sf = rec_first(d[3]);
            if (cnt == 0) continue;
            if (sf + cnt > node_count || at + cnt > out_cap) return -1;
            std::memcpy(out + 4 * (size_t)at, rec + 4 * (size_t)sf, 16 * (size_t)cnt);
            at += cnt;
        }
    // the rest (Cheney): `out` is the queue; a record's block goes to the end, and its link is re-based
    for (int q = 1 + Lp; q < at; ++q) {
        uint32_t *o = out + 4 * (size_t)q;
        const int cnt = rec_k(o[3]) * rec_L(o[2]), sf = rec_first(o[3]);
        if (cnt == 0) continue;
        if (sf + cnt > node_count || at + cnt > out_cap) return -1;
        std::memcpy(out + 4 * (size_t)at, rec + 4 * (size_t)sf, 16 * (size_t)cnt);
        o[3] = pack_link((uint32_t)at, (uint32_t)rec_k(o[3]));
        at += cnt;
    }
    return at;
}

}  // namespace reroot
}  // namespace uttt
