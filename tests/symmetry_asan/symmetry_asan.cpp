// Host sanitizer program for the board symmetries: uttt_sym_action_perm, uttt_sym_compose, uttt_sym_inverse,
// uttt_states_transform_host and uttt_states_symmetry_host (csrc/rules_api.cpp, csrc/uttt_sym.h) under
// AddressSanitizer + UBSan on a few hundred positions along random games, their terminal positions included.
// Checks what needs no second implementation: the permutations are permutations, the group laws, the transform
// and its inverse give the position back, the rules commute with it, the choice is in range, argument errors.
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
    std::vector<std::vector<int32_t>> perm(UTTT_SYM_COUNT, std::vector<int32_t>(81));
    for (int g = 0; g < UTTT_SYM_COUNT; ++g) {
        if (uttt_sym_action_perm(g, perm[g].data()) != UTTT_OK) ++failures;
        std::vector<int> seen(81, 0);
        for (int a = 0; a < 81; ++a) {
            if (perm[g][a] < 0 || perm[g][a] > 80) {
                ++failures;
                continue;
            }
            seen[perm[g][a]] += 1;
        }
        for (int a = 0; a < 81; ++a)
            if (seen[a] != 1) ++failures;
    }
    for (int g = 0; g < UTTT_SYM_COUNT; ++g) {
        const int inv = uttt_sym_inverse(g);
        if (inv < 0 || inv >= UTTT_SYM_COUNT || uttt_sym_compose(inv, g) != 0 || uttt_sym_compose(g, inv) != 0) ++failures;
        for (int h = 0; h < UTTT_SYM_COUNT; ++h) {
            const int k = uttt_sym_compose(g, h);
            if (k < 0 || k >= UTTT_SYM_COUNT) {
                ++failures;
                continue;
            }
            for (int a = 0; a < 81; ++a)
                if (perm[k][a] != perm[g][perm[h][a]]) ++failures;
        }
    }
    std::vector<int8_t> sym(n), inv(n), choice(n), choice_t(n);
    std::vector<uttt_state_t> t(n), back(n);
    long long moved = 0;
    int used = 0;
    for (int g = 0; g < UTTT_SYM_COUNT; ++g) {
        for (int64_t i = 0; i < n; ++i) {
            sym[i] = (int8_t)((g + i) % UTTT_SYM_COUNT);
            inv[i] = (int8_t)uttt_sym_inverse(sym[i]);
        }
        if (uttt_states_transform_host(pos.data(), n, sym.data(), t.data()) != UTTT_OK) ++failures;
        if (uttt_states_transform_host(t.data(), n, inv.data(), back.data()) != UTTT_OK) ++failures;
        for (int64_t i = 0; i < n; ++i) {
            if (std::memcmp(&back[i], &pos[i], sizeof(uttt_state_t)) != 0) ++failures;
            moved += std::memcmp(&t[i], &pos[i], sizeof(uttt_state_t)) != 0;
            if (uttt_state_is_done(&t[i]) != uttt_state_is_done(&pos[i]) ||
                uttt_state_is_lose(&t[i]) != uttt_state_is_lose(&pos[i]))
                ++failures;
            int32_t la[81], lb[81];
            const int na = uttt_state_legal_actions(&pos[i], la), nb = uttt_state_legal_actions(&t[i], lb);
            if (na != nb) {
                ++failures;
                continue;
            }
            std::vector<int> want(81, 0);
            for (int j = 0; j < na; ++j) want[perm[sym[i]][la[j]]] = 1;
            for (int j = 0; j < nb; ++j)
                if (!want[lb[j]]) ++failures;
        }
    }
    // in place: out may be states
    back = pos;
    for (int64_t i = 0; i < n; ++i) sym[i] = 5;
    if (uttt_states_transform_host(back.data(), n, sym.data(), back.data()) != UTTT_OK) ++failures;
    if (uttt_states_transform_host(pos.data(), n, sym.data(), t.data()) != UTTT_OK) ++failures;
    if (std::memcmp(back.data(), t.data(), sizeof(uttt_state_t) * (size_t)n) != 0) ++failures;
    if (uttt_states_symmetry_host(pos.data(), n, 7, choice.data()) != UTTT_OK) ++failures;
    if (uttt_states_symmetry_host(pos.data(), n, ~0ull, choice_t.data()) != UTTT_OK) ++failures;
    for (int64_t i = 0; i < n; ++i) {
        if (choice[i] < 0 || choice[i] >= UTTT_SYM_COUNT || choice_t[i] < 0 || choice_t[i] >= UTTT_SYM_COUNT) ++failures;
        else used |= 1 << choice[i];
    }
    if (used != 0xFF) ++failures;
    if (moved == 0) ++failures;
    int32_t p81[81];
    if (uttt_sym_action_perm(8, p81) != UTTT_ERR_ARG || uttt_sym_action_perm(-1, p81) != UTTT_ERR_ARG) ++failures;
    if (uttt_sym_action_perm(0, nullptr) != UTTT_ERR_ARG) ++failures;
    if (uttt_sym_compose(0, 8) != UTTT_ERR_ARG || uttt_sym_compose(-1, 0) != UTTT_ERR_ARG) ++failures;
    if (uttt_sym_inverse(8) != UTTT_ERR_ARG) ++failures;
    if (uttt_states_transform_host(nullptr, 1, sym.data(), t.data()) != UTTT_ERR_ARG) ++failures;
    if (uttt_states_transform_host(pos.data(), 1, nullptr, t.data()) != UTTT_ERR_ARG) ++failures;
    if (uttt_states_transform_host(nullptr, 0, nullptr, nullptr) != UTTT_OK) ++failures;
    if (uttt_states_symmetry_host(pos.data(), -1, 0, choice.data()) != UTTT_ERR_ARG) ++failures;
    if (uttt_states_symmetry_host(pos.data(), 1, 0, nullptr) != UTTT_ERR_ARG) ++failures;
    sym[0] = 8;
    if (uttt_states_transform_host(pos.data(), 1, sym.data(), t.data()) != UTTT_ERR_ARG) ++failures;
    sym[0] = -1;
    if (uttt_states_transform_host(pos.data(), 1, sym.data(), t.data()) != UTTT_ERR_ARG) ++failures;
    uttt_state_t bad = pos[0];
    bad.active = 40;
    sym[0] = 1;
    if (uttt_states_transform_host(&bad, 1, sym.data(), t.data()) != UTTT_ERR_ARG) ++failures;
    if (uttt_states_symmetry_host(&bad, 1, 0, choice.data()) != UTTT_ERR_ARG) ++failures;
    std::printf("symmetry_asan: %lld positions, %lld transformed states differ from their source, %d failures\n",
                (long long)n, moved, failures);
    return failures ? 1 : 0;
}
