// rules_api.cpp — host side of the C ABI: one position at a time, the value
// type behind `uttt_cpp.State` (cpp/python_bindings.cpp:53-74). Same bitboard
// code the kernels use (uttt_bits.h).
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

#include "uttt_bits.h"
#include "uttt_engine.h"
#include "uttt_match.h"
#include "uttt_noise.h"
#include "uttt_reroot.h"
#include "uttt_playout.h"
#include "uttt_solve.h"
#include "uttt_sym.h"

namespace uttt {
// Last error of the calling thread, for every entry point of the C ABI (uttt_last_error).
// Kept in this host-only file so the rules build on their own (tests/asan).
static thread_local std::string g_err;

void set_error(const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
}

// The argument checks uttt_solve_host and uttt_solve share.
int solve_check_args(const char *who, const uttt_state_t *states, int64_t n, int32_t max_nodes) {
    if (n < 0 || n > kSolveMaxStates || (!states && n > 0)) {
        set_error("%s: null states, or a count outside 0..%lld", who, (long long)kSolveMaxStates);
        return UTTT_ERR_ARG;
    }
    if (max_nodes < 1 || max_nodes > kSolveMaxNodes) {
        set_error("max_nodes must be 1..%d (got %d)", kSolveMaxNodes, max_nodes);
        return UTTT_ERR_ARG;
    }
    for (int64_t i = 0; i < n; ++i) {
        if (states[i].active < -1 || states[i].active > 8) {
            set_error("active_board must be -1..8 (state %lld has %d)", (long long)i, states[i].active);
            return UTTT_ERR_ARG;
        }
    }
    return UTTT_OK;
}

// The argument checks uttt_root_noise_host and uttt_engine_set_root_noise share.
int noise_check_args(const char *who, float epsilon, float alpha) {
    if (!(epsilon >= 0.0f && epsilon <= 1.0f)) {
        set_error("%s: epsilon must be in [0, 1] (got %g)", who, (double)epsilon);
        return UTTT_ERR_ARG;
    }
    if (!(alpha >= kNoiseAlphaMin && alpha <= kNoiseAlphaMax)) {
        set_error("%s: alpha must be in [1/32, 32] (got %g)", who, (double)alpha);
        return UTTT_ERR_ARG;
    }
    return UTTT_OK;
}

// The argument checks uttt_solve_overlay_host and uttt_eval_solve_dev share (beside solve_check_args /
// the engine's own).
int overlay_check_args(const char *who, int32_t max_empties, int32_t max_nodes, int32_t priors, const float *policy,
                       int64_t policy_ld, const float *value, int64_t value_ld) {
    if (!policy || !value) {
        set_error("%s: null policy or value", who);
        return UTTT_ERR_ARG;
    }
    if (max_empties < 0 || max_empties > kSolveMaxEmpty) {
        set_error("max_empties must be 0..%d (got %d)", kSolveMaxEmpty, max_empties);
        return UTTT_ERR_ARG;
    }
    if (max_nodes < 1 || max_nodes > kSolveMaxNodes) {
        set_error("max_nodes must be 1..%d (got %d)", kSolveMaxNodes, max_nodes);
        return UTTT_ERR_ARG;
    }
    if (priors != UTTT_PRIORS_KEEP && priors != UTTT_PRIORS_OPTIMAL) {
        set_error("priors must be UTTT_PRIORS_KEEP (0) or UTTT_PRIORS_OPTIMAL (1) (got %d)", priors);
        return UTTT_ERR_ARG;
    }
    if (policy_ld < 81) {
        set_error("policy_ld must be at least 81 (got %lld)", (long long)policy_ld);
        return UTTT_ERR_ARG;
    }
    if (value_ld < 1) {
        set_error("value_ld must be at least 1 (got %lld)", (long long)value_ld);
        return UTTT_ERR_ARG;
    }
    return UTTT_OK;
}
}  // namespace uttt

using namespace uttt;

extern "C" {

const char *uttt_last_error(void) { return g_err.c_str(); }

void uttt_state_initial(uttt_state_t *out) {
    std::memset(out, 0, sizeof(*out));
    out->active = -1;
}

int uttt_state_from_arrays(const int32_t pieces[81], const int32_t enemy[81], const int32_t main_p[9],
                           const int32_t main_e[9], int32_t active, uttt_state_t *out) {
    if (!pieces || !enemy || !main_p || !main_e || !out) {
        set_error("uttt_state_from_arrays: null pointer");
        return UTTT_ERR_ARG;
    }
    if (active < -1 || active > 8) {
        set_error("active_board must be -1..8 (got %d)", active);
        return UTTT_ERR_ARG;
    }
    uttt_state_t s;
    std::memset(&s, 0, sizeof(s));
    for (int a = 0; a < 81; ++a) {
        if ((uint32_t)pieces[a] > 1u || (uint32_t)enemy[a] > 1u) {
            set_error("pieces/enemy_pieces cells must be 0 or 1 (board %d cell %d)", a / 9, a % 9);
            return UTTT_ERR_ARG;
        }
        s.own[a / 27] |= (uint32_t)pieces[a] << (a % 27);
        s.opp[a / 27] |= (uint32_t)enemy[a] << (a % 27);
    }
    for (int b = 0; b < 9; ++b) {
        if ((uint32_t)main_p[b] > 1u || (uint32_t)main_e[b] > 1u) {
            set_error("main board entries must be 0 or 1 (board %d)", b);
            return UTTT_ERR_ARG;
        }
        s.mains |= ((uint32_t)main_p[b] << b) | ((uint32_t)main_e[b] << (16 + b));
    }
    s.active = active;
    *out = s;
    return UTTT_OK;
}

void uttt_state_to_arrays(const uttt_state_t *s, int32_t pieces[81], int32_t enemy[81], int32_t main_p[9],
                          int32_t main_e[9], int32_t *active) {
    for (int a = 0; a < 81; ++a) {
        if (pieces) pieces[a] = (int32_t)bit_of(s->own, a);
        if (enemy) enemy[a] = (int32_t)bit_of(s->opp, a);
    }
    for (int b = 0; b < 9; ++b) {
        if (main_p) main_p[b] = (int32_t)((s->mains >> b) & 1u);
        if (main_e) main_e[b] = (int32_t)((s->mains >> (16 + b)) & 1u);
    }
    if (active) *active = s->active;
}

int uttt_state_next(const uttt_state_t *s, int32_t action, uttt_state_t *out) {
    if (action < 0 || action > 80) {
        set_error("action must be 0..80 (got %d)", action);
        return UTTT_ERR_ARG;
    }
    *out = next_state(*s, action);
    return UTTT_OK;
}

int uttt_state_legal_actions(const uttt_state_t *s, int32_t out[81]) {
    uint32_t m[3];
    legal_mask(*s, m);
    int n = 0;
    for (int w = 0; w < 3; ++w)
        for (uint32_t bits = m[w]; bits; bits &= bits - 1u) out[n++] = 27 * w + __builtin_ctz(bits);
    return n;
}

int uttt_state_is_lose(const uttt_state_t *s) { return is_lose(*s) ? 1 : 0; }
int uttt_state_is_draw(const uttt_state_t *s) { return (!is_lose(*s) && legal_count(*s) == 0u) ? 1 : 0; }
int uttt_state_is_done(const uttt_state_t *s) { return is_done(*s) ? 1 : 0; }
int uttt_state_is_first_player(const uttt_state_t *s) { return is_first_player(*s) ? 1 : 0; }

void uttt_state_input_hwc(const uttt_state_t *s, float out[243]) {
    uint32_t m[3];
    legal_mask(*s, m);
    for (int a = 0; a < 81; ++a) {
        const int pos = image_index(a);
        out[pos * 3 + 0] = bit_of(s->own, a) ? 1.0f : 0.0f;
        out[pos * 3 + 1] = bit_of(s->opp, a) ? 1.0f : 0.0f;
        out[pos * 3 + 2] = bit_of(m, a) ? 1.0f : 0.0f;
    }
}

int uttt_states_input_hwc(const uttt_state_t *s, int64_t n, float *out) {
    if ((!s || !out) && n > 0) {
        set_error("uttt_states_input_hwc: null pointer");
        return UTTT_ERR_ARG;
    }
    for (int64_t i = 0; i < n; ++i) uttt_state_input_hwc(s + i, out + 243 * i);
    return UTTT_OK;
}

int uttt_state_to_string(const uttt_state_t *s, char *buf, int32_t cap) {
    // Layout of cpp/uttt_game.cpp:194-241 (board rows, main-board status, side, active board).
    const char *ox = is_first_player(*s) ? "ox" : "xo";
    std::string o;
    o.reserve(512);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) {
            for (int i = 0; i < 3; ++i) {
                const int b = r * 3 + i;
                for (int j = 0; j < 3; ++j) {
                    const int a = b * 9 + c * 3 + j;
                    o += bit_of(s->own, a) ? ox[0] : (bit_of(s->opp, a) ? ox[1] : '-');
                    o += ' ';
                }
                if (i < 2) o += "| ";
            }
            o += '\n';
        }
        if (r < 2) o += "---------------------\n";
    }
    o += "\nMain Board Status:\n";
    for (int b = 0; b < 9; ++b) {
        const bool mp = (s->mains >> b) & 1u, me = (s->mains >> (16 + b)) & 1u;
        o += (mp && me) ? 'D' : (mp ? ox[0] : (me ? ox[1] : '.'));
        if (b % 3 == 2) o += '\n';
    }
    o += "Next Player: ";
    o += ox[0];
    o += "\nActive Board: ";
    o += (s->active == -1) ? std::string("Any") : std::to_string(s->active);
    o += '\n';
    const int n = (int)o.size();
    if (!buf || n + 1 > cap) return -(n + 1);
    std::memcpy(buf, o.c_str(), (size_t)n + 1);
    return n;
}

int uttt_boltzman(const float *xs, int32_t n, float temperature, float *out) {
    // cpp/uttt_mcts.cpp:199-216: powf(x, 1/t), sequential f32 sum, divide if sum > 0.
    float sum = 0.0f;
    const float inv = 1.0f / temperature;
    for (int i = 0; i < n; ++i) {
        out[i] = std::pow(xs[i], inv);
        sum += out[i];
    }
    if (sum > 0)
        for (int i = 0; i < n; ++i) out[i] /= sum;
    return n;
}

int uttt_playout_host(const uttt_state_t *states, int64_t n, int32_t playouts, uint64_t seed, int32_t *wins,
                      int32_t *losses) {
    // game.py:277-287 with the counter-based draw of uttt_playout.h; what k_playout_states computes.
    if (n < 0 || ((!states || !wins || !losses) && n > 0)) {
        set_error("uttt_playout_host: null pointer or negative count");
        return UTTT_ERR_ARG;
    }
    if (playouts < 1 || playouts > kMaxPlayouts) {
        set_error("playouts must be 1..%d (got %d)", kMaxPlayouts, playouts);
        return UTTT_ERR_ARG;
    }
    for (int64_t i = 0; i < n; ++i) {
        if (states[i].active < -1 || states[i].active > 8) {
            set_error("active_board must be -1..8 (state %lld has %d)", (long long)i, states[i].active);
            return UTTT_ERR_ARG;
        }
    }
    for (int64_t i = 0; i < n; ++i) {
        uint64_t w[4];
        input_words(states[i], w);
        const uint64_t h = playout_key(w, seed);
        int32_t nw = 0, nl = 0;
        for (int32_t j = 0; j < playouts; ++j) {
            const int r = playout(states[i], h, (uint32_t)j);
            nw += r > 0;
            nl += r < 0;
        }
        wins[i] = nw;
        losses[i] = nl;
    }
    return UTTT_OK;
}

namespace {
struct HostStack {  // the host's frames: a local array (the device's are LDS)
    uint32_t f[kSolveMaxEmpty];
    uint32_t load(int d) const { return f[d]; }
    void store(int d, uint32_t x) { f[d] = x; }
};
}  // namespace

namespace {
// One position as uttt_solve.h defines it, the lanes one after another; av: its 81 action values. Returns
// false when the root answered without a search (terminal or too large).
bool solve_one(const uttt_state_t &s, int32_t max_nodes, int8_t av[81], int8_t &st, int8_t &val, int8_t &act,
               int64_t &total) {
    uint32_t m[3];
    legal_mask(s, m);
    std::memset(av, UTTT_SOLVE_UNKNOWN, 81);
    act = -1;
    total = 0;
    if (solve_root(s, m, st, val)) return false;
    bool every = true;
    int best = -2, best_a = -1;  // the lowest move that reaches the largest known value
    for (int a = next_legal_after(m, -1); a >= 0; a = next_legal_after(m, a)) {
        SolveLane ln;
        HostStack stack;
        solve_lane_begin(ln, next_state(s, a));
        while (ln.live) solve_step(ln, stack, max_nodes);
        total += ln.nodes;
        if (!ln.solved) {
            every = false;
            continue;
        }
        av[a] = (int8_t)-ln.v;
        if (av[a] > best) {
            best = av[a];
            best_a = a;
        }
    }
    if (solve_result(best, every, st, val)) act = (int8_t)best_a;
    return true;
}
}  // namespace

int uttt_solve_host(const uttt_state_t *states, int64_t n, int32_t max_nodes, int8_t *value, int8_t *action,
                    int8_t *status, int64_t *nodes, int8_t *action_values) {
    // game.py:240-274 as uttt_solve.h defines it; what k_solve_states computes.
    if (int rc = solve_check_args("uttt_solve_host", states, n, max_nodes)) return rc;
    for (int64_t i = 0; i < n; ++i) {
        int8_t av[81], st, val, act;
        int64_t total;
        solve_one(states[i], max_nodes, av, st, val, act, total);
        if (value) value[i] = val;
        if (action) action[i] = act;
        if (status) status[i] = st;
        if (nodes) nodes[i] = total;
        if (action_values) std::memcpy(action_values + i * 81, av, sizeof(av));
    }
    return UTTT_OK;
}

int uttt_solve_overlay_host(const uttt_state_t *states, int64_t n, int32_t max_empties, int32_t max_nodes,
                            int32_t priors, float *policy, int64_t policy_ld, float *value, int64_t value_ld,
                            int8_t *status) {
    // The overlay of uttt_solve.h over n caller-filled rows; what k_solve_leaves computes.
    if (int rc = solve_check_args("uttt_solve_overlay_host", states, n, max_nodes)) return rc;
    if (int rc = overlay_check_args("uttt_solve_overlay_host", max_empties, max_nodes, priors, policy, policy_ld,
                                    value, value_ld))
        return rc;
    for (int64_t i = 0; i < n; ++i) {
        const uttt_state_t &s = states[i];
        int8_t st = UTTT_OVERLAY_SKIPPED;
        if (!overlay_skips(s, max_empties)) {
            int8_t av[81], val, act;
            int64_t total;
            const bool searched = solve_one(s, max_nodes, av, st, val, act, total);
            if (st == UTTT_SOLVE_SOLVED) {
                value[i * value_ld] = (float)val;
                if (searched && priors == UTTT_PRIORS_OPTIMAL) {
                    uint32_t m[3];
                    legal_mask(s, m);
                    float *row = policy + i * policy_ld;
                    for (int a = 0; a < 81; ++a) row[a] = overlay_prior(bit_of(m, a) != 0u, av[a], val);
                }
            }
        }
        if (status) status[i] = st;
    }
    return UTTT_OK;
}

static int check_sym(const char *who, int32_t g) {
    if (g < 0 || g >= kSymCount) {
        set_error("%s: a symmetry must be 0..%d (got %d)", who, kSymCount - 1, g);
        return UTTT_ERR_ARG;
    }
    return UTTT_OK;
}

int uttt_sym_action_perm(int32_t g, int32_t out[81]) {
    if (int rc = check_sym("uttt_sym_action_perm", g)) return rc;
    if (!out) {
        set_error("uttt_sym_action_perm: null pointer");
        return UTTT_ERR_ARG;
    }
    for (int a = 0; a < 81; ++a) out[a] = sym_action(g, a);
    return UTTT_OK;
}

int uttt_sym_compose(int32_t g, int32_t h) {
    if (int rc = check_sym("uttt_sym_compose", g)) return rc;
    if (int rc = check_sym("uttt_sym_compose", h)) return rc;
    return sym_compose(g, h);
}

int uttt_sym_inverse(int32_t g) {
    if (int rc = check_sym("uttt_sym_inverse", g)) return rc;
    return sym_inverse(g);
}

static int check_sym_states(const char *who, const uttt_state_t *states, int64_t n, const void *a, const void *b) {
    if (n < 0 || ((!states || !a || !b) && n > 0)) {
        set_error("%s: null pointer or negative count", who);
        return UTTT_ERR_ARG;
    }
    for (int64_t i = 0; i < n; ++i) {
        if (states[i].active < -1 || states[i].active > 8) {
            set_error("active_board must be -1..8 (state %lld has %d)", (long long)i, states[i].active);
            return UTTT_ERR_ARG;
        }
    }
    return UTTT_OK;
}

int uttt_states_transform_host(const uttt_state_t *states, int64_t n, const int8_t *sym, uttt_state_t *out) {
    // T_g of uttt_sym.h for n states; what k_sym_leaves writes.
    if (int rc = check_sym_states("uttt_states_transform_host", states, n, sym, out)) return rc;
    for (int64_t i = 0; i < n; ++i)
        if (int rc = check_sym("uttt_states_transform_host", sym[i])) return rc;
    for (int64_t i = 0; i < n; ++i) out[i] = sym_state(states[i], sym[i]);
    return UTTT_OK;
}

int uttt_states_symmetry_host(const uttt_state_t *states, int64_t n, uint64_t seed, int8_t *sym) {
    // The hashed choice of uttt_sym.h; what k_sym_leaves chooses in UTTT_SYM_HASHED.
    if (int rc = check_sym_states("uttt_states_symmetry_host", states, n, sym, sym)) return rc;
    for (int64_t i = 0; i < n; ++i) {
        uint64_t w[4];
        input_words(states[i], w);
        sym[i] = (int8_t)sym_of_key(w, seed);
    }
    return UTTT_OK;
}

int uttt_root_noise_host(const uttt_state_t *states, int64_t n, const int64_t *stream, const int32_t *ply, float epsilon,
                         float alpha, uint64_t seed, float *eta, float *priors) {
    // uttt_noise.h for n roots with uniform priors; what k_root_noise writes into the roots' child blocks.
    if (int rc = noise_check_args("uttt_root_noise_host", epsilon, alpha)) return rc;
    if (int rc = check_sym_states("uttt_root_noise_host", states, n, stream, ply)) return rc;
    for (int64_t r = 0; r < n; ++r) {
        const int L = (int)legal_count(states[r]);
        float row[81];
        noise_eta_row(alpha, noise_key(seed, (uint64_t)stream[r], (uint32_t)ply[r]), L, row);
        const float up = L ? 1.0f / (float)L : 0.0f;
        for (int i = 0; i < L; ++i) {
            if (eta) eta[r * 81 + i] = row[i];
            if (priors) priors[r * 81 + i] = noise_mix(epsilon, row[i], up);
        }
    }
    return UTTT_OK;
}

int uttt_reroot_host(const uint32_t *records, int32_t node_count, const uttt_state_t *state, int32_t action,
                     uint32_t *out, int32_t *out_count) {
    // uttt_reroot.h for one tree; what k_reroot writes into the tree's other pool.
    if (!records || !state || !out || !out_count || node_count < 1) {
        set_error("uttt_reroot_host: null pointer or an empty tree");
        return UTTT_ERR_ARG;
    }
    if (state->active < -1 || state->active > 8) {
        set_error("active_board must be -1..8 (the root has %d)", state->active);
        return UTTT_ERR_ARG;
    }
    const int n = reroot::reroot_tree(records, node_count, *state, action, out);
    if (n < 0) {
        set_error("uttt_reroot_host: action %d is not a move of the root, or the records are not a search's tree", action);
        return UTTT_ERR_ARG;
    }
    *out_count = n;
    return UTTT_OK;
}

int uttt_match_check_host(const uttt_state_t *openings, int32_t n_openings, int32_t games, int32_t max_games,
                          int32_t paired) {
    if (games < 1 || games > max_games) {
        set_error("uttt_match_begin: %d games outside 1..%d (the match's max_games)", games, max_games);
        return UTTT_ERR_ARG;
    }
    if (paired && (games & 1)) {
        set_error("uttt_match_begin: a paired match plays every opening twice, and %d games is odd", games);
        return UTTT_ERR_ARG;
    }
    const int need = match_opening_of(games - 1, paired) + 1;
    if (!openings || n_openings < need) {
        set_error("uttt_match_begin: %d openings for %d %s games (%d needed)", openings ? n_openings : 0, games,
                  paired ? "paired" : "unpaired", need);
        return UTTT_ERR_ARG;
    }
    for (int i = 0; i < need; ++i) {
        if (openings[i].active < -1 || openings[i].active > 8) {
            set_error("active_board must be -1..8 (opening %d has %d)", i, openings[i].active);
            return UTTT_ERR_ARG;
        }
        if (is_done(openings[i])) {
            set_error("uttt_match_begin: opening %d is a finished game", i);
            return UTTT_ERR_ARG;
        }
    }
    return UTTT_OK;
}

int uttt_match_move_host(const uttt_state_t *state, const int32_t *visits, int32_t n_visits, int32_t ply, int64_t game,
                         uint64_t seed, int32_t sample_plies, uttt_state_t *next, int32_t *action, int32_t *result) {
    // uttt_match.h for one game; what k_match_move writes for it.
    if (!state || !visits || !next || !action || !result || ply < 0 || ply > 80 || game < 0) {
        set_error("uttt_match_move_host: null pointer, a ply outside 0..80 or a negative game id");
        return UTTT_ERR_ARG;
    }
    if (state->active < -1 || state->active > 8) {
        set_error("active_board must be -1..8 (the state has %d)", state->active);
        return UTTT_ERR_ARG;
    }
    uint32_t m[3];
    legal_mask(*state, m);
    const int L = (int)legal_count(*state);
    if (L == 0 || n_visits != L) {
        set_error("uttt_match_move_host: %d visit counts for a state with %d legal moves%s", n_visits, L,
                  L ? "" : " (a finished game)");
        return UTTT_ERR_ARG;
    }
    for (int i = 0; i < L; ++i)
        if (visits[i] < 0 || visits[i] > UTTT_MAX_SIMS) {
            set_error("uttt_match_move_host: visit count %d at rank %d outside 0..%d", visits[i], i, UTTT_MAX_SIMS);
            return UTTT_ERR_ARG;
        }
    const int i = match_choose(visits, L, ply, (uint64_t)game, seed, sample_plies);
    const int a = nth_legal(m, (uint32_t)i);
    *next = next_state(*state, a);
    *action = a;
    *result = match_result_after(*next, match_player_to_move((int)(game & 1), ply));
    return UTTT_OK;
}

uint64_t uttt_match_draw_host(uint64_t seed, int64_t game, int32_t ply) {
    return match_draw(seed, (uint64_t)game, (uint32_t)ply);
}

}  // extern "C"
