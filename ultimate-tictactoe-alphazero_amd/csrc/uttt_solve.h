// uttt_solve.h — exact endgame values (game.py:240-274 `alpha_beta` / `alpha_beta_action`) on the packed
// bitboards, compiled for both the host (uttt_solve_host, the checker's counterpart) and gfx950
// (k_solve_states, and k_solve_leaves inside the search's round loop). DESIGN.md §6c, §6d.
//
// A position is solved one legal move per lane: lane i takes the i-th legal action a in ascending order and
// searches the child c = next_state(s, a) with a full-depth fail-hard negamax, values -1 / 0 / +1, integer
// window (-1, +1), moves tried in ascending order. The window holds every value, so a lane's result is the
// child's exact value. A lane counts the nodes it visits (every invocation of the search, c and terminal
// nodes included) and stops unsolved when it would visit node number max_nodes + 1. No lane reads another
// lane's progress: the position's result is a function of the lanes' results alone, so the host (lanes one
// after another) and the device (64 lanes at once) agree in every output, the node counts included.
//
// The search is an iterative step machine, not recursion. A lane keeps the node it is at as a whole state in
// registers and one 4-byte frame per ancestor on an explicit stack: the action played from the ancestor, and
// what next_state cannot undo (the ancestor's active board) and the machine needs back (its window). The
// remaining moves of a node are recomputed from its state. The host's stack is a local array; the device's
// is LDS, indexed by depth, never a private array under a dynamic index (which the device compiler places in
// scratch; uttt_playout.h nth_legal).
#pragma once

#include "uttt_bits.h"

namespace uttt {

// The deepest search accepted: empties(s) of the root. 4 B per frame x kSolveMaxEmpty frames x 64 lanes x
// 4 waves per workgroup = 32 KB of LDS, five workgroups on a CU's 160 KB. Searches from more than ~24 empties
// rarely end within the largest budget, so a larger cap would buy LDS, not solved positions.
constexpr int kSolveMaxEmpty = 32;
static_assert(kSolveMaxEmpty == UTTT_SOLVE_MAX_EMPTY, "the public header states the cap");
constexpr int32_t kSolveMaxNodes = 1 << 22;  // per lane
constexpr int64_t kSolveMaxStates = 1 << 24;  // per call (one wave each; the grid stays far inside 2^31 threads)
// the argument checks of uttt_solve_host and uttt_solve (rules_api.cpp; host only)
int solve_check_args(const char *who, const uttt_state_t *states, int64_t n, int32_t max_nodes);
// at most 64: every legal move fills one of the root's empties, so one wave's lanes cover them all
static_assert(kSolveMaxEmpty >= 20 && kSolveMaxEmpty <= 64, "one lane per legal move of an accepted position");

// Empty cells in small boards that are neither won nor full. Every ply fills one of them and boards only
// close, so a search from s is at most empties(s) plies deep.
UTTT_HD int empties(const uttt_state_t &s) {
    const uint32_t open = ~(main_own(s) | main_opp(s)) & kCells;
    int n = 0;
#pragma unroll
    for (int w = 0; w < 3; ++w) {
        uint32_t boards = 0u;
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if ((open >> (3 * w + j)) & 1u) boards |= kCells << (9 * j);
        n += (int)popc32(~(s.own[w] | s.opp[w]) & boards & kWord);
    }
    return n;
}

// The state from which the legal action a led to n, given its active board: next_state's inverse. The sides
// swap back and the stone leaves; board a / 9 was open before a legal move into it, so both of its main bits
// are cleared, whether this move set them or not.
UTTT_HD uttt_state_t prev_state(const uttt_state_t &n, int a, int32_t active) {
    const int b = div9(a), w = div27(a);
    const uint32_t bit = 1u << (a - 27 * w);
    uttt_state_t p;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        p.own[i] = n.opp[i];
        p.opp[i] = n.own[i];
    }
    p.own[0] &= w == 0 ? ~bit : ~0u;
    p.own[1] &= w == 1 ? ~bit : ~0u;
    p.own[2] &= w == 2 ? ~bit : ~0u;
    const uint32_t keep = ~(1u << b) & kCells;
    p.mains = (main_opp(n) & keep) | ((main_own(n) & keep) << 16);
    p.active = active;
    return p;
}

// The lowest legal action above `last` (-1: the lowest of all), or -1 when there is none.
UTTT_HD int next_legal_after(const uint32_t m[3], int last) {
    uint32_t x[3];
#pragma unroll
    for (int w = 0; w < 3; ++w) {
        const int k = last + 1 - 27 * w;  // bits below k of word w are done
        x[w] = k <= 0 ? m[w] : (k >= 27 ? 0u : m[w] & (~0u << k));
    }
    if (x[0]) return __builtin_ctz(x[0]);
    if (x[1]) return 27 + __builtin_ctz(x[1]);
    if (x[2]) return 54 + __builtin_ctz(x[2]);
    return -1;
}

// A frame: action (bits 0-6) | the node's active board + 1 (7-10) | alpha + 1 (11-12) | beta + 1 (13-14).
UTTT_HD uint32_t solve_frame(int a, int32_t active, int alpha, int beta) {
    return (uint32_t)a | ((uint32_t)(active + 1) << 7) | ((uint32_t)(alpha + 1) << 11) | ((uint32_t)(beta + 1) << 13);
}

// One lane's machine. s is the node it is at, [alpha, beta] that node's window, d the frames below it.
// last < 0: the node has just been entered and is not yet counted; otherwise the child reached by action
// `last` has returned v.
struct SolveLane {
    uttt_state_t s;
    int32_t d, alpha, beta, last, v;
    int32_t nodes;
    int32_t live;    // still searching
    int32_t solved;  // finished within the budget: v is the exact value of the lane's root
};

UTTT_HD void solve_lane_begin(SolveLane &ln, const uttt_state_t &c) {
    ln.s = c;
    ln.d = 0;
    ln.alpha = -1;
    ln.beta = 1;
    ln.last = -1;
    ln.v = 0;
    ln.nodes = 0;
    ln.live = 1;
    ln.solved = 0;
}

// One step of a live lane: it enters the node (counts it, ends it if terminal) or takes a child's value,
// then either descends to the node's next move or returns to its parent. Stack: uint32_t load(int d),
// void store(int d, uint32_t frame), d in [0, kSolveMaxEmpty).
template <typename Stack>
UTTT_HD void solve_step(SolveLane &ln, Stack &st, int32_t max_nodes) {
    bool done = false;  // this node's value is known: r
    int r = 0;
    if (ln.last < 0) {
        if (ln.nodes >= max_nodes) {  // this would be node number max_nodes + 1
            ln.live = 0;
            return;
        }
        ln.nodes += 1;
        if (is_lose(ln.s)) {
            done = true;
            r = -1;
        }
    } else {
        const int score = -ln.v;
        if (score > ln.alpha) ln.alpha = score;
        if (ln.alpha >= ln.beta) {
            done = true;
            r = ln.alpha;
        }
    }
    int a = -1;
    if (!done) {
        uint32_t m[3];
        legal_mask(ln.s, m);
        a = next_legal_after(m, ln.last);
        if (a < 0) {  // no move at all: a draw, 0; no move left: the best so far
            done = true;
            r = ln.last < 0 ? 0 : ln.alpha;
        }
    }
    if (done) {
        if (ln.d == 0) {
            ln.v = r;
            ln.live = 0;
            ln.solved = 1;
            return;
        }
        ln.d -= 1;
        const uint32_t f = st.load(ln.d);
        ln.last = (int)(f & 0x7Fu);
        ln.s = prev_state(ln.s, ln.last, (int32_t)((f >> 7) & 0xFu) - 1);
        ln.alpha = (int)((f >> 11) & 3u) - 1;
        ln.beta = (int)((f >> 13) & 3u) - 1;
        ln.v = r;
    } else {
        // d <= empties(root) - 2 < kSolveMaxEmpty at every push (a node with a move left has an empty cell);
        // the guard keeps a store inside the stack whatever the caller passed
        if (ln.d >= kSolveMaxEmpty) {
            ln.live = 0;
            return;
        }
        st.store(ln.d, solve_frame(a, ln.s.active, ln.alpha, ln.beta));
        ln.d += 1;
        ln.s = next_state(ln.s, a);
        const int na = -ln.beta, nb = -ln.alpha;
        ln.alpha = na;
        ln.beta = nb;
        ln.last = -1;
    }
}

// The root's own answer, before any lane runs: terminal, too large, or to be searched.
//   returns true when the position needs no search: status / value are set (action -1, nodes 0).
UTTT_HD bool solve_root(const uttt_state_t &s, const uint32_t m[3], int8_t &status, int8_t &value) {
    value = 0;
    if (is_lose(s)) {
        status = UTTT_SOLVE_SOLVED;
        value = -1;
        return true;
    }
    if ((m[0] | m[1] | m[2]) == 0u) {
        status = UTTT_SOLVE_SOLVED;
        return true;
    }
    if (empties(s) > kSolveMaxEmpty) {
        status = UTTT_SOLVE_TOO_LARGE;
        return true;
    }
    status = UTTT_SOLVE_BUDGET;
    return false;
}

// A searched position's result from what its lanes found, the one rule of the host loops and the kernels'
// epilogues: best is the largest known action value (-2: none is known), every says that no lane ran out of
// budget. A known winning move decides the position whatever the other lanes did; otherwise every move must
// be known. Returns true, with status / value set, when the position is SOLVED.
UTTT_HD bool solve_result(int best, bool every, int8_t &status, int8_t &value) {
    if (best != 1 && !every) return false;
    status = UTTT_SOLVE_SOLVED;
    value = (int8_t)best;
    return true;
}

// ----------------------------------------------------------------- overlay --
// Exact values laid over an evaluator's rows (uttt_solve_overlay_host, k_solve_leaves). For a
// position s, its row (policy[81], value) and the parameters max_empties, max_nodes, priors:
//   empties(s) > max_empties: UTTT_OVERLAY_SKIPPED, nothing searched, the row untouched;
//   otherwise s is solved as above (solve_root, one lane per legal move, solve_result). Not SOLVED: the row
//   is untouched, status UTTT_SOLVE_BUDGET. SOLVED: value = (float)v, and with UTTT_PRIORS_OPTIMAL every
//   policy entry becomes overlay_prior of its action, unless s is terminal (it has no move to mark).
// With max_empties <= kSolveMaxEmpty, solve_root never answers TOO_LARGE here. The overlay does not divide:
// the apply's legal mask and sequential renormalisation turn the marks into exactly 1 / count.
UTTT_HD bool overlay_skips(const uttt_state_t &s, int32_t max_empties) { return empties(s) > max_empties; }

// Entry a of a SOLVED, searched position's policy under UTTT_PRIORS_OPTIMAL: av is the action's known value
// (UTTT_SOLVE_UNKNOWN when it is not known), v the position's.
UTTT_HD float overlay_prior(bool legal, int av, int v) { return legal && av == v ? 1.0f : 0.0f; }

// the argument checks of uttt_solve_overlay_host and uttt_eval_solve_dev (rules_api.cpp; host only)
int overlay_check_args(const char *who, int32_t max_empties, int32_t max_nodes, int32_t priors, const float *policy,
                       int64_t policy_ld, const float *value, int64_t value_ld);

}  // namespace uttt
