"""Inputs that reach the search kernels' second halves: leaves with more than 64 legal moves (actions 64-80
live in lanes 0-16's second registers) and paths deeper than 63 plies (levels 64-127 live in the lanes' second
path registers). Built from the oracle's rules alone (oracle.core), seeded with random.Random; the evaluators
are pure functions of the network input's bytes, so the oracle and the engine can be handed the same table.

A free move into a decided small board is what makes a state wide early in a game: every empty cell of the
eight other boards is legal. A prior-sum row of L entries is padded to L4 = (L + 3) & ~3, so L "pads" when it
is no multiple of 4; WIDE holds the padding values the walks below can produce (68 needs no pad)."""
import functools
import hashlib
import random

import numpy as np

WIDE = (65, 66, 67, 69, 70)
MAX_PLIES = 16        # of one random game of the wide walks
KEEP = range(66, 71)  # the wide walks keep a state with this many legal moves
N_ROOTS = 48
WIDE_SEED = 27        # the first of seeds 1-40 that meets every bound of test_wide_deep_host.py
DEEP_SEED = 7


def pack_states(ostates):
    """OrStates -> packed STATE_DTYPE rows (the engine's root format)."""
    from uttt_amd._lib import STATE_DTYPE
    arr = np.zeros(len(ostates), STATE_DTYPE)
    for i, s in enumerate(ostates):
        p, e, mp, me, a = s.arrays()
        for x in range(81):
            arr["own"][i, x // 27] |= int(p.reshape(81)[x]) << (x % 27)
            arr["opp"][i, x // 27] |= int(e.reshape(81)[x]) << (x % 27)
        arr["mains"][i] = sum(int(mp[b]) << b for b in range(9)) | sum(int(me[b]) << (16 + b) for b in range(9))
        arr["active"][i] = a
    return arr


@functools.lru_cache(maxsize=None)
def _wide_walk(n, seed):
    """n (parent, wide state) pairs: random games of at most MAX_PLIES plies from the initial state, each cut at
    its first state with 66-70 (KEEP) legal moves."""
    from oracle import core
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        s = core.OrState.initial()
        legal = s.legal_actions()
        for _ in range(MAX_PLIES):
            c = s.next(rng.choice(legal))
            legal = c.legal_actions()
            if c.is_done():
                break
            if len(legal) in KEEP:
                out.append((s, c))
                break
            s = c
    return tuple(out)


def wide_parents(n, seed):
    """(packed roots, OrStates): n states one move above a state with 66-70 legal moves."""
    ost = [p for p, _ in _wide_walk(n, seed)]
    return pack_states(ost), ost


def wide_roots(n, seed):
    """(packed roots, OrStates): the same walk's wide states themselves. A child at the decided board's cell
    index is a free move again with one legal move fewer, so one tree expands L - 1, L - 2, ... in turn."""
    ost = [c for _, c in _wide_walk(n, seed)]
    return pack_states(ost), ost


@functools.lru_cache(maxsize=None)
def _table_row(key):
    rs = np.random.RandomState(np.frombuffer(hashlib.sha256(key).digest()[:16], np.uint32))
    p = (10.0 ** rs.uniform(-3.0, 3.0, 81)).astype(np.float32)
    return p, np.float32(rs.uniform(-1.0, 1.0))


def spread_table_eval(log, zero_rows=None):
    """evaluator(x (243,) f32, CHW) -> (p[81] f32, v f32), a pure function of x.tobytes(): unnormalised priors
    spread over six decades (a stale rank in a sum's pad is as likely as not larger than the whole sum) and a
    value in (-1, 1). Appends the state's number of legal moves (plane 2 is the legal mask) to log.
    zero_rows: a set of x.tobytes() keys whose priors are all zero instead (the uniform branch)."""
    zeros = np.zeros(81, np.float32)

    def evaluate(x):
        x = np.ascontiguousarray(x, np.float32).reshape(243)
        key = x.tobytes()
        log.append(int(x[162:].sum()))
        p, v = _table_row(key)
        return (zeros if zero_rows and key in zero_rows else p), v

    return evaluate


def wide_count(log):
    return sum(1 for L in log if L in WIDE)


def wide_after_wider(log):
    """Wide leaves evaluated after a leaf with more legal moves in the same tree: what a pad that is not zeroed
    turns into a wrong sum on a wave that keeps its row."""
    n, top = 0, 0
    for L in log:
        if L in WIDE and top > L:
            n += 1
        top = max(top, L)
    return n


def deep_line(seed, games=3000):
    """(root OrState, line, make_eval): the longest of `games` random games; the root is its state after ply 1,
    line the states from the root to the game's terminal state. make_eval(log) is the evaluator that walks a
    search down the line: on line state d (d plies below the root) a prior of 1.0 on the line's move, 1e-6
    elsewhere, value 0, and d appended to log; off the line 1e-6 everywhere and value +1 (good for the side that
    left the line's opponent to move: the parent avoids it), -1 appended."""
    return deep_line_from(longest_game(seed, games))


@functools.lru_cache(maxsize=None)
def longest_game(seed, games):
    from oracle import core
    rng = random.Random(seed)
    best = []
    for _ in range(games):
        s = core.OrState.initial()
        acts = []
        while not s.is_done():
            a = rng.choice(s.legal_actions())
            acts.append(a)
            s = s.next(a)
        if len(acts) > len(best):
            best = acts
    return tuple(best)


def deep_line_from(best):
    """deep_line for a given game (its actions from the initial state)."""
    from oracle import core
    s = core.OrState.initial().next(best[0])
    line, moves = [s], {}
    for d, a in enumerate(best[1:]):
        moves[s.tensor_nchw().tobytes()] = (d, a)
        s = s.next(a)
        line.append(s)
    assert s.is_done()

    def make_eval(log):
        def evaluate(x):
            key = np.ascontiguousarray(x, np.float32).reshape(243).tobytes()
            p = np.full(81, 1e-6, np.float32)
            if key in moves:
                d, a = moves[key]
                log.append(d)
                p[a] = 1.0
                return p, np.float32(0.0)
            log.append(-1)
            return p, np.float32(1.0)
        return evaluate

    return line[0], line, make_eval


# ------------------------------------------------------------------ the oracle's results, computed once --
def wide_states(kind):
    """(packed roots, OrStates) of kind "parents" / "roots" at the suite's size and seed."""
    return (wide_parents if kind == "parents" else wide_roots)(N_ROOTS, WIDE_SEED)


def zero_keys():
    """The inputs of every fourth wide root: the rows test (d) zeroes."""
    return frozenset(s.tensor_nchw().tobytes() for s in wide_states("roots")[1][::4])


@functools.lru_cache(maxsize=None)
def oracle_wide(kind, S, B, tau=1.0, semantics="cpp", zero=False):
    """Per root of wide_states(kind): (scores, visits, the evaluator's log of legal-move counts) of the
    oracle's search with the spread table (semantics "py": pv_mcts.py's, float64 scores)."""
    from oracle import core
    search = core.pv_mcts_scores if semantics == "cpp" else core.pv_mcts_scores_py_callback
    out = []
    for s in wide_states(kind)[1]:
        log = []
        sc, vi, _ = search(s, tau, S, B, spread_table_eval(log, zero_keys() if zero else None))
        out.append((sc, vi, tuple(log)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def oracle_deep(S, B, tau=1.0, semantics="cpp"):
    """(scores, visits, log of line depths, SearchStats) of the oracle's search down deep_line(DEEP_SEED)."""
    from oracle import core
    root, _, make_eval = deep_line(DEEP_SEED)
    search = core.pv_mcts_scores if semantics == "cpp" else core.pv_mcts_scores_py_callback
    log = []
    sc, vi, st = search(root, tau, S, B, make_eval(log))
    return sc, vi, tuple(log), st


@functools.lru_cache(maxsize=None)
def oracle_wide_hash(kind, S, B):
    """Per root of wide_states(kind): (scores at 1.0, visits, log) of the oracle's search with its hash
    evaluator (pv_mcts_scores_hash); the log comes from a replay of the same search through the callback
    path, whose visits must equal the first's."""
    from oracle import core
    out = []
    for s in wide_states(kind)[1]:
        sc, vi, _ = core.pv_mcts_scores_hash(s, 1.0, S, B)
        log = []

        def logged(x):
            log.append(int(np.asarray(x, np.float32)[162:].sum()))
            return core.hash_eval(x)

        _, vi2, _ = core.pv_mcts_scores(s, 1.0, S, B, logged)
        assert np.array_equal(vi, vi2)
        out.append((sc, vi, tuple(log)))
    return tuple(out)
