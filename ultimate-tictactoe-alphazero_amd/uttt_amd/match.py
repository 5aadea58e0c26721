"""Match play on the device: two configured players, paired openings, an Elo difference with an interval.

arena._play_games keeps one State, one RandomState and one Python list per game on the host and runs a Python
loop body per game and ply. Here the games live on the GPU (engine.Match, csrc/uttt_match.h): per
iteration each player's engine searches the games in which that player is to move, straight from the match's
device arrays, and one kernel plays the searched moves. The host reads five counters per iteration.

Game g starts at openings[g // 2] (paired) or openings[g] (not), and player g % 2 takes the side to move there,
so games 2i and 2i+1 are one opening with the colours swapped. A move at a ply (counted from the opening) below
sample_plies is drawn in proportion to the root's visit counts, in integers, keyed by (seed, game, ply); a later
one is the most visited move, the first of equals: evaluate_best_player's temperature 0.
"""
import ctypes
import math

import numpy as np

from . import _lib
from ._lib import STATE_DTYPE, UtttState, check, ptr
from .engine import Engine, Match, as_states, initial_states


class Player:
    """One side of a match: evaluator_factory(engine) -> any engine evaluator (HashEvaluator, PlayoutEvaluator,
    arena.model_evaluator(model, ..., engine=engine), those wrapped in SolvedLeaves / SymmetricLeaves), searched
    with evaluate_count simulations per move in flushes of batch_size, on "py" (pv_mcts.py) or "cpp"
    (uttt_mcts.cpp) semantics."""

    def __init__(self, evaluator_factory, evaluate_count=50, batch_size=8, semantics="py"):
        if semantics not in Engine.SEMANTICS:
            raise ValueError(f"semantics must be 'py' or 'cpp' (got {semantics!r})")
        if int(evaluate_count) < 1:
            raise ValueError(f"evaluate_count must be at least 1 (got {evaluate_count})")
        self.evaluator_factory = evaluator_factory
        self.evaluate_count = int(evaluate_count)
        self.batch_size = int(batch_size)
        self.semantics = semantics


def match_draw(seed, game, ply):
    """The 64-bit draw of (seed, game, ply) (uttt_match_draw_host): what a sampled move scales by its visit sum."""
    return int(_lib.load().uttt_match_draw_host(ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), int(game), int(ply)))


def match_move_host(state, visits, ply, game, seed=0, sample_plies=0):
    """The move rule on the CPU (uttt_match_move_host), bit for bit the device's: state is one packed position,
    visits the root's counts in legal order -> (next state as a 1-element STATE_DTYPE array, action, result) with
    result -1 while the game is live, else player 0's half-points."""
    lib = _lib.load()
    st = as_states(state)
    v = np.ascontiguousarray(visits, np.int32).reshape(-1)
    nxt = np.zeros(1, STATE_DTYPE)
    a, r = ctypes.c_int32(), ctypes.c_int32()
    check(lib.uttt_match_move_host(st.ctypes.data_as(ctypes.POINTER(UtttState)), ptr(v, ctypes.c_int32), len(v), int(ply),
                                   int(game), ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), int(sample_plies),
                                   nxt.ctypes.data_as(ctypes.POINTER(UtttState)), ctypes.byref(a), ctypes.byref(r)))
    return nxt, a.value, r.value


def check_openings(openings, games, max_games, paired):
    """uttt_match_begin's argument check on the CPU (uttt_match_check_host): ValueError for a terminal opening,
    games outside 1..max_games, an odd paired match, or too few openings."""
    op = as_states(openings)
    check(_lib.load().uttt_match_check_host(op.ctypes.data_as(ctypes.POINTER(UtttState)), len(op), int(games),
                                            int(max_games), int(bool(paired))))


def random_openings(n, plies, seed=0):
    """n distinct non-terminal positions, each reached by `plies` uniformly random legal moves from the initial
    state: a STATE_DTYPE array, deterministic in (n, plies, seed). Runs on the host with the rules ABI. Candidate c
    = 0, 1, ... plays move p as the floor(draw(seed, c, p) * L / 2^64)-th of its L legal moves (match_draw); a
    candidate that ends early, ends terminal or repeats an earlier opening is skipped and the next counter drawn.
    ValueError when there are not n distinct positions to find (plies = 0 has one)."""
    n, plies = int(n), int(plies)
    if n < 1 or not 0 <= plies <= 80:
        raise ValueError(f"random_openings: n must be at least 1 and plies 0..80 (got {n}, {plies})")
    lib = _lib.load()
    out = np.zeros(n, STATE_DTYPE)
    seen = set()
    legal = (ctypes.c_int32 * 81)()
    found, c, limit = 0, 0, 64 * n + 1024
    while found < n:
        if c >= limit:
            raise ValueError(f"random_openings: only {found} distinct positions after {limit} candidates "
                             f"({plies} plies cannot give {n})")
        s, t = UtttState(), UtttState()
        lib.uttt_state_initial(ctypes.byref(s))
        ok = True
        for p in range(plies):
            L = lib.uttt_state_legal_actions(ctypes.byref(s), legal)
            if L == 0:
                ok = False
                break
            check(lib.uttt_state_next(ctypes.byref(s), legal[(match_draw(seed, c, p) * L) >> 64], ctypes.byref(t)))
            s, t = t, s
        c += 1
        key = bytes(s)
        if not ok or lib.uttt_state_is_done(ctypes.byref(s)) or key in seen:
            continue
        seen.add(key)
        out[found:found + 1] = np.frombuffer(key, STATE_DTYPE)
        found += 1
    return out


def elo_of(score):
    """-400 log10(1 / s - 1): the Elo difference at which the expected score is s; -inf at 0, +inf at 1."""
    s = float(score)
    if s <= 0.0:
        return -math.inf
    if s >= 1.0:
        return math.inf
    return -400.0 * math.log10(1.0 / s - 1.0)


def match_statistics(points, paired):
    """(score, se, pair_scores, elo, elo_low, elo_high) of player 0's per-game points (MatchResult's definition)."""
    pts = np.asarray(points, np.float64)
    x = pts.reshape(-1, 2).mean(axis=1) if paired else pts
    s = float(x.mean())
    se = float(x.std(ddof=1) / math.sqrt(len(x))) if len(x) > 1 else 0.0
    lo, hi = max(0.0, s - 1.96 * se), min(1.0, s + 1.96 * se)
    return s, se, x, elo_of(s), elo_of(lo), elo_of(hi)


class MatchResult:
    """What play_match returns. All from player 0's side.

      points       (games,) float64: 1 win, 0.5 draw, 0 loss per game
      actions      per game, the list of actions played from its opening;  plies: their counts (int32)
      wins / draws / losses, games
      counters     per iteration of the match, the five counters read at its start (engine.Match.COUNTS)
      pair_scores  x: with pairing x_i = the mean of the points of games 2i and 2i+1 (one opening, both colours);
                   without, x_i = game i's points
      score        s = mean(x);  se = std(x, ddof=1) / sqrt(len(x))
      elo          elo(s), with elo(s) = -400 log10(1 / s - 1): -inf at s = 0, +inf at s = 1
      elo_low / elo_high   elo at the ends of the 95% interval s -+ 1.96 se, clipped to [0, 1]

    The pairs, not the games, are the sample: the two games of an opening share it and are correlated, and the
    pair mean removes the opening's own advantage for one colour from the variance."""

    def __init__(self, points, actions, plies, paired, counters=None):
        # counters: the match's five counters (engine.Match.COUNTS) as read at the start of every iteration
        self.counters = list(counters) if counters is not None else []
        self.points = np.asarray(points, np.float64)
        self.actions = actions
        self.plies = np.asarray(plies, np.int32)
        self.paired = bool(paired)
        self.games = len(self.points)
        self.wins = int((self.points == 1.0).sum())
        self.draws = int((self.points == 0.5).sum())
        self.losses = int((self.points == 0.0).sum())
        self.score, self.se, self.pair_scores, self.elo, self.elo_low, self.elo_high = \
            match_statistics(self.points, self.paired)

    def __repr__(self):
        return (f"MatchResult(games={self.games}, +{self.wins} ={self.draws} -{self.losses}, score={self.score:.4f}, "
                f"elo={self.elo:+.1f} [{self.elo_low:+.1f}, {self.elo_high:+.1f}])")


def _search(engine, evaluator, x):
    """The ordinary rounds of a search already begun (BatchedSearch.run's loop)."""
    xin = x if getattr(evaluator, "needs_input", True) else None
    while True:
        n = engine.select(xin)
        if n == 0:
            return
        p, v = evaluator(x, n)
        engine.apply(p, v)


def play_match(player0, player1, games, openings=None, paired=True, sample_plies=0, seed=0, device=None, progress=None):
    """A match of `games` games between two Players on one GPU -> MatchResult (its docstring defines the
    statistics). openings: packed states (random_openings), games // 2 of them when paired, else games; None: the
    initial position for every game. Moves at a ply below sample_plies are sampled from the visit counts with
    `seed`, the others are the most visited move. progress(finished, games), when given, is called once per
    iteration. One Engine per player, sized to `games`; both run on torch's current stream on `device`."""
    import torch

    games = int(games)
    players = (player0, player1)
    if openings is None:
        openings = initial_states(max(1, games // 2 if paired else games))
    openings = as_states(openings)
    check_openings(openings, games, games, paired)
    dev = torch.cuda.current_device() if device is None else int(device)
    with torch.cuda.device(dev):
        engines = [Engine(games, p.evaluate_count, dev) for p in players]
        evaluators = [p.evaluator_factory(e) for p, e in zip(players, engines)]
        x = torch.zeros((games, 3, 9, 9), dtype=torch.float32, device=torch.device("cuda", dev))
        match = Match(games, dev)
        try:
            for e in engines:
                e.use_stream()
            match.begin(openings, games, paired, sample_plies, seed)
            counters = []
            while True:
                c = match.counts()
                counters.append(c)
                if progress:
                    progress(c[2], games)
                if c[0] == 0 and c[1] == 0:
                    break
                for m, (p, e, ev) in enumerate(zip(players, engines, evaluators)):
                    if c[m] == 0:
                        continue
                    match.search_begin(e, m, p.evaluate_count, p.batch_size, p.semantics)
                    _search(e, ev, x)
                    match.move(e, m)
                match.lists()
            st = match.state()
        finally:
            match.close()
            for e in engines:
                e.close()
    if (st["results"] < 0).any():
        raise _lib.EngineError("play_match: a game was left unfinished")
    plies = st["plies"]
    actions = [st["actions"][g, :plies[g]].astype(int).tolist() for g in range(games)]
    return MatchResult(st["results"].astype(np.float64) / 2.0, actions, plies, paired, counters)


__all__ = ["Player", "MatchResult", "play_match", "random_openings", "match_statistics", "match_move_host", "match_draw",
           "check_openings", "elo_of"]
