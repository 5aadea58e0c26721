"""Exact endgame values (include/uttt_engine.h uttt_solve / uttt_solve_host; game.py:240-274's alpha_beta and
alpha_beta_action) and what a maintainer reads from them: the blunder rate of a set of game
records, the share of solvable plies where the move played gave away game-theoretic value.

Engine.solve runs on the device, solve_host on the CPU; both return the same five arrays, bit for bit.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import STATE_DTYPE, UtttState, check, ptr
from .engine import as_states

SOLVED, BUDGET, TOO_LARGE = 1, 2, 3  # UTTT_SOLVE_*
SKIPPED = 0                          # UTTT_OVERLAY_SKIPPED: the overlay did not search the position
PRIORS_KEEP, PRIORS_OPTIMAL = 0, 1   # UTTT_PRIORS_*
UNKNOWN = -128                       # UTTT_SOLVE_UNKNOWN: an unsolved or illegal action's value
MAX_EMPTY = 32                       # UTTT_SOLVE_MAX_EMPTY: the deepest position searched

_LINES = (0x007, 0x038, 0x1C0, 0x049, 0x092, 0x124, 0x111, 0x054)
_CELLS = 0x1FF


def solve_with(call, states, max_nodes):
    """The five result arrays of one uttt_solve / uttt_solve_host call; `call` takes the C arguments after
    the engine handle."""
    st = as_states(states)
    n = len(st)
    value = np.zeros(n, np.int8)
    action = np.zeros(n, np.int8)
    status = np.zeros(n, np.int8)
    nodes = np.zeros(n, np.int64)
    action_values = np.zeros((n, 81), np.int8)
    check(call(st.ctypes.data_as(ctypes.POINTER(UtttState)), n, int(max_nodes), ptr(value, ctypes.c_int8),
               ptr(action, ctypes.c_int8), ptr(status, ctypes.c_int8), ptr(nodes, ctypes.c_int64),
               ptr(action_values, ctypes.c_int8)))
    return value, action, status, nodes, action_values


def solve_host(states, max_nodes=65536):
    """Engine.solve on the CPU (uttt_solve_host): needs no GPU."""
    return solve_with(_lib.load().uttt_solve_host, states, max_nodes)


def priors_mode(priors):
    """UTTT_PRIORS_* of "keep" / "optimal" (or of the number itself)."""
    if isinstance(priors, str):
        if priors not in ("keep", "optimal"):
            raise ValueError(f'priors must be "keep" or "optimal" (got {priors!r})')
        return PRIORS_OPTIMAL if priors == "optimal" else PRIORS_KEEP
    return int(priors)


def overlay_host(states, policy, value, max_empties, max_nodes, priors):
    """Engine.eval_solve_dev on the CPU (uttt_solve_overlay_host): lays the exact values of `states` over the
    rows policy ((n, >=81) float32, unit stride along the actions) and value ((n,) or (n, 1) float32) in place
    and returns the int8 status per row (SKIPPED / SOLVED / BUDGET)."""
    st = as_states(states)
    n = len(st)
    ok = (isinstance(policy, np.ndarray) and isinstance(value, np.ndarray) and policy.dtype == np.float32
          and value.dtype == np.float32 and policy.ndim == 2 and len(policy) == n and value.shape in ((n,), (n, 1)))
    if not ok or (n and (policy.strides[1] != 4 or policy.strides[0] % 4 or value.strides[0] % 4)):
        raise ValueError("overlay_host: policy (n, >=81) and value (n,) or (n, 1), float32 numpy rows")
    if policy.shape[1] < 81:
        raise ValueError("overlay_host: a policy row has 81 entries")
    if not (policy.flags.writeable and value.flags.writeable):
        raise ValueError("overlay_host: the rows are updated in place")
    status = np.zeros(n, np.int8)
    check(_lib.load().uttt_solve_overlay_host(
        st.ctypes.data_as(ctypes.POINTER(UtttState)), n, int(max_empties), int(max_nodes), priors_mode(priors),
        ptr(policy, ctypes.c_float), policy.strides[0] // 4 if n else 81, ptr(value, ctypes.c_float),
        value.strides[0] // 4 if n else 1, ptr(status, ctypes.c_int8)))
    return status


def empties(states):
    """Empty cells in small boards that are neither won nor full (csrc/uttt_solve.h `empties`): the bound on
    the depth of a search from each state, int array."""
    st = as_states(states)
    closed = (st["mains"] | (st["mains"] >> 16)) & _CELLS
    out = np.zeros(len(st), np.int64)
    for b in range(9):
        free = ~((st["own"][:, b // 3] | st["opp"][:, b // 3]) >> (9 * (b % 3))) & _CELLS
        count = np.zeros(len(st), np.int64)
        for c in range(9):
            count += (free >> c) & 1
        out += np.where((closed >> b) & 1, 0, count)
    return out


def _action_at(pos):
    R, C = divmod(pos, 9)
    return ((R // 3) * 3 + C // 3) * 9 + (R % 3) * 3 + C % 3


def states_from_inputs(x):
    """Packed states equivalent to the positions whose network inputs are x ((n, 243) or (n, 9, 9, 3) HWC, what
    the self-play records and the .history reader hold), for positions of real games: a small board is closed
    for the side with a line on it, or for both when it is full with no line; `active` is the one board with
    legal moves, or -1. The stones, the legal moves and every successor are the original's."""
    x = np.asarray(x).reshape(-1, 81, 3) != 0
    n = len(x)
    bits = np.zeros((3, n, 9), np.int64)  # [channel][position][board] -> 9-bit cells
    for pos in range(81):
        a = _action_at(pos)
        for ch in range(3):
            bits[ch, :, a // 9] |= x[:, pos, ch].astype(np.int64) << (a % 9)
    own, opp, legal = bits
    won_own = np.zeros((n, 9), bool)
    won_opp = np.zeros((n, 9), bool)
    for ln in _LINES:
        won_own |= (own & ln) == ln
        won_opp |= (opp & ln) == ln
    full = (own | opp) == _CELLS
    st = np.zeros(n, STATE_DTYPE)
    for b in range(9):
        st["own"][:, b // 3] |= (own[:, b] << (9 * (b % 3))).astype(np.uint32)
        st["opp"][:, b // 3] |= (opp[:, b] << (9 * (b % 3))).astype(np.uint32)
        st["mains"] |= ((won_own[:, b] | (full[:, b] & ~won_opp[:, b])).astype(np.uint32) << b)
        st["mains"] |= ((won_opp[:, b] | (full[:, b] & ~won_own[:, b])).astype(np.uint32) << (16 + b))
    boards = legal != 0
    st["active"] = np.where(boards.sum(axis=1) == 1, boards.argmax(axis=1), -1)
    return st


def blunder_report(states, actions, max_nodes=65536, engine=None):
    """Blunders among the plies of game records, by exact search. states: the positions before each move, as
    Engine.plies()["states"] gives them, or their network inputs ((n, 243) or (n, 9, 9, 3), the records' and
    the .history file's form); actions: the moves played. A ply is countable when its position is SOLVED and
    the played move's value is known; it is a blunder when that value is below the position's. With an
    Engine the positions are solved on its device, otherwise on the CPU (the same results).

    Returns {"countable": int64[MAX_EMPTY + 1], "blunders": int64[MAX_EMPTY + 1]} indexed by the position's
    empties, and "plies", the number of plies given."""
    if isinstance(states, np.ndarray) and states.dtype != STATE_DTYPE:  # numeric: network inputs
        states = states_from_inputs(states)
    st = as_states(states)
    actions = np.asarray(actions).astype(np.int64).reshape(-1)
    if len(actions) != len(st) or ((actions < 0) | (actions > 80)).any():
        raise ValueError("blunder_report: one action 0..80 per state")
    value, _, status, _, av = engine.solve(st, max_nodes) if engine is not None else solve_host(st, max_nodes)
    played = av[np.arange(len(st)), actions] if len(st) else np.zeros(0, np.int8)
    countable = (status == SOLVED) & (played != UNKNOWN)
    blunder = countable & (played < value)
    e = np.minimum(empties(st), MAX_EMPTY)  # countable plies have at most MAX_EMPTY
    return {"plies": len(st),
            "countable": np.bincount(e[countable], minlength=MAX_EMPTY + 1).astype(np.int64),
            "blunders": np.bincount(e[blunder], minlength=MAX_EMPTY + 1).astype(np.int64)}
