"""CPU tests of the exact endgame solver's host side (uttt_solve_host, csrc/uttt_solve.h): it equals an
independent pure-Python restatement of the definition (recursive fail-hard negamax per legal move on the oracle's
rules, Python-int node counts) in every output; hand-built terminal, winning and too-large positions; the
relation between value and action values; NULL outputs; argument checks."""
import ctypes
import random

import numpy as np
import pytest

SOLVED, BUDGET, TOO_LARGE, UNKNOWN, MAX_EMPTY = 1, 2, 3, -128, 32


# ------------------------------------------------------------ the restatement --
class _OutOfBudget(Exception):
    pass


def empties_py(s):
    p, e, mp, me, _ = s.arrays()
    p, e = np.asarray(p).reshape(9, 9), np.asarray(e).reshape(9, 9)
    return sum(int(((p[b] == 0) & (e[b] == 0)).sum()) for b in range(9) if not mp[b] and not me[b])


def _alpha_beta(s, alpha, beta, count, max_nodes):
    """game.py:240-260, counting every invocation; the invocation that would be number max_nodes + 1 gives up."""
    if count[0] == max_nodes:
        raise _OutOfBudget
    count[0] += 1
    if s.is_lose():
        return -1
    legal = s.legal_actions()
    if not legal:
        return 0
    for a in legal:
        score = -_alpha_beta(s.next(a), -beta, -alpha, count, max_nodes)
        if score > alpha:
            alpha = score
        if alpha >= beta:
            return alpha
    return alpha


def solve_py(s, max_nodes):
    """(value, action, status, nodes, action_values[81]) of one oracle state, from the definition."""
    av = [UNKNOWN] * 81
    if s.is_lose():
        return -1, -1, SOLVED, 0, av
    legal = s.legal_actions()
    if not legal:
        return 0, -1, SOLVED, 0, av
    if empties_py(s) > MAX_EMPTY:
        return 0, -1, TOO_LARGE, 0, av
    nodes, unsolved = 0, 0
    for a in legal:
        count = [0]
        try:
            av[a] = -_alpha_beta(s.next(a), -1, 1, count, max_nodes)
        except _OutOfBudget:
            unsolved += 1
        nodes += count[0]
    known = [a for a in legal if av[a] != UNKNOWN]
    wins = [a for a in known if av[a] == 1]
    if wins:
        return 1, wins[0], SOLVED, nodes, av
    if not unsolved:
        best = max(av[a] for a in legal)
        return best, [a for a in legal if av[a] == best][0], SOLVED, nodes, av
    return 0, -1, BUDGET, nodes, av


# ------------------------------------------------------------------ helpers --
def pack(ostates):
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


def late_positions(core, count, max_empties, seed):
    """The first non-terminal position with at most max_empties empties of each of `count` seeded random games
    from the opening (games that end before they reach one are passed over)."""
    rng = random.Random(seed)
    out = []
    while len(out) < count:
        s = core.OrState.initial()
        while not s.is_done():
            if empties_py(s) <= max_empties:
                out.append(s)
                break
            s = s.next(rng.choice(s.legal_actions()))
    return out


def host_solve(lib, states, max_nodes, skip=()):
    """uttt_solve_host's outputs as a dict of arrays prefilled with 77; those named in `skip` are passed as NULL."""
    from uttt_amd._lib import UtttState
    states = np.ascontiguousarray(states)
    n = len(states)
    out = {"value": np.full(n, 77, np.int8), "action": np.full(n, 77, np.int8), "status": np.full(n, 77, np.int8),
           "nodes": np.full(n, 77, np.int64), "action_values": np.full((n, 81), 77, np.int8)}
    args = [None if k in skip else out[k].ctypes.data_as(ctypes.POINTER(
        ctypes.c_int64 if k == "nodes" else ctypes.c_int8)) for k in ("value", "action", "status", "nodes",
                                                                      "action_values")]
    rc = lib.uttt_solve_host(states.ctypes.data_as(ctypes.POINTER(UtttState)), n, max_nodes, *args)
    return rc, out


# Boards other than board 2 closed, nobody with a line on the main board: own holds 0, 1, 5, 7 (board 2 would
# complete the top row), the opponent 3, 4, 6, 8.
_MP = [1, 1, 0, 0, 0, 1, 0, 1, 0]
_ME = [0, 0, 0, 1, 1, 0, 1, 0, 1]


def board2_position(core, own_cells, opp_cells):
    p = np.zeros((9, 9), np.int32)
    e = np.zeros((9, 9), np.int32)
    p[2, own_cells] = 1
    e[2, opp_cells] = 1
    return core.OrState.from_arrays(p, e, _MP, _ME, 2)


def lost_position(core):
    z = np.zeros((9, 9), np.int32)
    return core.OrState.from_arrays(z, z, [0] * 9, [1, 0, 0, 0, 1, 0, 0, 0, 1], -1)


def drawn_position(core):
    z = np.zeros((9, 9), np.int32)
    return core.OrState.from_arrays(z, z, [1, 0, 1, 1, 0, 0, 0, 1, 1], [0, 1, 0, 0, 1, 1, 1, 0, 0], -1)


def open_boards_position(core, stones_per_board, active=-1):
    """Boards 0, 1, 5, 6, 7 closed for both sides (no three of them in a line), boards 2, 3, 4, 8 open with
    the given numbers of stones, alternating sides, no line: 36 - sum(stones) empties."""
    p = np.zeros((9, 9), np.int32)
    e = np.zeros((9, 9), np.int32)
    order = [0, 4, 8, 2, 6]  # own 0, opp 4, own 8, opp 2, own 6: no line within five stones
    for b, k in zip((2, 3, 4, 8), stones_per_board):
        for i in range(k):
            (p if i % 2 == 0 else e)[b, order[i]] = 1
    closed = [1, 1, 0, 0, 0, 1, 1, 1, 0]
    return core.OrState.from_arrays(p, e, closed, closed, active)


# -------------------------------------------------------------------- tests --
@pytest.fixture(scope="module")
def late10(oracle_lib):
    ostates = late_positions(oracle_lib, 60, 10, 2024)
    return ostates, pack(ostates)


@pytest.mark.parametrize("max_nodes", [65536, 16])
def test_host_equals_python_restatement(engine_lib, late10, max_nodes):
    ostates, packed = late10
    assert max(empties_py(s) for s in ostates) <= 10
    rc, got = host_solve(engine_lib, packed, max_nodes)
    assert rc == 0
    want = [solve_py(s, max_nodes) for s in ostates]
    for i, w in enumerate(want):
        assert (int(got["value"][i]), int(got["action"][i]), int(got["status"][i]), int(got["nodes"][i])) == w[:4], i
        assert got["action_values"][i].tolist() == w[4], i
    status = [w[2] for w in want]
    if max_nodes == 65536:
        assert all(x == SOLVED for x in status)
        values = [w[0] for w in want]
        assert all(values.count(v) >= 3 for v in (-1, 0, 1)), [values.count(v) for v in (-1, 0, 1)]
    else:
        assert SOLVED in status and BUDGET in status


def test_hand_built_positions(engine_lib, oracle_lib):
    core = oracle_lib
    win1 = board2_position(core, [0, 1, 5, 7], [3, 4, 6, 8])  # the only move, cell 2, wins board 2 and the game
    win2 = board2_position(core, [0, 1, 6, 8], [3, 4])        # cells 2 and 7 both win at once
    big = core.OrState.initial()
    at_cap = open_boards_position(core, [1, 1, 1, 1])       # 32 empties: searched
    over_cap = open_boards_position(core, [1, 1, 1, 0])     # 33: not searched
    assert empties_py(at_cap) == MAX_EMPTY and empties_py(over_cap) == MAX_EMPTY + 1
    ostates = [lost_position(core), drawn_position(core), win1, win2, big, at_cap, over_cap]
    assert ostates[0].is_lose() and ostates[1].is_draw() and win1.legal_actions() == [20]
    rc, got = host_solve(engine_lib, pack(ostates), 4096)
    assert rc == 0
    assert got["status"].tolist() == [SOLVED, SOLVED, SOLVED, SOLVED, TOO_LARGE, BUDGET, TOO_LARGE]
    assert got["value"].tolist() == [-1, 0, 1, 1, 0, 0, 0]
    assert got["action"].tolist() == [-1, -1, 20, 20, -1, -1, -1]
    assert got["nodes"][[0, 1, 4, 6]].tolist() == [0, 0, 0, 0]
    assert got["nodes"][2] == 1 and got["nodes"][5] == 4096 * 32
    for i in (0, 1, 4, 5, 6):
        assert (got["action_values"][i] == UNKNOWN).all()
    assert got["action_values"][2, 20] == 1 and (np.delete(got["action_values"][2], 20) == UNKNOWN).all()
    assert got["action_values"][3, 20] == 1 and got["action_values"][3, 25] == 1
    for i, s in enumerate(ostates[:5]):
        assert (int(got["value"][i]), int(got["action"][i]), int(got["status"][i]), int(got["nodes"][i])) == \
            solve_py(s, 4096)[:4], i


def test_value_is_the_largest_action_value(engine_lib, oracle_lib):
    ostates = late_positions(oracle_lib, 40, 12, 7)
    rc, got = host_solve(engine_lib, pack(ostates), 65536)
    assert rc == 0
    checked = 0
    for i, s in enumerate(ostates):
        legal = s.legal_actions()
        av = got["action_values"][i]
        assert (np.delete(av, legal) == UNKNOWN).all()
        if (av[legal] != UNKNOWN).all():
            assert got["status"][i] == SOLVED and got["value"][i] == av[legal].max()
            assert got["action"][i] == legal[int(np.argmax(av[legal]))]
            checked += 1
        elif got["status"][i] == SOLVED:
            assert got["value"][i] == 1 and av[got["action"][i]] == 1
    assert checked >= 20


def test_null_outputs_are_accepted(engine_lib, late10):
    packed = late10[1][:8]
    rc, full = host_solve(engine_lib, packed, 4096)
    assert rc == 0
    names = ("value", "action", "status", "nodes", "action_values")
    for skip in [(k,) for k in names] + [names]:
        rc, got = host_solve(engine_lib, packed, 4096, skip=skip)
        assert rc == 0
        for k in names:
            assert (got[k] == 77).all() if k in skip else np.array_equal(got[k], full[k]), (skip, k)


def test_arguments_are_checked(engine_lib):
    from uttt_amd import initial_states
    from uttt_amd._lib import UtttState
    for max_nodes in (0, -1, (1 << 22) + 1):
        rc, got = host_solve(engine_lib, initial_states(1), max_nodes)
        assert rc == -1 and got["status"][0] == 77  # UTTT_ERR_ARG, nothing written
        assert b"max_nodes" in engine_lib.uttt_last_error()
    rc, _ = host_solve(engine_lib, initial_states(1), 1 << 22)
    assert rc == 0
    st = initial_states(1)
    sp = st.ctypes.data_as(ctypes.POINTER(UtttState))
    assert engine_lib.uttt_solve_host(sp, -1, 16, None, None, None, None, None) == -1
    assert engine_lib.uttt_solve_host(None, 1, 16, None, None, None, None, None) == -1
    assert engine_lib.uttt_solve_host(None, 0, 16, None, None, None, None, None) == 0
    st["active"] = 9
    assert engine_lib.uttt_solve_host(sp, 1, 16, None, None, None, None, None) == -1


def test_python_layer_on_the_host(engine_lib, oracle_lib, late10):
    """solver.solve_host is the same call; empties and states_from_inputs agree with the oracle; a blunder report
    counts the plies it should."""
    from uttt_amd import solver
    ostates, packed = late10
    assert (solver.SOLVED, solver.BUDGET, solver.TOO_LARGE, solver.UNKNOWN, solver.MAX_EMPTY) == \
        (SOLVED, BUDGET, TOO_LARGE, UNKNOWN, MAX_EMPTY)
    rc, want = host_solve(engine_lib, packed, 65536)
    got = solver.solve_host(packed, 65536)
    for k, g in zip(("value", "action", "status", "nodes", "action_values"), got):
        assert g.dtype == want[k].dtype and np.array_equal(g, want[k]), k
    more = ostates + [oracle_lib.OrState.initial(), open_boards_position(oracle_lib, [1, 1, 1, 1])]
    assert solver.empties(pack(more)).tolist() == [empties_py(s) for s in more]
    rebuilt = solver.states_from_inputs(np.stack([s.tensor_hwc() for s in ostates]))
    again = solver.solve_host(rebuilt, 65536)
    for g, a in zip(got, again):
        assert np.array_equal(g, a)
    # every position played its best move: no blunders; its worst: a blunder wherever the values differ
    value, action, status, _, av = got
    assert (status == SOLVED).all()
    rep = solver.blunder_report(packed, action)
    assert rep["plies"] == len(packed) and rep["countable"].sum() == len(packed) and rep["blunders"].sum() == 0
    assert rep["countable"].tolist() == np.bincount([empties_py(s) for s in ostates], minlength=33).tolist()
    worst = np.array([min(s.legal_actions(), key=lambda a: av[i, a]) for i, s in enumerate(ostates)])
    differ = av[np.arange(len(packed)), worst] < value
    rep = solver.blunder_report(np.stack([s.tensor_hwc() for s in ostates]), worst)
    assert rep["blunders"].sum() == differ.sum() > 0
    with pytest.raises(ValueError):
        solver.blunder_report(packed, action[:-1])
