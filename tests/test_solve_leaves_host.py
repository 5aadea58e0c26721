"""CPU tests of the solver overlay's host side (uttt_solve_overlay_host, csrc/uttt_solve.h): it
equals a restatement in numpy on top of solver.solve_host in every row, status and untouched bit, over both
budgets, three depth limits, both priors modes, a padded row stride and a NULL status; hand-built won, lost and
drawn positions; argument checks; the Python layer."""
import ctypes

import numpy as np
import pytest

from test_solve_host import (BUDGET, SOLVED, UNKNOWN, board2_position, drawn_position, empties_py, late_positions,
                             lost_position, pack)

SKIPPED, KEEP, OPTIMAL = 0, 0, 1


_SOLVED = {}


def overlay_np(states, ostates, policy, value, max_empties, max_nodes, priors):
    """The definition: rows (copies) after the overlay, and the statuses."""
    from uttt_amd import solver
    policy, value = policy.copy(), value.copy()
    key = (states.tobytes(), max_nodes)
    if key not in _SOLVED:  # one solve per budget, shared by the cases
        _SOLVED[key] = solver.solve_host(states, max_nodes)
    v, _, st, _, av = _SOLVED[key]
    status = np.where(solver.empties(states) > max_empties, SKIPPED, st).astype(np.int8)
    for i in np.flatnonzero(status == SOLVED):
        value[i] = np.float32(v[i])
        if priors == OPTIMAL and not ostates[i].is_done():
            policy[i, :81] = ((av[i] != UNKNOWN) & (av[i] == v[i])).astype(np.float32)
    return policy, value, status


def overlay_c(lib, states, policy, value, max_empties, max_nodes, priors, with_status=True):
    from uttt_amd._lib import UtttState
    states = np.ascontiguousarray(states)
    status = np.full(len(states), 77, np.int8)
    f32 = ctypes.POINTER(ctypes.c_float)
    rc = lib.uttt_solve_overlay_host(states.ctypes.data_as(ctypes.POINTER(UtttState)), len(states), max_empties,
                                     max_nodes, priors, policy.ctypes.data_as(f32), policy.strides[0] // 4,
                                     value.ctypes.data_as(f32), value.strides[0] // 4,
                                     status.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)) if with_status else None)
    return rc, status


def random_rows(n, ld, seed):
    rng = np.random.RandomState(seed)
    return rng.rand(n, ld).astype(np.float32), (rng.rand(n).astype(np.float32) * 2 - 1)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def mixed(oracle_lib):
    """About 60 positions from the tails of random games: at most 10 empties, and 17..20 empties (the first
    position of a game with at most 20; deeper ones would search for minutes on the CPU at the large budget)."""
    small = late_positions(oracle_lib, 46, 10, 11)
    large = [s for s in late_positions(oracle_lib, 40, 20, 12) if empties_py(s) > 16][:14]
    assert len(large) == 14
    ostates = [s for pair in zip(small, large) for s in pair] + small[len(large):]
    return ostates, pack(ostates)


@pytest.mark.parametrize("max_nodes", [65536, 16])
@pytest.mark.parametrize("max_empties", [0, 10, 32])
def test_host_equals_the_restatement(engine_lib, mixed, max_nodes, max_empties):
    ostates, packed = mixed
    seen = set()
    for priors in (KEEP, OPTIMAL):
        for ld in (81, 96):
            policy, value = random_rows(len(packed), ld, 5 + ld + priors)
            want_p, want_v, want_s = overlay_np(packed, ostates, policy, value, max_empties, max_nodes, priors)
            before_p, before_v = policy.copy(), value.copy()
            rc, status = overlay_c(engine_lib, packed, policy, value, max_empties, max_nodes, priors,
                                   with_status=(ld == 81))
            assert rc == 0
            if ld == 81:
                assert status.tolist() == want_s.tolist()
            else:
                assert (status == 77).all()  # NULL: not written
            assert np.array_equal(bits(policy), bits(want_p)) and np.array_equal(bits(value), bits(want_v))
            untouched = want_s != SOLVED
            assert np.array_equal(bits(policy[untouched]), bits(before_p[untouched]))
            assert np.array_equal(bits(value[untouched]), bits(before_v[untouched]))
            assert np.array_equal(bits(policy[:, 81:]), bits(before_p[:, 81:]))  # the padding of every row
            if priors == KEEP:
                assert np.array_equal(bits(policy), bits(before_p))
            seen |= set(want_s.tolist())
    if max_empties == 0:
        assert seen == {SKIPPED}
    elif max_empties == 10:
        assert SKIPPED in seen and SOLVED in seen
        assert (BUDGET in seen) == (max_nodes == 16)
    else:
        assert SOLVED in seen and BUDGET in seen


def test_hand_built_positions(engine_lib, oracle_lib):
    core = oracle_lib
    win1 = board2_position(core, [0, 1, 5, 7], [3, 4, 6, 8])  # the only move, cell 2, wins the game
    # cells 2 and 3 win at once; after 7 or 8 the opponent's cell 3 wins board 2 and with it the game
    win2 = board2_position(core, [0, 1, 6], [4, 5])
    lost = lost_whatever(core)
    drawn = drawn_at_best(core)
    # terminal: lost with every board closed, drawn, and lost with 81 empties in open boards (past any limit)
    ostates = [win1, win2, lost, drawn, win1.next(20), drawn_position(core), lost_position(core)]
    assert ostates[4].is_lose() and empties_py(ostates[4]) == 0 and ostates[6].is_lose()
    packed = pack(ostates)
    legal = [s.legal_actions() for s in ostates]
    assert legal[0] == [20] and legal[1] == [20, 21, 25, 26]
    policy, value = random_rows(len(packed), 81, 3)
    before = policy.copy()
    rc, status = overlay_c(engine_lib, packed, policy, value, 32, 65536, OPTIMAL)
    assert rc == 0 and status.tolist() == [SOLVED] * 6 + [SKIPPED]
    assert value[:6].tolist() == [1.0, 1.0, -1.0, 0.0, -1.0, 0.0] and value[6] == random_rows(7, 81, 3)[1][6]
    assert np.flatnonzero(policy[0]).tolist() == [20] and policy[0, 20] == 1.0
    assert np.flatnonzero(policy[1]).tolist() == [20, 21] and policy[1, [20, 21, 25, 26]].tolist() == [1, 1, 0, 0]
    assert np.flatnonzero(policy[2]).tolist() == legal[2] and len(legal[2]) > 1  # lost: every move marked
    marked = np.flatnonzero(policy[3]).tolist()
    assert marked and set(marked) <= set(legal[3])
    for i in range(4):
        assert set(np.unique(policy[i]).tolist()) <= {0.0, 1.0}
    assert np.array_equal(bits(policy[4:]), bits(before[4:]))  # terminal: the value alone, or nothing
    # the marks of the drawn position are its moves of value 0, by the solver
    from uttt_amd import solver
    v, _, _, _, av = solver.solve_host(packed[3:4], 65536)
    assert v[0] == 0 and marked == np.flatnonzero(av[0] == 0).tolist()
    assert (av[0][legal[3]] <= 0).all()


def lost_whatever(core):
    """Board 2 alone is open, the mover must play in it and cannot win it at once, the opponent holds main
    boards 3, 4, 6, 8 and wins the game with board 2 (the line 2-4-6): in board 2 it has two open twos
    (cells 0, 1 and cells 3, 4), so whichever cell the mover takes, the other line completes."""
    p = np.zeros((9, 9), np.int32)
    e = np.zeros((9, 9), np.int32)
    e[2, [0, 1, 3, 4]] = 1
    p[2, [8]] = 1  # one stone: no line of its own to complete
    mp = [1, 1, 0, 0, 0, 1, 0, 1, 0]
    me = [0, 0, 0, 1, 1, 0, 1, 0, 1]
    return core.OrState.from_arrays(p, e, mp, me, 2)


def drawn_at_best(core):
    """Board 2 alone is open with two empty cells (2 and 5): nobody can complete a line in it, and no line on the
    main board is left for either side: the mover's best is the draw."""
    p = np.zeros((9, 9), np.int32)
    e = np.zeros((9, 9), np.int32)
    p[2, [0, 4, 7]] = 1
    e[2, [1, 3, 6, 8]] = 1
    mp = [1, 0, 0, 0, 1, 1, 1, 0, 0]
    me = [0, 1, 0, 1, 0, 0, 0, 1, 1]
    return core.OrState.from_arrays(p, e, mp, me, 2)


def test_hand_built_positions_are_what_they_claim(oracle_lib):
    """The two positions above by the pure-Python definition of test_solve_host."""
    from test_solve_host import solve_py
    s = lost_whatever(oracle_lib)
    value, _, status, _, av = solve_py(s, 65536)
    assert (value, status) == (-1, SOLVED) and all(av[a] == -1 for a in s.legal_actions())
    s = drawn_at_best(oracle_lib)
    value, _, status, _, av = solve_py(s, 65536)
    assert (value, status) == (0, SOLVED) and not s.is_done()


def test_arguments_are_checked(engine_lib):
    from uttt_amd import initial_states
    st = initial_states(1)
    for kw, word in (({"max_empties": 33}, b"max_empties"), ({"max_empties": -1}, b"max_empties"),
                     ({"max_nodes": 0}, b"max_nodes"), ({"max_nodes": (1 << 22) + 1}, b"max_nodes"),
                     ({"priors": 2}, b"priors"), ({"priors": -1}, b"priors")):
        args = {"max_empties": 10, "max_nodes": 16, "priors": OPTIMAL, **kw}
        policy, value = random_rows(1, 81, 0)
        before = policy.copy()
        rc, status = overlay_c(engine_lib, st, policy, value, **args)
        assert rc == -1 and status[0] == 77 and np.array_equal(policy, before), kw  # UTTT_ERR_ARG, nothing written
        assert word in engine_lib.uttt_last_error(), kw
    policy, value = random_rows(1, 80, 0)
    rc, _ = overlay_c(engine_lib, st, policy, value, 10, 16, KEEP)
    assert rc == -1 and b"policy_ld" in engine_lib.uttt_last_error()
    policy, value = random_rows(1, 81, 0)
    assert overlay_c(engine_lib, st, policy, value, 32, 1 << 22, KEEP)[0] == 0
    assert overlay_c(engine_lib, st, policy, value, 0, 1, OPTIMAL)[0] == 0
    st["active"] = 9
    assert overlay_c(engine_lib, st, policy, value, 10, 16, KEEP)[0] == -1


def test_python_layer_on_the_host(engine_lib, mixed):
    from uttt_amd import solver
    ostates, packed = mixed
    assert (solver.SKIPPED, solver.PRIORS_KEEP, solver.PRIORS_OPTIMAL) == (SKIPPED, KEEP, OPTIMAL)
    wide, value = random_rows(len(packed), 96, 9)
    policy = wide[:, 8:92]  # a view: rows 96 floats apart, 84 wide
    want_p, want_v, want_s = overlay_np(packed, ostates, policy, value, 10, 4096, OPTIMAL)
    status = solver.overlay_host(packed, policy, value, 10, 4096, "optimal")
    assert status.dtype == np.int8 and status.tolist() == want_s.tolist()
    assert np.array_equal(bits(policy), bits(want_p)) and np.array_equal(bits(value), bits(want_v))
    col = np.zeros((len(packed), 1), np.float32)
    assert solver.overlay_host(packed, policy, col, 10, 4096, solver.PRIORS_KEEP).tolist() == want_s.tolist()
    assert np.array_equal(col[:, 0][want_s == SOLVED], want_v[want_s == SOLVED])
    with pytest.raises(ValueError):
        solver.overlay_host(packed, policy, value, 10, 4096, "best")
    with pytest.raises(ValueError):
        solver.overlay_host(packed, policy.astype(np.float64), value, 10, 4096, "keep")
    with pytest.raises(ValueError):
        solver.overlay_host(packed, policy[:, :80], value, 10, 4096, "keep")
    with pytest.raises(ValueError):
        solver.overlay_host(packed, policy, value, 40, 4096, "keep")
