"""GPU tests of the exact endgame solver: k_solve_states (uttt_solve) against uttt_solve_host bit for bit in all
five outputs (the host is checked on its own against a pure-Python restatement in test_solve_host.py); the cap and
independence from a search in progress; blunder_report and alpha_beta_action_factory; the engine's lifecycle."""
import numpy as np
import pytest

from test_solve_host import (BUDGET, MAX_EMPTY, SOLVED, TOO_LARGE, board2_position, drawn_position, empties_py,
                             host_solve, late_positions, lost_position, open_boards_position, pack)

pytestmark = pytest.mark.gpu

WAVES_PER_BLOCK = 4  # csrc/engine/layout.h kWavesPerBlock: one wave per position
NAMES = ("value", "action", "status", "nodes", "action_values")


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import uttt_amd
    return uttt_amd


@pytest.fixture(scope="module")
def batch(oracle_lib):
    """67 roots with at most 12 empties (but the one too large): two late positions, then a lost, a drawn and
    the initial position, a root with a single legal move and a free-move root, another single-move root (its
    move fills board 2 with no line, which closes it for both sides), then more late positions."""
    core = oracle_lib
    late = late_positions(core, 90, 12, 99)
    free = [s for s in late if s.arrays()[4] == -1 and len(s.legal_actions()) > 1]
    rest = [s for s in late if s is not free[0]]
    single = board2_position(core, [0, 1, 5, 7], [3, 4, 6, 8])
    single2 = board2_position(core, [1, 3, 5, 8], [0, 2, 4, 7])
    ostates = (rest[:2] + [lost_position(core), drawn_position(core), core.OrState.initial(), single, free[0],
                           single2] + rest[2:])[:67]
    assert len(ostates) == 67 and single.legal_actions() == [20] and single2.legal_actions() == [24]
    assert all(empties_py(s) <= 12 for i, s in enumerate(ostates) if i != 4 and not s.is_done())
    assert sum(len(s.legal_actions()) == 1 for s in ostates) >= 2
    return ostates, pack(ostates)


def assert_equal_to_host(lib, got, states, max_nodes, tag):
    rc, want = host_solve(lib, states, max_nodes)
    assert rc == 0
    for k, g in zip(NAMES, got):
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (tag, k)
        assert np.array_equal(g, want[k]), (tag, k, np.nonzero(g != want[k])[0][:8])
    return want


@pytest.mark.parametrize("n", [1, WAVES_PER_BLOCK + 1, 67])
def test_kernel_equals_host(gpu, engine_lib, batch, n):
    """A lone wave, a partial workgroup, a grid tail; a budget every search fits and one that stops some lanes
    of a wave while others finish."""
    packed = batch[1]
    st = packed[:n] if n != WAVES_PER_BLOCK + 1 else packed[2:2 + n]  # the five special roots
    eng = gpu.Engine(4, 50)
    for max_nodes in (4096, 16):
        want = assert_equal_to_host(engine_lib, eng.solve(st, max_nodes), st, max_nodes, (n, max_nodes))
        if n == WAVES_PER_BLOCK + 1:
            assert want["status"].tolist() == [SOLVED, SOLVED, TOO_LARGE, SOLVED, want["status"][4]]
            assert want["value"][:4].tolist() == [-1, 0, 0, 1] and want["action"][:4].tolist() == [-1, -1, -1, 20]
        if n == 67 and max_nodes == 16:
            assert BUDGET in want["status"] and SOLVED in want["status"]
            # lanes of one wave on both sides of the budget
            some = (want["action_values"] != -128).any(axis=1) & (want["status"] == BUDGET)
            assert some.any()
        if n == 67 and max_nodes == 4096:
            assert (want["status"] == SOLVED).sum() >= 60 and {-1, 0, 1} <= set(want["value"].tolist())
    assert eng.kernel_stats("solve")["launches"] == 2
    with pytest.raises(ValueError):
        eng.solve(st, 0)
    with pytest.raises(ValueError):
        eng.solve(st, (1 << 22) + 1)


def test_cap_and_null_outputs(gpu, engine_lib, oracle_lib):
    """A position at exactly the cap, every lane cut short at 64 nodes: BUDGET with the host's node count (the
    lanes' deepest frames are in use); one empty more is TOO_LARGE. NULL outputs are skipped."""
    import ctypes
    from uttt_amd._lib import UtttState
    at_cap = open_boards_position(oracle_lib, [1, 1, 1, 1])
    over = open_boards_position(oracle_lib, [1, 1, 1, 0])
    assert empties_py(at_cap) == MAX_EMPTY and len(at_cap.legal_actions()) == 32
    st = pack([at_cap, over])
    eng = gpu.Engine(1, 50)
    want = assert_equal_to_host(engine_lib, eng.solve(st, 64), st, 64, "cap")
    assert want["status"].tolist() == [BUDGET, TOO_LARGE] and want["nodes"].tolist() == [64 * 32, 0]
    assert (want["action_values"] == -128).all()
    nodes = np.full(2, 77, np.int64)
    assert eng.lib.uttt_solve(eng.h, st.ctypes.data_as(ctypes.POINTER(UtttState)), 2, 64, None, None, None,
                              nodes.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), None) == 0
    assert nodes.tolist() == [64 * 32, 0]
    assert eng.lib.uttt_solve(eng.h, None, 1, 64, None, None, None, None, None) == -1
    assert eng.lib.uttt_solve(eng.h, None, 0, 64, None, None, None, None, None) == 0


def test_solve_is_independent_of_a_search_in_progress(gpu, engine_lib, batch):
    """A solve between uttt_search_select and uttt_search_apply leaves the search's root visits what they are
    without it, and is itself the host's."""
    import torch
    packed = batch[1]
    roots = gpu.initial_states(8)
    out = []
    for interleave in (False, True):
        bs = gpu.BatchedSearch(len(roots), 50)
        e = bs.engine
        e.search_begin(roots, 50, 8)
        pol = torch.zeros((len(roots), 81), dtype=torch.float32, device=bs.x.device)
        val = torch.zeros(len(roots), dtype=torch.float32, device=bs.x.device)
        rounds = 0
        while True:
            n = e.select(bs.x)
            if n == 0:
                break
            e.eval_hash(bs.x, n, pol, val)
            if interleave and rounds % 2 == 0:
                assert_equal_to_host(engine_lib, e.solve(packed[:9], 256), packed[:9], 256, rounds)
            e.apply(pol[:n], val[:n])
            rounds += 1
        assert rounds > 2
        out.append([v.copy() for v in e.root_visits()])
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert (out[0][0].sum(axis=1) == 50).all()


def test_blunder_report_on_golden_records(gpu):
    from conftest import golden
    from uttt_amd import solver
    d = golden("selfplay.npz")
    eng = gpu.Engine(1, 50)
    dev = solver.blunder_report(d["tensors"], d["actions"], 4096, engine=eng)
    host = solver.blunder_report(d["tensors"], d["actions"], 4096)
    assert dev["plies"] == host["plies"] == len(d["actions"])
    for k in ("countable", "blunders"):
        assert dev[k].dtype == np.int64 and dev[k].shape == (MAX_EMPTY + 1,) and np.array_equal(dev[k], host[k]), k
    assert host["countable"].sum() >= 50 and 0 < host["blunders"].sum() < host["countable"].sum()
    assert (host["blunders"] <= host["countable"]).all()
    # the packed states the engine's own records hold give the same report
    st = solver.states_from_inputs(d["tensors"])
    again = solver.blunder_report(st, d["actions"], 4096, engine=eng)
    assert np.array_equal(again["countable"], host["countable"]) and np.array_equal(again["blunders"], host["blunders"])


def test_alpha_beta_action_factory(gpu, engine_lib, batch):
    import evaluate_best_player
    import uttt_cpp
    ostates, packed = batch
    assert evaluate_best_player.EP_VS_ALPHABETA is False
    asked = []

    def fallback(state):
        asked.append(state)
        return state.legal_actions()[-1]

    next_action = evaluate_best_player.alpha_beta_action_factory(4096, fallback)
    rc, want = host_solve(engine_lib, packed, 4096)
    tried = 0
    for i in (0, 1, 5, 6, 7, 8):
        p, e, mp, me, act = ostates[i].arrays()
        state = uttt_cpp.State(p.tolist(), e.tolist(), mp.tolist(), me.tolist(), act)
        assert want["status"][i] == SOLVED
        assert next_action(state) == want["action"][i] and want["action"][i] in state.legal_actions()
        tried += 1
    assert tried == 6 and not asked
    opening = uttt_cpp.State()
    assert next_action(opening) == 80 and len(asked) == 1
    # a budget too small for a late position falls back as well
    tight = evaluate_best_player.alpha_beta_action_factory(1, fallback)
    i = int(np.nonzero(host_solve(engine_lib, packed, 1)[1]["status"] == BUDGET)[0][0])
    p, e, mp, me, act = ostates[i].arrays()
    state = uttt_cpp.State(p.tolist(), e.tolist(), mp.tolist(), me.tolist(), act)
    assert tight(state) == state.legal_actions()[-1] and len(asked) == 2


def test_engine_lifecycle_with_solves(gpu, engine_lib, batch):
    """Create -> solve 1 and 1,100 positions (past the solve buffers' first capacity of 1,024 rows) -> destroy,
    three times over in one process; every result is the host's."""
    from uttt_amd.engine import Engine
    st = np.resize(batch[1], 1100)
    rc, want = host_solve(engine_lib, st, 64)
    assert rc == 0
    for _ in range(3):
        e = Engine(4, 8)
        for n in (1, 1100):
            for k, g in zip(NAMES, e.solve(st[:n], 64)):
                assert np.array_equal(g, want[k][:n]), (n, k)
        assert e.lib.uttt_engine_destroy(e.h) == 0
        e.h = None
