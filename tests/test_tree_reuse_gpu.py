"""Tree reuse on the GPU (k_reroot, csrc/engine/reroot.h), hash evaluator throughout: the kernel's
pool against uttt_reroot_host byte for byte, the topped-up search and whole self-play games against the Python model
(tests/tree_reuse_model.py), independence of the driver and of the slot count, off meaning off, and the refusals."""
import ctypes

import numpy as np
import pytest

import tree_reuse_model as M
import wide_deep
from conftest import golden
from test_tree_reuse_host import FIXTURE_ROWS, fixture_state

pytestmark = pytest.mark.gpu

NOISE = (0.25, 0.3, 5)


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import uttt_amd
    return uttt_amd


def raw(tree):
    from uttt_amd import reuse
    return reuse.pack(tree).tobytes()


def run_rounds(gpu, e, x, ev):
    """The search's rounds to its end: select, hash evaluation, apply."""
    while True:
        n = e.select(x)
        if n == 0:
            break
        p, v = ev(x, n)
        e.apply(p, v)


# A second evaluator, for shapes the hash evaluator's concentrated visits do not reach: the same row for every
# position, priors rising with the action's square, value 0. Under a promoted node the visits then go to the high
# ranks, and with B = 1 a root's uniform priors and Q = 0 spread one visit over every child in turn.
TILT = np.arange(1, 82, dtype=np.float32) ** 2


def tilted(state):
    return TILT, np.float32(0.0)


class TiltedRows:
    """`tilted` as the engine's evaluator: rows applied from host arrays."""

    def __call__(self, x, n):
        return np.tile(TILT, (n, 1)), np.zeros(n, np.float32)


def ranked_action(tree, rank):
    """The root's move with the rank-th most visits (ties: the lower action)."""
    L = int(tree[0]["L"])
    order = sorted(range(L), key=lambda i: (-int(tree["N"][1 + i]), i))
    return int(tree["action"][1 + order[rank]])


def reroot_and_check(gpu, ostates, S, B, ranks, fallback_tree=None, tilt=False):
    """Search every root, re-root tree t at its ranks[t]-th most visited move (fallback_tree: at an unvisited one),
    compare the pool with the host mirror and with the model, finish the topped-up search, compare with the model."""
    import torch
    from uttt_amd import reuse
    roots = wide_deep.pack_states(ostates)
    n = len(roots)
    e = gpu.Engine(n, S)
    e.set_timing(True)
    e.set_tree_reuse(True)
    dev = torch.device("cuda", e.device)
    x = torch.zeros((n, 3, 9, 9), dtype=torch.float32, device=dev)
    ev = TiltedRows() if tilt else gpu.HashEvaluator(e)
    e.search_begin(roots, S, B)
    run_rounds(gpu, e, x, ev)
    before = [e.tree(t) for t in range(n)]
    models = {}
    for t, s in enumerate(ostates):  # identical roots share one model tree
        key = roots[t].tobytes()
        if key not in models:
            models[key] = (M.Tree(s, tilted) if tilt else M.Tree(s)).search(S, B)
        assert raw(before[t]) == raw(models[key].as_array()), ("search", t)
    # ranks[t]: the rank by visits, or ("move", i): the root's i-th move (negative: from the end)
    actions = [int(before[t]["action"][1 + r[1] % int(before[t][0]["L"])]) if isinstance(r, tuple)
               else ranked_action(before[t], r) for t, r in enumerate(ranks)]
    if fallback_tree is not None:
        tr = before[fallback_tree]
        cold = [int(tr["action"][1 + i]) for i in range(int(tr[0]["L"])) if tr["N"][1 + i] == 0]
        assert cold
        actions[fallback_tree] = cold[-1]
    e.reroot(actions, S)
    assert e.kernel_stats("reroot")["launches"] == 1
    after = [e.tree(t) for t in range(n)]
    for t in range(n):
        want = reuse.reroot_host(before[t], roots[t:t + 1], actions[t])
        assert len(after[t]) == len(want), (t, len(after[t]), len(want))
        assert raw(after[t]) == raw(want), ("reroot", t)
        c = before[t][1 + list(before[t]["action"][1:1 + before[t][0]["L"]]).index(actions[t])]
        if t == fallback_tree:
            assert c["k"] == 0 and int(after[t][0]["N"]) == 0 and len(after[t]) == 1 + int(after[t][0]["L"])
        elif ranks[t] == 0:  # the most visited move was expanded: the pool holds its subtree
            assert c["k"] > 0 and int(after[t][0]["N"]) == c["N"] - c["k"] and len(after[t]) >= 1 + int(after[t][0]["L"])
    # the topped-up search
    run_rounds(gpu, e, x, ev)
    visits, L = e.root_visits()
    scores, _ = e.scores(1.0)
    for t, s in enumerate(ostates):
        m = models[roots[t].tobytes()].reroot(actions[t])
        carried = m.done
        m.search(S, B)
        assert L[t] == len(m.legal()) and visits[t].sum() == S, t
        assert np.array_equal(visits[t, :L[t]], m.visits()), (t, carried)
        assert np.array_equal(scores[t, :L[t]].view(np.uint32), m.scores(1.0).view(np.uint32)), t
        assert raw(e.tree(t)) == raw(m.as_array()), ("topped up", t)
    e.close()
    return before, after, actions


# ------------------------------------------------------------------ 1, 2 --
def eight_roots(core):
    s0 = core.OrState.initial()
    fa, fb = (fixture_state(core, i) for i in FIXTURE_ROWS)
    return [s0, fa, fb, s0, fa, fb, s0, fa]


def test_kernel_equals_the_mirror_and_the_search_goes_on(gpu, oracle_lib):
    """8 trees from the initial position and two mid-game fixture positions, S = 16, B = 4: trees 0-2 re-rooted at
    their most visited move, the repeats of the same roots at the second and third most visited."""
    reroot_and_check(gpu, eight_roots(oracle_lib), 16, 4, [0, 0, 0, 1, 1, 1, 2, 2])


def promoted_shape(tree, action):
    """Of the root's child c with `action`: its rank in the root's block, k_c, L', the records each 64-item step of
    the level-2 copy appends (items: the duplicates, move by move and copy by copy), and the records under the
    merged children of rank 64 and up."""
    L0 = int(tree[0]["L"])
    rank = list(tree["action"][1:1 + L0]).index(action)
    c = tree[1 + rank]
    kc, Lp, fc = int(c["k"]), int(c["L"]), int(c["first"])
    sizes = [int(tree[fc + i * Lp + r]["k"]) * int(tree[fc + i * Lp + r]["L"]) for r in range(Lp) for i in range(kc)]
    steps = [sum(sizes[q:q + 64]) for q in range(0, len(sizes), 64)]
    return {"rank": rank, "kc": kc, "Lp": Lp, "steps": steps, "high": sum(sizes[64 * kc:])}


def test_wide_promoted_nodes_take_more_than_one_scan_group(gpu, oracle_lib):
    """B = 8 from the initial position: the promoted child holds 8 duplicate sets of its 9 moves (72 level-1
    duplicates: two steps of the level-2 copy) and flushes of 8 x L records below. (No position reached from the
    initial one has 81 moves again, so 8 x 81 children under a promoted node cannot be built; the next test
    builds the widest there is.)"""
    s0 = oracle_lib.OrState.initial()
    before, after, actions = reroot_and_check(gpu, [s0, s0], 40, 8, [0, 1])
    shape = promoted_shape(before[0], actions[0])
    assert shape["kc"] == 8 and shape["kc"] * shape["Lp"] > 64 and len(shape["steps"]) == 2
    assert len(after[0]) > 1 + 64  # and the scan reads more than one group of records


def test_promoted_nodes_with_more_than_64_moves(gpu, oracle_lib):
    """What the kernel does in halves and chunks, which the host mirror does not have. The tilted evaluator,
    S = 200, B = 8, on a position one move away from a free-move position with 66 moves, re-rooted at that move:
    the promoted node has L' > 64, so lanes merge a second half of ranks (64 and up), some of which were expanded
    (their blocks' places come after the first half's total); and one step of the level-2 copy appends more than
    256 records, the lane-parallel copy's second chunk of 4 x 64."""
    parent = list(wide_deep.wide_parents(2, wide_deep.WIDE_SEED)[1])[1]
    wide = next(a for a in parent.legal_actions() if len(parent.next(a).legal_actions()) > 64)
    move = parent.legal_actions().index(wide)
    before, after, actions = reroot_and_check(gpu, [parent], 200, 8, [("move", move)], tilt=True)
    shape = promoted_shape(before[0], actions[0])
    assert actions[0] == wide and shape["kc"] == 8 and shape["Lp"] > 64, shape
    assert shape["high"] > 0, shape         # merged children of rank >= 64 with blocks of their own
    assert max(shape["steps"]) > 256, shape  # one copy_blocks call with a second chunk
    assert int(after[0][0]["N"]) > 0 and len(after[0]) > 1 + shape["Lp"] + 256


def test_played_move_in_the_second_half_of_a_wide_root(gpu, oracle_lib):
    """Two roots with 66-70 legal moves, tilted evaluator, S = 140, B = 1: uniform root priors and Q = 0 visit every
    child of the root in turn, so the last moves (ranks 64 and up: the second ballot that looks for the played
    child) are expanded, and their subtrees are carried."""
    ost = list(wide_deep.wide_roots(2, wide_deep.WIDE_SEED)[1])
    before, after, actions = reroot_and_check(gpu, ost, 140, 1, [("move", -1), ("move", -2)], tilt=True)
    for t in range(2):
        shape = promoted_shape(before[t], actions[t])
        assert shape["rank"] >= 64 and shape["kc"] == 1, shape
        assert int(after[t][0]["N"]) >= 1 and len(after[t]) > 1 + shape["Lp"]


def test_one_tree_falls_back_to_a_fresh_root(gpu, oracle_lib):
    reroot_and_check(gpu, eight_roots(oracle_lib)[:4], 16, 4, [0, 0, 0, 0], fallback_tree=2)


# ------------------------------------------------------------------ 3 --
N_GAMES, SEED_BASE, SP_S, SP_B = 6, 300, 8, 4


@pytest.fixture(scope="module")
def model_games(oracle_lib):
    return {noise: [M.play_game(SEED_BASE + g, SP_S, SP_B, reuse=True, noise=noise, game=g) for g in range(N_GAMES)]
            for noise in (None, NOISE)}


def selfplay_records(gpu, monkeypatch, driver, slots=4, noise=None, reuse=True):
    monkeypatch.setenv("UTTT_ASYNC_ROUNDS", "0" if driver == "blocking" else "1")
    monkeypatch.setenv("UTTT_MOVE_LOOP", "1" if driver == "move_loop" else "0")
    sp = gpu.SelfPlay(slots, SP_S, SP_B, 1.0, cache_log2=0, tree_reuse=reuse, root_noise=noise)
    assert sp._device_count() != (driver == "blocking")
    sp.set_timing(driver != "async")  # one driver launches k_reroot as an ordinary launch, the others with events
    sp.run(0, N_GAMES, SEED_BASE)
    recs = sp.records(with_inputs=False)
    assert [r["game"] for r in recs] == list(range(N_GAMES))
    return recs, sp


def assert_games_equal(recs, want):
    for g, (r, w) in enumerate(zip(recs, want)):
        assert np.array_equal(r["actions"], w["actions"]), g
        assert np.array_equal(r["policies"].view(np.uint64), w["policies"].view(np.uint64)), g
        assert np.array_equal(r["values"], w["values"]), g


@pytest.mark.parametrize("driver", ("blocking", "async", "move_loop"))
def test_selfplay_games_equal_the_model(gpu, monkeypatch, model_games, driver):
    """4 slots, 6 games: slots are refilled with new games (fresh roots) while the others carry their trees."""
    recs, sp = selfplay_records(gpu, monkeypatch, driver)
    assert_games_equal(recs, model_games[None])
    assert sp.kernel_stats("reroot")["launches"] >= sp.kernel_stats("move_end")["launches"] > 0


def test_selfplay_with_root_noise_equals_the_model(gpu, monkeypatch, model_games):
    recs, sp = selfplay_records(gpu, monkeypatch, "blocking", noise=NOISE)
    assert_games_equal(recs, model_games[NOISE])
    recs, sp = selfplay_records(gpu, monkeypatch, "move_loop", noise=NOISE)
    assert_games_equal(recs, model_games[NOISE])
    assert any(not np.array_equal(a["actions"], b["actions"]) for a, b in zip(model_games[None], model_games[NOISE]))


# ------------------------------------------------------------------ 4 --
def test_records_do_not_depend_on_the_slot_count(gpu, monkeypatch, model_games):
    recs, _ = selfplay_records(gpu, monkeypatch, "move_loop", slots=2)
    assert_games_equal(recs, model_games[None])


# ------------------------------------------------------------------ 5 --
def test_off_is_off(gpu):
    """set_tree_reuse(False) after it had been on, with a reusing run in between: the golden game, bit for bit."""
    d = golden("selfplay.npz")
    sp = gpu.SelfPlay(3, 50, 8, 1.0, tree_reuse=True)
    sp.set_timing(True)
    sp.run(0, 2, 99)
    assert sp.kernel_stats("reroot")["launches"] > 0
    sp.reset_stats()
    bytes_on = sp.engine.device_bytes()
    sp.engine.set_tree_reuse(False)
    sp.run(0, 1, int(d["seeds"][0]))
    assert sp.kernel_stats("reroot")["launches"] == 0
    r = sp.records()[0]
    ln = int(d["lengths"][0])
    assert np.array_equal(r["actions"], d["actions"][:ln].astype(np.int64))
    assert np.array_equal(r["policies"].view(np.uint64), d["policies"][:ln].view(np.uint64))
    assert np.array_equal(r["values"], d["values"][:ln].astype(np.int64))
    # the second pool is reported
    plain = gpu.Engine(3, 50)
    pool = 3 * (82 + 81 * 50) * 16
    assert plain.device_bytes() >= pool and bytes_on >= plain.device_bytes() + pool
    plain.close()


# ------------------------------------------------------------------ 6 --
def test_refusals(gpu, oracle_lib):
    from uttt_amd._lib import EngineError, UtttState
    import torch
    s0 = oracle_lib.OrState.initial()
    roots = wide_deep.pack_states([s0, s0.next(40)])
    e = gpu.Engine(2, 16)
    x = torch.zeros((2, 3, 9, 9), dtype=torch.float32, device=torch.device("cuda", e.device))
    ev = gpu.HashEvaluator(e)
    # a finished py search cannot be re-rooted, and reuse must be on
    e.search_begin(roots, 16, 4)
    run_rounds(gpu, e, x, ev)
    with pytest.raises(EngineError, match="tree reuse is off"):
        e.reroot([0, 36], 16)
    e.search_begin(roots, 16, 4, semantics="py")
    run_rounds(gpu, e, x, ev)
    e.set_tree_reuse(True)
    with pytest.raises(ValueError, match="Python semantics"):
        e.reroot([0, 36], 16)
    with pytest.raises(ValueError, match="tree reuse is on"):
        e.search_begin(roots, 16, 4, semantics="py")
    fn = e.lib.uttt_search1_begin
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(UtttState), ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                   ctypes.c_float]
    for semantics in (0, 1):
        assert fn(e.h, roots[:1].ctypes.data_as(ctypes.POINTER(UtttState)), 16, 4, semantics, 1.0) == -1
        assert b"tree reuse is on" in e.lib.uttt_last_error()
    # an action of -1 and an illegal one are refused, and the engine goes on
    e.search_begin(roots, 16, 4)
    run_rounds(gpu, e, x, ev)
    for bad in ([-1, 36], [0, 0]):  # tree 1's root must play in board 4
        with pytest.raises(ValueError, match="not a legal move"):
            e.reroot(bad, 16)
    with pytest.raises(ValueError):
        e.reroot([0, 36], 8)  # fewer visits than the finished search's
    e.reroot([ranked_action(e.tree(t), 0) for t in range(2)], 16)
    run_rounds(gpu, e, x, ev)
    assert np.all(e.root_visits()[0].sum(axis=1) == 16)
    e.close()
