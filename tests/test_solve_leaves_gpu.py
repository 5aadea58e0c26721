"""GPU tests of the solver overlay inside the search (k_solve_leaves, uttt_eval_solve_dev, SolvedLeaves; DESIGN.md
6d): the kernel against uttt_solve_overlay_host bit for bit on the pending leaves of a stopped search; searches,
cached searches, self-play, the arena and the drop-in with SolvedLeaves against the CPU oracle, whose evaluator
callback rebuilds the leaf from its network input, evaluates the base on the host and applies the host overlay
(checked on its own against a restatement in test_solve_leaves_host.py)."""
import random

import numpy as np
import pytest

from test_playout_gpu import _host_counts, _pack, _state_from_input
from test_solve_host import empties_py, late_positions

pytestmark = pytest.mark.gpu

WAVES_PER_BLOCK = 4  # csrc/engine/layout.h kWavesPerBlock: one wave per leaf
N_TAIL = 4 * WAVES_PER_BLOCK + 1
SKIPPED, SOLVED, BUDGET = 0, 1, 2
P_SEARCH, SEED = 8, 0xC0FFEE
E, M = 10, 1024  # the overlay's parameters in the search tests


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import uttt_amd
    return uttt_amd


@pytest.fixture(scope="module")
def leaves(oracle_lib):
    """N_TAIL non-terminal roots: 12 with at most 10 empties, the initial position, 4 with 11..20 empties (the
    last five are the partial workgroup's: skipped and searched ones together)."""
    small = late_positions(oracle_lib, 12, 10, 31)
    mid = [s for s in late_positions(oracle_lib, 30, 20, 32) if empties_py(s) > 10][:4]
    ostates = small + [oracle_lib.OrState.initial()] + mid
    assert len(ostates) == N_TAIL and not any(s.is_done() for s in ostates)
    return _pack(ostates), ostates


@pytest.fixture(scope="module")
def late_roots(oracle_lib):
    """8 roots: 6 with 11 or 12 empties, whose leaves cross E = 10 within a few plies, then 2 with 9 or 10 (a
    search of 7 simulations in one batch of the Python semantics evaluates its root alone)."""
    rng = random.Random(5)
    above, below = [], []
    while len(above) < 6 or len(below) < 2:
        s = oracle_lib.OrState.initial()
        while not s.is_done():
            if empties_py(s) <= 12:
                if empties_py(s) >= 11:
                    above.append(s)
                elif empties_py(s) >= 9:
                    below.append(s)
                break
            s = s.next(rng.choice(s.legal_actions()))
    out = above[:6] + below[:2]
    return _pack(out), out


def _pattern(shape, seed):
    return (np.random.RandomState(seed).rand(*shape).astype(np.float32) * 2 - 1)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("n", [1, 5, N_TAIL])
def test_kernel_equals_host(gpu, leaves, n):
    """A lone wave, a partial workgroup, a grid tail: the rows of a search stopped after one select."""
    import torch
    from uttt_amd import solver
    packed, _ = leaves
    roots = packed[:n] if n != 5 else packed[N_TAIL - 5:]
    eng = gpu.Engine(N_TAIL, 50)
    eng.search_begin(roots, 50, 8)
    assert eng.select() == n
    st, _ = eng.pending()
    assert len(st) == n  # each tree's first leaf: a child of its root
    seen = set()
    for max_nodes in (4096, 16):
        for priors in (solver.PRIORS_KEEP, solver.PRIORS_OPTIMAL):
            for ld in (81, 96):
                pol, val = _pattern((n, ld), 1 + ld), _pattern((n, 2), 2)
                d_pol, d_val = torch.from_numpy(pol).cuda(), torch.from_numpy(val).cuda()
                d_status = torch.full((n,), 77, dtype=torch.int8, device="cuda") if ld == 81 else None
                # value rows two floats apart with ld 96, a (n, 1) column otherwise
                d_v = d_val[:, 0] if ld == 96 else d_val[:, :1].contiguous()
                eng.eval_solve_dev(d_pol, d_v, E, max_nodes, priors, d_status)
                h_pol, h_val = pol.copy(), (val.copy() if ld == 96 else val[:, :1].copy())
                want = solver.overlay_host(st, h_pol, h_val[:, 0] if ld == 96 else h_val, E, max_nodes, priors)
                torch.cuda.synchronize()
                assert np.array_equal(_bits(d_pol.cpu().numpy()), _bits(h_pol)), (n, max_nodes, priors, ld)
                got_v = d_val.cpu().numpy() if ld == 96 else d_v.cpu().numpy()
                assert np.array_equal(_bits(got_v), _bits(h_val)), (n, max_nodes, priors, ld)
                if d_status is not None:
                    assert d_status.cpu().numpy().tolist() == want.tolist(), (n, max_nodes, priors)
                seen |= set(want.tolist())
                if priors == solver.PRIORS_KEEP:
                    assert np.array_equal(_bits(h_pol), _bits(pol))
    if n == N_TAIL:
        assert seen == {SKIPPED, SOLVED, BUDGET}
    assert eng.kernel_stats("solve_leaves")["launches"] == 8
    p, v = torch.zeros((n, 81), device="cuda"), torch.zeros((n, 1), device="cuda")
    for bad in ({"max_empties": 33}, {"max_empties": -1}, {"max_nodes": 0}, {"max_nodes": (1 << 22) + 1},
                {"priors": 2}):
        with pytest.raises(ValueError):
            eng.eval_solve_dev(p, v, **{"max_empties": E, "max_nodes": M, "priors": 1, **bad})
    with pytest.raises(ValueError):
        eng.eval_solve_dev(torch.zeros((n, 80), device="cuda"), v, E, M, 1)  # policy_ld 80
    with pytest.raises(ValueError):
        eng.eval_solve_dev(torch.zeros((n, 96), device="cuda")[:, :80], v, E, M, 1)  # rows 96 apart, 80 wide
    with pytest.raises(ValueError):
        eng.eval_solve_dev(p, torch.zeros((n + 1, 1), device="cuda"), E, M, 1)
    with pytest.raises(ValueError):
        eng.eval_solve_dev(p, torch.zeros((n, 2), device="cuda"), E, M, 1)
    eng.close()


def _base_callback(lib, kind):
    from oracle import hashnp
    if kind == "hash":
        return lambda x, st: hashnp.hash_eval_np(x)
    ones = np.ones(81, np.float32)

    def playout(x, st):
        w, l = _host_counts(lib, st, P_SEARCH, SEED)
        return ones, np.float32(int(w[0]) - int(l[0])) / np.float32(P_SEARCH)

    return playout


def _overlay_callback(lib, kind, priors="optimal", max_empties=E, max_nodes=M):
    """The oracle's evaluator: the base on the host, then the host overlay on its one row."""
    from uttt_amd import solver
    base = _base_callback(lib, kind)

    def cb(x):
        st = _state_from_input(x)
        pol, val = base(x, st)
        pol = np.array(pol, np.float32).reshape(1, 81)
        val = np.array([val], np.float32)
        solver.overlay_host(st, pol, val, max_empties, max_nodes, priors)
        return pol[0], val[0]

    return cb


def _make(gpu, kind, engine, **kw):
    base = gpu.HashEvaluator(engine) if kind == "hash" else gpu.PlayoutEvaluator(engine, P_SEARCH, SEED)
    return gpu.SolvedLeaves(base, engine, max_empties=E, max_nodes=M, **kw)


def _oracle_visits(core, cb, ostate, sims, batch, semantics):
    if semantics == "cpp":
        return core.pv_mcts_scores(ostate, 1.0, sims, batch, cb)[1]
    return core.pv_mcts_scores_py_callback(ostate, 0.0, sims, batch, cb)[1]


@pytest.mark.parametrize("semantics", ["cpp", "py"])
@pytest.mark.parametrize("kind", ["hash", "playout"])
def test_search_matches_oracle(gpu, engine_lib, oracle_lib, late_roots, kind, semantics):
    roots, oroots = late_roots
    bs = gpu.BatchedSearch(8, 50)
    ev = _make(gpu, kind, bs.engine)
    assert ev.needs_input is (kind == "hash") and ev.device_count is True
    assert not any(hasattr(ev, a) for a in ("round_async", "round_move", "cheap", "rounds_per_call"))
    assert ev.status.dtype.itemsize * ev.status.numel() == bs.engine.max_trees
    cb = _overlay_callback(engine_lib, kind)
    for sims, batch in ((50, 8), (7, 100)):
        ev.reset_counts()
        bs.run(roots, ev, sims, batch, semantics)
        visits, L = bs.visits()
        for i, s in enumerate(oroots):
            vi = _oracle_visits(oracle_lib, cb, s, sims, batch, semantics)
            assert L[i] == vi.size and np.array_equal(visits[i, :L[i]], vi), (kind, semantics, sims, batch, i)
        counts = ev.counts()
        assert counts["solved"] > 0 and ev.solved == counts["solved"], (kind, semantics, sims, batch, counts)
        assert ev.budget == counts["budget"] and ev.skipped == counts["skipped"]
    assert bs.engine.kernel_stats("solve_leaves")["launches"] > 0


def test_priors_keep_in_a_search(gpu, engine_lib, oracle_lib, late_roots):
    roots, oroots = late_roots
    bs = gpu.BatchedSearch(8, 50)
    ev = _make(gpu, "hash", bs.engine, priors="keep")
    cb = _overlay_callback(engine_lib, "hash", priors="keep")
    bs.run(roots, ev, 50, 8)
    visits, L = bs.visits()
    for i, s in enumerate(oroots):
        assert np.array_equal(visits[i, :L[i]], _oracle_visits(oracle_lib, cb, s, 50, 8, "cpp")), i
    assert ev.solved > 0


def test_counts_over_more_calls_than_the_ring(gpu, late_roots):
    """The running counts are those of every call: searches one after another, past the ring's depth."""
    roots = late_roots[0]
    bs = gpu.BatchedSearch(8, 50)
    ev = _make(gpu, "playout", bs.engine)
    bs.run(roots, ev, 50, 8)
    one, rounds = ev.counts(), bs.rounds
    assert sum(one.values()) > 0 and rounds > 0
    for _ in range(ev.kRing // rounds + 2):
        bs.run(roots, ev, 50, 8)
    total = ev.counts()
    assert total == {k: v * (ev.kRing // rounds + 3) for k, v in one.items()}


def test_cache_is_exact(gpu, late_roots):
    """The overlaid evaluator is a function of the position: searches resolved from the evaluation table give the
    uncached visits."""
    roots = late_roots[0]
    out = []
    for cache in (0, 12):
        bs = gpu.BatchedSearch(8, 50, cache_log2=cache)
        ev = _make(gpu, "playout", bs.engine)
        for _ in range(2):
            bs.run(roots, ev, 50, 8)
            out.append(bs.visits()[0].copy())
        if cache:
            assert bs.engine.cache_stats()["hits"] > 0
        assert ev.solved > 0
    for v in out[1:]:
        assert np.array_equal(v, out[0])
    assert (out[0].sum(axis=1) == 50).all()


def test_selfplay_records_and_lifecycle(gpu, engine_lib, oracle_lib):
    core = oracle_lib
    seed_base, sims, batch, games = 321, 20, 8, 16
    recs, solved = [], []
    for lanes in (1, 2, 1):  # the last: the engines destroyed and created again
        sp = gpu.SelfPlay(games, sims, batch, 1.0, lanes=lanes)
        sp.set_evaluator(lambda eng: _make(gpu, "playout", eng))
        sp.run(0, games, seed_base)
        recs.append(sp.records())
        solved.append(sum(ln.evaluator.solved for ln in sp.lanes))
        # every row of every round is counted, whichever stream the lane runs on: read at once, nothing waited for
        for ln in sp.lanes:
            assert sum(ln.evaluator.counts().values()) == ln.leaves > 0, (lanes, ln.evaluator.counts(), ln.leaves)
        assert sum(sum(ln.evaluator.counts().values()) for ln in sp.lanes) == sp.leaves
        for ln in sp.lanes:
            ln.engine.close()
        del sp
    assert all(n > 0 for n in solved), solved
    a = recs[0]
    assert [r["game"] for r in a] == list(range(games))
    for b in recs[1:]:
        assert [r["game"] for r in b] == list(range(games))
        for ra, rb in zip(a, b):
            assert np.array_equal(ra["actions"], rb["actions"])
            assert np.array_equal(ra["policies"].view(np.uint64), rb["policies"].view(np.uint64))
            assert np.array_equal(ra["values"], rb["values"])
    # game 0 to its end against the oracle search composed with the reference's sampling
    cb = _overlay_callback(engine_lib, "playout")
    mt = core.MT(seed_base)
    s = core.OrState.initial()
    ply = 0
    while not s.is_done():
        scores = core.pv_mcts_scores(s, 1.0, sims, batch, cb)[0]
        pol, idx = core.policy_and_sample(mt, scores)
        legal = s.legal_actions()
        assert int(a[0]["actions"][ply]) == legal[idx], ply
        want = np.zeros(81, np.float64)
        want[legal] = pol
        assert np.array_equal(a[0]["policies"][ply].view(np.uint64), want.view(np.uint64)), ply
        s = s.next(legal[idx])
        ply += 1
    assert ply == len(a[0]["actions"])


def _oracle_arena(core, arena, cb, games, seed_base, sims, opp_sims, batch):
    all_actions, points = [], []
    for g in range(games):
        rng = np.random.RandomState(seed_base + g)
        s, acts = core.OrState.initial(), []
        while not s.is_done():
            if s.is_first_player() == (g % 2 == 0):
                vi = core.pv_mcts_scores_py_hash(s, 0.0, sims, batch)[1]
            else:
                vi = core.pv_mcts_scores_py_callback(s, 0.0, opp_sims, batch, cb)[1]
            acts.append(int(rng.choice(s.legal_actions(), p=arena.scores_from_visits(vi, 0.0))))
            s = s.next(acts[-1])
        all_actions.append(acts)
        points.append((0 if s.is_first_player() else 1) if s.is_lose() else 0.5)
    return all_actions, points


def test_arena_switch(gpu, engine_lib, oracle_lib):
    """Without opponent_solve the games are the playout opponent's of before; with it the opponent's leaves are
    overlaid (the oracle with the overlay callback plays the same games) and the counts are reported."""
    from test_playout_gpu import _playout_callback
    from uttt_amd import arena
    games, seed_base, sims, opp_sims, batch = 2, 50, 20, 30, 8
    kw = dict(playouts=P_SEARCH, opponent_evaluate_count=opp_sims, seed_base=seed_base, evaluate_count=sims,
              batch_size=batch, make_evaluator=lambda m, e: gpu.HashEvaluator(e), playout_seed=SEED)
    avg, points, actions = arena.evaluate_vs_playouts(None, games, **kw)
    want_actions, want_points = _oracle_arena(oracle_lib, arena, _playout_callback(engine_lib, P_SEARCH, SEED), games,
                                              seed_base, sims, opp_sims, batch)
    assert actions == want_actions and points == want_points
    assert avg == sum(p if g % 2 == 0 else 1 - p for g, p in enumerate(points)) / games
    solve = {"max_empties": 16, "max_nodes": M, "priors": "optimal"}  # these games end with boards still open
    avg2, points2, actions2, counts = arena.evaluate_vs_playouts(None, games, opponent_solve=solve, **kw)
    assert solve == {"max_empties": 16, "max_nodes": M, "priors": "optimal"}  # the caller's dict is left alone
    want_actions, want_points = _oracle_arena(oracle_lib, arena,
                                              _overlay_callback(engine_lib, "playout", max_empties=16), games,
                                              seed_base, sims, opp_sims, batch)
    assert actions2 == want_actions and points2 == want_points
    assert counts["solved"] > 0 and set(counts) == {"skipped", "solved", "budget"}


def test_dropin_switch(gpu, engine_lib, oracle_lib, late_roots):
    from test_playout_gpu import _playout_callback
    import evaluate_best_player
    import uttt_cpp
    plain = evaluate_best_player.mcts_action_factory(30, P_SEARCH)
    exact = evaluate_best_player.mcts_action_factory(30, P_SEARCH, solve={"max_empties": E, "max_nodes": M})
    assert isinstance(plain.evaluator, gpu.PlayoutEvaluator) and isinstance(exact.evaluator, gpu.SolvedLeaves)
    cbs = (_playout_callback(engine_lib, P_SEARCH, 0),
           lambda x: _overlay_with_seed0(engine_lib, x))
    for s in late_roots[1][:3]:
        p, e, mp, me, act = s.arrays()
        state = uttt_cpp.State(p.tolist(), e.tolist(), mp.tolist(), me.tolist(), act)
        for player, cb in zip((plain, exact), cbs):
            vi = oracle_lib.pv_mcts_scores_py_callback(s, 0.0, 30, 8, cb)[1].tolist()
            assert player(state) == s.legal_actions()[vi.index(max(vi))]
    assert exact.evaluator.solved > 0


def _overlay_with_seed0(lib, x):
    """The drop-in's playout seed is 0."""
    from uttt_amd import solver
    st = _state_from_input(x)
    w, l = _host_counts(lib, st, P_SEARCH, 0)
    pol = np.ones((1, 81), np.float32)
    val = np.array([np.float32(int(w[0]) - int(l[0])) / np.float32(P_SEARCH)], np.float32)
    solver.overlay_host(st, pol, val, E, M, "optimal")
    return pol[0], val[0]
