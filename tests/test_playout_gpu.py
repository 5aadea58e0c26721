"""GPU tests of the random-playout evaluator: k_playout_states against uttt_playout_host bit for bit; searches,
self-play, the arena and the drop-in with PlayoutEvaluator against the CPU oracle, whose evaluator callback
rebuilds the leaf from its network input and asks uttt_playout_host (checked on its own against a pure-Python
restatement in test_playout_host.py)."""
import ctypes
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WAVES_PER_BLOCK = 4  # csrc/engine/layout.h kWavesPerBlock: one wave per position
P_SEARCH, SEED = 8, 0xC0FFEE


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import uttt_amd
    return uttt_amd


def _pack(ostates):
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


def _host_counts(lib, states, playouts, seed):
    from uttt_amd._lib import UtttState
    states = np.ascontiguousarray(states)
    wins = np.zeros(len(states), np.int32)
    losses = np.zeros(len(states), np.int32)
    i32 = ctypes.POINTER(ctypes.c_int32)
    assert lib.uttt_playout_host(states.ctypes.data_as(ctypes.POINTER(UtttState)), len(states), playouts, seed,
                                 wins.ctypes.data_as(i32), losses.ctypes.data_as(i32)) == 0
    return wins, losses


@pytest.fixture(scope="module")
def positions(oracle_lib):
    """8 non-terminal positions along random games (the search roots), then lost and drawn final positions and
    more random ones: 4 * WAVES_PER_BLOCK + 1 in all."""
    core = oracle_lib
    rng = random.Random(77)
    mid, lost, drawn = [], [], []
    while len(mid) < 16 or len(lost) < 2 or len(drawn) < 1:
        s = core.OrState.initial()
        while not s.is_done():
            if rng.random() < 0.1 and len(mid) < 16:
                mid.append(s)
            s = s.next(rng.choice(s.legal_actions()))
        (lost if s.is_lose() else drawn).append(s)
    ostates = ([core.OrState.initial()] + mid[:7] + lost[:2] + drawn[:1] + mid[7:])[:4 * WAVES_PER_BLOCK + 1]
    assert len(ostates) == 4 * WAVES_PER_BLOCK + 1 and not any(s.is_done() for s in ostates[:8])
    return _pack(ostates), ostates


def _action_at(pos):
    R, C = divmod(pos, 9)
    return ((R // 3) * 3 + C // 3) * 9 + (R % 3) * 3 + C % 3


_LINES = (0x007, 0x038, 0x1C0, 0x049, 0x092, 0x124, 0x111, 0x054)


def _state_from_input(x):
    """A packed state equivalent to the one whose NCHW input is x, for positions of real games: a small board is
    closed for the side with a line on it, or for both when it is full with no line; `active` is the one board
    with legal moves, or -1 (equal keys either way when one board is open: the key reads stones and legal moves)."""
    from uttt_amd._lib import STATE_DTYPE
    bits = [[0] * 9 for _ in range(3)]  # [channel][board] -> 9-bit cells
    for ch in range(3):
        for pos in range(81):
            if x[ch * 81 + pos] != 0:
                a = _action_at(pos)
                bits[ch][a // 9] |= 1 << (a % 9)
    st = np.zeros(1, STATE_DTYPE)
    mains = 0
    for b in range(9):
        own, opp = bits[0][b], bits[1][b]
        st["own"][0, b // 3] |= own << (9 * (b % 3))
        st["opp"][0, b // 3] |= opp << (9 * (b % 3))
        won_own = any((own & ln) == ln for ln in _LINES)
        won_opp = any((opp & ln) == ln for ln in _LINES)
        full = (own | opp) == 0x1FF
        if won_own or (full and not won_opp):
            mains |= 1 << b
        if won_opp or (full and not won_own):
            mains |= 1 << (16 + b)
    st["mains"][0] = mains
    boards = [b for b in range(9) if bits[2][b]]
    st["active"][0] = boards[0] if len(boards) == 1 else -1
    return st


def _playout_callback(lib, playouts, seed):
    ones = np.ones(81, np.float32)

    def cb(x):
        w, l = _host_counts(lib, _state_from_input(x), playouts, seed)
        return ones, np.float32(int(w[0]) - int(l[0])) / np.float32(playouts)

    return cb


def _oracle_visits(core, cb, ostate, sims, batch, semantics):
    if semantics == "cpp":
        return core.pv_mcts_scores(ostate, 1.0, sims, batch, cb)[1]
    return core.pv_mcts_scores_py_callback(ostate, 0.0, sims, batch, cb)[1]


def test_state_from_input_round_trips(engine_lib, positions):
    """The callback's reconstruction gives the positions' own playouts (terminal ones have no legal channel and
    are never evaluated)."""
    packed, ostates = positions
    for i, s in enumerate(ostates):
        if s.is_done():
            continue
        a = _host_counts(engine_lib, packed[i:i + 1], 64, 3)
        b = _host_counts(engine_lib, _state_from_input(s.tensor_nchw()), 64, 3)
        assert a[0][0] == b[0][0] and a[1][0] == b[1][0], i


@pytest.mark.parametrize("n", [1, 5, 4 * WAVES_PER_BLOCK + 1])
def test_kernel_equals_host(gpu, engine_lib, positions, n):
    """A lone wave, a partial block, a grid tail; one pass, a full pass, a pass with one lane, four passes."""
    packed, ostates = positions
    # the n = 5 slice holds the lost and drawn positions
    st = packed[:n] if n != 5 else packed[6:11]
    if n != 1:
        assert any(s.is_lose() for s in (ostates[:n] if n != 5 else ostates[6:11]))
    eng = gpu.Engine(4, 50)
    for P in (1, 64, 65, 256):
        for seed in (0, 0xFEDCBA9876543210):
            wins, losses = eng.playouts(st, P, seed)
            hw, hl = _host_counts(engine_lib, st, P, seed)
            assert wins.dtype == np.int32 and np.array_equal(wins, hw) and np.array_equal(losses, hl), (n, P, seed)
            for i in range(len(st)):
                o = (ostates[:n] if n != 5 else ostates[6:11])[i]
                if o.is_lose():
                    assert (wins[i], losses[i]) == (0, P)
                elif o.is_draw():
                    assert (wins[i], losses[i]) == (0, 0)
    with pytest.raises(ValueError):
        eng.playouts(st, 0)
    with pytest.raises(ValueError):
        eng.playouts(st, 4097)


@pytest.mark.parametrize("semantics", ["cpp", "py"])
def test_search_matches_oracle(gpu, engine_lib, oracle_lib, positions, semantics):
    packed, ostates = positions
    roots, oroots = packed[:8], ostates[:8]
    bs = gpu.BatchedSearch(8, 50)
    ev = gpu.PlayoutEvaluator(bs.engine, P_SEARCH, SEED)
    assert ev.needs_input is False and ev.device_count is True
    assert not any(hasattr(ev, a) for a in ("round_async", "round_move", "cheap"))
    cb = _playout_callback(engine_lib, P_SEARCH, SEED)
    for sims, batch in ((50, 8), (7, 100)):
        bs.run(roots, ev, sims, batch, semantics)
        visits, L = bs.visits()
        for i, s in enumerate(oroots):
            vi = _oracle_visits(oracle_lib, cb, s, sims, batch, semantics)
            assert L[i] == vi.size and np.array_equal(visits[i, :L[i]], vi), (semantics, sims, batch, i)
    assert bs.engine.kernel_stats("playout")["launches"] > 0


def test_cache_is_exact(gpu, positions):
    """The evaluator is a function of the position: searches resolved from the evaluation table (the second run
    finds every leaf of the first) give the uncached visits."""
    roots = positions[0][:8]
    out = []
    for cache in (0, 12):
        bs = gpu.BatchedSearch(8, 50, cache_log2=cache)
        ev = gpu.PlayoutEvaluator(bs.engine, P_SEARCH, SEED)
        for _ in range(2):
            bs.run(roots, ev, 50, 8)
            out.append(bs.visits()[0].copy())
        if cache:
            assert bs.engine.cache_stats()["hits"] > 0
    for v in out[1:]:
        assert np.array_equal(v, out[0])
    assert (out[0].sum(axis=1) == 50).all()


def test_selfplay_records(gpu, engine_lib, oracle_lib):
    core = oracle_lib
    seed_base, sims, batch = 321, 20, 8
    recs = []
    for asy in (True, False):
        sp = gpu.SelfPlay(4, sims, batch, 1.0)
        sp.async_rounds = asy
        sp.set_evaluator(lambda eng: gpu.PlayoutEvaluator(eng, P_SEARCH, SEED))
        sp.run(0, 4, seed_base)
        recs.append(sp.records())
    a, b = recs
    assert [r["game"] for r in a] == [r["game"] for r in b] == [0, 1, 2, 3]
    for ra, rb in zip(a, b):
        assert np.array_equal(ra["actions"], rb["actions"])
        assert np.array_equal(ra["policies"].view(np.uint64), rb["policies"].view(np.uint64))
        assert np.array_equal(ra["values"], rb["values"])
    # game 0's opening against the oracle search composed with the reference's sampling
    cb = _playout_callback(engine_lib, P_SEARCH, SEED)
    mt = core.MT(seed_base)
    s = core.OrState.initial()
    for ply in range(6):
        scores = core.pv_mcts_scores(s, 1.0, sims, batch, cb)[0]
        pol, idx = core.policy_and_sample(mt, scores)
        legal = s.legal_actions()
        assert int(a[0]["actions"][ply]) == legal[idx], ply
        want = np.zeros(81, np.float64)
        want[legal] = pol
        assert np.array_equal(a[0]["policies"][ply].view(np.uint64), want.view(np.uint64)), ply
        s = s.next(legal[idx])


def test_arena_vs_playouts(gpu, engine_lib, oracle_lib):
    from uttt_amd import arena
    core = oracle_lib
    games, seed_base, sims, opp_sims, batch = 4, 50, 20, 30, 8
    avg, points, actions = arena.evaluate_vs_playouts(
        None, games, playouts=P_SEARCH, opponent_evaluate_count=opp_sims, seed_base=seed_base, evaluate_count=sims,
        batch_size=batch, make_evaluator=lambda m, e: gpu.HashEvaluator(e), playout_seed=SEED)
    cb = _playout_callback(engine_lib, P_SEARCH, SEED)
    total = 0.0
    for g in range(games):
        rng = np.random.RandomState(seed_base + g)
        s, acts = core.OrState.initial(), []
        while not s.is_done():
            model_moves = s.is_first_player() == (g % 2 == 0)
            if model_moves:
                vi = core.pv_mcts_scores_py_hash(s, 0.0, sims, batch)[1]
            else:
                vi = core.pv_mcts_scores_py_callback(s, 0.0, opp_sims, batch, cb)[1]
            legal = s.legal_actions()
            sc = arena.scores_from_visits(vi, 0.0)
            acts.append(int(rng.choice(legal, p=sc)))
            s = s.next(acts[-1])
        assert actions[g] == acts, g
        point = (0 if s.is_first_player() else 1) if s.is_lose() else 0.5
        assert points[g] == point, g
        total += point if g % 2 == 0 else 1 - point
    assert avg == total / games


def test_dropin_mcts_action_and_default_output(gpu, engine_lib, oracle_lib, positions, tmp_path, monkeypatch, capsys):
    import dual_network
    import evaluate_best_player
    import uttt_cpp
    cb = _playout_callback(engine_lib, P_SEARCH, 0)
    next_action = evaluate_best_player.mcts_action_factory(30, P_SEARCH)
    for s in positions[1][:3]:
        p, e, mp, me, act = s.arrays()
        state = uttt_cpp.State(p.tolist(), e.tolist(), mp.tolist(), me.tolist(), act)
        vi = oracle_lib.pv_mcts_scores_py_callback(s, 0.0, 30, 8, cb)[1].tolist()
        assert next_action(state) == s.legal_actions()[vi.index(max(vi))]
    # the default output is the reference's: no VS_MCTS line unless EP_VS_MCTS is set
    assert evaluate_best_player.EP_VS_MCTS is False
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(evaluate_best_player, "EP_GAME_COUNT", 2)
    dual_network.dual_network()
    capsys.readouterr()
    evaluate_best_player.evaluate_best_player()
    out = capsys.readouterr().out
    assert "VS_Random" in out and "VS_MCTS" not in out
    monkeypatch.setattr(evaluate_best_player, "EP_VS_MCTS", True)
    evaluate_best_player.evaluate_best_player()
    lines = capsys.readouterr().out.splitlines()
    assert lines[-1].startswith("VS_MCTS ") and float(lines[-1].split()[1]) in (0.0, 0.25, 0.5, 0.75, 1.0)
    assert any(ln.startswith("VS_Random ") for ln in lines)
