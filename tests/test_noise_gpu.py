"""Root noise and the temperature schedule on the GPU (k_root_noise, k_move_end): the priors the
kernel writes against uttt_root_noise_host bit for bit, off meaning off, the search following the noisy priors,
self-play records against a host loop on the first plies, independence of the driver, and the refusals."""
import ctypes

import numpy as np
import pytest

import wide_deep

pytestmark = pytest.mark.gpu

NOISE = (0.25, 0.3, 5)  # the self-play tests' (epsilon, alpha, seed)


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import uttt_amd
    return uttt_amd


@pytest.fixture(scope="module")
def six_roots(gpu, oracle_lib):
    """Two each of L = 81, L = 9 and a free-move root with 66-70 moves: (packed, OrStates, L)."""
    s0 = oracle_lib.OrState.initial()
    ost = [s0, s0, s0.next(1), s0.next(79)] + list(wide_deep.wide_roots(2, wide_deep.WIDE_SEED)[1])
    L = np.array([len(s.legal_actions()) for s in ost], np.int32)
    assert list(L[:4]) == [81, 81, 9, 9] and all(66 <= x <= 70 for x in L[4:])
    return wide_deep.pack_states(ost), ost, L


@pytest.fixture(scope="module")
def opening_roots(gpu, oracle_lib):
    """The initial state and 7 of the 81 states after one move: no game ends before ply 17, so a search of
    S <= 8 simulations from here never reaches a terminal state."""
    s0 = oracle_lib.OrState.initial()
    ost = [s0] + [s0.next(a) for a in (0, 1, 13, 40, 44, 62, 80)]
    return wide_deep.pack_states(ost), ost


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------ 1 --
@pytest.mark.parametrize("alpha", (0.3, 1.0 / 32.0, 32.0))
def test_root_priors_equal_the_host_bit_for_bit(gpu, six_roots, alpha):
    from uttt_amd import noise
    roots, _, L = six_roots
    e = gpu.Engine(len(roots), 50)
    e.set_timing(True)
    e.set_root_noise(0.25, alpha, 7)
    e.search_begin(roots, 50, 8)
    pri, n_legal = e.root_priors()
    _, want = noise.root_noise_host(roots, np.arange(len(roots)), 0, 0.25, alpha, seed=7)
    assert np.array_equal(n_legal, L)
    for t in range(len(roots)):
        assert np.array_equal(bits(pri[t]), bits(want[t])), (alpha, t, L[t])
        assert not np.all(pri[t, :L[t]] == np.float32(1.0) / np.float32(L[t]))
    assert e.kernel_stats("root_noise")["launches"] == 1
    # the trees are keyed by their index: the two initial states differ
    assert not np.array_equal(pri[0], pri[1])
    e.close()


# ------------------------------------------------------------------ 2 --
def test_off_is_off(gpu, six_roots, oracle_lib):
    roots, ost, L = six_roots
    e = gpu.Engine(len(roots), 50)

    def uniform():
        pri, n_legal = e.root_priors()
        assert np.array_equal(n_legal, L)
        for t in range(len(roots)):
            assert np.all(bits(pri[t, :L[t]]) == bits(np.float32(1.0) / np.float32(L[t]))), t
            assert np.all(pri[t, L[t]:] == 0.0)

    e.search_begin(roots, 50, 8)
    uniform()
    e.set_root_noise(0.25, 0.3, 7)
    e.set_root_noise(0.0, 0.3, 7)
    e.search_begin(roots, 50, 8)
    uniform()
    assert e.kernel_stats("root_noise")["launches"] == 0
    e.close()
    bs = gpu.BatchedSearch(len(roots), 50)
    bs.run(roots, gpu.HashEvaluator(bs.engine), 50, 8)
    visits, n_legal = bs.visits()
    for i, s in enumerate(ost):
        _, vi, _ = oracle_lib.pv_mcts_scores_hash(s, 1.0, 50, 8)
        assert n_legal[i] == vi.size and np.array_equal(visits[i, :n_legal[i]], vi), i
    assert bs.engine.kernel_stats("root_noise")["launches"] == 0


# ------------------------------------------------------------------ 3 --
def visits_from_priors(p, S, B):
    """The root's visit counts when every value is 0 and no terminal state is reached, from DESIGN.md "Exact
    semantics": every Q is 0, so a descent picks the first arg-max of u = (p * sqrtf(total)) / (1 + n) over the
    root's children (strict '>' from -1e9: the first maximum; with total = 0 every u is 0 and rank 0 wins), and
    with no virtual loss a flush holds k = min(B, S - i) copies of the one leaf below that child, all backed up
    through it: n[pick] += k."""
    p = np.asarray(p, np.float32)
    n = np.zeros(len(p), np.int64)
    left = S
    while left > 0:
        sq = np.sqrt(np.float32(n.sum()), dtype=np.float32)
        u = (p * sq) / (1 + n).astype(np.float32)
        assert u.dtype == np.float32
        pick = int(np.argmax(u))
        k = min(B, left)
        n[pick] += k
        left -= k
    return n


def search_value0(e, roots, S, B):
    """A search whose evaluator returns all-ones policy rows and value 0, applied from host arrays."""
    e.search_begin(roots, S, B)
    while True:
        n = e.select(None)
        if n == 0:
            break
        e.apply(np.ones((n, 81), np.float32), np.zeros(n, np.float32))
    return e.root_visits()


@pytest.mark.parametrize("S,B", [(8, 1), (8, 3)])
def test_the_search_follows_the_noisy_priors(gpu, opening_roots, S, B):
    roots, ost = opening_roots
    e = gpu.Engine(len(roots), 50)
    # the rule itself first, on the unmodified path: uniform priors
    visits, L = search_value0(e, roots, S, B)
    for t in range(len(roots)):
        uni = np.full(L[t], np.float32(1.0) / np.float32(L[t]), np.float32)
        assert np.array_equal(visits[t, :L[t]], visits_from_priors(uni, S, B)), ("rule", t)
    moved = 0
    for eps, alpha in ((0.25, 0.3), (1.0, 1.0)):
        e.set_root_noise(eps, alpha, 11)
        e.search_begin(roots, S, B)
        pri, _ = e.root_priors()
        noisy, L2 = search_value0(e, roots, S, B)
        assert np.array_equal(L, L2)
        for t in range(len(roots)):
            assert noisy[t].sum() == S
            assert np.array_equal(noisy[t, :L[t]], visits_from_priors(pri[t, :L[t]], S, B)), (eps, alpha, t)
            moved += not np.array_equal(noisy[t], visits[t])
    assert moved > 0
    e.close()


# ------------------------------------------------------------------ 4 --
def test_selfplay_records_equal_a_host_loop_on_the_first_plies(gpu, oracle_lib):
    import torch
    from uttt_amd import noise
    core = oracle_lib
    slots, n_games, seed_base, S, B, plies_hot = 16, 24, 100, 8, 1, 3
    dev = torch.device("cuda", torch.cuda.current_device())
    ones = torch.ones((slots, 81), dtype=torch.float32, device=dev)
    zeros = torch.zeros((slots, 1), dtype=torch.float32, device=dev)

    def evaluator(x, n):
        return ones[:n], zeros[:n]

    sp = gpu.SelfPlay(slots, S, B, 1.0, evaluator=evaluator, cache_log2=0, root_noise=NOISE,
                      temperature_plies=plies_hot, late_temperature=0.0)
    sp.run(0, n_games, seed_base)
    recs = sp.records(with_inputs=False)
    assert [r["game"] for r in recs] == list(range(n_games))
    first_moves = set()
    for g, r in enumerate(recs):
        assert len(r["actions"]) >= 17
        mt = core.MT(seed_base + g)
        s = core.OrState.initial()
        for ply in range(6):
            legal = s.legal_actions()
            packed = wide_deep.pack_states([s])
            assert packed[0].tobytes() == r["states"][ply].tobytes(), (g, ply)
            _, pri = noise.root_noise_host(packed, [g], [ply], NOISE[0], NOISE[1], seed=NOISE[2])
            visits = visits_from_priors(pri[0, :len(legal)], S, B).astype(np.float32)
            if ply < plies_hot:
                scores = core.boltzman(visits, 1.0)
            else:
                scores = np.zeros(len(legal), np.float32)
                scores[int(np.argmax(visits))] = 1.0
            pol, idx = core.policy_and_sample(mt, scores)
            want = np.zeros(81, np.float64)
            want[legal] = pol
            assert np.array_equal(r["policies"][ply].view(np.uint64), want.view(np.uint64)), (g, ply)
            assert int(r["actions"][ply]) == legal[idx], (g, ply)
            if ply >= plies_hot:
                assert np.count_nonzero(r["policies"][ply]) == 1
            s = s.next(legal[idx])
        first_moves.add(tuple(r["actions"][:4].tolist()))
    assert len(first_moves) > 1


# ------------------------------------------------------------------ 5 --
def hash_records(gpu, monkeypatch, n_games=32, seed=4242, slots=16, lanes=1, blocking=False, cache_log2=0, **kw):
    monkeypatch.setenv("UTTT_ASYNC_ROUNDS", "0" if blocking else "1")
    sp = gpu.SelfPlay(slots, 50, 8, 1.0, lanes=lanes, cache_log2=cache_log2, **kw)
    assert sp._device_count() != blocking
    sp.run(0, n_games, seed)
    recs = sp.records(with_inputs=False)
    assert [r["game"] for r in recs] == list(range(n_games))
    return recs, sp


def same_records(a, b):
    return all(np.array_equal(x["actions"], y["actions"]) and np.array_equal(x["values"], y["values"]) and
               np.array_equal(x["policies"].view(np.uint64), y["policies"].view(np.uint64)) and
               x["states"].tobytes() == y["states"].tobytes() for x, y in zip(a, b)) and len(a) == len(b)


def test_records_do_not_depend_on_the_driver(gpu, oracle_lib, monkeypatch):
    both = dict(root_noise=NOISE, temperature_plies=8, late_temperature=0.0)
    base, sp = hash_records(gpu, monkeypatch, blocking=True, **both)
    moves = sp.kernel_stats("move_end")["launches"]
    assert sp.kernel_stats("root_noise")["launches"] >= moves > 0  # once per move begin (the empty last one too)
    for name, kw in (("pipelined", {}), ("two lanes", dict(lanes=2)), ("cache", dict(cache_log2=12)),
                     ("other slots", dict(slots=7))):
        other, _ = hash_records(gpu, monkeypatch, **kw, **both)
        assert same_records(base, other), name
    # from ply 8 on the most visited move is played: a one-hot target
    for r in base:
        assert all(np.count_nonzero(p) == 1 for p in r["policies"][8:])
        assert any(np.count_nonzero(p) > 1 for p in r["policies"][:8])
    reseeded, _ = hash_records(gpu, monkeypatch, root_noise=(NOISE[0], NOISE[1], NOISE[2] + 1), temperature_plies=8)
    assert not same_records(base, reseeded)
    quiet, _ = hash_records(gpu, monkeypatch, temperature_plies=8)
    assert not same_records(base, quiet)
    # both off through the new arguments: the oracle's games, as before
    off, sp = hash_records(gpu, monkeypatch, root_noise=None, temperature_plies=None)
    assert sp.kernel_stats("root_noise")["launches"] == 0
    for g, r in enumerate(off):
        ref = oracle_lib.self_play_game_hash(4242 + g, 1.0, 50, 8)
        assert np.array_equal(r["actions"], ref["actions"].astype(np.int64)), g
        assert np.array_equal(r["policies"].view(np.uint64), ref["policies"].view(np.uint64)), g
        assert np.array_equal(r["values"], ref["values"].astype(np.int64)), g


# ------------------------------------------------------------------ 6 --
def test_refusals_leave_the_engine_usable(gpu, six_roots, oracle_lib):
    from uttt_amd._lib import UtttState
    roots, ost, L = six_roots
    e = gpu.Engine(len(roots), 50)
    e.set_root_noise(0.25, 0.3, 7)
    with pytest.raises(ValueError, match="root noise is on"):
        e.search_begin(roots, 50, 8, semantics="py")
    fn = e.lib.uttt_search1_begin
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(UtttState), ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                   ctypes.c_float]
    for semantics in (0, 1):
        assert fn(e.h, roots[:1].ctypes.data_as(ctypes.POINTER(UtttState)), 50, 8, semantics, 1.0) == -1
        assert b"root noise is on" in e.lib.uttt_last_error()
    for bad in ((-0.5, 0.3), (1.5, 0.3), (0.25, 0.01), (0.25, 64.0)):
        with pytest.raises(ValueError):
            e.set_root_noise(*bad)
    with pytest.raises(ValueError):
        e.set_temperature_schedule(-1, 0.0)
    with pytest.raises(ValueError):
        e.set_temperature_schedule(4, -1.0)
    # one plain CPP search afterwards, with the noise still on: the priors the host gives, 50 simulations
    bs_x = np.ones((len(roots), 81), np.float32)
    e.search_begin(roots, 50, 8)
    pri, _ = e.root_priors()
    from uttt_amd import noise
    _, want = noise.root_noise_host(roots, np.arange(len(roots)), 0, 0.25, 0.3, seed=7)
    assert np.array_equal(bits(pri), bits(want))
    while True:
        n = e.select(None)
        if n == 0:
            break
        e.apply(bs_x[:n], np.zeros(n, np.float32))
    visits, _ = e.root_visits()
    assert np.all(visits.sum(axis=1) == 50)
    # and with it off, PY semantics begin again
    e.set_root_noise(0.0)
    e.search_begin(roots, 50, 8, semantics="py")
    e.close()
