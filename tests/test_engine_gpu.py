"""GPU parity tests: the HIP engine against the golden fixtures (the reference's
own outputs) and against the CPU oracle, bit for bit, through the C ABI.

Evaluators: the device hash evaluator (deterministic, exercises zero /
subnormal / sparse priors) and the real DualNetwork, whose outputs are
recorded and replayed into the oracle so search parity is checked
independently of network numerics."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, PKG, REPO, golden

pytestmark = pytest.mark.gpu

NETCAL = os.path.join(GOLDEN, "netcal.npz")
CONFIGS = [(50, 8), (50, 1), (50, 1024), (400, 8), (10, 2), (30, 3), (1, 1), (7, 100), (64, 64)]


def _pos_states(d):
    from uttt_amd._lib import STATE_DTYPE
    n = len(d["pos_active"])
    out = np.zeros(n, STATE_DTYPE)
    for i in range(n):
        p = d["pos_pieces"][i].astype(np.uint32)
        e = d["pos_enemy"][i].astype(np.uint32)
        for a in range(81):
            out["own"][i, a // 27] |= p[a] << (a % 27)
            out["opp"][i, a // 27] |= e[a] << (a % 27)
        mains = 0
        for b in range(9):
            mains |= int(d["pos_main_p"][i][b]) << b
            mains |= int(d["pos_main_e"][i][b]) << (16 + b)
        out["mains"][i] = mains
        out["active"][i] = d["pos_active"][i]
    return out


def _oracle_state(core, st):
    p = np.zeros(81, np.int32)
    e = np.zeros(81, np.int32)
    for a in range(81):
        p[a] = (int(st["own"][a // 27]) >> (a % 27)) & 1
        e[a] = (int(st["opp"][a // 27]) >> (a % 27)) & 1
    mp = [(int(st["mains"]) >> b) & 1 for b in range(9)]
    me = [(int(st["mains"]) >> (16 + b)) & 1 for b in range(9)]
    return core.OrState.from_arrays(p.reshape(9, 9), e.reshape(9, 9), mp, me, int(st["active"]))


def _random_positions(core, n, seed):
    from uttt_amd import as_states  # noqa: F401
    from uttt_amd._lib import STATE_DTYPE
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        s = core.OrState.initial()
        while not s.is_done() and len(out) < n:
            if rng.random() < 0.3:
                out.append(s)
            s = s.next(rng.choice(s.legal_actions()))
    arr = np.zeros(n, STATE_DTYPE)
    for i, s in enumerate(out):
        p, e, mp, me, a = s.arrays()
        for x in range(81):
            arr["own"][i, x // 27] |= int(p.reshape(81)[x]) << (x % 27)
            arr["opp"][i, x // 27] |= int(e.reshape(81)[x]) << (x % 27)
        arr["mains"][i] = sum(int(mp[b]) << b for b in range(9)) | sum(int(me[b]) << (16 + b) for b in range(9))
        arr["active"][i] = a
    return arr, out


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import uttt_amd
    return uttt_amd


def test_search_matches_golden(gpu, oracle_lib):
    d = golden("search.npz")
    roots = _pos_states(d)
    bs = gpu.BatchedSearch(len(roots), 400)
    ev = gpu.HashEvaluator(bs.engine)
    checked = 0
    for (S, B) in CONFIGS:
        bs.run(roots, ev, S, B)
        for tau in (1.0, 0.0, 0.5):
            sc, L = bs.scores(tau)
            rows = np.nonzero((d["sims"] == S) & (d["batch"] == B) & (d["temp"] == np.float32(tau)))[0]
            assert len(rows) == len(roots)
            for r in rows:
                pi = int(d["pos"][r])
                n = int(d["n"][r])
                assert L[pi] == n
                assert np.array_equal(sc[pi, :n].view(np.uint32), d["scores"][r][:n].view(np.uint32)), (S, B, tau, pi)
                checked += 1
    assert checked == len(d["n"])


def test_search_matches_oracle_random_positions(gpu, oracle_lib):
    core = oracle_lib
    roots, ostates = _random_positions(core, 384, seed=5)
    bs = gpu.BatchedSearch(len(roots), 400)
    ev = gpu.HashEvaluator(bs.engine)
    for (S, B) in [(50, 8), (200, 4), (400, 8), (33, 5)]:
        bs.run(roots, ev, S, B)
        visits, L = bs.visits()
        for i, s in enumerate(ostates):
            _, vi, _ = core.pv_mcts_scores_hash(s, 1.0, S, B)
            assert L[i] == vi.size
            assert np.array_equal(visits[i, :L[i]], vi), (S, B, i)
            assert visits[i].sum() == S


def test_search_matches_oracle_large_flushes(gpu, oracle_lib):
    """Flushes of up to 64-100 copies append k x L children per node, more than 64 scan groups of
    the wave arg-max's tie search when L > 40 (the tie search covered 64 groups only)."""
    core = oracle_lib
    roots, ostates = _random_positions(core, 96, seed=41)
    bs = gpu.BatchedSearch(len(roots), 400)
    ev = gpu.HashEvaluator(bs.engine)
    for (S, B) in [(400, 64), (300, 100)]:
        bs.run(roots, ev, S, B)
        visits, L = bs.visits()
        for i, s in enumerate(ostates):
            _, vi, _ = core.pv_mcts_scores_hash(s, 1.0, S, B)
            assert np.array_equal(visits[i, :L[i]], vi), (S, B, i)
            assert visits[i].sum() == S


def test_selfplay_matches_reference_driver(gpu):
    """Golden games = reference self_play_cpp.play after np.random.seed(1234 + g)."""
    d = golden("selfplay.npz")
    ng = len(d["lengths"])
    for slots in (5, 16):
        sp = gpu.SelfPlay(slots, 50, 8, 1.0)
        sp.run(0, ng, int(d["seeds"][0]))
        recs = sp.records()
        assert [r["game"] for r in recs] == list(range(ng))
        off = 0
        for g, r in enumerate(recs):
            ln = int(d["lengths"][g])
            sl = slice(off, off + ln)
            assert len(r["actions"]) == ln
            assert np.array_equal(r["actions"], d["actions"][sl].astype(np.int64))
            assert np.array_equal(r["policies"].view(np.uint64), d["policies"][sl].view(np.uint64))
            assert np.array_equal(r["values"], d["values"][sl].astype(np.int64))
            assert np.array_equal(r["inputs"].reshape(ln, 243), d["tensors"][sl].astype(np.float32))
            off += ln


def test_selfplay_matches_oracle_and_is_slot_invariant(gpu, oracle_lib):
    """Records equal the oracle's for any slot count and any number of lanes
    (engines on separate streams, round-robined by SelfPlay.step)."""
    core = oracle_lib
    n_games, seed = 24, 777
    ref = [core.self_play_game_hash(seed + g, 1.0, 30, 4) for g in range(n_games)]
    for slots, lanes in ((1, 1), (7, 1), (32, 1), (8, 2), (12, 3)):
        sp = gpu.SelfPlay(slots, 30, 4, 1.0, lanes=lanes)
        sp.run(0, n_games, seed)
        recs = sp.records()
        assert len(recs) == n_games
        for g, r in enumerate(recs):
            assert np.array_equal(r["actions"], ref[g]["actions"].astype(np.int64)), (slots, lanes, g)
            assert np.array_equal(r["policies"].view(np.uint64), ref[g]["policies"].view(np.uint64))
            assert np.array_equal(r["values"], ref[g]["values"].astype(np.int64))


@pytest.mark.parametrize("batch", ["2", "4"])
def test_batched_hash_rounds_change_no_record(gpu, oracle_lib, batch, monkeypatch):
    """Several one-dispatch hash rounds per host call (UTTT_ROUND_BATCH; the rounds enqueued past a move's
    end find every tree done): records still equal the oracle's bit for bit, with two lanes too."""
    monkeypatch.setenv("UTTT_ROUND_BATCH", batch)
    n_games, seed = 12, 808
    ref = [oracle_lib.self_play_game_hash(seed + g, 1.0, 30, 4) for g in range(n_games)]
    for lanes in (1, 2):
        sp = gpu.SelfPlay(8, 30, 4, 1.0, lanes=lanes)
        sp.run(0, n_games, seed)
        recs = sp.records()
        assert len(recs) == n_games
        for g, r in enumerate(recs):
            assert np.array_equal(r["actions"], ref[g]["actions"].astype(np.int64)), (batch, lanes, g)
            assert np.array_equal(r["policies"].view(np.uint64), ref[g]["policies"].view(np.uint64))


def test_move_loop_in_c_equals_the_python_round_loop(gpu, oracle_lib, monkeypatch):
    """One lane with the hash evaluator runs each move's round loop in one C call (uttt_rounds_hash_move,
    SelfPlay._steps_move_loop); UTTT_MOVE_LOOP=0 keeps the Python round loop. Both give the oracle's records,
    the same totals (simulations, rounds with leaves, leaves, finished games) and play the same moves per
    steps(k) call. The evaluation cache is off here: with it on, whether a tree hits a position another tree
    inserts in the same round depends on timing, which moves leaves between rounds (never a record)."""
    n_games, seed = 20, 909
    ref = [oracle_lib.self_play_game_hash(seed + g, 1.0, 30, 4) for g in range(n_games)]
    stats = {}
    for loop in ("1", "0"):
        monkeypatch.setenv("UTTT_MOVE_LOOP", loop)
        sp = gpu.SelfPlay(6, 30, 4, 1.0, cache_log2=0)
        sp.begin(0, n_games, seed)
        per_call = [sp.steps(5) for _ in range(3)]
        per_call.append(sp.steps())
        recs = sp.records()
        assert len(recs) == n_games
        for g, r in enumerate(recs):
            assert np.array_equal(r["actions"], ref[g]["actions"].astype(np.int64)), (loop, g)
            assert np.array_equal(r["policies"].view(np.uint64), ref[g]["policies"].view(np.uint64)), (loop, g)
        stats[loop] = (per_call, sp.sims, sp.rounds, sp.leaves, sp.finished, sp.moves)
    assert stats["1"] == stats["0"]


_UNFUSED_CHILD = """
import sys
import numpy as np
import uttt_amd
sp = uttt_amd.SelfPlay(6, 30, 4, 1.0, cache_log2=0)
sp.run(0, int(sys.argv[2]), int(sys.argv[3]))
recs = sp.records(with_inputs=False)
np.savez(sys.argv[1], games=np.array([r["game"] for r in recs]), lengths=np.array([len(r["actions"]) for r in recs]),
         actions=np.concatenate([r["actions"] for r in recs]), policies=np.concatenate([r["policies"] for r in recs]))
"""


def test_unfused_hash_rounds_match_the_oracle(gpu, oracle_lib, tmp_path):
    """UTTT_FUSED_ROUNDS=0 (read once per process, so a fresh child): each hash round is the public calls'
    select + scan, hash evaluation and apply, nothing is staged (flush_dev_apply finds nothing at the move's
    end), and the C move loop waits on the ring slot's tag. One lane; records equal the oracle's bit for bit."""
    n_games, seed = 8, 515
    ref = [oracle_lib.self_play_game_hash(seed + g, 1.0, 30, 4) for g in range(n_games)]
    out = str(tmp_path / "unfused.npz")
    env = dict(os.environ, UTTT_FUSED_ROUNDS="0", PYTHONPATH=os.pathsep.join((REPO, PKG)))
    r = subprocess.run([sys.executable, "-c", _UNFUSED_CHILD, out, str(n_games), str(seed)], capture_output=True,
                       text=True, env=env, timeout=60, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    with np.load(out) as z:
        games, lengths, actions, policies = z["games"], z["lengths"], z["actions"], z["policies"]
    assert games.tolist() == list(range(n_games))
    off = 0
    for g, n in enumerate(lengths.tolist()):
        assert np.array_equal(actions[off:off + n], ref[g]["actions"].astype(np.int64)), g
        assert np.array_equal(policies[off:off + n].view(np.uint64), ref[g]["policies"].view(np.uint64)), g
        off += n
    assert off == len(actions)


@pytest.mark.parametrize("budget", ["1", "3"])
def test_select_budget_changes_no_record(gpu, oracle_lib, budget, monkeypatch):
    """UTTT_SELECT_BUDGET (in-place completions per tree and k_select launch) only spreads a move's
    simulations over more or fewer launches: records still equal the oracle's bit for bit."""
    monkeypatch.setenv("UTTT_SELECT_BUDGET", budget)
    n_games, seed = 8, 606
    ref = [oracle_lib.self_play_game_hash(seed + g, 1.0, 30, 4) for g in range(n_games)]
    sp = gpu.SelfPlay(8, 30, 4, 1.0, cache_log2=12)
    sp.run(0, n_games, seed)
    recs = sp.records()
    assert len(recs) == n_games
    for g, r in enumerate(recs):
        assert np.array_equal(r["actions"], ref[g]["actions"].astype(np.int64)), (budget, g)
        assert np.array_equal(r["policies"].view(np.uint64), ref[g]["policies"].view(np.uint64)), (budget, g)


def _hash_sync_visits(gpu, roots, sims, batch):
    """Root visits of a hash-evaluator search through the blocking round loop (select, eval, apply)."""
    import torch
    bs = gpu.BatchedSearch(len(roots), sims)
    e = bs.engine
    e.search_begin(roots, sims, batch)
    pol = torch.zeros((len(roots), 81), dtype=torch.float32, device=bs.x.device)
    val = torch.zeros(len(roots), dtype=torch.float32, device=bs.x.device)
    while True:
        n = e.select(bs.x)
        if n == 0:
            break
        e.eval_hash(bs.x, n, pol, val)
        e.apply(pol[:n], val[:n])
    return e.root_visits()


def _hash_round(e, r, pol, val):
    """One uttt_round_hash_async round in ring slot r % 8; returns its [pending, stopped, left] counts."""
    import time
    slot = r % 8
    tag = e.round_hash_async(slot, pol, val)
    ring = e.count_ring()
    t0 = time.time()
    while int(ring[slot, 3]) != tag:
        assert time.time() - t0 < 30, "round tag not stored"
    return ring[slot, :3].copy()


def test_fused_hash_rounds_and_host_flush_match_the_blocking_loop(gpu, oracle_lib):
    """uttt_round_hash_async (k_round: the previous round's apply and the next select in one launch, the
    round's own apply staged) gives the blocking loop's root visits on 64 trees; and on a one-tree search,
    uttt_search_select_host / apply_host after two staged hash rounds apply the staged round first, so the
    mixed search also ends with the blocking loop's visits."""
    import ctypes

    import torch
    from uttt_amd import _lib
    roots, _ = _random_positions(oracle_lib, 64, seed=29)
    sims, batch = 50, 8
    ref_v, ref_l = _hash_sync_visits(gpu, roots, sims, batch)
    e = gpu.Engine(len(roots), sims)
    dev = torch.device("cuda", e.device)
    pol = torch.zeros((len(roots), 81), dtype=torch.float32, device=dev)
    val = torch.zeros(len(roots), dtype=torch.float32, device=dev)
    e.search_begin(roots, sims, batch)
    for r in range(10 * sims):
        if _hash_round(e, r, pol, val)[2] == 0:
            break
    v, L = e.root_visits()
    assert np.array_equal(L, ref_l) and np.array_equal(v, ref_v)

    # one-tree searches of every root (trees are independent without the evaluation cache, so each must
    # end with its row of the 64-tree visits): two staged hash rounds, then the host-flush path
    lib = _lib.load()
    e1 = gpu.Engine(1, sims)
    leaf = np.zeros(1, _lib.STATE_DTYPE)
    x_hwc = np.zeros(243, np.float32)
    mixed = 0
    for i in range(len(roots)):
        e1.search_begin(roots[i:i + 1], sims, batch)
        ended = False
        for r in range(2):
            ended = _hash_round(e1, r, pol, val)[2] == 0
            if ended:
                break
        mixed += not ended
        for _ in range(10 * sims):
            k, n = ctypes.c_int32(), ctypes.c_int32()
            _lib.check(lib.uttt_search_select_host(e1.h, leaf.ctypes.data_as(ctypes.POINTER(_lib.UtttState)),
                                                   ctypes.byref(k), ctypes.byref(n)))
            if n.value == 0:
                break
            _lib.check(lib.uttt_states_input_hwc(leaf.ctypes.data_as(ctypes.POINTER(_lib.UtttState)), 1,
                                                 x_hwc.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
            x = torch.from_numpy(np.ascontiguousarray(x_hwc.reshape(81, 3).T).reshape(1, 243)).to(dev)
            e1.eval_hash(x, 1, pol, val)
            p1 = np.ascontiguousarray(pol[:1].cpu().numpy())
            v1 = np.ascontiguousarray(val[:1].cpu().numpy())
            _lib.check(lib.uttt_search_apply_host(e1.h, ctypes.c_void_p(p1.ctypes.data), 81,
                                                  ctypes.c_void_p(v1.ctypes.data), 1))
        v, L = e1.root_visits()
        assert L[0] == ref_l[i] and np.array_equal(v[0], ref_v[i]), i
    assert mixed >= len(roots) // 2  # most searches did start the host path with a staged round


@pytest.mark.parametrize("depth", ["2", "3"])
def test_round_lookahead_leaves_every_round_count_readable(gpu, oracle_lib, depth, monkeypatch):
    """Rounds enqueued ahead of their count (UTTT_ROUND_LOOKAHEAD) and dropped when a lane's last game
    ends, or when a move completes, get count 0: every RoundCount an evaluator saw is readable after
    the run (round 4's bench crashed on one left unread), and the records still equal the oracle's."""
    monkeypatch.setenv("UTTT_ROUND_LOOKAHEAD", depth)
    n_games, seed = 10, 919
    ref = [oracle_lib.self_play_game_hash(seed + g, 1.0, 30, 4) for g in range(n_games)]
    seen = []

    def make(eng):
        inner = gpu.HashEvaluator(eng)

        def ev(x, n):
            seen.append(n)
            return inner(x, n)
        ev.device_count = True
        ev.cheap = True
        return ev

    sp = gpu.SelfPlay(4, 30, 4, 1.0, lanes=2)
    sp.set_evaluator(make)
    sp.run(0, n_games, seed)
    assert seen and all(int(n) >= 0 for n in seen)
    recs = sp.records()
    assert len(recs) == n_games
    for g, r in enumerate(recs):
        assert np.array_equal(r["actions"], ref[g]["actions"].astype(np.int64)), (depth, g)
        assert np.array_equal(r["policies"].view(np.uint64), ref[g]["policies"].view(np.uint64)), (depth, g)


@pytest.mark.parametrize("tau", [0.0, 0.5, 2.0])
def test_selfplay_other_temperatures_match_oracle(gpu, oracle_lib, tau):
    """k_move_end's one-hot (tau 0) and pow (tau != 1) score paths against the oracle's
    boltzman (uttt_mcts.cpp:199-216) and self_play_cpp.play (:63-92)."""
    n_games, seed = 6, 4242
    ref = [oracle_lib.self_play_game_hash(seed + g, tau, 30, 4) for g in range(n_games)]
    sp = gpu.SelfPlay(3, 30, 4, tau)
    sp.run(0, n_games, seed)
    recs = sp.records()
    assert len(recs) == n_games
    for g, r in enumerate(recs):
        assert np.array_equal(r["actions"], ref[g]["actions"].astype(np.int64)), (tau, g)
        assert np.array_equal(r["policies"].view(np.uint64), ref[g]["policies"].view(np.uint64)), (tau, g)
        assert np.array_equal(r["values"], ref[g]["values"].astype(np.int64))


def test_engine_lifecycle_regrows_and_destroys(gpu, oracle_lib):
    """Create -> self-play -> self-play again with a larger record arena (the arena's regrowth) -> playouts of 1
    and of 1,100 positions (past the playout buffers' first capacity of 1,024 rows) -> destroy, three times over
    in one process. Every call returns UTTT_OK, both runs' records equal the oracle's, and the playout counts
    equal uttt_playout_host's. (No assertion on free device memory: the machine's is not this process's alone;
    that destroy frees every block is the sanitizer program's and the owner type's part.)"""
    import ctypes
    import torch
    from uttt_amd._lib import UtttState
    from uttt_amd.engine import Engine
    n_games, seed, sims, batch = 4, 3131, 8, 2
    ref = [oracle_lib.self_play_game_hash(seed + g, 1.0, sims, batch) for g in range(n_games)]

    def play(e, ev, x, arena_plies):
        e.selfplay_begin(0, n_games, seed, 1.0, sims, batch, arena_plies)
        while e.move_begin() > 0:
            while True:
                n = e.select(x)
                if n == 0:
                    break
                e.apply(*ev(x, n))
            e.move_end()
        ids, off, ln = e.games()
        pl = e.plies(with_inputs=False)
        assert ids.tolist() == list(range(n_games))
        for g, o, n in zip(ids.tolist(), off.tolist(), ln.tolist()):
            assert np.array_equal(pl["actions"][o:o + n].astype(np.int64), ref[g]["actions"].astype(np.int64)), g
            assert np.array_equal(pl["policies"][o:o + n].view(np.uint64), ref[g]["policies"].view(np.uint64)), g
            assert np.array_equal(pl["values"][o:o + n].astype(np.int64), ref[g]["values"].astype(np.int64)), g
        return pl

    def host_counts(lib, st, playouts, sd):
        w, l = np.zeros(len(st), np.int32), np.zeros(len(st), np.int32)
        i32 = ctypes.POINTER(ctypes.c_int32)
        assert lib.uttt_playout_host(st.ctypes.data_as(ctypes.POINTER(UtttState)), len(st), playouts, sd,
                                     w.ctypes.data_as(i32), l.ctypes.data_as(i32)) == 0
        return w, l

    for _ in range(3):
        e = Engine(4, 8)
        ev = gpu.HashEvaluator(e)
        x = torch.zeros((4, 3, 9, 9), dtype=torch.float32, device=torch.device("cuda", e.device))
        first = play(e, ev, x, 4 * 81)
        again = play(e, ev, x, 8 * 81)
        for key in ("states", "policies", "actions", "values"):
            assert first[key].tobytes() == again[key].tobytes(), key
        st = np.resize(first["states"], 1100)  # the games' positions, repeated
        for n in (1, 1100):
            wins, losses = e.playouts(st[:n], 64, seed=9)
            ends = np.ascontiguousarray(st[[0, n - 1]])
            hw, hl = host_counts(e.lib, ends, 64, 9)
            assert (wins[0], losses[0], wins[n - 1], losses[n - 1]) == (hw[0], hl[0], hw[1], hl[1]), n
        assert e.lib.uttt_engine_destroy(e.h) == 0
        e.h = None


def test_play_uses_and_advances_global_numpy_rng(gpu):
    import self_play_cpp
    from oracle.hashnp import make_hash_model
    d = golden("selfplay.npz")
    model = make_hash_model()
    off = 0
    for g in range(3):
        np.random.seed(int(d["seeds"][g]))
        h = self_play_cpp.play(model)
        ln = int(d["lengths"][g])
        assert len(h) == ln
        for i in range(ln):
            assert np.array_equal(np.asarray(h[i][1]).view(np.uint64), d["policies"][off + i].view(np.uint64))
            assert h[i][2] == d["values"][off + i]
            assert h[i][0].shape == (9, 9, 3)
        # one random_sample() (two MT words) per ply, exactly like np.random.choice
        ref = np.random.RandomState(int(d["seeds"][g]))
        for _ in range(ln):
            ref.random_sample()
        assert np.random.get_state()[2] == ref.get_state()[2]
        assert np.array_equal(np.random.get_state()[1], ref.get_state()[1])
        off += ln


def test_uttt_cpp_callback_search_matches_golden(gpu):
    import uttt_cpp
    from oracle.hashnp import hash_eval_np
    d = golden("search.npz")
    calls = []

    def model(states):
        calls.append(len(states))
        out = []
        for s in states:
            x = np.asarray(s.to_input_tensor(), np.float32).reshape(9, 9, 3).transpose(2, 0, 1)
            p, v = hash_eval_np(x)
            out.append((p, float(v)))
        return out

    rows = np.nonzero(((d["sims"] == 50) & (d["batch"] == 8)) | ((d["sims"] == 30) & (d["batch"] == 3)))[0]
    for dedup in (True, False):
        for r in rows[::2]:
            i = int(d["pos"][r])
            st = uttt_cpp.State(d["pos_pieces"][i].reshape(9, 9).tolist(), d["pos_enemy"][i].reshape(9, 9).tolist(),
                                d["pos_main_p"][i].tolist(), d["pos_main_e"][i].tolist(), int(d["pos_active"][i]))
            calls.clear()
            sc = np.asarray(uttt_cpp.pv_mcts_scores(model=model, state=st, temperature=float(d["temp"][r]),
                                                    evaluate_count=int(d["sims"][r]), batch_size=int(d["batch"][r]),
                                                    dedup=dedup), np.float32)
            n = int(d["n"][r])
            assert np.array_equal(sc.view(np.uint32), d["scores"][r][:n].view(np.uint32))
            assert len(calls) == d["flushes"][r]
            if not dedup:
                assert sum(calls) == d["evals"][r]
    # the default is the reference's call pattern (python_bindings.cpp:11-47): the k queued copies per flush
    r = rows[0]
    i = int(d["pos"][r])
    st = uttt_cpp.State(d["pos_pieces"][i].reshape(9, 9).tolist(), d["pos_enemy"][i].reshape(9, 9).tolist(),
                        d["pos_main_p"][i].tolist(), d["pos_main_e"][i].tolist(), int(d["pos_active"][i]))
    calls.clear()
    sc = np.asarray(uttt_cpp.pv_mcts_scores(model=model, state=st, temperature=float(d["temp"][r]),
                                            evaluate_count=int(d["sims"][r]), batch_size=int(d["batch"][r])), np.float32)
    assert np.array_equal(sc.view(np.uint32), d["scores"][r][:int(d["n"][r])].view(np.uint32))
    assert len(calls) == d["flushes"][r] and sum(calls) == d["evals"][r]


def test_uttt_cpp_resident_search_resumes_and_recovers(gpu):
    """uttt_cpp.pv_mcts_scores runs the whole search as one resident wave (round 6, uttt_search1_*). A model
    slower than the wave's 100 ms wait for a command (the wave exits; the next flush resumes it with the
    command it did not see applied first), and a model that raises mid-search (the wave is left resident;
    the next search stops it first) both leave the golden scores bit-exact."""
    import time
    import uttt_cpp
    from oracle.hashnp import hash_eval_np
    d = golden("search.npz")
    rows = np.nonzero((d["sims"] == 50) & (d["batch"] == 8))[0]
    r = int(rows[0])
    i = int(d["pos"][r])

    def state():
        return uttt_cpp.State(d["pos_pieces"][i].reshape(9, 9).tolist(), d["pos_enemy"][i].reshape(9, 9).tolist(),
                              d["pos_main_p"][i].tolist(), d["pos_main_e"][i].tolist(), int(d["pos_active"][i]))

    def evaluate(states):
        out = []
        for s in states:
            x = np.asarray(s.to_input_tensor(), np.float32).reshape(9, 9, 3).transpose(2, 0, 1)
            p, v = hash_eval_np(x)
            out.append((p, float(v)))
        return out

    calls = []

    def slow(states):
        calls.append(len(states))
        if len(calls) in (2, 4):
            time.sleep(0.25)
        return evaluate(states)

    def search(model):
        return np.asarray(uttt_cpp.pv_mcts_scores(model=model, state=state(), temperature=float(d["temp"][r]),
                                                  evaluate_count=50, batch_size=8), np.float32)

    n = int(d["n"][r])
    sc = search(slow)
    assert np.array_equal(sc.view(np.uint32), d["scores"][r][:n].view(np.uint32))
    assert len(calls) == d["flushes"][r]

    def failing(states):
        raise RuntimeError("model failure")

    with pytest.raises(RuntimeError, match="model failure"):
        search(failing)
    sc = search(evaluate)
    assert np.array_equal(sc.view(np.uint32), d["scores"][r][:n].view(np.uint32))


def test_uttt_cpp_distinct_copy_results_match_oracle(gpu, oracle_lib):
    """The reference applies each queued copy's own result in order (uttt_mcts.cpp:138-167). A model whose
    result changes with every state it is handed (a hash salted by a running count) gives each copy of a
    flush a different row; the resident search (k_search1, rows loaded in chunks of 8) must equal the oracle
    bit for bit, at batches above and below the chunk (k up to 16: a second chunk is reloaded)."""
    import uttt_cpp
    from oracle import core
    from oracle.hashnp import hash_eval_np
    _, ostates = _random_positions(core, 6, 4242)
    for S, B, T in ((50, 8, 1.0), (30, 3, 0.5), (100, 16, 1.0), (60, 12, 0.0)):
        for os_ in ostates:
            cnt = [0]

            def oracle_eval(x):
                cnt[0] += 1
                return hash_eval_np(np.asarray(x, np.float32), 0x9E3779B9 + cnt[0])

            ref_sc, _, st = core.pv_mcts_scores(os_, T, S, B, oracle_eval)
            n_ref = cnt[0]
            cnt[0] = 0

            def model(states):
                out = []
                for s in states:
                    x = np.asarray(s.to_input_tensor(), np.float32).reshape(9, 9, 3).transpose(2, 0, 1)
                    out.append(oracle_eval(x.reshape(-1)))
                return [(p, float(v)) for p, v in out]

            p, e, mp, me, a = os_.arrays()
            st_ = uttt_cpp.State(np.asarray(p).reshape(9, 9).tolist(), np.asarray(e).reshape(9, 9).tolist(),
                                 [int(v) for v in mp], [int(v) for v in me], int(a))
            sc = np.asarray(uttt_cpp.pv_mcts_scores(model=model, state=st_, temperature=T, evaluate_count=S,
                                                    batch_size=B), np.float32)
            assert cnt[0] == n_ref == st.evals
            assert np.array_equal(sc.view(np.uint32), np.asarray(ref_sc, np.float32).view(np.uint32)), (S, B, T)


def test_network_gpu_matches_cpu_fp32(gpu):
    """Value within 1e-5 of CPU fp32 (north star). The random-init net is saturated
    (|logits| up to ~1e2..1e3), so the policy is checked on its logits, relative to
    their scale (fp32 accumulation-order noise), not after the softmax that
    amplifies it. Plain and BN-folded channels-last forms."""
    import torch
    from uttt_amd.model import FoldedDualNetwork, policy_logits, random_network
    d = golden("network.npz")
    cpu = random_network(0)
    x = torch.from_numpy(d["x"])
    with torch.no_grad():
        p_ref, v_ref = cpu(x)
    assert np.allclose(p_ref.numpy(), d["policy"], atol=1e-6) and np.allclose(v_ref.numpy(), d["value"], atol=1e-6)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    rng = np.random.RandomState(0)
    xr = torch.from_numpy((rng.rand(256, 3, 9, 9) < 0.3).astype(np.float32))
    z_cpu, v_cpu = policy_logits(cpu, xr)
    g = random_network(0, "cuda")
    for net in (g, FoldedDualNetwork(g).to("cuda")):
        z, v = policy_logits(net, xr.cuda())
        assert (v.cpu() - v_cpu).abs().max().item() <= 1e-5
        # logits: 1e-4 of the row's scale (fp32 reordering on this saturated net: ~6e-6 folded vs plain on CPU)
        scale = z_cpu.abs().amax(dim=1, keepdim=True).clamp_min(1.0)
        assert ((z.cpu() - z_cpu).abs() / scale).max().item() <= 1e-4


@pytest.mark.parametrize("netkind", ["seed0", "calibrated"])
def test_nn_in_the_loop_search_replays_exactly(gpu, oracle_lib, netkind):
    """Engine + real DualNetwork (PyTorch-ROCm) on the GPU; every (input -> output) pair the
    network produced is replayed into the oracle: visit counts must be equal. The
    calibrated (non-saturated) net gives wide, realistic trees."""
    import torch
    from uttt_amd.model import calibrated_network, random_network
    core = oracle_lib
    roots, ostates = _random_positions(core, 64, seed=11)
    net = random_network(0, "cuda") if netkind == "seed0" else calibrated_network(NETCAL, "cuda")
    table = {}

    class Recording(gpu.NetworkEvaluator):
        def __call__(self, x, n):
            p, v = super().__call__(x, n)
            xs = x[:n].cpu().numpy().reshape(n, 243)
            ps, vs = p.cpu().numpy(), v.cpu().numpy().reshape(-1)
            for i in range(n):
                table[xs[i].tobytes()] = (ps[i].copy(), np.float32(vs[i]))
            return p, v

    bs = gpu.BatchedSearch(len(roots), 50)
    bs.run(roots, Recording(net, len(roots)), 50, 8)
    visits, L = bs.visits()

    def replay(x):
        return table[np.asarray(x, np.float32).reshape(243).tobytes()]

    for i, s in enumerate(ostates):
        _, vi, _ = core.pv_mcts_scores(s, 1.0, 50, 8, replay)
        assert np.array_equal(visits[i, :L[i]], vi), i
    assert torch.cuda.is_available()


def test_full_size_4096x50_properties_and_samples(gpu, oracle_lib):
    """BASELINE size (4096 trees x 50 sims, B=8): every root's visits sum to 50;
    a sample of trees is bit-checked against the oracle."""
    core = oracle_lib
    roots, ostates = _random_positions(core, 4096, seed=21)
    bs = gpu.BatchedSearch(4096, 400)
    ev = gpu.HashEvaluator(bs.engine)
    for (S, B) in [(50, 8), (400, 8)]:
        bs.run(roots, ev, S, B)
        visits, L = bs.visits()
        assert (visits.sum(axis=1) == S).all()
        for i in range(0, 4096, 97):
            _, vi, _ = core.pv_mcts_scores_hash(ostates[i], 1.0, S, B)
            assert np.array_equal(visits[i, :L[i]], vi), (S, B, i)


def test_fused_evaluator_matches_cpu_fp32(gpu, oracle_lib):
    """Stem-from-bitboards + Winograd tower + HIP heads vs the plain DualNetwork on CPU
    fp32, on real pending leaves of a search, for both tower kernels; the saturated seed-0
    net (logits checked relative to their scale) and the calibrated one (post-softmax
    policy and value within 1e-5 absolute)."""
    from uttt_amd.model import calibrated_network, random_network
    from uttt_amd.nnfast import FusedNetworkEvaluator
    roots, _ = _random_positions(oracle_lib, 300, seed=13)
    bs = gpu.BatchedSearch(len(roots), 50)
    for make, sat in ((lambda d: random_network(0, d), True), (lambda d: calibrated_network(NETCAL, d), False)):
        net = make("cuda")
        _fused_vs_cpu(gpu, bs, roots, FusedNetworkEvaluator(net, bs.engine), make("cpu"), sat)


def _fused_vs_cpu(gpu, bs, roots, fused, cpu, saturated):
    import torch
    from uttt_amd.model import policy_logits
    e = bs.engine
    e.use_stream()
    e.search_begin(roots, 50, 8)
    for _ in range(3):  # a few rounds: leaves at depth 1 and 2
        n = e.select(bs.x)
        z, v = fused.forward(n, softmax=False)
        z_cpu, v_cpu = policy_logits(cpu, bs.x[:n].cpu())
        assert (v.cpu() - v_cpu.reshape(-1)).abs().max().item() <= 1e-5
        scale = z_cpu.abs().amax(dim=1, keepdim=True).clamp_min(1.0)
        assert ((z.cpu() - z_cpu).abs() / scale).max().item() <= 1e-4
        p, v2 = fused.forward(n, softmax=True)
        assert torch.allclose(p.sum(dim=1).cpu(), torch.ones(n), atol=1e-5)
        if not saturated:  # (a saturated softmax turns logit rounding noise into O(1) differences)
            assert (p.cpu() - torch.softmax(z_cpu, dim=1)).abs().max().item() <= 1e-5
        e.apply(p, v2)


@pytest.fixture(scope="module")
def trained_net(gpu):
    """The seed-0 DualNetwork after ~300 Adam steps of this build's train_network (HIP-graph step,
    batch 128) on a learnable history: 64 self-play games of the engine with the hash evaluator
    (policy targets = search visit distributions, value targets = half the game outcome). Weights, BatchNorm statistics and so the
    split-f16 kernels' weight-derived scales (U scale per conv, stem bound) are those of a trained
    net, not of the initialisation."""
    import torch
    from uttt_amd import train
    from uttt_amd.model import random_network
    sp = gpu.SelfPlay(64, 50, 8, 1.0)
    sp.run(0, 64, 2024)
    # value targets halved: a value head fitted to +-1 game outcomes saturates tanh, which would
    # hide value differences; the policy targets are the searches' visit distributions
    hist = [[x, p, 0.5 * v] for x, p, v in gpu.history_from_records(sp.records())]
    net = random_network(0, "cuda").train()
    epochs = max(1, -(-300 // -(-len(hist) // train.BATCH_SIZE)))
    losses = train.train_network(net, hist, epochs=epochs, device=torch.device("cuda", 0), log=None)
    assert losses[-1] < losses[0], losses  # it learned something
    return net.eval(), losses


def test_fused_matches_fp32_on_trained_net(gpu, trained_net):
    """The north star's 1e-5 network bound on TRAINED weights: the fused evaluator (split-f16
    tower with the trained net's weight-derived scales) against the same model's own fp32
    PyTorch forward on the CPU, on the netcal positions (dual_network.py:89-121): value and every
    post-softmax policy entry within 1e-5 absolute."""
    import copy

    import torch
    from uttt_amd.nnfast import FusedNetworkEvaluator
    d = golden("netcal.npz")
    x = torch.from_numpy(d["x"].astype(np.float32))
    # The trained trunk is what is under test (its BatchNorm statistics and weight-derived kernel
    # scales). How far the heads' last linear layers drive tanh / softmax into saturation on these
    # out-of-distribution positions depends on the training run (MIOpen's algorithm choices differ
    # between boxes), and a saturated output would hide the comparison; so those two layers are scaled
    # by exact powers of two until the outputs are mostly unsaturated. Both sides see the same net.
    net = copy.deepcopy(trained_net[0]).cpu().eval()
    with torch.no_grad():
        for _ in range(30):
            pr, vr = net(x)
            sat_v = float(vr.abs().median()) >= 0.95
            sat_p = float(pr.max(dim=1).values.median()) >= 0.95
            if not (sat_v or sat_p):
                break
            for layer, sat in ((net.value_fc2, sat_v), (net.policy_fc, sat_p)):
                if sat:
                    layer.weight.mul_(0.5)
                    layer.bias.mul_(0.5)
    # mostly not saturated: the comparison is not hidden behind tanh / softmax clamping
    assert float(vr.abs().median()) < 0.95 and float(pr.max(dim=1).values.median()) < 0.95
    states = _rules_states(d["rules_index"])
    fe = FusedNetworkEvaluator(copy.deepcopy(net).cuda().eval(), None, max_batch=len(states))
    p, v = fe.forward_states(states)
    ep = float((p.cpu() - pr).abs().max())
    ev = float((v.cpu() - vr.reshape(-1)).abs().max())
    assert ev <= 1e-5 and ep <= 1e-5, (ep, ev)


@pytest.mark.parametrize("netkind", ["seed0", "calibrated", "trained"])
def test_fused_evaluator_search_replays_exactly(gpu, oracle_lib, netkind, request):
    """Search with the fused evaluator; its outputs replayed into the oracle give
    the same root visit counts."""
    from uttt_amd.model import calibrated_network, random_network
    from uttt_amd.nnfast import FusedNetworkEvaluator
    core = oracle_lib
    roots, ostates = _random_positions(core, 48, seed=17)
    bs = gpu.BatchedSearch(len(roots), 50)
    if netkind == "trained":
        net = request.getfixturevalue("trained_net")[0]
    else:
        net = random_network(0, "cuda") if netkind == "seed0" else calibrated_network(NETCAL, "cuda")
    fused = FusedNetworkEvaluator(net, bs.engine)
    table = {}

    def recording(x, n):
        p, v = fused(x, n)
        xs = x[:n].cpu().numpy().reshape(n, 243)
        ps, vs = p.cpu().numpy(), v.cpu().numpy().reshape(-1)
        for i in range(n):
            table[xs[i].tobytes()] = (ps[i].copy(), np.float32(vs[i]))
        return p, v

    bs.run(roots, recording, 50, 8)  # plain function: needs_input -> select writes x
    visits, L = bs.visits()
    for i, s in enumerate(ostates):
        _, vi, _ = core.pv_mcts_scores(s, 1.0, 50, 8, lambda x: table[np.asarray(x, np.float32).tobytes()])
        assert np.array_equal(visits[i, :L[i]], vi), i


def test_fused_selfplay_lanes_are_bit_identical(gpu):
    """Self-play with the fused network evaluator on the calibrated (non-saturated) net:
    1 lane without the evaluation cache, 1 lane with it, and 2 lanes sharing it (two
    engines on two streams, network calls overlapping) give the same records bit for
    bit - every kernel computes a board independently of the batch it is in, so cached
    outputs equal fresh ones. The rounds run without a per-round host sync (the count read
    on the device, lanes pipelined across moves, SelfPlay.steps) except in the last
    configuration, the blocking lockstep loop: same records. (The number of network rounds may
    differ by a few: with lanes a move apart, a shared-cache hit can empty a round.)"""
    from uttt_amd.model import calibrated_network
    from uttt_amd.nnfast import FusedNetworkEvaluator
    net = calibrated_network(NETCAL, "cuda")
    out = []
    # the last two: the tower as one dataflow launch per forward (round 6), the count read on the device
    for lanes, cache, asy, tower in ((1, 0, True, "layers"), (1, 16, True, "layers"), (2, 16, True, "layers"),
                                     (2, 16, False, "layers"), (1, 0, True, "dataflow"), (2, 16, True, "dataflow")):
        sp = gpu.SelfPlay(16, 50, 8, 1.0, lanes=lanes, cache_log2=cache)
        sp.async_rounds = asy
        sp.set_evaluator(lambda eng: FusedNetworkEvaluator(net, eng, tower=tower))
        sp.run(0, 12, 4321)
        out.append(sp.records())
        if cache:
            assert sp.cache_stats()["hits"] > 0
    a = out[0]
    for b in out[1:]:
        assert [r["game"] for r in a] == [r["game"] for r in b] == list(range(12))
        for ra, rb in zip(a, b):
            assert np.array_equal(ra["actions"], rb["actions"])
            assert np.array_equal(ra["policies"].view(np.uint64), rb["policies"].view(np.uint64))
            assert np.array_equal(ra["values"], rb["values"])


def test_eval_cache_replacement_is_exact(gpu):
    """A tiny shared table (2^6 entries for 32 trees, two lanes on two streams): nearly every
    insert finds its 8 probe slots taken and replaces an entry another lane may be reading
    (cache_insert CAS 2 -> 1, rewrite, republish; cache_lookup re-checks flag and key after its
    drained payload loads). Records equal the no-cache run bit for bit, hits and replacements
    both happen."""
    from uttt_amd.model import calibrated_network
    from uttt_amd.nnfast import FusedNetworkEvaluator
    net = calibrated_network(NETCAL, "cuda")
    out, stats = [], []
    for lanes, cache in ((1, 0), (2, 6), (2, 7)):
        sp = gpu.SelfPlay(32, 50, 8, 1.0, lanes=lanes, cache_log2=cache)
        sp.set_evaluator(lambda eng: FusedNetworkEvaluator(net, eng))
        sp.run(0, 24, 99)
        out.append(sp.records())
        stats.append(sp.cache_stats())
    for st in stats[1:]:
        assert st["replacements"] > 0 and st["hits"] > 0 and st["inserts"] > (1 << 7), st
    a = out[0]
    for b in out[1:]:
        assert [r["game"] for r in a] == [r["game"] for r in b] == list(range(24))
        for ra, rb in zip(a, b):
            assert np.array_equal(ra["actions"], rb["actions"])
            assert np.array_equal(ra["policies"].view(np.uint64), rb["policies"].view(np.uint64))
            assert np.array_equal(ra["values"], rb["values"])


def test_eval_cache_is_exact(gpu, oracle_lib):
    """With the evaluation cache on, repeated and overlapping searches resolve
    leaves from the table and still match the oracle bit for bit."""
    core = oracle_lib
    roots, ostates = _random_positions(core, 256, seed=23)
    bs = gpu.BatchedSearch(len(roots), 400, cache_log2=16)
    ev = gpu.HashEvaluator(bs.engine)
    for rep, (S, B) in enumerate([(50, 8), (50, 8), (120, 4), (50, 1)]):
        bs.run(roots, ev, S, B)
        visits, L = bs.visits()
        for i in range(0, len(ostates), 5):
            _, vi, _ = core.pv_mcts_scores_hash(ostates[i], 1.0, S, B)
            assert np.array_equal(visits[i, :L[i]], vi), (rep, S, B, i)
    st = bs.engine.cache_stats()
    assert st["hits"] > 0 and st["inserts"] > 0


def test_nonfinite_evaluator_output_is_refused(gpu, oracle_lib):
    """SURVEY §5 failure detection. A NaN value or an Inf legal prior from the evaluator stops its
    tree (the reference would back it up silently, uttt_mcts.cpp:144-166) and the search end raises
    UTTT_ERR_NONFINITE; the poisoned row is neither expanded nor cached, so a later search with the
    same table and a clean evaluator matches the oracle bit for bit."""
    from uttt_amd._lib import EngineError
    core = oracle_lib
    roots, ostates = _random_positions(core, 64, seed=31)
    bs = gpu.BatchedSearch(len(roots), 400, cache_log2=14)
    ev = gpu.HashEvaluator(bs.engine)

    class Poison:
        def __init__(self, kind):
            self.kind, self.calls = kind, 0

        def __call__(self, x, n):
            p, v = ev(x, n)
            self.calls += 1
            if self.calls == 3:
                p, v = p.clone(), v.clone()
                if self.kind == "value":
                    v[n // 2] = float("nan")
                else:
                    p[n // 2, :] = float("inf")
            return p, v

    for kind in ("value", "policy"):
        with pytest.raises(EngineError, match="NONFINITE"):
            bs.run(roots, Poison(kind), 50, 8)
            bs.scores(1.0)
    inserts = bs.engine.cache_stats()["inserts"]
    assert inserts > 0
    bs.run(roots, ev, 50, 8)
    visits, L = bs.visits()
    for i, s in enumerate(ostates):
        _, vi, _ = core.pv_mcts_scores_hash(s, 1.0, 50, 8)
        assert np.array_equal(visits[i, :L[i]], vi), i
    assert bs.engine.cache_stats()["hits"] > 0


def test_nonfinite_in_async_selfplay_leaves_the_move_unended(gpu, oracle_lib):
    """Self-play with device-count rounds and asynchronous move ends: a NaN value stops its tree,
    the move end that follows changes nothing (the search's failure flag: k_move_end / k_finalize /
    k_archive skip, k_finalize records the first failed tree), and the host raises UTTT_ERR_NONFINITE when it
    reads that move's result. Every game
    archived before the failure equals the oracle's."""
    import torch
    from uttt_amd._lib import EngineError
    core = oracle_lib
    n_games, seed = 12, 4242

    class PoisonDev:
        device_count = True

        def __init__(self, eng):
            self.h = gpu.HashEvaluator(eng)
            self.calls = 0

        def __call__(self, x, n):
            p, v = self.h(x, n)
            self.calls += 1
            if self.calls >= 700:  # some games have been archived by then
                v.fill_(float("nan"))
            return p, v

    sp = gpu.SelfPlay(4, 30, 4, 1.0)
    sp.set_evaluator(PoisonDev)
    with pytest.raises(EngineError, match="NONFINITE"):
        sp.run(0, n_games, seed)
    torch.cuda.synchronize()
    recs = sp.records()
    assert 0 < len(recs) < n_games
    for r in recs:
        ref = core.self_play_game_hash(seed + r["game"], 1.0, 30, 4)
        assert np.array_equal(r["actions"], ref["actions"].astype(np.int64)), r["game"]
        assert np.array_equal(r["policies"].view(np.uint64), ref["policies"].view(np.uint64))


def test_split_f16_winograd_conv_matches_f64(gpu):
    """The split-f16 F(3x3,3x3) kernel (wino3h) vs an f64 direct conv: within 1e-5 of each
    board's output scale (the bar the f32 kernels meet) for ragged board counts (partial last
    7-board group), inputs spanning 1e-3..1e3 in scale (the per-board power-of-two V scaling),
    with and without residual; the per-board y_amax row equals each board's max(y) exactly."""
    import torch
    import torch.nn.functional as F
    from uttt_amd.model import fold_bn, random_network
    from uttt_amd.nnfast import conv3x3_wino3h, wino3h_weights
    net = random_network(3)
    g = torch.Generator().manual_seed(2)
    # n covers every residue mod 7 (a 7-board group is two 32-tile sets) and multi-group sizes
    for blk_i, n, scale in ((5, 1, 1.0), (5, 2, 1e-3), (3, 3, 1.0), (0, 4, 1.0), (2, 5, 1.0), (7, 6, 1.0),
                            (15, 7, 1e3), (1, 8, 1.0), (4, 11, 1.0), (5, 257, 30.0), (9, 1000, 1.0),
                            (11, 1603, 1.0)):
        blk = net.residual_blocks[blk_i]
        w, b = fold_bn(blk.conv1, blk.bn1)
        u, su = wino3h_weights(w)
        u, w, b = u.cuda(), w.cuda(), b.cuda()
        x = (torch.relu(torch.randn(n, 81, 128, generator=g)) * scale).cuda()
        r = (torch.randn(n, 81, 128, generator=g) * scale).cuda()
        xn = x.reshape(n, 9, 9, 128).permute(0, 3, 1, 2)
        ref = F.conv2d(xn.double(), w.double(), b.double(), padding=1).permute(0, 2, 3, 1).reshape(n, 81, 128)
        for res in (None, r):
            ya = torch.zeros(n, dtype=torch.int32, device="cuda")
            y = conv3x3_wino3h(x, u, su, b, res, y_amax=ya)
            want = torch.relu(ref + (res.double() if res is not None else 0)).float()
            err = (y - want).abs().reshape(n, -1).amax(dim=1)
            bscale = want.abs().reshape(n, -1).amax(dim=1).clamp_min(1e-30)
            assert (err / bscale).max().item() <= 1e-5, (blk_i, n, scale, res is None, (err / bscale).max().item())
            assert torch.equal(ya.view(torch.float32), y.reshape(n, -1).amax(dim=1))


def _rules_states(idx):
    """Packed engine states of rules.npz rows."""
    from uttt_amd._lib import STATE_DTYPE
    r = golden("rules.npz")
    out = np.zeros(len(idx), STATE_DTYPE)
    for j, i in enumerate(idx):
        p = r["pieces"][i].astype(np.uint32)
        e = r["enemy"][i].astype(np.uint32)
        for a in range(81):
            out["own"][j, a // 27] |= p[a] << (a % 27)
            out["opp"][j, a // 27] |= e[a] << (a % 27)
        out["mains"][j] = sum(int(r["main_p"][i][b]) << b for b in range(9)) | \
            sum(int(r["main_e"][i][b]) << (16 + b) for b in range(9))
        out["active"][j] = r["active"][i]
    return out


def test_networks_match_reference_on_calibrated_net(gpu):
    """North-star network bound on a NON-saturated net (tests/golden/netcal.npz: the
    reference's own dual_network.py on CPU fp32, calibrated BatchNorm statistics, values in
    about [-0.9, 0.25], median max policy 0.13): every GPU evaluator - the fused HIP
    evaluator with the split-f16 tower (default) and with the f32-MFMA tower, and the
    PyTorch-ROCm DualNetwork plain and BN-folded - within 1e-5 absolute on the value and
    on every post-softmax policy entry."""
    import torch
    from uttt_amd.model import FoldedDualNetwork, calibrated_network
    from uttt_amd.nnfast import FusedNetworkEvaluator
    d = golden("netcal.npz")
    states = _rules_states(d["rules_index"])
    x = torch.from_numpy(d["x"].astype(np.float32))
    # the fixture's inputs are these states' tensors (uttt_game.cpp:244-280, NCHW)
    r = golden("rules.npz")
    hwc = r["tensor"][d["rules_index"]].reshape(-1, 9, 9, 3).transpose(0, 3, 1, 2)
    assert np.array_equal(hwc, d["x"])
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    net = calibrated_network(NETCAL, "cuda")
    outs = {}
    for conv in ("wino3h",):
        fe = FusedNetworkEvaluator(net, None, max_batch=len(states), conv=conv)
        p, v = fe.forward_states(states)
        outs["fused-" + conv] = (p.cpu().numpy(), v.cpu().numpy())
    with torch.no_grad():
        p, v = net(x.cuda())
        outs["torch"] = (p.cpu().numpy(), v.cpu().numpy().reshape(-1))
        p, v = FoldedDualNetwork(net).to("cuda")(x.cuda())
        outs["torch-folded"] = (p.cpu().numpy(), v.cpu().numpy().reshape(-1))
    errs = {k: (float(np.abs(p - d["policy"]).max()), float(np.abs(v - d["value"]).max())) for k, (p, v) in outs.items()}
    for k, (ep, ev) in errs.items():
        assert ev <= 1e-5 and ep <= 1e-5, (k, errs)
    # the net is not saturated: parity above is not hidden by tanh / softmax clamping
    assert np.abs(d["value"]).max() < 0.95 and np.median(d["policy"].max(axis=1)) < 0.5


def test_fused_outputs_do_not_depend_on_the_batch(gpu):
    """A position's fused-evaluator outputs are bit-identical whether it is evaluated
    alone, in a batch of 64, or at an odd offset inside a batch of 1,000 other positions
    (per-board V scaling in the split-f16 tower): the evaluation cache's premise."""
    import torch
    from uttt_amd.model import calibrated_network
    from uttt_amd.nnfast import FusedNetworkEvaluator
    d = golden("netcal.npz")
    r = golden("rules.npz")
    mine = _rules_states(d["rules_index"][:64])
    rng = np.random.RandomState(9)
    others = _rules_states(rng.choice(np.nonzero(r["n_legal"] > 0)[0], 1000, replace=False))
    net = calibrated_network(NETCAL, "cuda")
    for conv in ("wino3h",):
        fe = FusedNetworkEvaluator(net, None, max_batch=1100, conv=conv)
        p0, v0 = (t.clone() for t in fe.forward_states(mine))
        big = np.concatenate([others[:37], mine, others[37:]])
        p1, v1 = fe.forward_states(big)
        assert torch.equal(p1[37:37 + 64], p0) and torch.equal(v1[37:37 + 64], v0), conv
        for i in (0, 13, 63):
            p2, v2 = fe.forward_states(mine[i:i + 1])
            assert torch.equal(p2[0], p0[i]) and torch.equal(v2[0], v0[i]), (conv, i)


def test_dataflow_tower_equals_per_conv_launches(gpu):
    """The tower as one persistent dataflow launch (uttt_nn_tower_wino3h_dev, round 6) gives the same
    output bits as the 32 per-conv launches, for batch sizes across the 7-board group residues, a last group
    of one set, and the engine's full 4,096; repeated launches alternate the two counter blocks (each launch
    resets the block the next one uses) and leave max row 0 zero for the next forward."""
    import torch
    from uttt_amd.model import calibrated_network
    from uttt_amd.nnfast import FusedNetworkEvaluator
    r = golden("rules.npz")
    rng = np.random.RandomState(17)
    pool = _rules_states(rng.choice(np.nonzero(r["n_legal"] > 0)[0], 4096, replace=True))
    net = calibrated_network(NETCAL, "cuda")
    fl = FusedNetworkEvaluator(net, None, max_batch=4096, tower="layers")
    fd = FusedNetworkEvaluator(net, None, max_batch=4096, tower="dataflow")
    for n in (29, 31, 35, 64, 200, 1373, 4096):
        p0, v0 = (t.clone() for t in fl.forward_states(pool[:n]))
        a0 = fl.buf[0][:n].clone()
        for rep in range(2):
            p1, v1 = fd.forward_states(pool[:n])
            assert torch.equal(fd.buf[0][:n], a0), (n, rep)
            assert torch.equal(p1, p0) and torch.equal(v1, v0), (n, rep)
            torch.cuda.synchronize()
            half = fd.ctl.numel() // 2  # the block the next launch uses was reset by this one
            assert int(fd.ctl[fd.ctl_parity * half:(fd.ctl_parity + 1) * half].abs().sum()) == 0, (n, rep)
            assert int(fd.bamax[0].abs().sum()) == 0, (n, rep)


def test_split_f16_conv_is_batch_independent(gpu):
    """Conv-level form of the same property: 64 boards convolved alone and inside a batch
    whose other boards are x1e3 / x1e-3 outliers give equal output bits (the V scale is per
    board; a batch-wide scale would push these boards' low halves into f16 subnormals)."""
    import torch
    from uttt_amd.model import fold_bn, random_network
    from uttt_amd.nnfast import conv3x3_wino3h, wino3h_weights
    net = random_network(3)
    w, b = fold_bn(net.residual_blocks[4].conv2, net.residual_blocks[4].bn2)
    u, su = wino3h_weights(w)
    u, b = u.cuda(), b.cuda()
    g = torch.Generator().manual_seed(4)
    x = torch.relu(torch.randn(64, 81, 128, generator=g)).cuda()
    r = torch.randn(64, 81, 128, generator=g).cuda()
    y0 = conv3x3_wino3h(x, u, su, b, r)
    big = torch.relu(torch.randn(200, 81, 128, generator=g)).cuda()
    big[5] *= 1e3
    big[150] *= 1e-3
    rbig = torch.randn(200, 81, 128, generator=g).cuda()
    for off in (0, 3, 101, 136):
        xb, rb = big.clone(), rbig.clone()
        xb[off:off + 64], rb[off:off + 64] = x, r
        xb[(off + 70) % 200] *= 1e3
        yb = conv3x3_wino3h(xb, u, su, b, rb)
        assert torch.equal(yb[off:off + 64], y0), off


def test_conv_channel_split_kernel_gives_the_same_bits(gpu):
    """Small batches run the tower conv as k_wino3s_conv (the 128 output channels split over 2
    workgroups per set, the transform only over slots that hold a tile): it gives output and per-board
    max bits equal to the persistent kernel's, for batch sizes covering partial groups of 7 and partial
    sets, plain and residual forms (and so does the automatic choice)."""
    import torch
    from uttt_amd.model import fold_bn, random_network
    from uttt_amd.nnfast import conv3x3_wino3h, set_conv_split, wino3h_weights
    net = random_network(5)
    w, b = fold_bn(net.residual_blocks[2].conv1, net.residual_blocks[2].bn1)
    u, su = wino3h_weights(w)
    u, b = u.cuda(), b.cuda()
    g = torch.Generator().manual_seed(9)
    try:
        for n in (1, 2, 3, 4, 5, 7, 8, 11, 14, 25, 50, 71):
            x = torch.relu(torch.randn(n, 81, 128, generator=g)).cuda()
            x[n // 2] *= 1e3
            r = torch.randn(n, 81, 128, generator=g).cuda()
            for res in (None, r):
                set_conv_split(1)
                ya0 = torch.zeros(n, dtype=torch.int32, device="cuda")
                y0 = conv3x3_wino3h(x, u, su, b, res, y_amax=ya0)
                for split in (2, -1):
                    set_conv_split(split)
                    ya = torch.zeros(n, dtype=torch.int32, device="cuda")
                    y = conv3x3_wino3h(x, u, su, b, res, y_amax=ya)
                    assert torch.equal(y, y0) and torch.equal(ya, ya0), (n, split, res is None)
    finally:
        set_conv_split(-1)


# ---------------------------------------------------------------- arena path --
def test_py_semantics_search_matches_reference_pv_mcts(gpu):
    """UTTT_SEMANTICS_PY on the engine == the reference's pv_mcts.pv_mcts_scores
    (tests/golden/pvpy.npz): 42 positions x 7 (S, B) x 3 temperatures, all searched
    together per configuration, float64 score bits; ZeroDivisionError where the
    reference raises it (S <= B)."""
    from uttt_amd.arena import PvMcts, scores_from_visits
    import uttt_cpp
    d = golden("pvpy.npz")
    npos = len(d["pos_active"])
    states = [uttt_cpp.State(d["pos_pieces"][i].reshape(9, 9).tolist(), d["pos_enemy"][i].reshape(9, 9).tolist(),
                             d["pos_main_p"][i].tolist(), d["pos_main_e"][i].tolist(), int(d["pos_active"][i]))
              for i in range(npos)]
    pm = PvMcts(npos, 64)
    ev = gpu.HashEvaluator(pm.engine)
    cfgs = sorted(set(zip(d["sims"].tolist(), d["batch"].tolist())))
    for S, B in cfgs:
        visits = pm.visits(states, ev, S, B)
        for r in np.nonzero((d["sims"] == S) & (d["batch"] == B))[0]:
            v = visits[int(d["pos"][r])]
            n = int(d["n"][r])
            if n < 0:
                with pytest.raises(ZeroDivisionError):
                    scores_from_visits(v, float(d["temp"][r]))
                continue
            sc = np.asarray(scores_from_visits(v, float(d["temp"][r])), np.float64)
            assert sc.size == n, (S, B, r)
            assert np.array_equal(sc.view(np.uint64), d["scores"][r, :n].view(np.uint64)), (S, B, r)


def test_py_semantics_random_positions_match_oracle(gpu, oracle_lib):
    """Fresh random positions at several (S, B), engine vs the pinned oracle restatement."""
    from uttt_amd.arena import PvMcts
    core = oracle_lib
    roots, ostates = _random_positions(core, 200, seed=29)
    pm = PvMcts(len(roots), 200)
    ev = gpu.HashEvaluator(pm.engine)
    for S, B in [(50, 8), (200, 4), (33, 5), (50, 1)]:
        visits = pm.visits(roots, ev, S, B)
        for i in range(0, len(ostates), 3):
            _, vi, _ = core.pv_mcts_scores_py_hash(ostates[i], 1.0, S, B)
            assert np.array_equal(visits[i], vi), (S, B, i)


def test_arena_matches_reference_games(gpu):
    """uttt_amd.arena.evaluate_network with the two salted hash players of the fixture:
    every game's moves and first-player point equal the reference's evaluate_network
    play() after np.random.seed(seed + g); model0's average point follows."""
    from oracle.hashnp import make_hash_model
    from uttt_amd import arena
    d = golden("pvpy.npz")
    s0, s1 = (int(x) for x in d["arena_salts"])
    ng = len(d["arena_lengths"])
    avg, points, actions = arena.evaluate_network(make_hash_model(s0), make_hash_model(s1), ng, 1.0,
                                                  int(d["arena_seeds"][0]))
    off = 0
    for g in range(ng):
        n = int(d["arena_lengths"][g])
        assert actions[g] == d["arena_actions"][off:off + n].astype(int).tolist(), g
        assert points[g] == d["arena_points"][g], g
        off += n
    want = sum(p if g % 2 == 0 else 1 - p for g, p in enumerate(d["arena_points"].tolist())) / ng
    assert avg == want


def test_python_self_play_matches_reference(gpu):
    """arena.self_play_py (self_play.py, BASELINE configs[0], all games concurrent) ==
    the reference's self_play.play after np.random.seed(seed + g): inputs, float64
    policy bits, values; and the drop-in self_play.play on the global RNG for one game."""
    from oracle.hashnp import make_hash_model
    from uttt_amd import arena
    d = golden("pvpy.npz")
    ng = len(d["sp_lengths"])
    games = arena.self_play_py(make_hash_model(0), ng, int(d["sp_seeds"][0]))
    off = 0
    for g in range(ng):
        n = int(d["sp_lengths"][g])
        sl = slice(off, off + n)
        h = games[g]
        assert len(h) == n, g
        assert all(r[0].dtype == np.float64 for r in h)
        assert np.array_equal(np.asarray([r[0].reshape(243) for r in h]).astype(np.uint8), d["sp_tensors"][sl]), g
        assert np.array_equal(np.asarray([r[1] for r in h], np.float64).view(np.uint64),
                              d["sp_policies"][sl].view(np.uint64)), g
        assert [r[2] for r in h] == d["sp_values"][sl].astype(int).tolist(), g
        off += n
    import self_play
    np.random.seed(int(d["sp_seeds"][1]))
    h = self_play.play(make_hash_model(0))
    n0, n1 = int(d["sp_lengths"][0]), int(d["sp_lengths"][1])
    assert [r[2] for r in h] == d["sp_values"][n0:n0 + n1].astype(int).tolist()
    assert np.array_equal(np.asarray([r[1] for r in h], np.float64).view(np.uint64),
                          d["sp_policies"][n0:n0 + n1].view(np.uint64))


def test_train_network_runs_on_gpu(gpu):
    """uttt_amd.train on the GPU (one process): finite, decreasing loss on a learnable
    synthetic history; the saved state dict loads back into DualNetwork."""
    import torch
    from uttt_amd import train
    from uttt_amd.model import DualNetwork, random_network
    rng = np.random.RandomState(0)
    xs = (rng.rand(256, 9, 9, 3) < 0.3).astype(np.float64)
    pol = np.zeros((256, 81))
    pol[np.arange(256), rng.randint(0, 81, 256)] = 1.0
    hist = [[xs[i], pol[i], int(i % 3) - 1] for i in range(256)]
    model = random_network(0)
    losses = train.train_network(model, hist, epochs=6, batch_size=64, device=torch.device("cuda", 0), log=None)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    DualNetwork().load_state_dict(model.state_dict())


def test_f16_mode_conv_error_and_batch_independence(gpu):
    """The conv's optional f16 mode (uttt_nn_conv3x3_wino3h_f16: M = Vhi Uhi, one f16 MFMA product per point,
    SURVEY §8(f) rank 1's fast evaluator) against an f64 direct conv: within 5e-3 of each board's output scale
    (measured 1.7e-3 .. 3.8e-3, tools/diag/f16_mode_check.py; the product's split-f16 form: 1-2e-6), the
    per-board max row exact, different from the product's bits, and a board's outputs independent of the
    batch it is in."""
    import torch
    import torch.nn.functional as F
    from uttt_amd.model import fold_bn, random_network
    from uttt_amd.nnfast import conv3x3_wino3h, wino3h_weights
    net = random_network(3)
    g = torch.Generator().manual_seed(4)
    for blk_i, n, scale in ((5, 1, 1.0), (3, 9, 1e-3), (15, 30, 1e3), (9, 700, 1.0)):
        w, b = fold_bn(net.residual_blocks[blk_i].conv1, net.residual_blocks[blk_i].bn1)
        u, su = wino3h_weights(w)
        u, w, b = u.cuda(), w.cuda(), b.cuda()
        x = (torch.relu(torch.randn(n, 81, 128, generator=g)) * scale).cuda()
        r = (torch.randn(n, 81, 128, generator=g) * scale).cuda()
        ref = F.conv2d(x.reshape(n, 9, 9, 128).permute(0, 3, 1, 2).double(), w.double(), b.double(),
                       padding=1).permute(0, 2, 3, 1).reshape(n, 81, 128)
        for res in (None, r):
            ya = torch.zeros(n, dtype=torch.int32, device="cuda")
            y = conv3x3_wino3h(x, u, su, b, res, y_amax=ya, precision="f16")
            want = torch.relu(ref + (res.double() if res is not None else 0)).float()
            err = (y - want).abs().reshape(n, -1).amax(dim=1) / want.abs().reshape(n, -1).amax(dim=1).clamp_min(1e-30)
            assert err.max().item() <= 5e-3, (blk_i, n, res is None, err.max().item())
            assert torch.equal(ya.view(torch.float32), y.reshape(n, -1).amax(dim=1))
            assert not torch.equal(y, conv3x3_wino3h(x, u, su, b, res))  # it is not the product's form
            k = min(n, 5)
            yk = conv3x3_wino3h(x[:k].contiguous(), u, su, b, res[:k].contiguous() if res is not None else None,
                                precision="f16")
            assert torch.equal(y[:k], yk)


def test_f16_mode_evaluator_and_search(gpu, oracle_lib):
    """FusedNetworkEvaluator(precision="f16") on search leaves: the calibrated net's value and post-softmax
    policy within 3e-2 of the fp32 DualNetwork (measured 1.6e-2 / 1.4e-2 on 400 positions), and a self-play
    move through it completes with legal, normalised scores. The f32-level evaluator stays the default; the
    f16 mode is opt-in (precision="f16" or UTTT_NN_PRECISION=f16)."""
    import torch
    from uttt_amd.model import calibrated_network, policy_logits
    from uttt_amd.nnfast import FusedNetworkEvaluator
    roots, _ = _random_positions(oracle_lib, 200, seed=21)
    bs = gpu.BatchedSearch(len(roots), 50)
    e = bs.engine
    e.use_stream()
    net, cpu = calibrated_network(NETCAL, "cuda"), calibrated_network(NETCAL, "cpu")
    fused = FusedNetworkEvaluator(net, e, precision="f16")
    assert FusedNetworkEvaluator(net, e).precision == "f32"
    e.search_begin(roots, 50, 8)
    for _ in range(3):
        n = e.select(bs.x)
        p, v = fused.forward(n, softmax=True)
        z_cpu, v_cpu = policy_logits(cpu, bs.x[:n].cpu())
        assert (v.cpu() - v_cpu.reshape(-1)).abs().max().item() <= 3e-2
        assert (p.cpu() - torch.softmax(z_cpu, dim=1)).abs().max().item() <= 3e-2
        assert torch.allclose(p.sum(dim=1).cpu(), torch.ones(n), atol=1e-5)
        e.apply(p, v)
    sp = gpu.SelfPlay(64, 50, 8, 1.0)
    sp.set_evaluator(lambda eng: FusedNetworkEvaluator(net, eng, precision="f16"))
    sp.run(0, 8, 11)
    plies = gpu.history_from_records(sp.records())
    assert len(plies) > 0
    for x, pol, val in plies:
        assert abs(sum(pol) - 1.0) < 1e-6 and val in (-1, 0, 1)
