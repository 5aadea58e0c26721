"""Tree reuse on the CPU: the Python model of the search (tests/tree_reuse_model.py) anchored to the
oracle, uttt_reroot_host (csrc/uttt_reroot.h) against the model's own re-root record for record, the node pool's
bound over whole games, and the leaves a game saves. No GPU."""
import numpy as np
import pytest

import tree_reuse_model as M
import wide_deep
from conftest import golden

FIXTURE_ROWS = (20, 35)  # two mid-game positions of tests/golden/rules.npz (plies 20 and 35 of its first game)
GAME_SEEDS = (1, 4, 5)   # picked on the model alone: each game evaluates fewer leaves with reuse on


def fixture_state(core, i):
    r = golden("rules.npz")
    s = core.OrState.from_arrays(r["pieces"][i], r["enemy"][i], r["main_p"][i], r["main_e"][i], int(r["active"][i]))
    assert not s.is_done()
    return s


def records(tree):
    from uttt_amd import reuse
    return reuse.pack(tree.as_array() if isinstance(tree, M.Tree) else tree).tobytes()


# ------------------------------------------------------------------ 1 --
def test_model_without_reuse_is_the_oracle(oracle_lib, engine_lib):
    """The golden (S, B) rows small enough for a Python search, on every golden position: visits and scores."""
    core = oracle_lib
    d = golden("search.npz")
    pos = [core.OrState.from_arrays(d["pos_pieces"][i], d["pos_enemy"][i], d["pos_main_p"][i], d["pos_main_e"][i],
                                    int(d["pos_active"][i])) for i in range(len(d["pos_active"]))]
    configs = sorted({(int(s), int(b)) for s, b in zip(d["sims"], d["batch"]) if s <= 64})
    assert configs
    checked = 0
    trees = {}
    for r in range(len(d["n"])):
        S, B, tau, pi, n = int(d["sims"][r]), int(d["batch"][r]), float(d["temp"][r]), int(d["pos"][r]), int(d["n"][r])
        if (S, B) not in configs:
            continue
        if (S, B, pi) not in trees:
            trees[S, B, pi] = M.Tree(pos[pi]).search(S, B)
            _, vi, st = core.pv_mcts_scores_hash(pos[pi], 1.0, S, B)
            assert np.array_equal(trees[S, B, pi].visits(), vi), (S, B, pi)
            assert trees[S, B, pi].evals == st.flushes, (S, B, pi)
        sc = trees[S, B, pi].scores(tau)
        assert len(sc) == n and np.array_equal(sc.view(np.uint32), d["scores"][r][:n].view(np.uint32)), (S, B, tau, pi)
        checked += 1
    assert checked >= 3 * len(pos)


# ------------------------------------------------------------------ 2 --
def searched(core, which, S, B):
    s = core.OrState.initial() if which == "initial" else fixture_state(core, which)
    return s, M.Tree(s).search(S, B)


@pytest.mark.parametrize("which", ("initial",) + FIXTURE_ROWS)
@pytest.mark.parametrize("S,B", [(16, 1), (16, 4), (50, 8)])
def test_reroot_host_equals_the_model(oracle_lib, engine_lib, which, S, B):
    from uttt_amd import reuse
    s, t = searched(oracle_lib, which, S, B)
    packed = wide_deep.pack_states([s])
    legal, vis = t.legal(), t.visits()
    for a in legal:  # every move of the root: promoted children of every k, unexpanded and terminal ones
        want = t.reroot(a)
        got = reuse.reroot_host(t.as_array(), packed, a)
        assert len(got) == len(want.nodes), (a, len(got), len(want.nodes))
        assert records(got) == records(want), a
        c = t.nodes[1 + legal.index(a)]
        if c[M.K]:
            assert got[0]["N"] == c[M.N] - c[M.K] == got["N"][1:1 + got[0]["L"]].sum() == want.done
        else:
            assert len(got) == 1 + len(s.next(a).legal_actions()) and want.done == 0
    assert int(vis.sum()) == S


def test_reroot_host_covers_the_named_cases(oracle_lib, engine_lib):
    """A promoted child with k = 1 and with k = 4, an unexpanded promoted child, and a level-1 duplicate that was
    never expanded beside an expanded one: each is present in the trees the test above walks."""
    core = oracle_lib
    for B in (1, 4):
        s, t = searched(core, "initial", 16, B)
        legal, vis = t.legal(), t.visits()
        top = t.nodes[1 + int(np.argmax(vis))]
        assert top[M.K] == B and top[M.LL] == len(s.next(top[M.ACT]).legal_actions())
        cold = t.nodes[1 + int(np.argmin(vis))]
        assert cold[M.N] == 0 and cold[M.K] == 0
        fresh = t.reroot(cold[M.ACT])
        assert records(fresh) == records(M.Tree(s.next(cold[M.ACT])))
        if B == 4:
            Lp = top[M.LL]
            mixed = 0
            for r in range(Lp):
                ks = [t.nodes[top[M.FIRST] + i * Lp + r][M.K] for i in range(4)]
                mixed += any(ks) and not all(ks)
            assert mixed > 0
            kept = t.reroot(top[M.ACT])
            assert kept.done == top[M.N] - 4 > 0 and kept.nodes[0][M.LL] == Lp


def test_reroot_host_refuses_what_is_not_a_move(oracle_lib, engine_lib):
    from uttt_amd import reuse
    s = fixture_state(oracle_lib, FIXTURE_ROWS[0])
    t = M.Tree(s).search(16, 4)
    illegal = next(a for a in range(81) if a not in t.legal())
    for a in (-1, 81, illegal):
        with pytest.raises(ValueError):
            reuse.reroot_host(t.as_array(), wide_deep.pack_states([s]), a)


# ------------------------------------------------------------------ 3 --
@pytest.fixture(scope="module")
def games(oracle_lib, engine_lib):
    out = {}
    for seed in GAME_SEEDS:
        on, off = [], []
        out[seed] = (M.play_game(seed, 16, 4, reuse=True, trace=on), on, M.play_game(seed, 16, 4, reuse=False, trace=off), off)
    return out


def test_node_count_stays_within_the_pool(games):
    S = 16
    for seed, (_, trace, _, _) in games.items():
        assert trace and all(nodes <= 82 + 81 * S for _, _, nodes in trace), seed
        assert all(0 <= carried <= S - 1 for carried, _, _ in trace), seed
        assert any(carried > 0 for carried, _, _ in trace), seed


def test_reuse_evaluates_fewer_leaves(games, oracle_lib):
    for seed, (on, on_trace, off, off_trace) in games.items():
        assert on["evals"] < off["evals"], (seed, on["evals"], off["evals"])
        assert on["evals"] / len(on_trace) < off["evals"] / len(off_trace), seed
        # reuse off is the oracle's game
        ref = oracle_lib.self_play_game_hash(seed, 1.0, 16, 4)
        assert np.array_equal(off["actions"], ref["actions"].astype(np.int64)), seed
        assert np.array_equal(off["policies"].view(np.uint64), ref["policies"].view(np.uint64)), seed
        assert np.array_equal(off["values"], ref["values"].astype(np.int64)), seed
