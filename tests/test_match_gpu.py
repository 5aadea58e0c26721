"""Match play on the GPU (k_match_move, k_match_lists, csrc/engine/match.h), hash evaluators on both
sides: player 0 searches 24 simulations in flushes of 4, player 1 48 in flushes of 8. The device match against
arena._play_games at temperature 0, against a host-driven replica (PvMcts.visits on host states and
uttt_match_move_host) with sampled plies and an opening book, independence of where a game sits among the others,
the pairing, and the refusals."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIMS = (24, 48)
BATCH = (4, 8)
SEED = 20260317
SAMPLE = 6


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import uttt_amd
    return uttt_amd


def players(gpu, semantics="py"):
    from uttt_amd import match
    return [match.Player(gpu.HashEvaluator, SIMS[m], BATCH[m], semantics) for m in (0, 1)]


@pytest.fixture(scope="module")
def book(gpu):
    """34 openings of 3 plies: after an odd number of plies the side to move is not the reference's first player."""
    from uttt_amd import match
    return match.random_openings(34, 3, SEED)


def per_game(book, games):
    """The opening list of an unpaired match that starts game g where the paired one does."""
    return book[np.arange(games) // 2]


class HostSearch:
    """arena.PvMcts with a player's own batch size and semantics: what arena._play_games calls per move."""

    def __init__(self, gpu, games, m, semantics):
        self.search = gpu.BatchedSearch(games, SIMS[m])
        self.engine = self.search.engine
        self.m, self.semantics = m, semantics

    def visits(self, states, evaluator, evaluate_count=50, batch_size=8):
        roots = gpu_states(states)
        self.search.run(roots, evaluator, SIMS[self.m], BATCH[self.m], semantics=self.semantics)
        v, L = self.search.visits()
        return [v[i, :L[i]].copy() for i in range(len(roots))]


def gpu_states(states):
    import uttt_amd
    return states if isinstance(states, np.ndarray) else uttt_amd.as_states(states)


def replica(gpu, openings, games, paired, sample_plies, seed):
    """The match driven from the host: per iteration the lists as k_match_lists builds them, per player one
    PvMcts.visits over its games' states, per game uttt_match_move_host. Returns (actions, plies, results,
    counters per iteration)."""
    from uttt_amd import match
    searches = [HostSearch(gpu, games, m, "py") for m in (0, 1)]
    evs = [gpu.HashEvaluator(s.engine) for s in searches]
    states = openings[np.arange(games) // 2 if paired else np.arange(games)].copy()
    plies = np.zeros(games, np.int32)
    results = np.full(games, -1, np.int8)
    actions = [[] for _ in range(games)]
    counters = []
    while True:
        live = [g for g in range(games) if results[g] < 0]
        lists = [[g for g in live if (g + plies[g]) % 2 == m] for m in (0, 1)]
        done = results[results >= 0]
        counters.append((len(lists[0]), len(lists[1]), len(done), int(done.sum()), int((done == 1).sum())))
        if not live:
            break
        for m in (0, 1):
            if not lists[m]:
                continue
            vis = searches[m].visits(states[lists[m]], evs[m])
            for g, v in zip(lists[m], vis):
                nxt, a, r = match.match_move_host(states[g:g + 1], v, int(plies[g]), g, seed, sample_plies)
                states[g] = nxt[0]
                actions[g].append(a)
                plies[g] += 1
                results[g] = r
    return actions, plies, results, counters


@pytest.fixture(scope="module")
def unpaired67(gpu, book):
    from uttt_amd import match
    return match.play_match(*players(gpu), 67, per_game(book, 67), paired=False, sample_plies=SAMPLE, seed=SEED)


@pytest.mark.parametrize("semantics", ["py", "cpp"])
def test_equals_the_arena(gpu, semantics):
    """10 games from the initial position, every move the most visited one: the games arena._play_games plays at
    temperature 0 with the same two players. Crosses 81-move roots, games of different lengths and iterations in
    which one player's list is empty (ply 0: every even game is player 0's, no game player 1's)."""
    from uttt_amd import arena, match
    games = 10
    res = match.play_match(*players(gpu, semantics), games, openings=None, paired=False, sample_plies=0)
    searches = [HostSearch(gpu, games, m, semantics) for m in (0, 1)]
    evs = [gpu.HashEvaluator(s.engine) for s in searches]
    avg, points, actions = arena._play_games(searches, evs, SIMS, games, 0, 0, 8, None)
    assert res.actions == actions
    mine = [p if g % 2 == 0 else 1 - p for g, p in enumerate(points)]
    assert res.points.tolist() == mine and abs(res.points.mean() - avg) < 1e-12
    assert res.counters[0] == (5, 5, 0, 0, 0) and res.counters[-1][:3] == (0, 0, games)
    assert len(set(res.plies.tolist())) > 1 and res.plies.tolist() == [len(a) for a in actions]
    assert any(c[0] == 0 or c[1] == 0 for c in res.counters[:-1])


@pytest.mark.parametrize("games,paired", [(67, False), (66, True)])
def test_equals_a_host_driven_replica(gpu, book, unpaired67, games, paired):
    from uttt_amd import match
    if paired:
        res = match.play_match(*players(gpu), games, book, paired=True, sample_plies=SAMPLE, seed=SEED)
        openings = book
    else:
        res, openings = unpaired67, per_game(book, games)
    actions, plies, results, counters = replica(gpu, openings, games, paired, SAMPLE, SEED)
    assert res.actions == actions
    assert res.plies.tolist() == plies.tolist()
    assert (res.points * 2).tolist() == results.tolist()
    assert res.counters == counters
    assert res.counters[-1][2] == games and res.counters[-1][3] == int(results.sum())
    assert (res.wins, res.draws, res.losses) == tuple(int((results == k).sum()) for k in (2, 1, 0))
    if paired:  # the pair scores are the means over games 2i, 2i + 1
        assert np.array_equal(res.pair_scores, results.reshape(-1, 2).mean(axis=1) / 2.0)


def test_order_independence(gpu, book, unpaired67):
    """The 67 games dealt to other ids through a permuted opening list. A game that keeps its id (and so its first
    mover and its draws) plays the same moves whatever games surround it, although its place in the lists and the
    tree that searches it change as the others end at other plies. With no sampled ply a game is a function of its
    opening and its first mover alone, so there every game that keeps its parity keeps its moves."""
    from uttt_amd import match
    games = 67
    base = per_game(book, games)
    rng = np.random.RandomState(5)
    fixed = np.arange(games) % 3 == 0
    perm = np.arange(games)
    moving = np.nonzero(~fixed)[0]
    perm[moving] = rng.permutation(moving)
    assert (perm != np.arange(games)).sum() > 30
    dealt = base.copy()
    dealt[perm] = base  # game perm[g] starts where game g started
    res = match.play_match(*players(gpu), games, dealt, paired=False, sample_plies=SAMPLE, seed=SEED)
    for g in np.nonzero(fixed)[0]:
        assert res.actions[g] == unpaired67.actions[g], g
        assert res.points[g] == unpaired67.points[g]
    assert any(res.actions[perm[g]] != unpaired67.actions[g] for g in moving)  # the others did change
    # no sampling: every game that lands on an id of its own parity is the same game
    a0 = match.play_match(*players(gpu), games, base, paired=False, sample_plies=0)
    a1 = match.play_match(*players(gpu), games, dealt, paired=False, sample_plies=0)
    assert any(a0.actions[g] != unpaired67.actions[g] for g in range(games))  # and the sampled plies did sample
    same = [g for g in range(games) if perm[g] % 2 == g % 2]
    assert len(same) > 30 and any(perm[g] != g for g in same)
    for g in same:
        assert a1.actions[perm[g]] == a0.actions[g], g
        assert a1.points[perm[g]] == a0.points[g]


def run_search(gpu, match_h, e, ev, x, player, m):
    match_h.search_begin(e, player, SIMS[m], BATCH[m], "py")
    while True:
        n = e.select(x)
        if n == 0:
            break
        p, v = ev(x, n)
        e.apply(p, v)


def test_pairing(gpu, book):
    """Before the first move games 2i and 2i + 1 stand on opening i, and the first movers are opposite: player 0's
    list is the even games, player 1's the odd ones, and after player 0 alone has moved only the even games have."""
    import torch
    from uttt_amd.engine import Match
    games = 66
    mh = Match(games)
    mh.begin(book, games, paired=True, sample_plies=0, seed=0)
    st = mh.state()
    assert st["states"][0::2].tobytes() == book[:33].tobytes() and st["states"][1::2].tobytes() == book[:33].tobytes()
    assert (st["plies"] == 0).all() and (st["results"] == -1).all() and (st["actions"] == -1).all()
    assert mh.counts() == (33, 33, 0, 0, 0)
    e = gpu.Engine(games, SIMS[0])
    ev = gpu.HashEvaluator(e)
    x = torch.zeros((games, 3, 9, 9), dtype=torch.float32, device="cuda")
    run_search(gpu, mh, e, ev, x, 0, 0)
    roots = e.root_visits()
    assert len(roots[0]) == 33
    mh.move(e, 0)
    mh.lists()
    st = mh.state()
    assert (st["plies"][0::2] == 1).all() and (st["plies"][1::2] == 0).all()
    assert (st["actions"][0::2, 0] >= 0).all() and (st["actions"][1::2] == -1).all()
    assert st["states"][1::2].tobytes() == book[:33].tobytes()
    # every game is now player 1's to move: the moved even games and the untouched odd ones
    assert mh.counts()[:3] == (0, 66, 0)
    mh.close()
    e.close()


def test_refusals(gpu, book):
    import torch
    from uttt_amd._lib import EngineError
    from uttt_amd.engine import Match
    games = 4
    mh = Match(games)
    with pytest.raises(ValueError):
        mh.begin(book, 6, paired=True)  # games > max_games
    with pytest.raises(ValueError):
        mh.begin(book, 3, paired=True)  # paired and odd
    with pytest.raises(ValueError):
        mh.begin(book[:1], 4, paired=True)  # two openings needed
    e = gpu.Engine(games, SIMS[0])
    ev = gpu.HashEvaluator(e)
    x = torch.zeros((games, 3, 9, 9), dtype=torch.float32, device="cuda")
    with pytest.raises(EngineError, match="UTTT_ERR_ORDER"):
        mh.counts()  # no match has begun
    mh.begin(book, games, paired=True)
    with pytest.raises(EngineError, match="UTTT_ERR_ORDER"):
        mh.search_begin(e, 0, SIMS[0], BATCH[0])  # the lists' counters were never read
    assert mh.counts() == (2, 2, 0, 0, 0)
    e.set_root_noise(0.25, 0.3, 1)
    with pytest.raises(ValueError, match="root noise"):
        mh.search_begin(e, 0, SIMS[0], BATCH[0], "cpp")
    e.set_root_noise(0.0)
    e.set_tree_reuse(True)
    with pytest.raises(ValueError, match="tree reuse"):
        mh.search_begin(e, 0, SIMS[0], BATCH[0], "cpp")
    e.set_tree_reuse(False)
    with pytest.raises(EngineError, match="UTTT_ERR_ORDER"):
        mh.move(e, 0)  # no search begun
    e.use_stream(e.own_stream())
    with pytest.raises(ValueError, match="stream"):
        mh.search_begin(e, 0, SIMS[0], BATCH[0])
    e.use_stream()
    run_search(gpu, mh, e, ev, x, 0, 0)
    mh.move(e, 0)
    with pytest.raises(EngineError, match="UTTT_ERR_ORDER"):
        mh.move(e, 0)  # a second move without lists
    with pytest.raises(EngineError, match="UTTT_ERR_ORDER"):
        mh.search_begin(e, 0, SIMS[0], BATCH[0])  # player 0's list is stale
    mh.lists()
    assert mh.counts()[:3] == (0, 4, 0)
    with pytest.raises(ValueError, match="no live game"):
        mh.search_begin(e, 0, SIMS[0], BATCH[0])  # an empty list
    st = mh.state()
    assert st["plies"].tolist() == [1, 0, 1, 0]
    mh.close()
    e.close()
