"""Match play on the CPU (csrc/uttt_match.h through uttt_match_move_host / uttt_match_draw_host / uttt_match_check_host,
uttt_amd/match.py): the move rule against a model written here from the rules ABI, the draw, the
opening book, uttt_match_begin's argument errors and the statistics on hand values. No GPU."""
import ctypes
import math

import numpy as np
import pytest

SEED = 20260317  # the committed seed of the sampled cases


@pytest.fixture(scope="module")
def mt(engine_lib):
    from uttt_amd import match
    return match


def _c(st):
    from uttt_amd._lib import UtttState
    return st.ctypes.data_as(ctypes.POINTER(UtttState))


def legal_of(lib, st):
    buf = (ctypes.c_int32 * 81)()
    n = lib.uttt_state_legal_actions(_c(st), buf)
    return [int(buf[i]) for i in range(n)]


def next_of(lib, st, a):
    from uttt_amd._lib import STATE_DTYPE
    out = np.zeros(1, STATE_DTYPE)
    assert lib.uttt_state_next(_c(st), int(a), _c(out)) == 0
    return out


def model_move(lib, mt, st, N, ply, game, seed, sample_plies):
    """The issue's move rule, from uttt_state_legal_actions / _next / _is_lose / _is_done and Python integers."""
    legal = legal_of(lib, st)
    N = [int(v) for v in N]
    assert len(N) == len(legal)
    T = sum(N)
    if ply >= sample_plies or T == 0:
        i = N.index(max(N))
    else:
        x = (mt.match_draw(seed, game, ply) * T) >> 64
        acc, i = 0, None
        for j, v in enumerate(N):
            acc += v
            if acc > x:
                i = j
                break
    a = legal[i]
    nxt = next_of(lib, st, a)
    mover = (game + ply) % 2
    if lib.uttt_state_is_lose(_c(nxt)):
        res = 2 if mover == 0 else 0
    elif lib.uttt_state_is_done(_c(nxt)):
        res = 1
    else:
        res = -1
    return nxt, a, res


@pytest.fixture(scope="module")
def positions(engine_lib):
    """Positions of random games by what the move rule meets there: {"L1", "L2", "L3": a state with that many legal
    moves, "win": (state, rank of a move that wins), "draw": (state, rank of a move that fills the board to a draw),
    "wide": a free-move state with more than 64 moves}, and the initial state under "L81"."""
    import uttt_amd
    lib = engine_lib
    rng = np.random.RandomState(7)
    found = {"L81": uttt_amd.initial_states(1)}
    want = {"L1", "L2", "L3", "win", "draw", "wide"}
    for _ in range(3000):
        st = uttt_amd.initial_states(1)
        ply = 0
        while True:
            legal = legal_of(lib, st)
            if not legal:
                break
            L = len(legal)
            if L <= 3 and f"L{L}" not in found:
                found[f"L{L}"] = st
            if L > 64 and ply > 0 and "wide" not in found:
                found["wide"] = st
            if ply > 16 and not ("win" in found and "draw" in found):
                for r, a in enumerate(legal):
                    nx = next_of(lib, st, a)
                    if lib.uttt_state_is_lose(_c(nx)):
                        found.setdefault("win", (st, r))
                    elif lib.uttt_state_is_done(_c(nx)):
                        found.setdefault("draw", (st, r))
            st = next_of(lib, st, legal[rng.randint(L)])
            ply += 1
            if lib.uttt_state_is_lose(_c(st)):
                break
        if want <= set(found):
            break
    assert want <= set(found), sorted(want - set(found))
    return found


def both(lib, mt, st, N, ply, game, seed, sample_plies):
    got = mt.match_move_host(st, N, ply, game, seed, sample_plies)
    exp = model_move(lib, mt, st, N, ply, game, seed, sample_plies)
    assert got[0].tobytes() == exp[0].tobytes() and got[1:] == exp[1:], (N, ply, game, seed, sample_plies, got[1:], exp[1:])
    return got


def test_first_max_with_ties(engine_lib, mt, positions):
    lib = engine_lib
    st = positions["L81"]
    legal = legal_of(lib, st)
    assert len(legal) == 81
    for N, want in (([0] * 81, 0), ([3] * 81, 0), ([1] * 40 + [5, 5] + [1] * 39, 40), ([0] * 80 + [1], 80),
                    ([2] * 64 + [7] + [7] * 16, 64), ([9] + [0] * 79 + [9], 0)):
        _, a, res = both(lib, mt, st, N, 0, 0, SEED, 0)
        assert a == legal[want] and res == -1
    # a sampled ply with no visit at all falls back to the first maximum
    _, a, _ = both(lib, mt, st, [0] * 81, 0, 5, SEED, 81)
    assert a == legal[0]
    st3 = positions["L3"]
    for N, want in (([4, 4, 1], 0), ([1, 4, 4], 1), ([0, 0, 0], 0), ([1, 2, 3], 2)):
        assert both(lib, mt, st3, N, 30, 1, SEED, 6)[1] == legal_of(lib, st3)[want]


def test_sampled_index_on_the_boundaries(engine_lib, mt, positions):
    """N = [1, 0, 3], T = 4: x = 0 takes index 0, x = 1, 2, 3 take index 2 (the empty entry 1 is never chosen, since
    its prefix sum does not pass x = 1). Every x is reached by searching seeds."""
    lib = engine_lib
    st = positions["L3"]
    legal = legal_of(lib, st)
    seen = {}
    for seed in range(200):
        x = (mt.match_draw(seed, 11, 2) * 4) >> 64
        if x in seen:
            continue
        seen[x] = seed
        _, a, _ = both(lib, mt, st, [1, 0, 3], 2, 11, seed, 6)
        assert a == legal[0 if x == 0 else 2], (x, seed)
        if len(seen) == 4:
            break
    assert sorted(seen) == [0, 1, 2, 3]
    # at ply == sample_plies the same row is no longer sampled
    assert both(lib, mt, st, [1, 0, 3], 6, 11, seen[0], 6)[1] == legal[2]


def test_one_move_and_eighty_one(engine_lib, mt, positions):
    lib = engine_lib
    st1 = positions["L1"]
    for sample in (0, 81):
        assert both(lib, mt, st1, [17], 40, 3, SEED, sample)[1] == legal_of(lib, st1)[0]
    rng = np.random.RandomState(3)
    for key in ("L81", "wide"):
        st = positions[key]
        L = len(legal_of(lib, st))
        assert L > 64
        hit_high = 0
        for game in range(40):
            N = rng.randint(0, 4, L)
            N[rng.randint(64, L)] += 6  # weight beyond entry 63, which one lane per move could not hold
            _, a, _ = both(lib, mt, st, N, 1, game, SEED, 8)
            hit_high += legal_of(lib, st).index(a) >= 64
            both(lib, mt, st, N, 9, game, SEED, 8)
        assert hit_high > 0


def test_winning_and_drawing_moves(engine_lib, mt, positions):
    lib = engine_lib
    for key, per_mover in (("win", {0: 2, 1: 0}), ("draw", {0: 1, 1: 1})):
        st, r = positions[key]
        L = len(legal_of(lib, st))
        N = [1] * L
        N[r] = 9
        for game, ply in ((0, 40), (1, 40), (0, 41), (1, 41)):
            nxt, a, res = both(lib, mt, st, N, ply, game, SEED, 0)
            assert res == per_mover[(game + ply) % 2]
            assert lib.uttt_state_is_done(_c(nxt))


def test_move_host_argument_errors(engine_lib, mt, positions):
    st, r = positions["win"]
    L = len(legal_of(engine_lib, st))
    N = [1] * L
    N[r] = 9
    done = mt.match_move_host(st, N, 40, 0)[0]
    with pytest.raises(ValueError):
        mt.match_move_host(done, [1], 41, 0)  # a finished game
    with pytest.raises(ValueError):
        mt.match_move_host(st, N + [1], 40, 0)  # a row of another length
    with pytest.raises(ValueError):
        mt.match_move_host(st, [-1] + N[1:], 40, 0)
    with pytest.raises(ValueError):
        mt.match_move_host(st, N, 81, 0)


def test_the_draw(engine_lib, mt, positions):
    d = mt.match_draw(SEED, 5, 3)
    assert d == mt.match_draw(SEED, 5, 3) and 0 <= d < 1 << 64
    assert len({d, mt.match_draw(SEED + 1, 5, 3), mt.match_draw(SEED, 6, 3), mt.match_draw(SEED, 5, 4)}) == 4
    # (seed, game, ply) are not interchangeable
    assert mt.match_draw(1, 2, 3) != mt.match_draw(2, 1, 3) and mt.match_draw(1, 2, 3) != mt.match_draw(1, 3, 2)
    # N = [1, 3]: index 1 with probability 3/4; 4,096 games, five binomial standard deviations
    st = positions["L2"]
    legal = legal_of(engine_lib, st)
    hits = sum(mt.match_move_host(st, [1, 3], 0, g, SEED, 1)[1] == legal[1] for g in range(4096))
    assert abs(hits / 4096 - 0.75) <= 0.034, hits / 4096
    # the same frequency straight from the draws, as the model computes it
    assert hits == sum(((mt.match_draw(SEED, g, 0) * 4) >> 64) >= 1 for g in range(4096))


def test_random_openings(engine_lib, mt):
    import uttt_amd
    lib = engine_lib
    a = mt.random_openings(34, 3, SEED)
    assert a.tobytes() == mt.random_openings(34, 3, SEED).tobytes()
    assert a.tobytes() != mt.random_openings(34, 3, SEED + 1).tobytes()
    assert a[:10].tobytes() == mt.random_openings(10, 3, SEED).tobytes()  # a prefix: the counter's order
    assert len({a[i:i + 1].tobytes() for i in range(34)}) == 34
    for plies in (1, 3, 4, 9):
        b = mt.random_openings(12, plies, SEED)
        assert len({b[i:i + 1].tobytes() for i in range(12)}) == 12
        for i in range(12):
            s = b[i:i + 1]
            stones = sum(bin(int(w)).count("1") for w in list(s["own"][0]) + list(s["opp"][0]))
            assert stones == plies and not lib.uttt_state_is_done(_c(s))
    one = mt.random_openings(1, 0, SEED)
    assert one.tobytes() == uttt_amd.initial_states(1).tobytes()
    with pytest.raises(ValueError):
        mt.random_openings(2, 0, SEED)  # there is one position at ply 0
    with pytest.raises(ValueError):
        mt.random_openings(0, 3, SEED)
    # every first move is reached: the draw's scaling covers 0..80
    first = mt.random_openings(81, 1, SEED)
    assert len({first[i:i + 1].tobytes() for i in range(81)}) == 81


def test_match_begin_argument_errors(engine_lib, mt, positions):
    import uttt_amd
    lib = engine_lib
    op = mt.random_openings(8, 3, SEED)
    mt.check_openings(op, 16, 16, True)
    mt.check_openings(op, 8, 16, False)
    mt.check_openings(op, 2, 2, True)
    st, r = positions["win"]
    L = len(legal_of(lib, st))
    N = [1] * L
    N[r] = 9
    done = mt.match_move_host(st, N, 40, 0)[0]
    bad = op.copy()
    bad[3] = done[0]
    for args, word in (((bad, 16, 16, True), b"finished"),   # a terminal opening
                       ((op, 17, 16, False), b"max_games"),  # games > max_games
                       ((op, 0, 16, True), b"max_games"),
                       ((op, 7, 16, True), b"odd"),          # paired with an odd games
                       ((op, 18, 32, True), b"openings"),    # 9 openings needed, 8 given
                       ((op, 9, 32, False), b"openings")):
        with pytest.raises(ValueError):
            mt.check_openings(*args)
        assert word in lib.uttt_last_error(), (args[1:], lib.uttt_last_error())
    # a terminal opening past the ones the games use is not looked at
    mt.check_openings(bad, 6, 16, True)
    assert lib.uttt_match_check_host(None, 0, 2, 2, 1) == -1


def test_statistics_on_hand_values(mt):
    # all wins: s = 1, se = 0, the Elo difference and both ends +inf
    r = mt.MatchResult([1.0] * 8, [[]] * 8, [0] * 8, True)
    assert (r.wins, r.draws, r.losses, r.score, r.se) == (8, 0, 0, 1.0, 0.0)
    assert r.elo == math.inf and r.elo_low == math.inf and r.elo_high == math.inf
    r = mt.MatchResult([0.0] * 4, [[]] * 4, [0] * 4, False)
    assert r.elo == -math.inf and r.losses == 4
    # all draws: s = 1/2, elo 0, se 0
    r = mt.MatchResult([0.5] * 6, [[]] * 6, [0] * 6, True)
    assert (r.score, r.se, r.elo, r.elo_low, r.elo_high, r.draws) == (0.5, 0.0, 0.0, 0.0, 0.0, 6)
    # four pairs (1, 1), (1, 1/2), (1/2, 0), (1, 0): x = 1, 3/4, 1/4, 1/2; s = 5/8; the deviations 3/8, 1/8, -3/8,
    # -1/8 have squares summing to 20/64 = 5/16, so the variance (ddof 1) is 5/48 and se = sqrt(5/48) / 2 =
    # 0.161374...; the interval is 0.625 -+ 1.96 * 0.161374 = [0.308707, 0.941293]; elo(5/8) = 400 log10(5/3) = 88.74
    pts = [1, 1, 1, 0.5, 0.5, 0, 1, 0]
    r = mt.MatchResult(pts, [[]] * 8, [0] * 8, True)
    assert np.array_equal(r.pair_scores, [1.0, 0.75, 0.25, 0.5])
    se = math.sqrt(5.0 / 48.0) / 2.0
    assert r.score == 0.625 and abs(r.se - se) < 1e-15 and abs(se - 0.161374) < 1e-6
    assert (r.wins, r.draws, r.losses) == (4, 2, 2)
    assert abs(r.elo - 400.0 * math.log10(5.0 / 3.0)) < 1e-9 and abs(r.elo - 88.7395) < 1e-3
    lo, hi = 0.625 - 1.96 * se, 0.625 + 1.96 * se
    assert abs(r.elo_low + 400.0 * math.log10(1.0 / lo - 1.0)) < 1e-9 and r.elo_low < 0.0
    assert abs(r.elo_high + 400.0 * math.log10(1.0 / hi - 1.0)) < 1e-9 and r.elo_high > 400.0
    # the same games unpaired: x is the games' points, the same s, another se
    u = mt.MatchResult(pts, [[]] * 8, [0] * 8, False)
    assert u.score == 0.625 and abs(u.se - np.std(pts, ddof=1) / math.sqrt(8)) < 1e-15 and len(u.pair_scores) == 8
    # the interval is clipped to [0, 1]: one loss among wins has an upper end of +inf
    c = mt.MatchResult([1, 1, 1, 1, 1, 1, 1, 0], [[]] * 8, [0] * 8, False)
    assert c.elo_high == math.inf and math.isfinite(c.elo_low) and math.isfinite(c.elo)
