"""The inputs of test_wide_deep_gpu.py, checked on the oracle alone: the wide walks' trees do evaluate leaves
with 65-70 legal moves whose prior-sum row needs a pad, narrower ones after wider ones, and the deep line's
search does walk more than 64 plies down. A device comparison on these inputs therefore never passes on trees
that stayed narrow or shallow. The bounds are fixed; a seed that misses one is replaced, not the bound."""
import statistics

import wide_deep as wd


def _counts(kind, S, B):
    ref = wd.oracle_wide(kind, S, B)
    return [wd.wide_count(log) for _, _, log in ref], sum(wd.wide_after_wider(log) for _, _, log in ref)


def test_wide_walks_keep_what_they_promise(oracle_lib):
    """48 roots each; every kept state has 66-70 legal moves, its parent is one move above it, and the wide
    roots' free-move children (the decided board's cell index) have one legal move fewer."""
    _, parents = wd.wide_states("parents")
    roots, wide = wd.wide_states("roots")
    assert len(parents) == len(wide) == len(roots) == wd.N_ROOTS
    narrower = 0
    for p, w in zip(parents, wide):
        L = len(w.legal_actions())
        assert L in wd.KEEP and not w.is_done()
        assert any(p.next(a).tensor_nchw().tobytes() == w.tensor_nchw().tobytes() for a in p.legal_actions())
        narrower += any(len(w.next(a).legal_actions()) == L - 1 for a in w.legal_actions())
    assert narrower == wd.N_ROOTS


def test_wide_parents_one_copy_per_flush(oracle_lib):
    """wide_parents(48, seed 27), S = 100, B = 1: every tree evaluates a wide leaf (got min 1, median 3) and
    there are at least 24 wide-after-wider events over the 48 trees (got 106)."""
    wc, waw = _counts("parents", 100, 1)
    print("wide leaves per root: min", min(wc), "median", statistics.median(wc), "wide-after-wider", waw)
    assert min(wc) >= 1
    assert waw >= 24


def test_wide_parents_batched_flushes(oracle_lib):
    """wide_parents(48, seed 27): at least 40 of 48 trees evaluate a wide leaf at S = 100, B = 8 (got 40) and at
    S = 200, B = 3 (got 46)."""
    for S, B in ((100, 8), (200, 3)):
        wc, _ = _counts("parents", S, B)
        n = sum(1 for c in wc if c)
        print((S, B), "roots with a wide leaf:", n)
        assert n >= 40, (S, B, n)


def test_wide_roots_expand_narrower_wide_leaves(oracle_lib):
    """wide_roots(48, seed 27), S = 200, B = 3: at least 36 of 48 trees evaluate a wide leaf (got 38)."""
    wc, waw = _counts("roots", 200, 3)
    n = sum(1 for c in wc if c)
    print("roots with a wide leaf:", n, "wide-after-wider", waw)
    assert n >= 36


def test_deep_line_is_walked_to_its_end(oracle_lib):
    """deep_line(seed 7): a 76-ply game, so the terminal state lies 75 plies below the root; S = 150, B = 1
    evaluates line states down to 74 plies (required: >= 70) and then reaches the terminal state (the longest
    path has 75 edges, and simulations end on a terminal node). In pv_mcts.py's semantics the same."""
    _, line, _ = wd.deep_line(wd.DEEP_SEED)
    assert line[-1].is_done() and not any(s.is_done() for s in line[:-1])
    for semantics in ("cpp", "py"):
        _, vi, log, st = wd.oracle_deep(150, 1, semantics=semantics)
        print(semantics, "line plies", len(line) - 1, "deepest evaluated", max(log), "terminal sims", st.terminal)
        assert max(log) >= 70
        assert max(log) == len(line) - 2 and st.max_depth == len(line) - 1 and st.terminal >= 1
        assert int(vi.sum()) == (150 if semantics == "cpp" else 149)
