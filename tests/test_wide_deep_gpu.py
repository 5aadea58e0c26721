"""The search kernels' second halves against the oracle, bit for bit: leaves with 65-70 legal moves (actions
64-80 in lanes 0-16's second registers, a prior-sum row that needs a pad past lane 63) and a path 75 plies deep
(levels 64-127 in the lanes' second path registers). The inputs come from tests/wide_deep.py and are proven on
the oracle alone by test_wide_deep_host.py; every test here re-asserts from the oracle's replay log that its
trees do reach such leaves or depths before it compares anything.

The spread table's priors cover six decades and are not normalised, so a rank left in a row's pad by a wider
leaf moves q = p / sum by large factors: no tolerance is needed or used."""
import os
import subprocess
import sys

import numpy as np
import pytest

import wide_deep as wd
import wide_deep_main as dev
from conftest import PKG, REPO

pytestmark = pytest.mark.gpu

# trees (of 48) that must evaluate a wide leaf on the oracle: the configurations test_wide_deep_host.py bounds,
# and a quarter of the trees for every other one (enough that a wrong pad cannot hide behind narrow trees)
BOUNDS = {("parents", 100, 1): 48, ("parents", 100, 8): 40, ("parents", 200, 3): 40, ("roots", 200, 3): 36}
TABLE_CONFIGS = [(k, S, B) for k in ("parents", "roots") for S, B in ((100, 1), (100, 8), (200, 3))]


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import uttt_amd
    return uttt_amd


def _assert_wide(ref, kind, S, B, table=True):
    """table: the reference's semantics with the spread table, which BOUNDS is about."""
    logs = [log for _, _, log in ref]
    n = sum(1 for log in logs if wd.wide_count(log))
    assert n >= (BOUNDS.get((kind, S, B), wd.N_ROOTS // 4) if table else wd.N_ROOTS // 4), (kind, S, B, n)
    if table and (kind, S, B) == ("parents", 100, 1):
        assert sum(wd.wide_after_wider(log) for log in logs) >= 24


def _assert_deep(ref):
    _, line, _ = wd.deep_line(wd.DEEP_SEED)
    _, _, log, st = ref
    assert max(log) >= 70 and st.max_depth == len(line) - 1 >= 64 and st.terminal >= 1


def _bits(a, dtype=np.float32):
    a = np.ascontiguousarray(a, dtype)
    return a.view(np.uint32 if dtype == np.float32 else np.uint64)


def _child(tmp_path, mode, **env):
    out = str(tmp_path / f"{mode}.npz")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join((REPO, PKG, os.path.join(REPO, "tests"))), **env)
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "wide_deep_main.py"), mode, out],
                       capture_output=True, text=True, env=env, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


# ---------------------------------------------------------------- (a) deduplicated apply, table evaluator --
@pytest.mark.parametrize("kind,S,B", TABLE_CONFIGS)
def test_dedup_apply_of_wide_leaves_matches_oracle(gpu, oracle_lib, kind, S, B):
    """BatchedSearch.run with the table computed on the host (k_select, k_apply's seq_sum_legal): root visits
    and the scores at two temperatures equal the oracle's."""
    ref = wd.oracle_wide(kind, S, B)
    _assert_wide(ref, kind, S, B)
    roots, _ = wd.wide_states(kind)
    bs = gpu.BatchedSearch(len(roots), S)
    bs.run(roots, dev.table_evaluator(wd.spread_table_eval([])), S, B)
    visits, L = bs.visits()
    for i, (_, vi, _) in enumerate(ref):
        assert L[i] == vi.size and np.array_equal(visits[i, :L[i]], vi), (kind, S, B, i)
    for tau in (1.0, 0.5):
        sc, L = bs.scores(tau)
        for i, (rs, _, _) in enumerate(wd.oracle_wide(kind, S, B, tau)):
            assert np.array_equal(_bits(sc[i, :L[i]]), _bits(rs)), (kind, S, B, tau, i)


# ------------------------------------------------------------------------------ (b) each copy's own row --
@pytest.mark.parametrize("S,B", dev.CPP_CONFIGS)
def test_resident_search_of_wide_leaves_matches_oracle(gpu, oracle_lib, S, B):
    """uttt_cpp.pv_mcts_scores, the default resident wave (k_search1): B = 1 sums in the wave's s_row, B > 1
    per copy in s_copies (chunk_sums; B = 16 spans two chunks of kCopyChunk = 8). The wave keeps both across
    the leaves of a search, so a narrower wide leaf after a wider one reads the wider one's ranks in its pad
    unless the pad is zeroed."""
    for kind in ("parents", "roots"):
        ref = wd.oracle_wide(kind, S, B)
        _assert_wide(ref, kind, S, B)
        got = dev.cpp_scores(wd.wide_states(kind)[1], wd.spread_table_eval([]), S, B)
        bad = [i for i, (rs, _, _) in enumerate(ref) if not np.array_equal(_bits(got[i]), _bits(rs))]
        assert not bad, (kind, S, B, bad)


def test_per_flush_search_of_wide_leaves_matches_oracle(gpu, oracle_lib, tmp_path):
    """The same searches under UTTT_SEARCH1=0 (read once per process, so a fresh child): a k_flush1 launch per
    flush, B = 1 summing in a row of LDS that no earlier leaf of the launch wrote."""
    got = _child(tmp_path, "cpp", UTTT_SEARCH1="0")
    for kind in ("parents", "roots"):
        for S, B in dev.CPP_CONFIGS:
            ref = wd.oracle_wide(kind, S, B)
            _assert_wide(ref, kind, S, B)
            sc = got[f"{kind}_{S}_{B}"]
            bad = [i for i, (rs, _, _) in enumerate(ref) if not np.array_equal(_bits(sc[i, :rs.size]), _bits(rs))]
            assert not bad, (kind, S, B, bad)


# ------------------------------------------------------------------------------------ (c) hash evaluator --
def _check_hash(kind, S, B, visits, L, scores, how):
    ref = wd.oracle_wide_hash(kind, S, B)
    _assert_wide(ref, kind, S, B, table=False)
    for i, (rs, vi, _) in enumerate(ref):
        assert L[i] == vi.size and np.array_equal(visits[i, :L[i]], vi), (how, kind, S, B, i)
        assert np.array_equal(_bits(scores[i, :L[i]]), _bits(rs)), (how, kind, S, B, i)


def test_hash_rounds_of_wide_leaves_match_oracle(gpu, oracle_lib):
    """The device hash evaluator: one-dispatch k_round1 rounds (uttt_round_hash_async), and the blocking
    select / eval_hash / apply loop."""
    for kind in ("parents", "roots"):
        roots, _ = wd.wide_states(kind)
        for S, B in dev.HASH_CONFIGS:
            _check_hash(kind, S, B, *dev.hash_round_visits(roots, S, B), "fused")
            bs = gpu.BatchedSearch(len(roots), S)
            bs.run(roots, gpu.HashEvaluator(bs.engine), S, B)
            _check_hash(kind, S, B, *bs.visits(), bs.scores(1.0)[0], "blocking")


def test_unfused_hash_rounds_of_wide_leaves_match_oracle(gpu, oracle_lib, tmp_path):
    """UTTT_FUSED_ROUNDS=0 (read once per process, so a fresh child): every round of uttt_round_hash_async is
    k_select, k_scan, k_hash_leaves and k_apply."""
    got = _child(tmp_path, "hash", UTTT_FUSED_ROUNDS="0")
    for kind in ("parents", "roots"):
        for S, B in dev.HASH_CONFIGS:
            k = f"{kind}_{S}_{B}"
            _check_hash(kind, S, B, got[k + "_visits"], got[k + "_L"], got[k + "_scores"], "unfused")


# -------------------------------------------------------------------------------------- (d) py semantics --
@pytest.mark.parametrize("zero", [False, True])
def test_py_semantics_of_wide_leaves_match_oracle(gpu, oracle_lib, zero):
    """pv_mcts.py's semantics (the root is evaluated by the first flush, so with wide roots the first sum runs
    np_sum_f32_legal past the first 64 actions' ranks); zero: every fourth wide root's row is all zero, the
    float64-uniform branch on a wide leaf."""
    from uttt_amd.arena import PvMcts, scores_from_visits
    pm = PvMcts(wd.N_ROOTS, 200)
    for kind, S, B in (("roots", 100, 1), ("roots", 100, 8), ("roots", 200, 3), ("parents", 100, 1)):
        ref = wd.oracle_wide(kind, S, B, 1.0, "py", zero)
        _assert_wide(ref, kind, S, B, table=False)
        roots, ost = wd.wide_states(kind)
        if kind == "roots":  # the first evaluation is the wide root's own
            assert all(log[0] == len(s.legal_actions()) for (_, _, log), s in zip(ref, ost))
        visits = pm.visits(roots, dev.table_evaluator(wd.spread_table_eval([], wd.zero_keys() if zero else None)),
                           S, B)
        for i, (rs, vi, _) in enumerate(ref):
            assert np.array_equal(visits[i], vi), (kind, S, B, i)
            assert np.array_equal(_bits(scores_from_visits(visits[i], 1.0), np.float64), _bits(rs, np.float64))


# ---------------------------------------------------------------------------------- (e) evaluation cache --
def test_eval_cache_of_wide_leaves_is_exact(gpu, oracle_lib):
    """Wide roots searched twice on one engine with the evaluation cache on (the second search completes its
    leaves in place from the records' cached prior sums) and once without: all equal the oracle."""
    kind, S, B = "roots", 200, 3
    ref = wd.oracle_wide(kind, S, B)
    _assert_wide(ref, kind, S, B)
    roots, _ = wd.wide_states(kind)
    cached = gpu.BatchedSearch(len(roots), S, cache_log2=16)
    plain = gpu.BatchedSearch(len(roots), S)
    hits = []
    for bs in (cached, cached, plain):
        bs.run(roots, dev.table_evaluator(wd.spread_table_eval([])), S, B)
        visits, L = bs.visits()
        sc, _ = bs.scores(1.0)
        for i, (rs, vi, _) in enumerate(ref):
            assert L[i] == vi.size and np.array_equal(visits[i, :L[i]], vi), i
            assert np.array_equal(_bits(sc[i, :L[i]]), _bits(rs)), i
        if bs is cached:
            hits.append(cached.engine.cache_stats()["hits"])
    assert hits[1] > hits[0] >= 0 and cached.engine.cache_stats()["inserts"] > 0


# -------------------------------------------------------------------------------------------- (f) depth --
def test_deep_line_matches_oracle(gpu, oracle_lib):
    """A path 75 plies deep: the select's path_hi / prec_hi, the terminal back-up's and expand_backup's second
    halves, the queued path's entries 64.., and apply_wave's w_hi, through the deduplicated apply in both
    semantics and through the resident search."""
    from uttt_amd.arena import PvMcts, scores_from_visits
    S, B = dev.DEEP
    root, _, make_eval = wd.deep_line(wd.DEEP_SEED)
    roots = wd.pack_states([root])
    ref = wd.oracle_deep(S, B)
    _assert_deep(ref)
    assert ref[3].nodes <= 82 + 81 * S  # the pool of an engine sized for S simulations holds the tree

    bs = gpu.BatchedSearch(1, S)
    bs.run(roots, dev.table_evaluator(make_eval([])), S, B)
    visits, L = bs.visits()
    assert L[0] == ref[1].size and np.array_equal(visits[0, :L[0]], ref[1])
    for tau in (1.0, 0.5):
        assert np.array_equal(_bits(bs.scores(tau)[0][0, :L[0]]), _bits(wd.oracle_deep(S, B, tau)[0])), tau

    got = dev.cpp_scores([root], make_eval([]), S, B)
    assert np.array_equal(_bits(got[0]), _bits(ref[0]))

    pref = wd.oracle_deep(S, B, 1.0, "py")
    _assert_deep(pref)
    pv = PvMcts(1, S).visits(roots, dev.table_evaluator(make_eval([])), S, B)
    assert np.array_equal(pv[0], pref[1])
    assert np.array_equal(_bits(scores_from_visits(pv[0], 1.0), np.float64), _bits(pref[0], np.float64))


def test_deep_line_per_flush_search_matches_oracle(gpu, oracle_lib, tmp_path):
    """The deep line under UTTT_SEARCH1=0 (a fresh child): k_flush1's apply reads the queued path's entries
    64.. back from memory."""
    ref = wd.oracle_deep(*dev.DEEP)
    _assert_deep(ref)
    got = _child(tmp_path, "deep", UTTT_SEARCH1="0")
    assert np.array_equal(_bits(got["deep"][0, :ref[0].size]), _bits(ref[0]))
