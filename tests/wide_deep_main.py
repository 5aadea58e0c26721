"""The device side of test_wide_deep_gpu.py: the searches it compares with the oracle, as functions (run in the
test's process) and as a program (a fresh child for the switches that are read once per process:
UTTT_SEARCH1=0, the per-flush k_flush1 search of uttt_cpp.pv_mcts_scores, and UTTT_FUSED_ROUNDS=0, the hash
rounds as select / hash evaluation / apply launches).

    python wide_deep_main.py cpp OUT.npz      uttt_cpp.pv_mcts_scores over the wide sets
    python wide_deep_main.py deep OUT.npz     uttt_cpp.pv_mcts_scores down the deep line
    python wide_deep_main.py hash OUT.npz     uttt_round_hash_async rounds over the wide sets
"""
import sys
import time

import numpy as np

import wide_deep as wd

# B = 16: a flush spans two chunks of apply_wave's kCopyChunk = 8. S grows with B so that the trees hold enough
# flushes for a wrong prior sum to reach the root's visit counts: with the row pad that skipped ranks past lane
# 63, (100, 1) and (400, 8) and (800, 16) each gave wrong scores on the resident search; (100, 8) and (200, 16),
# a dozen flushes a tree, did not
CPP_CONFIGS = ((100, 1), (400, 8), (800, 16))
HASH_CONFIGS = ((100, 1), (200, 3))
DEEP = (150, 1)


def table_evaluator(evaluate):
    """A BatchedSearch evaluator from a host function x(243,) -> (p[81], v): rows computed on the host for
    x[:n], returned as device tensors."""
    import torch

    def run(x, n):
        xs = x[:n].cpu().numpy().reshape(n, 243)
        rows = [evaluate(xs[i]) for i in range(n)]
        p = torch.from_numpy(np.stack([r[0] for r in rows]).astype(np.float32)).to(x.device)
        v = torch.from_numpy(np.array([r[1] for r in rows], np.float32)).to(x.device)
        return p, v

    return run


def cpp_state(uttt_cpp, ostate):
    p, e, mp, me, a = ostate.arrays()
    return uttt_cpp.State(np.asarray(p).reshape(9, 9).tolist(), np.asarray(e).reshape(9, 9).tolist(),
                          [int(v) for v in mp], [int(v) for v in me], int(a))


def cpp_model(evaluate):
    """A uttt_cpp.pv_mcts_scores model from the same host function."""
    def model(states):
        out = []
        for s in states:
            x = np.asarray(s.to_input_tensor(), np.float32).reshape(9, 9, 3).transpose(2, 0, 1)
            p, v = evaluate(x)
            out.append((p, float(v)))
        return out
    return model


def cpp_scores(ostates, evaluate, S, B, tau=1.0):
    """uttt_cpp.pv_mcts_scores (one resident wave per search, or a launch per flush under UTTT_SEARCH1=0; each
    queued copy's own row applied) of every state -> list of float32 score arrays."""
    import uttt_cpp
    model = cpp_model(evaluate)
    return [np.asarray(uttt_cpp.pv_mcts_scores(model=model, state=cpp_state(uttt_cpp, s), temperature=tau,
                                               evaluate_count=S, batch_size=B), np.float32) for s in ostates]


def hash_round_visits(roots, S, B):
    """(visits, L, scores at 1.0) of a hash-evaluator search driven by uttt_round_hash_async alone (k_round1
    rounds, or under UTTT_FUSED_ROUNDS=0 the public calls' k_select / k_hash_leaves / k_apply)."""
    import torch
    import uttt_amd
    e = uttt_amd.Engine(len(roots), S)
    dev = torch.device("cuda", e.device)
    pol = torch.zeros((len(roots), 81), dtype=torch.float32, device=dev)
    val = torch.zeros(len(roots), dtype=torch.float32, device=dev)
    e.search_begin(roots, S, B)
    ring = e.count_ring()
    for r in range(10 * S):
        slot = r % 8
        tag = e.round_hash_async(slot, pol, val)
        t0 = time.time()
        while int(ring[slot, 3]) != tag:
            assert time.time() - t0 < 30, "round tag not stored"
        if ring[slot, 2] == 0:
            break
    # (the last round's staged apply is flushed by the first call that reads the trees)
    v, L = e.root_visits()
    sc, _ = e.scores(1.0)
    return v, L, sc


def _pad(rows):
    out = np.zeros((len(rows), 81), np.float32)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def main(mode, out):
    res = {}
    if mode == "cpp":
        for kind in ("parents", "roots"):
            _, ost = wd.wide_states(kind)
            for S, B in CPP_CONFIGS:
                res[f"{kind}_{S}_{B}"] = _pad(cpp_scores(ost, wd.spread_table_eval([]), S, B))
    elif mode == "deep":
        root, _, make_eval = wd.deep_line(wd.DEEP_SEED)
        res["deep"] = _pad(cpp_scores([root], make_eval([]), *DEEP))
    elif mode == "hash":
        for kind in ("parents", "roots"):
            roots, _ = wd.wide_states(kind)
            for S, B in HASH_CONFIGS:
                v, L, sc = hash_round_visits(roots, S, B)
                res[f"{kind}_{S}_{B}_visits"], res[f"{kind}_{S}_{B}_L"], res[f"{kind}_{S}_{B}_scores"] = v, L, sc
    else:
        raise SystemExit(f"unknown mode {mode}")
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
