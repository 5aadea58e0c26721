#!/usr/bin/env python3
"""Cost of evaluating leaves through board symmetries on the headline workload: continuous
self-play of --games trees x --sims simulations, batch --batch, the fused network (seed-0 DualNetwork), --lanes
lanes, evaluation cache 2^--cache-log2 entries. Writes one JSON object (--out, default
profiles/symmetry/bench.json) and prints it on one line.

For each of off (the plain FusedNetworkEvaluator, what bench.py runs), hashed and average
(SymmetricLeaves): --passes passes, interleaved over the modes, each a fresh SelfPlay aged --age moves, warmed
--warmup moves and timed over --steps moves between device synchronisations: simulations/s as min / median /
max over the passes, the cache hit rate of the timed window, and, from a pass of their own with the engine's
dispatch events on (--timing-steps moves after the last timed window), the k_sym_leaves / k_sym_rows times per
launch.

usage: python tools/bench_symmetry.py [--games 4096] [--sims 50] [--age 300] [--steps 60] [--passes 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "ultimate-tictactoe-alphazero_amd")]

MODES = ("off", "hashed", "average")


def one_pass(args, net, mode, last):
    import torch
    from uttt_amd import SelfPlay, SymmetricLeaves
    from uttt_amd.nnfast import FusedNetworkEvaluator
    sp = SelfPlay(args.games, args.sims, args.batch, 1.0, cache_log2=args.cache_log2, lanes=args.lanes)

    def make(eng):
        fe = FusedNetworkEvaluator(net, eng)
        return fe if mode == "off" else SymmetricLeaves(fe, eng, mode, seed=args.seed)

    sp.set_evaluator(make)
    total = args.age + args.warmup + args.steps + args.timing_steps + 2
    sp.begin(0, total * args.games, 1234, arena_plies=total * args.games)
    sp.steps(args.age + args.warmup)
    torch.cuda.synchronize()
    c0, leaves0, rounds0 = sp.cache_stats(), sp.leaves, sp.rounds
    t0 = time.perf_counter()
    done = sp.steps(args.steps)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    c1 = sp.cache_stats()
    hits, misses = c1["hits"] - c0["hits"], c1["misses"] - c0["misses"]
    row = {"sims_per_s": done / elapsed, "cache_hit_rate": hits / max(1, hits + misses),
           "leaves_per_round": (sp.leaves - leaves0) / max(1, sp.rounds - rounds0)}
    if last and mode != "off":  # the kernels alone: their dispatches' own start and stop events
        sp.reset_stats()
        sp.set_timing(True)
        sp.steps(args.timing_steps)
        torch.cuda.synchronize()
        row["kernels"] = {}
        for k in ("sym_leaves", "sym_rows"):
            st = sp.kernel_stats(k)
            row["kernels"][k] = {"launches": st["launches"], "us_per_launch": 1e3 * st["ms"] / max(1, st["launches"])}
        sp.set_timing(False)
    for ln in sp.lanes:
        ln.engine.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--lanes", type=int, default=2)
    ap.add_argument("--cache-log2", type=int, default=23)
    ap.add_argument("--age", type=int, default=300, help="self-play moves before the timed window (bench.py's 300)")
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--steps", type=int, default=60, help="self-play moves of the timed window")
    ap.add_argument("--timing-steps", type=int, default=5)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0, help="the hashed choice's seed")
    ap.add_argument("--modes", type=lambda s: s.split(","), default=list(MODES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "symmetry", "bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_symmetry needs the MI355X (no GPU visible)")
    from uttt_amd.model import random_network
    net = random_network(0, "cuda")
    rows = {m: [] for m in args.modes}
    for i in range(args.passes):  # interleaved: each pass of one mode beside the others'
        for m in args.modes:
            rows[m].append(one_pass(args, net, m, i == args.passes - 1))
    out = {"metric": "leaf evaluation through board symmetries: cost on the headline self-play workload",
           "device": torch.cuda.get_device_name(0), "unit": "simulations/s",
           "config": {k: getattr(args, k) for k in ("games", "sims", "batch", "lanes", "cache_log2", "age", "warmup",
                                                    "steps", "passes", "seed")},
           "net": "seed-0 DualNetwork, fused evaluator (f32-level split-f16 tower)",
           "data": "synthetic: self-play games from seed 1234", "modes": {}}
    for m, rs in rows.items():
        rates = [r["sims_per_s"] for r in rs]
        out["modes"][m] = {"min": min(rates), "median": statistics.median(rates), "max": max(rates),
                           "passes": rates, "cache_hit_rate": [r["cache_hit_rate"] for r in rs],
                           "leaves_per_round": [r["leaves_per_round"] for r in rs]}
        if "kernels" in rs[-1]:
            out["modes"][m]["kernels"] = rs[-1]["kernels"]
    if "off" in out["modes"]:
        for m in out["modes"]:
            out["modes"][m]["relative_to_off"] = out["modes"][m]["median"] / out["modes"]["off"]["median"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
