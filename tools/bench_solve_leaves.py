#!/usr/bin/env python3
"""Cost and effect of the solver overlay inside the search (DESIGN.md "Exact endgame values inside the search").
Writes one JSON object (--out, default profiles/solve_leaves/bench.json) and prints it on one line:

  cost      simulations/s of continuous self-play, --games trees x --sims, one lane, evaluation cache off, on
            the generic device-count round loop: PlayoutEvaluator(--playouts) alone, and wrapped in
            SolvedLeaves at every (max_empties, max_nodes) of the sweep; per configuration the shares of
            leaves solved, over budget and skipped during the timed windows, and k_solve_leaves' time per
            launch from its dispatch events in a pass of its own. Windows interleaved over the configurations.
  effect    --effect-games self-play games to their end with PlayoutEvaluator(--playouts), --sims simulations,
            temperature 1, with and without the overlay at each swept (max_empties, max_nodes): the blunder
            rate of the records by solver.blunder_report (--report-nodes nodes per move, on the device).

Every rate: warm-up, then --windows timed windows, each ended by a device synchronise; median and range.

usage: python tools/bench_solve_leaves.py [--games 4096] [--sims 50] [--empties 8,12,16] [--nodes 256,1024,4096]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "ultimate-tictactoe-alphazero_amd")]


def spread(rates):
    return {"median": statistics.median(rates), "min": min(rates), "max": max(rates), "windows": len(rates)}


def makers(args):
    """name -> (make(engine), (max_empties, max_nodes) or None); the unwrapped evaluator first."""
    from uttt_amd import PlayoutEvaluator, SolvedLeaves
    out = {"playout": (lambda eng: PlayoutEvaluator(eng, args.playouts, 0), None)}
    for e in args.empties:
        for m in args.nodes:
            out[f"E{e}_M{m}"] = (lambda eng, e=e, m=m: SolvedLeaves(PlayoutEvaluator(eng, args.playouts, 0), eng,
                                                                    max_empties=e, max_nodes=m, priors="optimal"),
                                 (e, m))
    return out


def bench_cost(args):
    import torch
    from uttt_amd import SelfPlay
    total_steps = args.age + args.warmup + args.windows * args.steps + args.timing_steps + 2
    cfg = makers(args)
    runs, rates = {}, {k: [] for k in cfg}
    for name, (make, _) in cfg.items():
        sp = SelfPlay(args.games, args.sims, args.batch, 1.0, cache_log2=0, lanes=1)
        sp.set_evaluator(make)
        sp.begin(0, total_steps * args.games, 1234, arena_plies=total_steps * args.games)
        sp.steps(args.age + args.warmup)
        torch.cuda.synchronize()
        if cfg[name][1]:
            sp.evaluator.reset_counts()
        runs[name] = sp
    leaves = {k: 0 for k in cfg}
    for _ in range(args.windows):  # interleaved: each window of one configuration beside the others'
        for name, sp in runs.items():
            l0 = sp.leaves
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            done = sp.steps(args.steps)
            torch.cuda.synchronize()
            rates[name].append(done / (time.perf_counter() - t0))
            leaves[name] += sp.leaves - l0
    out = {"games": args.games, "sims": args.sims, "batch": args.batch, "lanes": 1, "eval_cache": "off",
           "playouts_per_leaf": args.playouts, "priors": "optimal", "steps_per_window": args.steps,
           "age_steps": args.age, "unit": "simulations/s", "configurations": {}}
    base = None
    for name, (_, em) in cfg.items():
        row = spread(rates[name])
        row["leaves_per_step"] = leaves[name] / (args.windows * args.steps)
        if em is None:
            base = row["median"]
        else:
            sp = runs[name]
            counts = sp.evaluator.counts()
            rows = max(1, sum(counts.values()))
            row.update(max_empties=em[0], max_nodes=em[1], rows=rows,
                       share_solved=counts["solved"] / rows, share_budget=counts["budget"] / rows,
                       share_skipped=counts["skipped"] / rows, relative_to_unwrapped=row["median"] / base)
            # the kernel alone: its dispatch's own start and stop events, in a pass of its own
            sp.reset_stats()
            sp.set_timing(True)
            sp.steps(args.timing_steps)
            st = sp.kernel_stats("solve_leaves")
            sp.set_timing(False)
            row["kernel"] = {"launches": st["launches"], "us_per_launch": 1e3 * st["ms"] / max(1, st["launches"])}
        out["configurations"][name] = row
    for sp in runs.values():
        for ln in sp.lanes:
            ln.engine.close()
    return out


def bench_effect(args):
    import numpy as np
    from uttt_amd import Engine, SelfPlay, solver
    judge = Engine(4, 50)
    out = {"games": args.effect_games, "sims": args.sims, "temperature": 1.0, "playouts_per_leaf": args.playouts,
           "report_max_nodes": args.report_nodes, "late": f"at most {args.late} empties", "configurations": {}}
    for name, (make, em) in makers(args).items():
        sp = SelfPlay(args.effect_games, args.sims, args.batch, 1.0, lanes=1)
        sp.set_evaluator(make)
        sp.run(0, args.effect_games, 4321)
        recs = sp.records(with_inputs=False)
        states = np.concatenate([r["states"] for r in recs])
        actions = np.concatenate([r["actions"] for r in recs])
        rep = solver.blunder_report(states, actions, args.report_nodes, engine=judge)
        countable, blunders = int(rep["countable"].sum()), int(rep["blunders"].sum())
        late_c, late_b = int(rep["countable"][:args.late + 1].sum()), int(rep["blunders"][:args.late + 1].sum())
        row = {"plies": rep["plies"], "countable": countable, "blunders": blunders,
               "blunder_rate": blunders / max(1, countable), "late_countable": late_c, "late_blunders": late_b,
               "late_blunder_rate": late_b / max(1, late_c),
               "countable_by_empties": rep["countable"].tolist(), "blunders_by_empties": rep["blunders"].tolist()}
        if em:
            row.update(max_empties=em[0], max_nodes=em[1],
                       **{"leaf_" + k: v for k, v in sp.evaluator.counts().items()})
        out["configurations"][name] = row
        for ln in sp.lanes:
            ln.engine.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--playouts", type=int, default=64)
    ap.add_argument("--empties", type=lambda s: [int(x) for x in s.split(",")], default=[8, 12, 16])
    ap.add_argument("--nodes", type=lambda s: [int(x) for x in s.split(",")], default=[256, 1024, 4096])
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30, help="self-play moves per timed window")
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--age", type=int, default=100, help="self-play moves before the timed windows (mixed game ages)")
    ap.add_argument("--timing-steps", type=int, default=10, help="moves of the kernel-timing pass")
    ap.add_argument("--effect-games", type=int, default=256)
    ap.add_argument("--report-nodes", type=int, default=65536)
    ap.add_argument("--late", type=int, default=16, help="the blunder report's late plies: at most this many empties")
    ap.add_argument("--skip-cost", action="store_true")
    ap.add_argument("--skip-effect", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "solve_leaves", "bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_solve_leaves needs the MI355X (no GPU visible)")
    out = {"metric": "solver overlay inside the search: cost and effect", "device": torch.cuda.get_device_name(0),
           "data": "synthetic: self-play games from seeds 1234 (cost) and 4321 (effect)"}
    import inspect
    from uttt_amd import SolvedLeaves
    sig = inspect.signature(SolvedLeaves.__init__).parameters
    # the defaults SolvedLeaves ships, chosen from this sweep (the cheapest point measured)
    out["shipped_defaults"] = {k: sig[k].default for k in ("max_empties", "max_nodes", "priors")}
    if not args.skip_cost:
        out["cost"] = bench_cost(args)
    if not args.skip_effect:
        out["effect"] = bench_effect(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
