#!/usr/bin/env python3
"""What tree reuse costs and saves. Writes one JSON object (--out, default
profiles/tree_reuse/bench.json) and prints it on one line. Nothing here is a gate: a loss is written down as a loss.

  bench_py   (with --parent-tree DIR, a built checkout of the parent commit) bench.py --gpus 1 --steps K --warmup W
             of the parent and of this tree, --bench-runs runs each, interleaved, each run a process of its own:
             the off path against the parent's. bench.py never turns the feature on.
  network    bench.py's workload (continuous self-play of --games trees x --sims simulations, batch --batch, the
             fused seed-0 network, --lanes lanes, cache 2^--cache-log2) with reuse off and on: --passes passes
             each, interleaved. Per pass: slot-moves/s, leaves sent to the evaluator per slot-move, the cache's hit
             rate, k_reroot's time per move (the engine's dispatch events, a pass of its own with timing on).
  hash       the same with the hash evaluator (one lane, no cache: the tree kernels alone).
  carried    the visits a move begins with, mean over live slots and moves: the blocking driver on --carried-games
             slots with the hash evaluator, the root visits read back after every move begin.

usage: python tools/bench_tree_reuse.py [--parent-tree DIR] [--passes 3] [--bench-runs 3]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "ultimate-tictactoe-alphazero_amd")]


def bench_py(tree, steps, warmup):
    """One bench.py run of the tree at `tree`, in a process of its own: its result line's value."""
    r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warmup)], cwd=tree, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit(f"bench.py in {tree} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    return json.loads(lines[-1])["value"]


def spread(xs):
    return {"runs": xs, "min": min(xs), "median": statistics.median(xs), "max": max(xs),
            "spread_rel": (max(xs) - min(xs)) / statistics.median(xs)}


def selfplay_pass(args, net, reuse, timing=False):
    """One aged, timed window of continuous self-play; net None: the hash evaluator."""
    import torch
    from uttt_amd import SelfPlay
    if net is None:
        sp = SelfPlay(args.games, args.sims, args.batch, 1.0, cache_log2=0, tree_reuse=reuse)
    else:
        from uttt_amd.nnfast import FusedNetworkEvaluator
        sp = SelfPlay(args.games, args.sims, args.batch, 1.0, cache_log2=args.cache_log2, lanes=args.lanes,
                      tree_reuse=reuse)
        sp.set_evaluator(lambda eng: FusedNetworkEvaluator(net, eng))
    total = args.age + args.warmup + args.steps + 2
    sp.begin(0, total * args.games, 1234, arena_plies=total * args.games)
    sp.steps(args.age + args.warmup)
    torch.cuda.synchronize()
    if timing:
        sp.reset_stats()
        sp.set_timing(True)
    c0, leaves0 = sp.cache_stats(), sp.leaves
    t0 = time.perf_counter()
    sp.steps(args.steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    c1 = sp.cache_stats()
    hits, misses = c1["hits"] - c0["hits"], c1["misses"] - c0["misses"]
    moves = args.steps * args.games  # continuous self-play: every slot plays every move
    row = {"moves_per_s": moves / dt, "leaf_evaluations_per_move": (sp.leaves - leaves0) / moves,
           "cache_hit_rate": hits / max(1, hits + misses)}
    if timing:
        st = sp.kernel_stats("reroot")
        row = {"reroot_launches": st["launches"], "reroot_us_per_launch": 1e3 * st["ms"] / max(1, st["launches"]),
               "trees_per_launch": args.games // (1 if net is None else args.lanes)}
    for ln in sp.lanes:
        ln.engine.close()
    return row


def evaluator_rows(args, net):
    rows = {"off": [], "on": []}
    for _ in range(args.passes):  # interleaved
        for mode in ("off", "on"):
            rows[mode].append(selfplay_pass(args, net, mode == "on"))
    out = {m: dict(spread([r["moves_per_s"] for r in rs]),
                   leaf_evaluations_per_move=[r["leaf_evaluations_per_move"] for r in rs],
                   cache_hit_rate=[r["cache_hit_rate"] for r in rs]) for m, rs in rows.items()}
    out["on_relative_to_off"] = {"moves_per_s": out["on"]["median"] / out["off"]["median"],
                                 "leaf_evaluations_per_move": statistics.median(out["on"]["leaf_evaluations_per_move"]) /
                                 statistics.median(out["off"]["leaf_evaluations_per_move"])}
    out["k_reroot"] = selfplay_pass(args, net, True, timing=True)
    return out


def carried(args):
    """Mean visits a move's root begins with, reuse on, by ply range (the blocking driver, hash evaluator)."""
    os.environ["UTTT_ASYNC_ROUNDS"] = "0"
    try:
        from uttt_amd import SelfPlay
        sp = SelfPlay(args.carried_games, args.sims, args.batch, 1.0, cache_log2=0, tree_reuse=True)
        eng = sp.engine
        seen = []
        begin = eng.move_begin

        def move_begin():
            live = begin()
            visits, _ = eng.root_visits()
            seen.append((live, int(visits.sum())))
            return live

        eng.move_begin = move_begin
        moves = args.age + args.steps
        sp.begin(0, (moves + 2) * args.carried_games, 1234, arena_plies=(moves + 2) * args.carried_games)
        sp.steps(moves)
        eng.move_begin = begin
        for ln in sp.lanes:
            ln.engine.close()
    finally:
        os.environ.pop("UTTT_ASYNC_ROUNDS", None)
    live = sum(n for n, _ in seen[1:])
    return {"slots": args.carried_games, "moves": len(seen) - 1, "evaluate_count": args.sims,
            "mean_carried_visits_per_move": sum(v for _, v in seen[1:]) / max(1, live),
            "note": "every slot's first move begins with 0 visits and is left out; a slot refilled with a new game counts"}


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
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--carried-games", type=int, default=512)
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit: bench.py of both, interleaved")
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--parts", type=lambda s: s.split(","), default=["bench_py", "network", "hash", "carried"])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tree_reuse", "bench.json"))
    args = ap.parse_args()
    out = {"metric": "tree reuse: leaves evaluated and moves per second on the headline self-play workload, off and on",
           "unit": "slot-moves/s",
           "config": {k: getattr(args, k) for k in ("games", "sims", "batch", "lanes", "cache_log2", "age", "warmup",
                                                    "steps", "passes", "carried_games")},
           "net": "seed-0 DualNetwork, fused evaluator (f32-level split-f16 tower)",
           "data": "synthetic: self-play games from seed 1234"}
    if "bench_py" in args.parts and args.parent_tree:  # before this process opens the GPU itself
        series = {"parent": [], "this": []}
        trees = {"parent": os.path.abspath(args.parent_tree), "this": REPO}
        for i in range(args.bench_runs):  # the pair's order alternates: neither tree always runs after the other
            for name in (("parent", "this") if i % 2 == 0 else ("this", "parent")):
                series[name].append(bench_py(trees[name], args.steps, args.warmup))
        out["bench_py"] = {"command": f"bench.py --gpus 1 --steps {args.steps} --warmup {args.warmup}",
                           "unit": "simulations/s", "what": "the reuse-off path against the parent commit's",
                           "order": "parent, this, this, parent, parent, this, ... on one GPU, a process per run",
                           "parent": spread(series["parent"]), "this": spread(series["this"])}
        out["bench_py"]["this_within_parent_range"] = (
            out["bench_py"]["this"]["median"] >= out["bench_py"]["parent"]["min"])
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_tree_reuse needs the MI355X (no GPU visible)")
    out["device"] = torch.cuda.get_device_name(0)
    if "network" in args.parts:
        from uttt_amd.model import random_network
        out["network"] = evaluator_rows(args, random_network(0, "cuda"))
        save(args, out)  # (a part that fails later leaves the earlier ones on disk)
    if "hash" in args.parts:
        out["hash"] = evaluator_rows(args, None)
        save(args, out)
    if "carried" in args.parts:
        out["carried"] = carried(args)
    save(args, out)
    print(json.dumps(out))


def save(args, out):
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
