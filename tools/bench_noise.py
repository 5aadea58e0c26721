#!/usr/bin/env python3
"""Cost and effect of root noise and the temperature schedule. Writes one JSON object (--out,
default profiles/noise/bench.json) and prints it on one line.

  bench_py   (with --parent-tree DIR, a built checkout of the parent commit) bench.py --gpus 1 --steps K --warmup W
             of the parent and of this tree, --bench-runs runs each, interleaved, each run a process of its own:
             both series and their spreads. bench.py never turns the feature on.
  headline   bench.py's workload (continuous self-play of --games trees x --sims simulations, batch --batch, the
             fused seed-0 network, --lanes lanes, cache 2^--cache-log2) with noise off and with noise
             (--epsilon, --alpha) on: --passes passes each, interleaved, simulations/s as min / median / max.
  kernel     k_root_noise's own time per launch at --games trees (every root the initial state, 81 legal moves,
             and every root a 9-move reply), from the engine's dispatch events (uttt_engine_kernel_stats).
  effect     --effect-games hash-evaluator self-play games from one seed base: the number of distinct sequences
             of the first 4 moves with neither feature, with noise, with the schedule (--plies, 0.0), with both.

usage: python tools/bench_noise.py [--parent-tree DIR] [--passes 3] [--bench-runs 3]
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


def headline_pass(args, net, noise):
    import torch
    from uttt_amd import SelfPlay
    from uttt_amd.nnfast import FusedNetworkEvaluator
    sp = SelfPlay(args.games, args.sims, args.batch, 1.0, cache_log2=args.cache_log2, lanes=args.lanes,
                  root_noise=(args.epsilon, args.alpha, args.seed) if noise else None)
    sp.set_evaluator(lambda eng: FusedNetworkEvaluator(net, eng))
    total = args.age + args.warmup + args.steps + 2
    sp.begin(0, total * args.games, 1234, arena_plies=total * args.games)
    sp.steps(args.age + args.warmup)
    torch.cuda.synchronize()
    c0, leaves0 = sp.cache_stats(), sp.leaves
    t0 = time.perf_counter()
    done = sp.steps(args.steps)
    torch.cuda.synchronize()
    rate = done / (time.perf_counter() - t0)
    c1 = sp.cache_stats()
    hits, misses = c1["hits"] - c0["hits"], c1["misses"] - c0["misses"]
    # noise makes the games diverge, so fewer leaves are answered by the evaluation cache and more by the network:
    # the hit rate and the leaves sent to the network say how much of a rate difference is that
    row = {"sims_per_s": rate, "cache_hit_rate": hits / max(1, hits + misses),
           "network_leaves_per_move": (sp.leaves - leaves0) / args.steps,
           "root_noise_launches": sp.kernel_stats("root_noise")["launches"]}
    for ln in sp.lanes:
        ln.engine.close()
    return row


def kernel_time(args):
    from uttt_amd import Engine, initial_states
    from uttt_amd._lib import UtttState
    import ctypes
    out = {}
    first = initial_states(args.games)
    reply = initial_states(1)
    nxt = initial_states(1)
    from uttt_amd import _lib
    _lib.check(_lib.load().uttt_state_next(reply.ctypes.data_as(ctypes.POINTER(UtttState)), 1,
                                           nxt.ctypes.data_as(ctypes.POINTER(UtttState))))
    for name, roots in (("81_moves", first), ("9_moves", nxt.repeat(args.games))):
        e = Engine(args.games, args.sims)
        e.set_root_noise(args.epsilon, args.alpha, args.seed)
        for timed in (False, True):  # a warm-up, then the timed launches
            e.reset_stats()
            e.set_timing(timed)
            for _ in range(args.kernel_launches):
                e.search_begin(roots, args.sims, args.batch)
            e.root_priors()  # synchronises the stream and drains the events
        st = e.kernel_stats("root_noise")
        out[name] = {"trees": args.games, "launches": st["launches"], "us_per_launch": 1e3 * st["ms"] / st["launches"]}
        e.close()
    return out


def effect(args):
    from uttt_amd import SelfPlay
    rows = {}
    for name, kw in (("neither", {}),
                     ("noise", dict(root_noise=(args.epsilon, args.alpha, args.seed))),
                     ("schedule", dict(temperature_plies=args.plies, late_temperature=0.0)),
                     ("both", dict(root_noise=(args.epsilon, args.alpha, args.seed), temperature_plies=args.plies,
                                   late_temperature=0.0))):
        sp = SelfPlay(args.effect_games, args.sims, args.batch, 1.0, **kw)
        sp.run(0, args.effect_games, args.effect_seed)
        recs = sp.records(with_inputs=False)
        openings = {tuple(r["actions"][:4].tolist()) for r in recs}
        rows[name] = {"games": len(recs), "distinct_first_4_moves": len(openings),
                      "mean_plies": sum(len(r["actions"]) for r in recs) / len(recs)}
        for ln in sp.lanes:
            ln.engine.close()
    return rows


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
    ap.add_argument("--epsilon", type=float, default=0.25)
    ap.add_argument("--alpha", type=float, default=0.3)
    ap.add_argument("--seed", type=int, default=0, help="the noise seed")
    ap.add_argument("--plies", type=int, default=8, help="the schedule of the effect measure: (plies, 0.0)")
    ap.add_argument("--kernel-launches", type=int, default=50)
    ap.add_argument("--effect-games", type=int, default=1024)
    ap.add_argument("--effect-seed", type=int, default=1234, help="the effect measure's seed base")
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit: bench.py of both, interleaved")
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--parts", type=lambda s: s.split(","), default=["bench_py", "headline", "kernel", "effect"])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "noise", "bench.json"))
    args = ap.parse_args()
    out = {"metric": "root noise and temperature schedule: cost on the headline self-play workload, and effect",
           "unit": "simulations/s",
           "config": {k: getattr(args, k) for k in ("games", "sims", "batch", "lanes", "cache_log2", "age", "warmup",
                                                    "steps", "passes", "epsilon", "alpha", "seed", "plies")},
           "net": "seed-0 DualNetwork, fused evaluator (f32-level split-f16 tower)",
           "data": "synthetic: self-play games from seed 1234"}
    if "bench_py" in args.parts and args.parent_tree:  # before this process opens the GPU itself
        series = {"parent": [], "this": []}
        trees = {"parent": os.path.abspath(args.parent_tree), "this": REPO}
        for i in range(args.bench_runs):  # the pair's order alternates: neither tree always runs after the other
            for name in (("parent", "this") if i % 2 == 0 else ("this", "parent")):
                series[name].append(bench_py(trees[name], args.steps, args.warmup))
        out["bench_py"] = {"command": f"bench.py --gpus 1 --steps {args.steps} --warmup {args.warmup}",
                           "order": "parent, this, this, parent, parent, this, ... on one GPU, a process per run",
                           "parent": spread(series["parent"]), "this": spread(series["this"])}
        out["bench_py"]["this_within_parent_range"] = (
            out["bench_py"]["this"]["median"] >= out["bench_py"]["parent"]["min"])
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_noise needs the MI355X (no GPU visible)")
    out["device"] = torch.cuda.get_device_name(0)
    if "headline" in args.parts:
        from uttt_amd.model import random_network
        net = random_network(0, "cuda")
        rows = {"off": [], "on": []}
        for _ in range(args.passes):  # interleaved
            for mode in ("off", "on"):
                rows[mode].append(headline_pass(args, net, mode == "on"))
        out["headline"] = {m: dict(spread([r["sims_per_s"] for r in rs]),
                                   cache_hit_rate=[r["cache_hit_rate"] for r in rs],
                                   network_leaves_per_move=[r["network_leaves_per_move"] for r in rs],
                                   root_noise_launches=rs[-1]["root_noise_launches"]) for m, rs in rows.items()}
        out["headline"]["on_relative_to_off"] = out["headline"]["on"]["median"] / out["headline"]["off"]["median"]
    if "kernel" in args.parts:
        out["kernel"] = kernel_time(args)
    if "effect" in args.parts:
        out["effect"] = {"games": args.effect_games, "seed_base": args.effect_seed, "evaluator": "hash",
                         "noise": [args.epsilon, args.alpha], "schedule": [args.plies, 0.0], "rows": effect(args)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
