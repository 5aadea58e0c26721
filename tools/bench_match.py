#!/usr/bin/env python3
"""Match play on the device: its throughput against arena._play_games, and one question answered
with it. Writes one JSON object (--out, default profiles/match/bench.json) and prints it on one line.

  throughput  wall time per match and per iteration (one move of every live game) at --games games, hash
              evaluators on both sides, --sims simulations, every game from the initial position with the most
              visited move (so both paths play the same games): match.play_match against arena._play_games at
              temperature 0 driving the same players, --runs runs each, interleaved, the order alternating; both
              timings include creating the two engines. Median and range; no threshold.
  question    a --question-games paired match from openings of --opening-plies plies, PlayoutEvaluator(--playouts)
              on both sides, player 0 with SolvedLeaves(max_empties, max_nodes) and player 1 without: the Elo
              difference the exact endgame is worth, with its 95% interval from the pair scores.

usage: python tools/bench_match.py [--games 256,1024,4096] [--runs 5] [--parts throughput,question]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "ultimate-tictactoe-alphazero_amd")]


def spread(xs):
    return {"runs": xs, "min": min(xs), "median": statistics.median(xs), "max": max(xs),
            "spread_rel": (max(xs) - min(xs)) / statistics.median(xs)}


def device_match(args, games):
    import torch
    import uttt_amd
    from uttt_amd import match
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    players = [match.Player(uttt_amd.HashEvaluator, args.sims, args.batch) for _ in range(2)]
    res = match.play_match(players[0], players[1], games, openings=None, paired=False, sample_plies=0)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, len(res.counters) - 1, res


def host_match(args, games):
    import torch
    import uttt_amd
    from uttt_amd import arena
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    searches = [arena.PvMcts(games, args.sims) for _ in range(2)]
    evs = [uttt_amd.HashEvaluator(s.engine) for s in searches]
    iters = [0]

    def progress(done, total):
        iters[0] += 1

    avg, points, actions = arena._play_games(searches, evs, (args.sims, args.sims), games, 0, 0, args.batch, progress)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    for s in searches:
        s.engine.close()
    return dt, iters[0], (avg, actions)


def throughput(args):
    rows = {}
    for games in args.games:
        series = {"device": [], "arena": []}
        iters = {}
        same = True
        for i in range(args.runs):
            for name in (("device", "arena") if i % 2 == 0 else ("arena", "device")):
                dt, it, res = (device_match if name == "device" else host_match)(args, games)
                series[name].append(dt)
                iters[name] = it
                if name == "device":
                    dev_res = res
                else:
                    host_res = res
            same = same and dev_res.actions == host_res[1] and abs(dev_res.score - host_res[0]) < 1e-12
        rows[str(games)] = {
            "iterations": iters, "same_games_on_both_paths": same,
            "device_s_per_match": spread(series["device"]), "arena_s_per_match": spread(series["arena"]),
            "device_ms_per_iteration": 1e3 * statistics.median(series["device"]) / max(1, iters["device"]),
            "arena_ms_per_iteration": 1e3 * statistics.median(series["arena"]) / max(1, iters["arena"]),
            "arena_over_device": statistics.median(series["arena"]) / statistics.median(series["device"])}
    return rows


def question(args):
    import torch
    import uttt_amd
    from uttt_amd import match
    overlays = []

    def solved(engine):
        ev = uttt_amd.SolvedLeaves(uttt_amd.PlayoutEvaluator(engine, args.playouts, args.playout_seed), engine,
                                   max_empties=args.max_empties, max_nodes=args.max_nodes)
        overlays.append(ev)
        return ev

    def plain(engine):
        return uttt_amd.PlayoutEvaluator(engine, args.playouts, args.playout_seed)

    games = args.question_games
    openings = match.random_openings(games // 2, args.opening_plies, args.seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = match.play_match(match.Player(solved, args.sims, args.batch), match.Player(plain, args.sims, args.batch), games,
                           openings, paired=True, sample_plies=args.sample_plies, seed=args.seed)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"games": games, "opening_plies": args.opening_plies, "sample_plies": args.sample_plies, "seed": args.seed,
            "player0": f"PlayoutEvaluator({args.playouts}) + SolvedLeaves(max_empties={args.max_empties}, "
                       f"max_nodes={args.max_nodes})",
            "player1": f"PlayoutEvaluator({args.playouts})", "sims": args.sims, "batch": args.batch,
            "wins": res.wins, "draws": res.draws, "losses": res.losses, "score": res.score, "se": res.se,
            "elo": res.elo, "elo_low": res.elo_low, "elo_high": res.elo_high,
            "interval_contains_zero": bool(res.elo_low <= 0.0 <= res.elo_high),
            "mean_plies": float(res.plies.mean()), "seconds": dt}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=lambda s: [int(x) for x in s.split(",")], default=[256, 1024, 4096])
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--question-games", type=int, default=4096)
    ap.add_argument("--opening-plies", type=int, default=4)
    ap.add_argument("--sample-plies", type=int, default=0)
    ap.add_argument("--playouts", type=int, default=64)
    ap.add_argument("--playout-seed", type=int, default=0)
    ap.add_argument("--max-empties", type=int, default=8)
    ap.add_argument("--max-nodes", type=int, default=256)
    ap.add_argument("--seed", type=int, default=0, help="the opening book's and the sampled plies' seed")
    ap.add_argument("--parts", type=lambda s: s.split(","), default=["throughput", "question"])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "match", "bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_match needs the MI355X (no GPU visible)")
    out = {"metric": "match play on the device: wall time against arena._play_games, and one Elo difference",
           "unit": "seconds per match",
           "config": {k: getattr(args, k) for k in ("games", "sims", "batch", "runs")},
           "device": torch.cuda.get_device_name(0),
           "data": "synthetic: hash evaluators from the initial position; random openings for the question"}
    if "throughput" in args.parts:
        device_match(args, 64)  # a warm-up of both paths: the library's first launches, torch's allocator
        host_match(args, 64)
        out["throughput"] = throughput(args)
    if "question" in args.parts:
        out["question"] = question(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
