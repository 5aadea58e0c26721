#!/usr/bin/env python3
"""Exact endgame solver throughput. Prints one JSON line:

  solve             uttt_solve (k_solve_states) on --positions positions with at most --max-empties empties at
                    --max-nodes: positions/s and nodes/s of the whole call (copy in, kernel, copy out,
                    synchronise), and of the kernel alone from its dispatch events in a separate pass
  host              uttt_solve_host on one core of the same box, the same inputs (the first --host-positions)
  solved_share      SOLVED / BUDGET counts of the device run by the positions' empties
  blunders          solver.blunder_report over one hash-evaluator self-play run (--games games x --sims)

Every rate: warm-up, then --windows timed windows, each ended by a device synchronise; median and range.

usage: python tools/bench_solver.py [--positions 4096] [--max-empties 16] [--max-nodes 65536]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "ultimate-tictactoe-alphazero_amd")]


def late_positions(lib, n, max_empties, seed):
    """n non-terminal positions with at most max_empties empties from the tails of uniformly random games
    (every second such ply on average), from a seed."""
    import numpy as np
    from uttt_amd import solver
    from uttt_amd._lib import STATE_DTYPE, UtttState
    rng = np.random.RandomState(seed)
    sp = ctypes.POINTER(UtttState)
    legal = (ctypes.c_int32 * 81)()
    out = []
    while len(out) < n:
        game = np.zeros(82, STATE_DTYPE)
        lib.uttt_state_initial(game[0:1].ctypes.data_as(sp))
        k = 0
        while True:
            m = lib.uttt_state_legal_actions(game[k:k + 1].ctypes.data_as(sp), legal)
            if m == 0:
                break
            lib.uttt_state_next(game[k:k + 1].ctypes.data_as(sp), int(legal[rng.randint(m)]),
                                game[k + 1:k + 2].ctypes.data_as(sp))
            k += 1
        tail = game[:k]  # the final position is terminal
        keep = (solver.empties(tail) <= max_empties) & (rng.randint(2, size=k) == 0)
        out.extend(tail[keep])
    return np.array(out[:n], STATE_DTYPE)


def spread(rates):
    return {"median": statistics.median(rates), "min": min(rates), "max": max(rates), "windows": len(rates)}


def windows(call, args, per_call):
    """Rates of `call` over timed windows; per_call: the units one call does, by name."""
    rates = {k: [] for k in per_call}
    calls = 0
    for _ in range(args.windows):
        t0, c = time.perf_counter(), 0
        while c == 0 or time.perf_counter() - t0 < args.window_seconds:
            call()
            c += 1
        dt = time.perf_counter() - t0
        for k, v in per_call.items():
            rates[k].append(c * v / dt)
        calls += c
    return {**{k: spread(v) for k, v in rates.items()}, "calls": calls}


def bench_solve(args, pos):
    import numpy as np
    import torch
    from uttt_amd import Engine, solver
    eng = Engine(4, 50)
    n = len(pos)
    for _ in range(2):
        value, action, status, nodes, av = eng.solve(pos, args.max_nodes)
    torch.cuda.synchronize()
    total = int(nodes.sum())
    out = {"positions": n, "max_nodes": args.max_nodes, "max_empties": args.max_empties, "nodes_per_call": total,
           "units": "positions/s, nodes/s",
           "call": windows(lambda: eng.solve(pos, args.max_nodes), args, {"positions": n, "nodes": total})}
    # the kernel alone: its dispatch's own start and stop events, in a pass of its own
    eng.reset_stats()
    eng.set_timing(True)
    for _ in range(args.kernel_launches):
        eng.solve(pos, args.max_nodes)
    st = eng.kernel_stats("solve")
    eng.set_timing(False)
    sec = st["ms"] / 1e3 / st["launches"]
    out["kernel_only"] = {"positions": n / sec, "nodes": total / sec, "launches": st["launches"],
                          "ms_per_launch": st["ms"] / st["launches"]}
    e = solver.empties(pos)
    out["mean_value"] = float(value[status == solver.SOLVED].mean())
    share = {"empties": list(range(args.max_empties + 1)),
             "solved": np.bincount(e[status == solver.SOLVED], minlength=args.max_empties + 1).tolist(),
             "budget": np.bincount(e[status == solver.BUDGET], minlength=args.max_empties + 1).tolist()}
    share["solved_share"] = float((status == solver.SOLVED).mean())
    return out, share, eng


def bench_host(args, lib, pos):
    import numpy as np
    from uttt_amd import solver
    n = min(len(pos), args.host_positions)
    sub = np.ascontiguousarray(pos[:n])
    nodes = solver.solve_host(sub, args.max_nodes)[3]
    total = int(nodes.sum())
    return {"positions": n, "max_nodes": args.max_nodes, "nodes_per_call": total, "cores": 1,
            "units": "positions/s, nodes/s",
            **windows(lambda: solver.solve_host(sub, args.max_nodes), args, {"positions": n, "nodes": total})}


def bench_blunders(args, eng):
    import numpy as np
    from uttt_amd import HashEvaluator, SelfPlay, solver
    sp = SelfPlay(min(args.games, 1024), args.sims, args.batch, 1.0)
    sp.set_evaluator(HashEvaluator)
    sp.run(0, args.games, 1234)
    recs = sp.records()
    x = np.concatenate([r["inputs"].reshape(len(r["actions"]), 243) for r in recs])
    actions = np.concatenate([r["actions"] for r in recs])
    t0 = time.perf_counter()
    rep = solver.blunder_report(x, actions, args.max_nodes, engine=eng)
    dt = time.perf_counter() - t0
    countable, blunders = int(rep["countable"].sum()), int(rep["blunders"].sum())
    return {"player": "hash evaluator, %d simulations, temperature 1" % args.sims, "games": len(recs),
            "plies": rep["plies"], "max_nodes": args.max_nodes, "countable": countable, "blunders": blunders,
            "blunder_rate": blunders / max(countable, 1), "countable_by_empties": rep["countable"].tolist(),
            "blunders_by_empties": rep["blunders"].tolist(), "report_seconds": dt}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=4096)
    ap.add_argument("--max-empties", type=int, default=16)
    ap.add_argument("--max-nodes", type=int, default=65536)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-seconds", type=float, default=0.5)
    ap.add_argument("--kernel-launches", type=int, default=5)
    ap.add_argument("--host-positions", type=int, default=4096)
    ap.add_argument("--games", type=int, default=256, help="self-play games of the blunder report")
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--skip-blunders", action="store_true")
    args = ap.parse_args()
    import torch
    from uttt_amd import _lib
    lib = _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("bench_solver needs the MI355X (no GPU visible)")
    pos = late_positions(lib, args.positions, args.max_empties, 7)
    solve, share, eng = bench_solve(args, pos)
    out = {"metric": "exact endgame solver throughput", "device": torch.cuda.get_device_name(0),
           "data": "synthetic: tails of uniformly random games (seed 7); self-play games from seed 1234",
           "solve": solve, "host": bench_host(args, lib, pos), "solved_share": share}
    if not args.skip_blunders:
        out["blunders"] = bench_blunders(args, eng)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
