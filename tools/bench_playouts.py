#!/usr/bin/env python3
"""Random-playout evaluator throughput (DESIGN.md "Playout evaluator"). Prints one JSON line:

  playouts          uttt_playouts (k_playout_states) at --positions x --playouts: playouts/s of the whole call
                    (copy in, kernel, copy out, synchronise), and of the kernel alone from its dispatch events
                    in a separate pass
  selfplay          simulations/s of continuous self-play, --games trees x --sims, one lane, evaluation cache
                    off (every queued leaf is evaluated), with PlayoutEvaluator, with HashEvaluator on the same
                    generic device-count round loop (the evaluator's cost alone), and with HashEvaluator as the
                    project runs it (one-dispatch rounds, the move loop in C); windows interleaved
  host              uttt_playout_host on one core of the same box: playouts/s

Every figure: warm-up, then --windows timed windows, each ended by a device synchronise; median and range.

usage: python tools/bench_playouts.py [--positions 4096] [--playouts 64] [--games 4096] [--sims 50]
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


def random_positions(lib, n, seed):
    """n non-terminal positions along uniformly random games (every fifth ply on average), from a seed."""
    import numpy as np
    from uttt_amd._lib import STATE_DTYPE, UtttState
    rng = np.random.RandomState(seed)
    out = np.zeros(n, STATE_DTYPE)
    sp = ctypes.POINTER(UtttState)
    cur, nxt = np.zeros(1, STATE_DTYPE), np.zeros(1, STATE_DTYPE)
    legal = (ctypes.c_int32 * 81)()
    k = 0
    while k < n:
        lib.uttt_state_initial(cur.ctypes.data_as(sp))
        while k < n:
            m = lib.uttt_state_legal_actions(cur.ctypes.data_as(sp), legal)
            if m == 0:
                break
            if rng.randint(5) == 0:
                out[k] = cur[0]
                k += 1
            lib.uttt_state_next(cur.ctypes.data_as(sp), int(legal[rng.randint(m)]), nxt.ctypes.data_as(sp))
            cur, nxt = nxt, cur
    return out


def spread(rates):
    return {"median": statistics.median(rates), "min": min(rates), "max": max(rates), "windows": len(rates)}


def bench_playouts(args, lib, pos):
    import torch
    from uttt_amd import Engine
    eng = Engine(4, 50)
    n, P = len(pos), args.playouts
    for _ in range(3):
        eng.playouts(pos, P, 1)
    torch.cuda.synchronize()
    rates, calls = [], 0
    for w in range(args.windows):
        t0, c = time.perf_counter(), 0
        while time.perf_counter() - t0 < args.window_seconds:
            eng.playouts(pos, P, w * 1000 + c)  # returns after its own synchronise
            c += 1
        rates.append(c * n * P / (time.perf_counter() - t0))
        calls += c
    # the kernel alone: its dispatch's own start and stop events, in a pass of its own
    eng.reset_stats()
    eng.set_timing(True)
    for c in range(20):
        eng.playouts(pos, P, c)
    st = eng.kernel_stats("playout")
    eng.set_timing(False)
    wins, losses = eng.playouts(pos, P, 0)
    return {"positions": n, "playouts_per_position": P, "unit": "playouts/s", "call": spread(rates), "calls": calls,
            "kernel_only": {"value": st["launches"] * n * P / (st["ms"] / 1e3), "launches": st["launches"],
                            "ms_per_launch": st["ms"] / st["launches"]},
            "mean_result": float((wins.astype(float) - losses).sum() / (n * P))}


def bench_host(args, lib, pos):
    import numpy as np
    from uttt_amd._lib import UtttState
    n, P = min(len(pos), args.host_positions), args.playouts
    sub = np.ascontiguousarray(pos[:n])
    wins, losses = np.zeros(n, np.int32), np.zeros(n, np.int32)
    i32 = ctypes.POINTER(ctypes.c_int32)

    def call(seed):
        rc = lib.uttt_playout_host(sub.ctypes.data_as(ctypes.POINTER(UtttState)), n, P, seed, wins.ctypes.data_as(i32),
                                   losses.ctypes.data_as(i32))
        assert rc == 0
    call(1)
    rates = []
    for w in range(args.windows):
        t0, c = time.perf_counter(), 0
        while time.perf_counter() - t0 < args.window_seconds:
            call(w * 1000 + c)
            c += 1
        rates.append(c * n * P / (time.perf_counter() - t0))
    return {"positions": n, "playouts_per_position": P, "unit": "playouts/s", "cores": 1, **spread(rates)}


def bench_selfplay(args):
    import torch
    from uttt_amd import HashEvaluator, PlayoutEvaluator, SelfPlay

    class HashGeneric:
        """HashEvaluator without its one-call rounds: the round loop PlayoutEvaluator runs on."""
        needs_input = False
        device_count = True

        def __init__(self, eng):
            self.inner = HashEvaluator(eng)

        def __call__(self, x, n):
            return self.inner(x, n)

    makers = {"playout": lambda eng: PlayoutEvaluator(eng, args.playouts, 0), "hash_same_loop": HashGeneric,
              "hash": HashEvaluator}
    total_steps = args.age + args.warmup + args.windows * args.steps + 2
    runs, rates = {}, {k: [] for k in makers}
    for name, make in makers.items():
        sp = SelfPlay(args.games, args.sims, args.batch, 1.0, cache_log2=0, lanes=1)
        sp.set_evaluator(make)
        sp.begin(0, total_steps * args.games, 1234, arena_plies=total_steps * args.games)
        sp.steps(args.age + args.warmup)
        torch.cuda.synchronize()
        runs[name] = sp
    leaves = {}
    for w in range(args.windows):  # interleaved: each window of one evaluator beside the others'
        for name, sp in runs.items():
            l0 = sp.leaves
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            done = sp.steps(args.steps)
            torch.cuda.synchronize()
            rates[name].append(done / (time.perf_counter() - t0))
            leaves[name] = (sp.leaves - l0) / args.steps
    out = {"games": args.games, "sims": args.sims, "batch": args.batch, "lanes": 1, "eval_cache": "off",
           "steps_per_window": args.steps, "age_steps": args.age, "unit": "simulations/s"}
    for name in makers:
        out[name] = spread(rates[name])
        out[name]["leaves_per_step"] = leaves[name]
    out["playout"]["playouts_per_leaf"] = args.playouts
    out["playout"]["leaf_playouts_per_s"] = out["playout"]["median"] / (args.games * args.sims) * \
        leaves["playout"] * args.playouts
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=4096)
    ap.add_argument("--playouts", type=int, default=64)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-seconds", type=float, default=0.5)
    ap.add_argument("--steps", type=int, default=30, help="self-play moves per timed window")
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--age", type=int, default=100, help="self-play moves before the timed windows (a mix of game ages)")
    ap.add_argument("--host-positions", type=int, default=256)
    ap.add_argument("--skip-selfplay", action="store_true")
    args = ap.parse_args()
    import torch
    from uttt_amd import _lib
    lib = _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("bench_playouts needs the MI355X (no GPU visible)")
    pos = random_positions(lib, args.positions, 7)
    out = {"metric": "random-playout evaluator throughput", "device": torch.cuda.get_device_name(0),
           "data": "synthetic: positions of uniformly random games (seed 7); self-play games from seed 1234",
           "playouts": bench_playouts(args, lib, pos), "host": bench_host(args, lib, pos)}
    if not args.skip_selfplay:
        out["selfplay"] = bench_selfplay(args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
