"""Batched self-play and batched search on the engine.

The reference plays SP_GAME_COUNT games one after another, each move one
search whose flushes call the network at batch <= 8 (self_play_cpp.py:104-130,
pv_mcts_cpp.py:37-87). Here all games of a shard advance together: each round
every live tree contributes its one pending leaf to a single network batch.
"""
import collections
import contextlib
import math
import os
import time

import numpy as np
import torch

from .engine import Engine, RoundCount, initial_states


def _bucket(n, cap, quantum=256):
    """Round a batch up so the network sees few distinct shapes (MIOpen tuning)."""
    if n <= 64:
        b = 1 << max(0, math.ceil(math.log2(max(n, 1))))
    else:
        b = ((n + quantum - 1) // quantum) * quantum
    return min(b, cap)


class HashEvaluator:
    """Device hash evaluator (bit-reproducible; the parity and kernel-bench evaluator). With a
    RoundCount for n (device-count rounds) it reads the pending leaves' states and the count on the
    device (Engine.eval_hash_dev), so SelfPlay pipelines its rounds as with the fused network."""

    device_count = True
    cheap = True  # SelfPlay keeps two rounds in flight: the host's reaction, not the kernels, set the pace

    def __call__(self, x, n):
        if isinstance(n, RoundCount):
            self.engine.eval_hash_dev(self.policy, self.value)
            return self.policy, self.value
        self.engine.eval_hash(x, n, self.policy, self.value)
        return self.policy[:n], self.value[:n]

    def __init__(self, engine):
        self.engine = engine
        dev = torch.device("cuda", engine.device)
        self.policy = torch.zeros((engine.max_trees, 81), dtype=torch.float32, device=dev)
        self.value = torch.zeros((engine.max_trees, 1), dtype=torch.float32, device=dev)
        # rounds per C call (UTTT_ROUND_BATCH, default 1): a call may enqueue up to 4 one-dispatch rounds whose
        # last tag alone is polled, but the rounds enqueued past a move's end then outnumber the host time
        # saved: tree-only 4096 x 50, interleaved (profiles/r6/sweeps/u6j): 1 round per call, 3 in flight
        # 558-567M sims/s; 2 x 3 509-511M; 2 x 4 471-472M; 4 x 2 508-509M; 1 x 4 548-551M
        self.rounds_per_call = max(1, min(4, int(os.environ.get("UTTT_ROUND_BATCH", "1"))))

    def round_async(self, engine, slot):
        """rounds_per_call whole rounds in one C call (Engine.rounds_hash_async: per round one k_round1 launch
        that applies the previous round's evaluation, descends, evaluates the new leaves and publishes the
        counts; the last round's apply is staged for the next call or the move's end). SelfPlay.steps then
        polls the last round's tag in the host count ring instead of an event."""
        if self.rounds_per_call == 1:
            return engine.round_hash_async(slot, self.policy, self.value)
        return engine.rounds_hash_async(slot, self.policy, self.value, self.rounds_per_call)

    def round_move(self, engine, slot, depth):
        """A move's whole round loop in one C call (Engine.rounds_hash_move): `depth` rounds in flight, the
        host spinning on their tags in C, until a round leaves no tree with simulations."""
        return engine.rounds_hash_move(slot, self.policy, self.value, depth)


class PlayoutEvaluator:
    """Random-playout evaluator (game.py:277-287 as the leaf evaluation; no weights): value = mean result of
    `playouts` uniformly random games from the leaf, uniform priors. Reads the pending leaves' states and the
    count on the device (Engine.eval_playout_dev) after a blocking or an asynchronous select alike, and is a
    function of the position and the seed alone: bit-reproducible and exact under the evaluation cache. It has
    no one-call rounds, so SelfPlay runs it on the generic device-count path, one round in flight."""

    needs_input = False
    device_count = True

    def __init__(self, engine, playouts=64, seed=0):
        if not 1 <= int(playouts) <= 4096:
            raise ValueError(f"playouts must be 1..4096 (got {playouts})")
        self.engine = engine
        self.playouts = int(playouts)
        self.seed = int(seed)
        dev = torch.device("cuda", engine.device)
        self.policy = torch.zeros((engine.max_trees, 81), dtype=torch.float32, device=dev)
        self.value = torch.zeros((engine.max_trees, 1), dtype=torch.float32, device=dev)

    def __call__(self, x, n):
        self.engine.eval_playout_dev(self.policy, self.value, self.playouts, self.seed)
        if isinstance(n, RoundCount):
            return self.policy, self.value
        return self.policy[:n], self.value[:n]


class SolvedLeaves:
    """Any evaluator with an exact endgame: after `base` has filled the round's rows, the engine lays the
    solver's values over them (Engine.eval_solve_dev). A leaf with at most `max_empties` empty
    cells in open boards that `max_nodes` nodes per move prove gets its exact value and, with
    priors="optimal", priors on its optimal moves only; every other leaf keeps what `base` wrote. A function
    of the position and these parameters alone (given that `base` is one of the position), so exact under the
    evaluation cache: SelfPlay.set_evaluator clears the table; a BatchedSearch user who changes the parameters
    on a cached engine calls Engine.cache_clear.

    The overlay launches on the engine's stream, which in BatchedSearch and SelfPlay is the stream the
    evaluator runs on, so it is ordered after `base` and before the apply. It has no one-call rounds:
    SelfPlay runs it on the generic device-count loop, as it runs PlayoutEvaluator.

    solved / budget / skipped: rows overlaid, searched without a proof, and not searched, over all calls.
    The kernel writes each call's statuses into the next row of a device ring of kRing x max_trees bytes
    prefilled with -1 (`status` is the latest call's row), so a round costs nothing beyond the overlay; the
    rows are summed into three device totals when the ring is full (every kRing calls) and when a count is
    read, and only a read copies anything back, on the engine's stream.

    The defaults are the cheapest point of the measured sweep: a launch lasts as long as its
    slowest lane, about 1 us per step and two steps per node, so max_nodes is the overlay's latency per round;
    at 8 empties 256 nodes already prove all but 0.06% of the leaves searched."""

    kRing = 32  # status rows kept before they are folded into the totals

    def __init__(self, base, engine, max_empties=8, max_nodes=256, priors="optimal"):
        from . import solver
        if not 0 <= int(max_empties) <= solver.MAX_EMPTY:
            raise ValueError(f"max_empties must be 0..{solver.MAX_EMPTY} (got {max_empties})")
        if not 1 <= int(max_nodes) <= 1 << 22:
            raise ValueError(f"max_nodes must be 1..{1 << 22} (got {max_nodes})")
        self.base = base
        self.engine = engine
        self.max_empties = int(max_empties)
        self.max_nodes = int(max_nodes)
        self.priors = solver.priors_mode(priors)
        if self.priors not in (solver.PRIORS_KEEP, solver.PRIORS_OPTIMAL):
            raise ValueError(f"priors must be keep or optimal (got {priors!r})")
        self.needs_input = getattr(base, "needs_input", True)
        self.device_count = getattr(base, "device_count", False)
        # One status row per call, kRing calls deep, every entry -1 until its call writes it (rows past the
        # round's count stay -1): the kernel writes the statuses where the counts will later be taken from, so
        # a round costs nothing beyond the overlay itself. The rows are folded into the totals when the ring
        # is full and when a count is read, never per round.
        dev = torch.device("cuda", engine.device)
        self._ring = torch.full((self.kRing, engine.max_trees), -1, dtype=torch.int8, device=dev)
        self._used = 0
        self._totals = torch.zeros(3, dtype=torch.int64, device=dev)  # skipped, solved, budget
        self.status = self._ring[0]  # the statuses of the latest call: max_trees bytes, -1 past its count
        torch.cuda.current_stream(dev).synchronize()  # the fill, before the engine's stream writes into it

    def __call__(self, x, n):
        p, v = self.base(x, n)
        if self._used == self.kRing:
            self._fold()
        self.status = self._ring[self._used]
        self._used += 1
        self.engine.eval_solve_dev(p, v, self.max_empties, self.max_nodes, self.priors, self.status)
        return p, v

    def _fold(self):
        if self._used:
            with torch.cuda.stream(self.engine.stream):  # ordered after the overlays that wrote the rows
                rows = self._ring[:self._used]
                self._totals += torch.stack([(rows == k).sum() for k in (0, 1, 2)])
                rows.fill_(-1)
            self._used = 0

    def counts(self):
        """{"skipped", "solved", "budget"}: rows of all calls so far (one read-back)."""
        self._fold()
        with torch.cuda.stream(self.engine.stream):  # the copy behind the fold, on the stream that ran it
            k, s, b = self._totals.tolist()
        return {"skipped": k, "solved": s, "budget": b}

    def reset_counts(self):
        self._fold()
        with torch.cuda.stream(self.engine.stream):
            self._totals.zero_()

    @property
    def solved(self):
        return self.counts()["solved"]

    @property
    def budget(self):
        return self.counts()["budget"]

    @property
    def skipped(self):
        return self.counts()["skipped"]


def parse_symmetry(spec):
    """A symmetry setting -> None (off) or (mode, seed): spec is None / "off", "hashed", "average", a fixed
    symmetry 0..7 (int or digit), or a (mode, seed) pair; a string may end in ":seed" (UTTT_SYMMETRY's form)."""
    if spec is None:
        return None
    if isinstance(spec, tuple):
        if len(spec) != 2:
            raise ValueError(f"a symmetry pair is (mode, seed) (got {spec!r})")
        mode = parse_symmetry(spec[0])
        return None if mode is None else (mode[0], int(spec[1]))
    seed = 0
    if isinstance(spec, str):
        spec, _, tail = spec.strip().partition(":")
        if tail:
            seed = int(tail, 0)
        if spec in ("", "off"):
            return None
        if spec.isdigit():
            spec = int(spec)
    if spec in ("hashed", "average"):
        return spec, seed
    if isinstance(spec, (int, np.integer)) and not isinstance(spec, bool) and 0 <= int(spec) <= 7:
        return int(spec), seed
    raise ValueError(f"symmetry must be off, hashed, average or 0..7, with an optional :seed (got {spec!r})")


def symmetry_from_env():
    """UTTT_SYMMETRY = off (default) | hashed | average | 0..7, with an optional :seed, as parse_symmetry reads it."""
    return parse_symmetry(os.environ.get("UTTT_SYMMETRY", "off"))


def with_symmetry(evaluator, engine, symmetry):
    """`evaluator` as it is (symmetry None / "off") or wrapped in SymmetricLeaves."""
    sym = parse_symmetry(symmetry)
    if sym is None:
        return evaluator
    return SymmetricLeaves(evaluator, engine, mode=sym[0], seed=sym[1])


class SymmetricLeaves:
    """Any evaluator that takes its leaves from the caller, seen through a symmetry of the square:
    the round's pending leaves are transformed on the device (Engine.sym_pending_dev), `base` evaluates the
    images, and the rows are mapped back to the leaves' own actions (Engine.sym_rows_dev; the value of a
    position and of its image are the same). mode:

      "hashed"   one symmetry per leaf, chosen by the playout key of the position's 243 input bits and `seed`
                 (symmetry.hashed_symmetry): along a search path the network's errors decorrelate, at the cost
                 of two small launches per round;
      "average"  the mean over all eight, accumulated in f32 in the order g = 0..7 and multiplied by 0.125:
                 eight evaluations per round;
      0..7       that symmetry for every leaf.

    A base with forward_device_states(states, n) (FusedNetworkEvaluator) gets the transformed states and
    reads the count on the device: device_count is the base's and needs_input is False. Any other base is
    called as base(x, n) with the wrapper's own NCHW buffer of the images and a host count (NetworkEvaluator,
    arena.ModelEvaluator, HashEvaluator): device_count is False, and the base's one-call rounds (round_async,
    round_move, cheap) are not exposed. A base that reads the engine's pending leaves itself would not see
    the images and is refused with a TypeError: PlayoutEvaluator, SolvedLeaves (wrap the other way round:
    SolvedLeaves(SymmetricLeaves(...)), the overlay last), another SymmetricLeaves, and any base asked for a
    device count it could only serve from the engine's own leaves (HashEvaluator with a RoundCount).
    One row per leaf: per-copy applies are out of scope, as for SolvedLeaves.

    Cache rule: the result is a function of the position, the mode and the seed (given that `base` is one of
    the position), so a search stays exact under the evaluation cache while they do not change.
    SelfPlay.set_evaluator clears the table; a BatchedSearch user who changes the mode or the seed on a cached
    engine calls Engine.cache_clear.

    The engine's kernels launch on the engine's stream, which in BatchedSearch and SelfPlay is the stream the
    evaluator runs on, so transform, evaluation and back-mapping are ordered. forward_kw (e.g. softmax=False)
    is passed on to forward_device_states."""

    def __init__(self, base, engine, mode="hashed", seed=0, **forward_kw):
        if isinstance(mode, str) and mode not in ("hashed", "average"):
            raise ValueError(f"mode must be 'hashed', 'average' or a symmetry 0..7 (got {mode!r})")
        if not isinstance(mode, str):
            if isinstance(mode, bool) or not isinstance(mode, (int, np.integer)) or not 0 <= int(mode) <= 7:
                raise ValueError(f"mode must be 'hashed', 'average' or a symmetry 0..7 (got {mode!r})")
            mode = int(mode)
        self._states_path = callable(getattr(base, "forward_device_states", None))
        if isinstance(base, (PlayoutEvaluator, SolvedLeaves, SymmetricLeaves)) or \
                (not self._states_path and not getattr(base, "needs_input", True)):
            raise TypeError(f"{type(base).__name__} reads the engine's pending leaves itself and would not see "
                            "the transformed ones: it cannot be wrapped in SymmetricLeaves")
        self.base = base
        self.engine = engine
        self.mode = mode
        self.seed = int(seed)
        self.forward_kw = forward_kw
        self.needs_input = False  # the wrapper builds the images' input itself, when the base reads one
        self.device_count = self._states_path and bool(getattr(base, "device_count", False))
        dev = torch.device("cuda", engine.device)
        n = engine.max_trees
        self.states = torch.zeros((n, 8), dtype=torch.int32, device=dev)
        self.sym = torch.zeros((n,), dtype=torch.int8, device=dev)
        self.x = None if self._states_path else torch.zeros((n, 3, 9, 9), dtype=torch.float32, device=dev)
        self.policy = torch.zeros((n, 81), dtype=torch.float32, device=dev)
        self.value = torch.zeros((n, 1), dtype=torch.float32, device=dev)
        torch.cuda.current_stream(dev).synchronize()  # the fills, before the engine's stream writes into them

    def _pass(self, n, mode, g_or_seed, accumulate, scale):
        self.engine.sym_pending_dev(mode, g_or_seed, self.states, self.sym, self.x)
        if self._states_path:
            p, v = self.base.forward_device_states(self.states, n, **self.forward_kw)
        else:
            p, v = self.base(self.x, n)
            p = p if p.dtype == torch.float32 and p.stride(1) == 1 else p.float().contiguous()
            v = v if v.dtype == torch.float32 else v.float()
        rows = len(p)
        out_v = self.value[:rows] if v.dim() == 2 else self.value[:rows, 0]
        self.engine.sym_rows_dev(self.sym, p, v, self.policy[:rows], out_v, accumulate, scale)

    def __call__(self, x, n):
        if isinstance(n, RoundCount) and not self.device_count:
            raise TypeError(f"{type(self.base).__name__} could serve a device count only from the engine's own "
                            "pending leaves: SymmetricLeaves calls it with a host count")
        if self.mode == "average":
            for g in range(8):
                self._pass(n, "fixed", g, g > 0, 0.125 if g == 7 else 1.0)
        elif self.mode == "hashed":
            self._pass(n, "hashed", self.seed, False, 1.0)
        else:
            self._pass(n, "fixed", self.mode, False, 1.0)
        if isinstance(n, RoundCount):
            return self.policy, self.value
        return self.policy[:n], self.value[:n]


class NetworkEvaluator:
    """DualNetwork (or any model with its call signature) on the engine's device."""

    def __init__(self, model, max_batch):
        self.model = model
        self.max_batch = max_batch

    @torch.no_grad()
    def __call__(self, x, n):
        nb = _bucket(n, self.max_batch)
        p, v = self.model(x[:nb])
        return p[:n].float(), v[:n].float()


def model_evaluator_factory(model, kind=None, symmetry=None):
    """make(engine) -> evaluator for a model: the fused HIP evaluator for a DualNetwork (the
    drop-ins' default, nnfast.evaluator_kind), else the model called on the engine's NCHW batch.
    symmetry (parse_symmetry's forms; default off): the evaluator wrapped in SymmetricLeaves."""
    from .nnfast import FusedNetworkEvaluator, evaluator_kind
    parse_symmetry(symmetry)  # a bad setting fails here, not at the first engine
    if evaluator_kind(model, kind) == "fused":
        return lambda eng: with_symmetry(FusedNetworkEvaluator(model, eng), eng, symmetry)
    return lambda eng: with_symmetry(NetworkEvaluator(model, eng.max_trees), eng, symmetry)


class BatchedSearch:
    """pv_mcts_scores (uttt_mcts.cpp:84-196) for many root states at once."""

    def __init__(self, max_trees, max_sims=50, device=None, cache_log2=0):
        self.engine = Engine(max_trees, max_sims, device)
        if cache_log2:
            self.engine.set_cache(cache_log2, 0)
        dev = torch.device("cuda", self.engine.device)
        self.x = torch.zeros((max_trees, 3, 9, 9), dtype=torch.float32, device=dev)
        self.rounds = 0

    def run(self, roots, evaluator, evaluate_count=50, batch_size=8, semantics="cpp"):
        e = self.engine
        e.use_stream()
        e.search_begin(roots, evaluate_count, batch_size, semantics)
        self.rounds = 0
        x = self.x if getattr(evaluator, "needs_input", True) else None
        while True:
            n = e.select(x)
            if n == 0:
                break
            p, v = evaluator(self.x, n)
            e.apply(p, v)
            self.rounds += 1

    def scores(self, temperature):
        return self.engine.scores(temperature)

    def visits(self):
        return self.engine.root_visits()


class _TagReady:
    """Readiness of a one-call round: its ring slot's word 3 holds the round's tag (stored by k_scan or k_round1
    after the counts, which are drained first), polled like an event."""
    __slots__ = ("buf", "tag")

    def __init__(self, buf, tag):
        self.buf, self.tag = buf, tag

    def query(self):
        return int(self.buf[3]) == self.tag


class _Lane:
    """One engine + its stream, input buffer and evaluator."""

    def __init__(self, slots, evaluate_count, device, cache_log2, cache_clear_every, own_stream):
        self.engine = Engine(slots, evaluate_count, device)
        if cache_log2:
            self.engine.set_cache(cache_log2, cache_clear_every)
        # lanes run on their engines' own streams: streams created later (e.g. from
        # torch's pool) can share one of the few hardware queues and serialize
        self.stream = self.engine.own_stream() if own_stream else None
        dev = torch.device("cuda", self.engine.device)
        self.x = torch.zeros((slots, 3, 9, 9), dtype=torch.float32, device=dev)
        self.evaluator = None
        self.rounds = 0
        self.finished = 0
        self.count_ring = None  # pinned counts of the rounds in flight (async rounds, Engine.count_copy)
        self.ring_pos = 0
        self.spec = True        # enqueue the next round's network before its count is known
        self._no_rows = None
        self.leaves = 0         # pending leaves of this lane's rounds (the rows its evaluator was asked for)

    def no_rows(self):
        """(policy, value) device buffers for an apply with no pending leaf (nothing is read)."""
        if self._no_rows is None:
            dev = torch.device("cuda", self.engine.device)
            self._no_rows = (torch.zeros((1, 81), dtype=torch.float32, device=dev),
                             torch.zeros((1,), dtype=torch.float32, device=dev))
        return self._no_rows

    def use_stream(self):
        self.engine.use_stream(self.stream)


class SelfPlay:
    """Concurrent self-play of games [begin, end) with `slots` trees in flight.

    Game g draws its moves from numpy's legacy MT19937 seeded seed_base + g, so
    its record equals self_play_cpp.play after np.random.seed(seed_base + g)
    (same model), independent of slot count, shard or GPU count.

    lanes > 1 splits the slots (and the game range) over that many engines, each
    on its own HIP stream with its own evaluator. A step round-robins the lanes:
    while the host waits for one lane's pending count, the other lanes' network
    evaluations run, and their convolution kernels fill each other's partial
    last waves on the GPU. Records are unchanged (each game depends only on its id)."""

    def __init__(self, slots, evaluate_count=50, batch_size=8, temperature=1.0, device=None, evaluator=None,
                 model=None, cache_log2=None, cache_clear_every=0, lanes=1, evaluator_kind=None, symmetry=None,
                 root_noise=None, temperature_plies=None, late_temperature=0.0, tree_reuse=False):
        """root_noise: None or (epsilon, alpha[, seed]), Dirichlet noise on every move's root priors, keyed by the
        global game id and the ply (Engine.set_root_noise). temperature_plies: moves from that ply on use
        late_temperature instead of temperature (Engine.set_temperature_schedule). tree_reuse: every move's search
        starts from the subtree under the move just played and tops the root up to evaluate_count visits
        (Engine.set_tree_reuse). All off by default."""
        self.tree_reuse = bool(tree_reuse)
        from .noise import parse_root_noise, parse_temperature_plies
        self.root_noise = parse_root_noise(root_noise)
        self.temperature_plies, self.late_temperature = parse_temperature_plies(temperature_plies, late_temperature)
        if lanes < 1 or slots % lanes:
            raise ValueError("slots must be a positive multiple of lanes")
        per = slots // lanes
        if cache_log2 is None:  # ~2048 entries per slot (2^23 = 3 GB of HBM for 4096 games)
            cache_log2 = min(23, max(12, int(math.ceil(math.log2(max(per, 1)))) + 11))
        self.lanes = []
        for i in range(lanes):
            self.lanes.append(_Lane(per, evaluate_count, device, cache_log2 if i == 0 else 0, cache_clear_every,
                                    lanes > 1))
            if i and cache_log2:  # one table for all lanes: games in different lanes share positions
                self.lanes[i].engine.share_cache(self.lanes[0].engine)
        for ln in self.lanes:  # the same settings on every lane's engine: a game's record does not see its lane
            if self.root_noise is not None:
                ln.engine.set_root_noise(*self.root_noise)
            if self.temperature_plies is not None:
                ln.engine.set_temperature_schedule(self.temperature_plies, self.late_temperature)
            if self.tree_reuse:
                ln.engine.set_tree_reuse(True)
        self.engine = self.lanes[0].engine
        self.x = self.lanes[0].x
        self.slots = slots
        self.evaluate_count = evaluate_count
        self.batch_size = batch_size
        self.temperature = temperature
        if evaluator is None and model is not None:
            self.set_evaluator(model_evaluator_factory(model, evaluator_kind, symmetry))
        elif parse_symmetry(symmetry) is not None:
            raise ValueError("symmetry applies to the model's evaluator: wrap your own in SymmetricLeaves")
        elif evaluator is None:
            self.set_evaluator(HashEvaluator)
        else:
            self.evaluator = evaluator
        self.sims = 0
        self.moves = 0
        self.cache_clear_every = cache_clear_every  # periodic clears need the blocking move boundary
        # rounds without a per-round host sync when every lane's evaluator reads the count on
        # the device (FusedNetworkEvaluator); UTTT_ASYNC_ROUNDS=0 keeps the blocking loop
        self.async_rounds = os.environ.get("UTTT_ASYNC_ROUNDS", "1") != "0"

    # one evaluator object per lane (each owns its buffers); with one lane the
    # attribute form is kept for compatibility
    def set_evaluator(self, make):
        """make(engine) -> evaluator, called once per lane. A new evaluator may compute other
        values: the shared evaluation table is cleared (its owner is lane 0)."""
        for ln in self.lanes:
            ln.evaluator = make(ln.engine)
        self.lanes[0].engine.cache_clear()

    @property
    def evaluator(self):
        return self.lanes[0].evaluator

    @evaluator.setter
    def evaluator(self, ev):
        if len(self.lanes) > 1:
            raise ValueError("with lanes > 1 use set_evaluator(make) (one evaluator per lane)")
        self.lanes[0].evaluator = ev

    @property
    def rounds(self):
        return sum(ln.rounds for ln in self.lanes)

    @property
    def finished(self):
        return sum(ln.finished for ln in self.lanes)

    @property
    def leaves(self):
        """Pending leaves of all rounds the device-count loop (steps) read back."""
        return sum(ln.leaves for ln in self.lanes)

    def _ctx(self, ln):
        return torch.cuda.stream(ln.stream) if ln.stream is not None else contextlib.nullcontext()

    def begin(self, game_begin, game_end, seed_base, arena_plies=None):
        n = len(self.lanes)
        span = game_end - game_begin
        for i, ln in enumerate(self.lanes):
            gb = game_begin + span * i // n
            ge = game_begin + span * (i + 1) // n
            if ln.stream is None:
                ln.engine.use_stream()
            else:
                ln.use_stream()
            with self._ctx(ln):
                ln.engine.selfplay_begin(gb, ge, seed_base, self.temperature, self.evaluate_count, self.batch_size,
                                         arena_plies if arena_plies is None else -(-arena_plies // n))
            ln.rounds = ln.finished = 0
        self.sims = self.moves = 0

    def _device_count(self):
        return (self.async_rounds and not self.cache_clear_every and
                all(getattr(ln.evaluator, "device_count", False) for ln in self.lanes))

    def step(self):
        """One move for every live game. Returns the simulations it ran (0 = all games over)."""
        if self._device_count():
            return self.steps(1)
        live = []
        for ln in self.lanes:
            with self._ctx(ln):
                live.append(ln.engine.move_begin())
        active = [ln for ln, n in zip(self.lanes, live) if n > 0]
        if not active:
            return 0
        queue = collections.deque(active)
        while queue:
            ln = queue.popleft()
            e = ln.engine
            with self._ctx(ln):
                x = ln.x if getattr(ln.evaluator, "needs_input", True) else None
                n = e.select(x)  # waits for this lane's previous round only
                if n == 0:
                    continue
                p, v = ln.evaluator(ln.x, n)
                e.apply(p, v)
                ln.rounds += 1
            queue.append(ln)
        for ln in active:
            with self._ctx(ln):
                ln.finished = ln.engine.move_end()
        self.moves += 1
        done = sum(live) * self.evaluate_count
        self.sims += done
        return done

    def steps(self, k=None, progress=None):
        """k moves of every lane (None: until every lane's games are over); returns the
        simulations run. With device-count evaluators (FusedNetworkEvaluator) the lanes are
        pipelined. A round's select, network and apply are enqueued without a host sync (the
        pending count stays on the device, Engine.select_async), and the host reads each round's
        counts back - a pinned copy right after the select's scan - only to decide whether to
        enqueue the next round (some tree has simulations left after this one) or end the move,
        while the current round's network still runs; so each lane's stream always holds work
        and no round is enqueued that would find nothing. A lane's move end and its next move's
        roots are enqueued the same way (Engine.move_end_async / move_begin_async; the counters
        are read when they have landed), so no lane idles at a move boundary, neither for the
        host nor for the other lane. Per lane the select launches
        are the blocking loop's minus its final empty one, each game depends only on its id,
        and every lane plays exactly k moves:
        records and totals are those of k lockstep steps (UTTT_ASYNC_ROUNDS=0)."""
        if not self._device_count():
            total, i = 0, 0
            while k is None or i < k:
                d = self.step()
                if d == 0:
                    break
                total += d
                i += 1
                if progress:
                    progress(self.finished, None)
            return total
        depth = self._lookahead()
        if (len(self.lanes) == 1 and depth > 1 and os.environ.get("UTTT_MOVE_LOOP", "1") != "0"
                and getattr(self.lanes[0].evaluator, "round_move", None) is not None
                and getattr(self.lanes[0].evaluator, "rounds_per_call", 1) == 1):
            return self._steps_move_loop(self.lanes[0], k, depth, progress)
        spin = depth > 1
        for ln in self.lanes:
            if ln.count_ring is None:
                ln.count_ring = ln.engine.count_ring()  # the scan writes each round's counts here
            r = getattr(ln.evaluator, "rounds_per_call", 1)
            if len(ln.count_ring) < (depth + 1) * r and not (r > 1 and len(ln.count_ring) >= depth * r):
                raise ValueError(f"round look-ahead {depth} x {r} rounds per call needs more count slots")

        def fill(ln, q):
            # rounds in flight per lane: one (the next is enqueued once this one's count is read), or,
            # with a cheap evaluator, `depth`: the host's reaction then hides under the GPU's work; a
            # round enqueued past the move's last finds every tree done and changes nothing
            while len(q) < depth:
                q.append(self._enqueue_round(ln, ln.spec if depth == 1 else True))
            return q

        state = {}
        for ln in self.lanes:
            with self._ctx(ln):
                live = ln.engine.move_begin()  # the first move of the call: blocking, gives the live count
            if live > 0:
                ln.cur_live = live
                ln.moves_left = k
                ln.result_pending = False
                state[id(ln)] = (ln, fill(ln, collections.deque()))
        total = moves = 0
        while state:
            # serve whichever lane's oldest round count has landed (polling: waiting on one lane in
            # turn would leave the other lane's stream empty once it runs ahead)
            ready = [key for key in state if state[key][1][0][1].query()]
            if not ready:
                # cheap rounds (the hash evaluator, ~30 us each): spin, since a 20-us sleep lasts 60-100 us on
                # Linux and the three rounds in flight drain meanwhile
                if not spin:
                    time.sleep(2e-5)
                continue
            for key in ready:
                ln, q = state[key]
                rc, ev, spec, buf = q.popleft()
                if ln.result_pending:  # the previous move's end: its counters landed before this count
                    ln.finished, ln.cur_live = ln.engine.move_result()
                    ln.result_pending = False
                    if progress:
                        progress(self.finished, None)
                if isinstance(buf, list):  # several rounds per call: leaves summed, the last round's `left`
                    n, more = sum(int(b[0]) for b in buf), int(buf[-1][2])
                else:
                    n, more = int(buf[0]), int(buf[2])
                rc.n = n
                ln.leaves += n
                if n > 0:
                    ln.rounds += 1
                if not spec:  # the network was held back until the count was known
                    with self._ctx(ln):
                        if n > 0:
                            p, v = ln.evaluator(None, rc)
                            ln.engine.apply(p, v)
                        else:
                            ln.engine.apply(*ln.no_rows())
                ln.spec = n > 0  # a round with leaves predicts another
                if ln.cur_live == 0:  # every game of the lane is over: this move was empty
                    # the rounds queued behind this one found no live tree either: their counts are 0
                    # (left unread, a RoundCount raises when a caller later sizes a batch by it)
                    for rc_empty, *_ in q:
                        rc_empty.n = 0
                    q.clear()
                    del state[key]
                    continue
                if more > 0:  # some tree has simulations left once this round is applied
                    fill(ln, q)
                    continue
                # this round completes the move (the rounds already enqueued behind it are empty: no
                # tree has a simulation left, so their counts are 0): end it and begin the next, both on
                # the stream, without waiting
                for rc_empty, *_ in q:
                    rc_empty.n = 0
                q.clear()
                total += ln.cur_live * self.evaluate_count
                moves += 1
                ln.moves_left = None if ln.moves_left is None else ln.moves_left - 1
                with self._ctx(ln):
                    ln.engine.move_end_async()
                    ln.result_pending = True
                    if ln.moves_left == 0:
                        ev_end = torch.cuda.Event()
                        ev_end.record()
                        ln.end_event = ev_end
                        del state[key]
                        continue
                    ln.engine.move_begin_async()
                fill(ln, q)
        for ln in self.lanes:  # the last move's counters
            if getattr(ln, "result_pending", False):
                ln.end_event.synchronize()
                ln.finished, ln.cur_live = ln.engine.move_result()
                ln.result_pending = False
                if progress:
                    progress(self.finished, None)
        self.moves += moves / len(self.lanes)
        self.sims += total
        return total

    def _steps_move_loop(self, ln, k, depth, progress):
        """steps() for one lane whose evaluator runs a move's rounds in one C call (HashEvaluator.round_move,
        round 6: tree-only self-play was bound by the host's per-round Python; UTTT_MOVE_LOOP=0 keeps the
        Python round loop). Per move: the round loop in C (`depth` rounds in flight, spinning on their tags),
        then the move's end and the next move's roots enqueued without waiting; the previous move's counters
        are read once the next move's first count has landed (its end ran before it on the stream). Same
        rounds, records and totals as the Python loop."""
        e = ln.engine
        if ln.count_ring is None:
            ln.count_ring = e.count_ring()
        with self._ctx(ln):
            live = e.move_begin()  # the first move of the call: blocking, gives the live count
        if live <= 0:
            return 0
        ln.cur_live = live
        total = moves = 0
        pending = False  # a move's end enqueued whose counters were not read yet
        while k is None or moves < k:
            n_rounds, leaves, with_leaves = ln.evaluator.round_move(e, ln.ring_pos % len(ln.count_ring), depth)
            ln.ring_pos += n_rounds
            if pending:  # the previous move's end ran before this move's first round
                ln.finished, ln.cur_live = e.move_result()
                pending = False
                if progress:
                    progress(self.finished, None)
            if ln.cur_live == 0:  # every game of the lane is over: this move was empty
                break
            ln.leaves += leaves
            ln.rounds += with_leaves
            total += ln.cur_live * self.evaluate_count
            moves += 1
            e.move_end_async()
            pending = True
            if k is not None and moves == k:
                break
            e.move_begin_async()
        if pending:
            with self._ctx(ln):
                ev = torch.cuda.Event()
                ev.record()
            ev.synchronize()
            ln.finished, ln.cur_live = e.move_result()
            if progress:
                progress(self.finished, None)
        self.moves += moves
        self.sims += total
        return total

    def _lookahead(self):
        """Rounds in flight per lane: UTTT_ROUND_LOOKAHEAD, else 3 when every lane's evaluator is cheap
        (the device hash evaluator: a round's kernels take about as long as the host's reaction to its
        count, so with one round in flight the GPU idled between rounds; with the fused rounds three in
        flight beat two in 3 of 3 interleaved runs, 395M against 387M sims/s,
        profiles/r5/ab/tree_shape/), else 1 (a network round is milliseconds: the host keeps up, and an
        empty look-ahead round would cost its 32 conv launches)."""
        env = os.environ.get("UTTT_ROUND_LOOKAHEAD")
        if env:
            return max(1, int(env))
        if not all(getattr(ln.evaluator, "cheap", False) for ln in self.lanes):
            return 1
        # calls in flight: their rounds' ring slots must not be reused before the call is read (8 slots)
        r = max(getattr(ln.evaluator, "rounds_per_call", 1) for ln in self.lanes)
        return 3 if r == 1 else max(1, 8 // r)

    def _enqueue_round(self, ln, spec):
        """Select of one round on the lane's stream, its counts stored by the scan into a slot of the
        engine's host count ring (no copy operation), and - speculatively, when the lane's previous round had leaves (always,
        with look-ahead) - the network and apply, all without a host sync. Otherwise (a lane whose
        rounds are answered by the cache or by terminal positions: the network would run empty) the
        host enqueues the network once the count shows leaves."""
        rc = RoundCount()
        slot = ln.ring_pos % len(ln.count_ring)
        buf = ln.count_ring[slot]
        one_call = getattr(ln.evaluator, "round_async", None)
        if spec and one_call is not None:
            # whole rounds in one C call, on the engine's stream; readiness is the tag the last round stores
            # into its ring slot after the counts (no event, no torch stream context per round). With several
            # rounds per call, the counts of the call's slots are summed (the last one's `left` decides)
            r = getattr(ln.evaluator, "rounds_per_call", 1)
            ln.ring_pos += r
            slots = [ln.count_ring[(slot + i) % len(ln.count_ring)] for i in range(r)]
            last = slots[-1]
            return rc, _TagReady(last, one_call(ln.engine, slot)), spec, (slots if r > 1 else last)
        ln.ring_pos += 1
        with self._ctx(ln):
            # readiness: the tag the scan stores into the ring slot after the counts (round 5; a torch event
            # per round before)
            ready = _TagReady(buf, ln.engine.select_async_tag(slot))
            if spec:
                p, v = ln.evaluator(None, rc)
                ln.engine.apply(p, v)
        return rc, ready, spec, buf

    def run(self, game_begin, game_end, seed_base, progress=None):
        self.begin(game_begin, game_end, seed_base)
        t0 = time.time()
        self.steps(None, (lambda f, _: progress(f, game_end - game_begin)) if progress else None)
        return time.time() - t0

    def kernel_stats(self, name):
        out = {"ms": 0.0, "launches": 0, "bytes": 0}
        for ln in self.lanes:
            st = ln.engine.kernel_stats(name)
            for k in out:
                out[k] += st[k]
        return out

    def cache_stats(self):
        out = {"hits": 0, "misses": 0, "inserts": 0, "replacements": 0}
        for ln in self.lanes:
            st = ln.engine.cache_stats()
            for k in out:
                out[k] += st[k]
        return out

    def set_timing(self, on=True):
        for ln in self.lanes:
            ln.engine.set_timing(on)

    def reset_stats(self):
        for ln in self.lanes:
            ln.engine.reset_stats()

    def records(self, with_inputs=True):
        """Finished games sorted by id: dict of per-game lists."""
        out = []
        for ln in self.lanes:
            ids, off, ln_ = ln.engine.games()
            pl = ln.engine.plies(with_inputs)
            for g, o, n in zip(ids.tolist(), off.tolist(), ln_.tolist()):
                rec = {"game": g, "actions": pl["actions"][o:o + n].astype(np.int64),
                       "policies": pl["policies"][o:o + n], "values": pl["values"][o:o + n].astype(np.int64),
                       "states": pl["states"][o:o + n]}
                if with_inputs:
                    rec["inputs"] = pl["inputs_hwc"][o:o + n].reshape(n, 9, 9, 3)
                out.append(rec)
        out.sort(key=lambda r: r["game"])
        return out


def default_lanes(slots):
    """Lanes the drop-ins use: two engines on two streams once the per-lane batch stays large
    (Lanes), one below that."""
    return 2 if slots >= 1024 and slots % 2 == 0 else 1


def history_from_records(records):
    """The reference .history schema (self_play_cpp.py:59, :95-99): a flat list of
    [input (9,9,3) f32, policy (81,) f64, value int] over games in id order."""
    hist = []
    for r in records:
        for i in range(len(r["actions"])):
            hist.append([r["inputs"][i], r["policies"][i], int(r["values"][i])])
    return hist


__all__ = ["BatchedSearch", "SelfPlay", "HashEvaluator", "PlayoutEvaluator", "NetworkEvaluator", "history_from_records",
           "initial_states", "model_evaluator_factory", "default_lanes", "SymmetricLeaves", "parse_symmetry",
           "symmetry_from_env", "with_symmetry"]
