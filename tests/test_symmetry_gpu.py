"""GPU tests of the board symmetries (k_sym_leaves, k_sym_rows, uttt_nn_stem_states_dev, SymmetricLeaves; DESIGN.md
6e): the kernels against the host transform bit for bit on the pending leaves of a stopped search; searches and
cached searches with SymmetricLeaves(HashEvaluator) against the CPU oracle, whose evaluator callback rebuilds the
leaf from its network input, applies the host transform (checked on its own against numpy's rot90 / fliplr in
test_symmetry_host.py), evaluates the hash evaluator on the image and maps the row back; the fused network through
the wrapper against forward_states of the transformed states, bit for bit; self-play on the device-count path
against the blocking loop; the overlay on top; refused bases and bad arguments."""
import ctypes
import random

import numpy as np
import pytest

from test_playout_gpu import _pack, _state_from_input

pytestmark = pytest.mark.gpu

WAVES_PER_BLOCK = 4  # csrc/engine/layout.h kWavesPerBlock: one wave per leaf
N_TAIL = 4 * WAVES_PER_BLOCK + 1
SEED = 0xC0FFEE


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import uttt_amd
    return uttt_amd


@pytest.fixture(scope="module")
def roots(oracle_lib):
    """N_TAIL non-terminal positions at mixed depths, the initial position first; some with a free move."""
    rng = random.Random(41)
    out = [oracle_lib.OrState.initial()]
    while len(out) < N_TAIL:
        s = oracle_lib.OrState.initial()
        while len(out) < N_TAIL:
            s = s.next(rng.choice(s.legal_actions()))
            if s.is_done():
                break
            if rng.random() < 0.1:
                out.append(s)
    packed = _pack(out)
    assert (packed["active"][1:] == -1).any() and (packed["active"] >= 0).any()
    return packed, out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _nchw(lib, states):
    from uttt_amd._lib import UtttState
    out = np.zeros((len(states), 9, 9, 3), np.float32)
    assert lib.uttt_states_input_hwc(states.ctypes.data_as(ctypes.POINTER(UtttState)), len(states),
                                     out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))) == 0
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2))


def _stopped(gpu, roots, n):
    """An engine of N_TAIL trees whose search of n roots stopped after one select: (engine, leaves, their input)."""
    import torch
    packed = roots[0]
    eng = gpu.Engine(N_TAIL, 50)
    eng.search_begin(packed[:n] if n != 5 else packed[N_TAIL - 5:], 50, 8)
    x = torch.zeros((N_TAIL, 3, 9, 9), device="cuda")
    assert eng.select(x) == n
    st, _ = eng.pending()
    assert len(st) == n
    return eng, st, x[:n].cpu().numpy()


@pytest.mark.parametrize("n", [1, 5, N_TAIL])
def test_kernels_equal_host(gpu, engine_lib, roots, n):
    """A lone wave, a partial workgroup, a grid tail: fixed g for each of 0..7 and the hashed choice."""
    import torch
    from uttt_amd import symmetry
    from uttt_amd._lib import STATE_DTYPE
    eng, st, x = _stopped(gpu, roots, n)
    assert np.array_equal(x, _nchw(engine_lib, st))
    rng = np.random.RandomState(n)
    cases = [("fixed", g) for g in range(8)] + [("hashed", SEED), ("hashed", 0)]
    for ci, (mode, arg) in enumerate(cases):
        d_st = torch.full((N_TAIL, 8), -7, dtype=torch.int32, device="cuda")
        d_sym = torch.full((N_TAIL,), 99, dtype=torch.int8, device="cuda")
        d_x = torch.full((N_TAIL, 3, 9, 9), 5.0, device="cuda")
        eng.sym_pending_dev(mode, arg, d_st, d_sym, d_x)
        want_sym = np.full(n, arg, np.int8) if mode == "fixed" else symmetry.hashed_symmetry(st, arg)
        want_st = symmetry.transform_states(st, want_sym)
        torch.cuda.synchronize()
        got_st = d_st.cpu().numpy()
        assert got_st[:n].tobytes() == want_st.tobytes(), (n, mode, arg)
        assert (got_st[n:] == -7).all()
        assert d_sym.cpu().numpy()[:n].tolist() == want_sym.tolist() and (d_sym.cpu().numpy()[n:] == 99).all()
        if d_x is not None:
            got_x = d_x.cpu().numpy()
            assert np.array_equal(_bits(got_x[:n]), _bits(symmetry.transform_inputs(x, want_sym))), (n, mode, arg)
            assert np.array_equal(got_x[:n], _nchw(engine_lib, want_st))
            assert (got_x[n:] == 5.0).all()
        # the rows mapped back: leading dimension 81 and 96, a copy, an accumulation, a final scale
        for ld in (81, 96):
            for accumulate, scale in ((False, 1.0), (True, 1.0), (True, 0.125), (False, 0.5)):
                p = (rng.rand(N_TAIL, ld).astype(np.float32) * 2 - 1)
                v = (rng.rand(N_TAIL, 2).astype(np.float32) * 2 - 1)
                o_p = (rng.rand(N_TAIL, ld).astype(np.float32) * 2 - 1)
                o_v = (rng.rand(N_TAIL, 2).astype(np.float32) * 2 - 1)
                p[0, 3] = -0.0  # a copy keeps the sign of zero
                d_p, d_v, d_op, d_ov = (torch.from_numpy(a).cuda() for a in (p, v, o_p, o_v))
                # value rows two floats apart with ld 96, a (rows, 1) column otherwise
                v_in = d_v[:, 0] if ld == 96 else d_v[:, :1].contiguous()
                v_out = d_ov[:, 0] if ld == 96 else d_ov[:, :1].contiguous()
                eng.sym_rows_dev(d_sym, d_p, v_in, d_op, v_out, accumulate, scale)
                want_p, want_v = o_p.copy(), o_v[:, 0].copy()
                back = symmetry.policy_from_image(p[:n, :81], want_sym)
                vals = v[:n, 0]
                if accumulate:
                    back = want_p[:n, :81] + back
                    vals = want_v[:n] + vals
                if scale != 1.0:
                    back = back * np.float32(scale)
                    vals = vals * np.float32(scale)
                want_p[:n, :81] = back
                want_v[:n] = vals
                torch.cuda.synchronize()
                assert np.array_equal(_bits(d_op.cpu().numpy()), _bits(want_p)), (n, mode, arg, ld, accumulate, scale)
                got_v = d_ov.cpu().numpy()[:, 0] if ld == 96 else v_out.cpu().numpy()[:, 0]
                assert np.array_equal(_bits(got_v), _bits(want_v)), (n, mode, arg, ld, accumulate, scale)
                if ld == 96:
                    assert np.array_equal(d_ov.cpu().numpy()[:, 1], o_v[:, 1])
    assert eng.kernel_stats("sym_leaves")["launches"] == len(cases)
    assert eng.kernel_stats("sym_rows")["launches"] == len(cases) * 8
    eng.close()


def test_bad_arguments(gpu, roots):
    import torch
    eng, st, _ = _stopped(gpu, roots, 5)
    T = N_TAIL
    d_st = torch.zeros((T, 8), dtype=torch.int32, device="cuda")
    d_sym = torch.zeros((T,), dtype=torch.int8, device="cuda")
    p, v = torch.zeros((T, 81), device="cuda"), torch.zeros((T, 1), device="cuda")
    o_p, o_v = torch.zeros((T, 81), device="cuda"), torch.zeros((T, 1), device="cuda")
    for mode, arg in (("random", 0), ("fixed", 8), ("fixed", -1), (0, 0)):
        with pytest.raises(ValueError):
            eng.sym_pending_dev(mode, arg, d_st, d_sym)
    with pytest.raises(ValueError):
        eng.sym_pending_dev("fixed", 1, d_st[:T - 1], d_sym)  # fewer states than trees
    with pytest.raises(ValueError):
        eng.sym_pending_dev("fixed", 1, d_st, d_sym.to(torch.int32))
    with pytest.raises(ValueError):
        eng.sym_pending_dev("fixed", 1, d_st, d_sym, torch.zeros((T - 1, 3, 9, 9), device="cuda"))
    with pytest.raises(ValueError):
        eng.sym_rows_dev(d_sym, torch.zeros((T, 80), device="cuda"), v, o_p, o_v)  # policy_ld 80
    with pytest.raises(ValueError):
        eng.sym_rows_dev(d_sym, torch.zeros((T, 96), device="cuda")[:, :80], v, o_p, o_v)  # rows 96 apart, 80 wide
    with pytest.raises(ValueError):
        eng.sym_rows_dev(d_sym, p, torch.zeros((T + 1, 1), device="cuda"), o_p, o_v)
    with pytest.raises(ValueError):
        eng.sym_rows_dev(d_sym, p, torch.zeros((T, 2), device="cuda"), o_p, o_v)
    with pytest.raises(ValueError):
        eng.sym_rows_dev(d_sym, p, v, p, o_v)  # in place
    both = torch.zeros((T + 1, 81), device="cuda")
    with pytest.raises(ValueError):
        eng.sym_rows_dev(d_sym, both[:T], v, both[1:], o_v)  # the output one row into the input
    with pytest.raises(ValueError):
        eng.sym_rows_dev(d_sym, p, v, o_p, v[:, 0])  # the value column written over itself
    with pytest.raises(ValueError):
        eng.sym_rows_dev(d_sym, p[:4], v[:4], o_p[:4], o_v[:4])  # fewer rows than pending leaves
    with pytest.raises(ValueError):
        eng.sym_rows_dev(d_sym[:3], p, v, o_p, o_v)
    # the C ABI's own checks (what another binding would meet)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    lib = eng.lib
    assert lib.uttt_sym_pending_dev(eng.h, 2, 0, vp(d_st), vp(d_sym), None) == -1
    assert lib.uttt_sym_pending_dev(eng.h, 0, 8, vp(d_st), vp(d_sym), None) == -1
    assert lib.uttt_sym_pending_dev(eng.h, 0, 1, None, vp(d_sym), None) == -1
    assert lib.uttt_sym_rows_dev(eng.h, vp(d_sym), vp(p), 80, vp(v), 1, vp(o_p), 81, vp(o_v), 1, 0, 1.0) == -1
    assert lib.uttt_sym_rows_dev(eng.h, vp(d_sym), vp(p), 81, vp(v), 0, vp(o_p), 81, vp(o_v), 1, 0, 1.0) == -1
    assert lib.uttt_sym_rows_dev(eng.h, vp(d_sym), vp(p), 81, vp(v), 1, vp(p), 81, vp(o_v), 1, 0, 1.0) == -1
    assert lib.uttt_sym_rows_dev(eng.h, None, vp(p), 81, vp(v), 1, vp(o_p), 81, vp(o_v), 1, 0, 1.0) == -1
    assert lib.uttt_sym_rows_dev(eng.h, vp(d_sym), vp(both), 81, vp(v), 1, vp(both[1:]), 81, vp(o_v), 1, 0, 1.0) == -1
    assert b"overlap" in lib.uttt_last_error()
    assert lib.uttt_sym_rows_dev(None, vp(d_sym), vp(p), 81, vp(v), 1, vp(o_p), 81, vp(o_v), 1, 0, 1.0) == -1
    assert b"null pointer" in lib.uttt_last_error()
    for mode in ("random", 8, -1, 2.5, True):
        with pytest.raises(ValueError):
            gpu.SymmetricLeaves(gpu.HashEvaluator(eng), eng, mode)
    eng.close()


def test_refused_bases(gpu, roots):
    from uttt_amd.engine import RoundCount
    eng, _, _ = _stopped(gpu, roots, 5)
    hash_ev = gpu.HashEvaluator(eng)
    for base in (gpu.PlayoutEvaluator(eng, 8, 0), gpu.SolvedLeaves(hash_ev, eng),
                 gpu.SymmetricLeaves(hash_ev, eng, 1)):
        with pytest.raises(TypeError, match=type(base).__name__):
            gpu.SymmetricLeaves(base, eng)
    ev = gpu.SymmetricLeaves(hash_ev, eng, "hashed")
    assert ev.device_count is False and ev.needs_input is False
    assert not any(hasattr(ev, a) for a in ("round_async", "round_move", "cheap", "rounds_per_call"))
    with pytest.raises(TypeError, match="HashEvaluator"):  # its device-count path reads the engine's own leaves
        ev(None, RoundCount())
    eng.close()


def _sym_callback(lib, mode, seed):
    """The oracle's evaluator: the leaf rebuilt from its input, transformed on the host, the hash evaluator on the
    image's input, the row mapped back in numpy f32."""
    from oracle import hashnp
    from uttt_amd import symmetry

    def one(st, g):
        pol, val = hashnp.hash_eval_np(_nchw(lib, symmetry.transform_states(st, g))[0])
        return pol[symmetry.ACTION_PERM[g]], np.float32(val)

    def cb(x):
        st = _state_from_input(x)
        if mode == "average":
            acc, vacc = one(st, 0)
            for g in range(1, 8):
                pol, val = one(st, g)
                acc = acc + pol
                vacc = np.float32(vacc + val)
            return acc * np.float32(0.125), np.float32(vacc * np.float32(0.125))
        g = int(symmetry.hashed_symmetry(st, seed)[0]) if mode == "hashed" else mode
        return one(st, g)

    return cb


def _oracle_visits(core, cb, ostate, sims, batch, semantics):
    if semantics == "cpp":
        return core.pv_mcts_scores(ostate, 1.0, sims, batch, cb)[1]
    return core.pv_mcts_scores_py_callback(ostate, 0.0, sims, batch, cb)[1]


@pytest.mark.parametrize("semantics", ["cpp", "py"])
@pytest.mark.parametrize("mode", ["hashed", "average", 3])
def test_search_matches_oracle(gpu, engine_lib, oracle_lib, roots, mode, semantics):
    packed, oroots = roots[0][:8], roots[1][:8]
    bs = gpu.BatchedSearch(8, 50)
    ev = gpu.SymmetricLeaves(gpu.HashEvaluator(bs.engine), bs.engine, mode, seed=SEED)
    cb = _sym_callback(engine_lib, mode, SEED)
    bs.run(packed, ev, 50, 8, semantics)
    visits, L = bs.visits()
    for i, s in enumerate(oroots):
        vi = _oracle_visits(oracle_lib, cb, s, 50, 8, semantics)
        assert L[i] == vi.size and np.array_equal(visits[i, :L[i]], vi), (mode, semantics, i)
    assert bs.engine.kernel_stats("sym_leaves")["launches"] == bs.rounds * (8 if mode == "average" else 1)
    assert bs.engine.kernel_stats("encode")["launches"] == 0  # the wrapper builds the images' input itself
    if mode == "hashed":  # not the plain evaluator's search
        plain = gpu.BatchedSearch(8, 50)
        plain.run(packed, gpu.HashEvaluator(plain.engine), 50, 8, semantics)
        assert not np.array_equal(plain.visits()[0], visits)


@pytest.mark.parametrize("mode", ["hashed", "average"])
def test_cache_is_exact(gpu, roots, mode):
    """The wrapped evaluator is a function of position, mode and seed: searches resolved from the evaluation table
    give the uncached visits."""
    packed = roots[0][:8]
    out = []
    for cache in (0, 12):
        bs = gpu.BatchedSearch(8, 50, cache_log2=cache)
        ev = gpu.SymmetricLeaves(gpu.HashEvaluator(bs.engine), bs.engine, mode, seed=SEED)
        for _ in range(2):
            bs.run(packed, ev, 50, 8)
            out.append(bs.visits()[0].copy())
        if cache:
            assert bs.engine.cache_stats()["hits"] > 0
    for v in out[1:]:
        assert np.array_equal(v, out[0])
    assert (out[0].sum(axis=1) == 50).all()


@pytest.fixture(scope="module")
def network(gpu):
    from uttt_amd.model import random_network
    return random_network(0, "cuda")


@pytest.mark.parametrize("softmax", [False, True])
def test_fused_network_rows(gpu, roots, network, softmax):
    """17 leaves through the wrapper equal forward_states of the host-transformed states mapped back in numpy, bit
    for bit (every NN kernel computes a board from its own inputs only): fixed, hashed, and the average as eight
    such results accumulated in f32 in order and scaled by 0.125. Host count and device count."""
    import torch
    from uttt_amd import symmetry
    from uttt_amd.engine import RoundCount
    from uttt_amd.nnfast import FusedNetworkEvaluator
    eng, st, _ = _stopped(gpu, roots, N_TAIL)
    fe = FusedNetworkEvaluator(network, eng)

    def ref(sym):
        p, v = fe.forward_states(symmetry.transform_states(st, sym), softmax=softmax)
        return symmetry.policy_from_image(p.cpu().numpy(), sym), v.cpu().numpy().copy()

    want = {}
    for mode in (3, 6, "hashed"):
        sym = np.full(N_TAIL, mode, np.int8) if mode != "hashed" else symmetry.hashed_symmetry(st, SEED)
        want[mode] = ref(sym)
    acc, vacc = ref(np.zeros(N_TAIL, np.int8))
    for g in range(1, 8):
        p, v = ref(np.full(N_TAIL, g, np.int8))
        acc, vacc = acc + p, vacc + v
    want["average"] = (acc * np.float32(0.125), vacc * np.float32(0.125))
    assert len(set(symmetry.hashed_symmetry(st, SEED).tolist())) > 2
    for mode, (wp, wv) in want.items():
        ev = gpu.SymmetricLeaves(fe, eng, mode, seed=SEED, softmax=softmax)
        assert ev.device_count is True and ev.needs_input is False
        for n in (N_TAIL, RoundCount()):  # the count on the host, then read on the device
            ev.policy.fill_(7.0)
            ev.value.fill_(7.0)
            p, v = ev(None, n)
            torch.cuda.synchronize()
            assert np.array_equal(_bits(p.cpu().numpy()[:N_TAIL]), _bits(wp)), (mode, softmax, type(n))
            assert np.array_equal(_bits(v.cpu().numpy()[:N_TAIL, 0]), _bits(wv)), (mode, softmax, type(n))
    assert not np.array_equal(want[3][0], want[6][0])
    eng.close()


def test_selfplay_device_count_equals_blocking(gpu, network, monkeypatch):
    """16 games x 8 simulations on two lanes with SymmetricLeaves(Fused, "hashed"): the pipelined device-count
    rounds give the blocking loop's records."""
    from uttt_amd.nnfast import FusedNetworkEvaluator
    recs = []
    for async_rounds in ("1", "0"):
        monkeypatch.setenv("UTTT_ASYNC_ROUNDS", async_rounds)
        sp = gpu.SelfPlay(16, 8, 8, 1.0, lanes=2)
        sp.set_evaluator(lambda eng: gpu.SymmetricLeaves(FusedNetworkEvaluator(network, eng), eng, "hashed", seed=SEED))
        assert sp._device_count() is (async_rounds == "1")
        sp.run(0, 16, 77)
        recs.append(sp.records())
        assert sp.kernel_stats("sym_leaves")["launches"] > 0
        assert sp.kernel_stats("sym_leaves")["launches"] == sp.kernel_stats("sym_rows")["launches"]
        for ln in sp.lanes:
            ln.engine.close()
    a, b = recs
    assert [r["game"] for r in a] == [r["game"] for r in b] == list(range(16))
    assert all(len(r["actions"]) >= 17 for r in a)  # whole games: no game ends before its 17th ply
    for ra, rb in zip(a, b):
        assert np.array_equal(ra["actions"], rb["actions"])
        assert np.array_equal(ra["policies"].view(np.uint64), rb["policies"].view(np.uint64))
        assert np.array_equal(ra["values"], rb["values"])


def test_overlay_on_top_and_factories(gpu, roots, network):
    """SolvedLeaves(SymmetricLeaves(...)) runs, the overlay last; the opt-in plumbing builds the wrapper."""
    from uttt_amd import arena
    from uttt_amd.selfplay import model_evaluator_factory, parse_symmetry
    packed = roots[0][:8]
    bs = gpu.BatchedSearch(8, 50)
    inner = gpu.SymmetricLeaves(gpu.HashEvaluator(bs.engine), bs.engine, "hashed", seed=SEED)
    ev = gpu.SolvedLeaves(inner, bs.engine, max_empties=10, max_nodes=256)
    assert ev.needs_input is False and ev.device_count is False
    bs.run(packed, ev, 50, 8)
    assert (bs.visits()[0].sum(axis=1) == 50).all()
    assert sum(ev.counts().values()) > 0 and bs.engine.kernel_stats("sym_rows")["launches"] == bs.rounds
    assert parse_symmetry(None) is None and parse_symmetry("off") is None
    assert parse_symmetry("hashed:12") == ("hashed", 12) and parse_symmetry("5") == (5, 0)
    assert parse_symmetry("average") == ("average", 0) and parse_symmetry(7) == (7, 0)
    for bad in ("8", "mirror", -1, "hashed:x", ("mirror", 0), ("hashed",)):
        with pytest.raises(ValueError):
            parse_symmetry(bad)
    assert parse_symmetry(("off", 3)) is None and parse_symmetry(("hashed", 3)) == ("hashed", 3)
    plain = model_evaluator_factory(network)(bs.engine)
    wrapped = model_evaluator_factory(network, symmetry="average")(bs.engine)
    assert not isinstance(plain, gpu.SymmetricLeaves)
    assert isinstance(wrapped, gpu.SymmetricLeaves) and wrapped.mode == "average" and wrapped.device_count
    w2 = arena.model_evaluator(network, 8, bs.engine, symmetry="2:9")
    assert isinstance(w2, gpu.SymmetricLeaves) and (w2.mode, w2.seed) == (2, 9)
    assert not isinstance(arena.model_evaluator(network, 8, bs.engine), gpu.SymmetricLeaves)
    torch_ev = arena.model_evaluator(network, 8, bs.engine, kind="torch", symmetry="hashed")
    assert isinstance(torch_ev, gpu.SymmetricLeaves) and torch_ev.device_count is False
    bs.run(packed, torch_ev, 8, 8)  # a base called with the wrapper's own input buffer
    assert (bs.visits()[0].sum(axis=1) == 8).all()


def test_graphed_training_with_augment(gpu, engine_lib, roots):
    """train_network(augment=True) on the HIP-graph step: the captured step indexes the tensors EpochAugmenter
    rewrites in place, so the losses are deterministic under the seed, differ from augment=False, and each epoch's
    resident tensors are the transform of the pristine ones by that epoch's draw."""
    import torch
    from uttt_amd import symmetry, train
    from uttt_amd.model import DualNetwork
    packed = roots[0][:16]
    x = _nchw(engine_lib, packed).transpose(0, 2, 3, 1)
    rng = np.random.RandomState(6)
    hist = []
    for i in range(16):
        legal = np.nonzero(x[i, :, :, 2].reshape(81))[0]
        pol = np.zeros(81, np.float64)
        pol[rng.choice(legal, min(4, len(legal)), replace=False)] = 1.0
        hist.append([x[i], pol / pol.sum(), int(rng.randint(-1, 2))])
    x0, p0, _ = train.history_arrays(hist)
    seen = []
    orig = train.EpochAugmenter.epoch

    def spy(self, epoch):
        orig(self, epoch)
        seen.append((self.sym.clone(), self.x.cpu().numpy(), self.p.cpu().numpy(), self.x0.cpu().numpy()))

    def run(augment):
        torch.manual_seed(0)
        net = DualNetwork(filters=8, residual_num=1)
        return train.train_network(net, hist, epochs=3, batch_size=8, device=torch.device("cuda"), seed=5, log=None,
                                   graph=True, tune=False, augment=augment)

    train.EpochAugmenter.epoch = spy
    try:
        la, lb, ln = run(True), run(True), run(False)
    finally:
        train.EpochAugmenter.epoch = orig
    assert la == lb and la != ln and all(np.isfinite(la)), (la, lb, ln)
    assert len(seen) == 6
    for s, xe, pe, xk in seen[:3]:
        assert np.array_equal(xk, x0)
        assert np.array_equal(xe, symmetry.transform_inputs(x0, s.numpy()))
        assert np.array_equal(pe, symmetry.transform_policy(p0, s.numpy()))
    assert not torch.equal(seen[0][0], seen[1][0])
