"""The tower conv's index tables (csrc/wino3h_impl.h: the staging and transform indices a workgroup builds
once in LDS instead of recomputing them per chunk) change integer addressing only, so every output bit and
every y_amax row must equal what the kernel gave before the tables existed.

tests/golden/conv_index_tables.npz was recorded on the GPU from the commit before the tables: block 8's
conv1 of random_network(0) on seeded relu(randn) inputs with per-board maxima from board_amax, plain and
residual, at 1, 3, 4, 7, 8, 15 boards (one set; the board-3 seam shared by a group's two sets; a full group
with its empty 64th slot; a partial second group; all on the <= 28-board k_wino3s_conv path) and at 29 and
36 boards (the persistent k_wino3h_conv path; 36 boards add a sixth group holding a single board). The
outputs of all 103 boards in both forms are 8.5 MB, so the fixture keeps one SHA-256 digest per board of
the output bits (equal digests = equal bits; a mismatch names the board) and the y_amax rows themselves;
it also keeps digests of the inputs and weights, so a change of the seeded inputs is told apart from a
change of the kernel."""
import ctypes
import hashlib

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

SMALL = (1, 3, 4, 7, 8, 15)
PERSISTENT = (29, 36)
FIXTURE = "conv_index_tables.npz"


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import uttt_amd
    return uttt_amd


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).digest()


def board_digests(y):
    a = np.ascontiguousarray(y.detach().cpu().numpy())
    return np.stack([np.frombuffer(hashlib.sha256(a[i].tobytes()).digest(), np.uint8) for i in range(a.shape[0])])


_WEIGHTS = None


def weights():
    """(u, su, bias) of block 8's conv1 of random_network(0), on the device; built once."""
    global _WEIGHTS
    if _WEIGHTS is None:
        from uttt_amd.model import fold_bn, random_network
        from uttt_amd.nnfast import wino3h_weights
        net = random_network(0)
        w, b = fold_bn(net.residual_blocks[8].conv1, net.residual_blocks[8].bn1)
        u, su = wino3h_weights(w)
        _WEIGHTS = (u.cuda(), su, b.cuda())
    return _WEIGHTS


def inputs(n):
    """Seeded relu(randn) input and residual of n boards (CPU generator: the same values everywhere)."""
    import torch
    g = torch.Generator().manual_seed(1000 + n)
    x = torch.relu(torch.randn(n, 81, 128, generator=g))
    r = torch.relu(torch.randn(n, 81, 128, generator=g))
    return x.cuda(), r.cuda()


def run_conv(n, residual):
    """-> (y, y_amax row) of the product launch for n boards."""
    import torch
    from uttt_amd.nnfast import board_amax, conv3x3_wino3h
    u, su, b = weights()
    x, r = inputs(n)
    ya = torch.zeros(n, dtype=torch.int32, device="cuda")
    y = conv3x3_wino3h(x, u, su, b, r if residual else None, y_amax=ya, x_amax=board_amax(x))
    torch.cuda.synchronize()
    return y, ya


def record():
    """The fixture's arrays from the library that is loaded (run on the commit before the tables)."""
    u, su, b = weights()
    out = {"u_sha": np.frombuffer(sha(u), np.uint8), "su": np.float32(su)}
    for n in SMALL + PERSISTENT:
        x, r = inputs(n)
        out[f"x_sha_{n}"] = np.frombuffer(sha(x), np.uint8)
        out[f"r_sha_{n}"] = np.frombuffer(sha(r), np.uint8)
        for residual in (False, True):
            y, ya = run_conv(n, residual)
            key = f"{n}{'r' if residual else 'p'}"
            out[f"y_sha_{key}"] = board_digests(y)
            out[f"amax_{key}"] = ya.cpu().numpy()
    return out


def check_case(d, n, residual, what):
    u, su, _ = weights()
    x, r = inputs(n)
    assert sha(u) == d["u_sha"].tobytes() and np.float32(su) == d["su"], "weights differ from the recorded ones"
    assert sha(x) == d[f"x_sha_{n}"].tobytes() and sha(r) == d[f"r_sha_{n}"].tobytes(), \
        "seeded inputs differ from the recorded ones"
    y, ya = run_conv(n, residual)
    key = f"{n}{'r' if residual else 'p'}"
    bad = np.nonzero((board_digests(y) != d[f"y_sha_{key}"]).any(axis=1))[0]
    assert bad.size == 0, f"{what}: output bits of boards {bad.tolist()} of {n} changed"
    assert np.array_equal(ya.cpu().numpy(), d[f"amax_{key}"]), f"{what}: y_amax row of {n} boards changed"
    # the row is max(y) per board exactly
    assert np.array_equal(ya.cpu().numpy(), y.reshape(n, -1).amax(dim=1).view(ya.dtype).cpu().numpy())


@pytest.mark.parametrize("residual", (False, True), ids=("plain", "residual"))
@pytest.mark.parametrize("n", SMALL)
def test_small_batches_keep_the_recorded_bits(gpu, n, residual):
    check_case(golden(FIXTURE), n, residual, "k_wino3s_conv")


@pytest.mark.parametrize("residual", (False, True), ids=("plain", "residual"))
@pytest.mark.parametrize("n", PERSISTENT)
def test_persistent_kernel_keeps_the_recorded_bits_across_sets(gpu, n, residual):
    """29 and 36 boards take k_wino3h_conv (9 and 11 sets). With one workgroup per set a workgroup never
    meets a second set, so the launch is also run with 3 and with 2 workgroups (uttt_nn_wino3h_set_grid):
    with 3 every workgroup walks sets of both halves h (0, 3, 6, ...), with 2 each stays in one half; the
    tables built in the prologue must serve every set."""
    from uttt_amd import _lib
    lib = _lib.load()
    d = golden(FIXTURE)
    try:
        for grid in (0, 3, 2):
            _lib.check(lib.uttt_nn_wino3h_set_grid(grid))
            check_case(d, n, residual, f"k_wino3h_conv, grid {grid or 'default'}")
    finally:
        _lib.check(lib.uttt_nn_wino3h_set_grid(0))


def test_dataflow_tower_on_8_boards_equals_per_conv_launches(gpu):
    """k_wino3t_tower shares the staging and the transform: on 8 boards' stem outputs (two groups, the second
    of one board and one set) its final activation equals the 32 per-conv launches' bit for bit."""
    import torch
    from uttt_amd import _lib
    from uttt_amd.model import random_network
    from uttt_amd.nnfast import FusedNetworkEvaluator, _p
    lib = _lib.load()
    # 8 positions along a fixed line of play
    st = _lib.UtttState()
    lib.uttt_state_initial(ctypes.byref(st))
    states = np.zeros(8, _lib.STATE_DTYPE)
    for i, a in enumerate((40, 36, 4, 37, 13, 41, 49, 38)):
        states[i] = np.frombuffer(bytes(st), _lib.STATE_DTYPE)[0]
        nx = _lib.UtttState()
        assert lib.uttt_state_next(ctypes.byref(st), a, ctypes.byref(nx)) == 0
        st = nx
    net = random_network(0, "cuda")
    fl = FusedNetworkEvaluator(net, None, max_batch=8, tower="layers")
    fd = FusedNetworkEvaluator(net, None, max_batch=8, tower="dataflow")
    fl.forward_states(states)
    a0 = fl.buf[0].clone()
    assert float(a0.abs().max()) > 0.0
    for rep in range(2):  # both counter blocks
        dev = torch.from_numpy(states.view(np.int32).reshape(8, 8).copy()).cuda()
        _lib.check(lib.uttt_nn_stem_states(_p(dev), 8, _p(fd.stem_w), _p(fd.stem_b), _p(fd.buf[0]), fd._stream()))
        fd._tower_dataflow(fd._stream(), None, 8)
        torch.cuda.synchronize()
        assert torch.equal(fd.buf[0], a0), rep
