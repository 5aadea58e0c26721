"""The residual-tower conv (csrc/wino3h_conv.hip, csrc/wino3h_impl.h) at its numerical edges, against an
f64 direct conv on the CPU: inputs that reach the transform's growth bound max|V| = 36 max|x|, the switch
points of the per-board power-of-two scale, boards whose maximum is 0, one bound for all boards, the cleared
max row, the device-resident board count, weights far from unit scale, and values that are not finite.

The bar is the project's own: error at most 1e-5 of each board's output maximum, and the
y_amax row equal to max(y) per board exactly. Every case runs plain and with a residual at n = 1, 5, 8, 29
boards: the channel-split kernel (up to 28 boards) and the persistent kernel, full and partial 7-board groups.
B^T is written here from the Toom-Cook points {0, 1, -1, 2, inf}, not read from the kernel's header."""
import copy
import ctypes

import numpy as np
import pytest

from conftest import GOLDEN, golden

pytestmark = pytest.mark.gpu

NS = (1, 5, 8, 29)
NMAX = max(NS)
POINTS = (0.0, 1.0, -1.0, 2.0)  # + the point at infinity
SENTINEL = 0x7FC5A5A5  # a NaN bit pattern, as int32


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import uttt_amd
    return uttt_amd


def toom_cook_bt():
    """Row i of a finite point: the coefficients (ascending) of prod_{j != i} (x - p_j); the point at
    infinity's row: those of prod_j (x - p_j)."""
    rows = [np.concatenate([np.poly([q for j, q in enumerate(POINTS) if j != i])[::-1], [0.0]]) for i in range(4)]
    rows.append(np.poly(POINTS)[::-1])
    return np.array(rows, np.float64)


class Conv:
    """One folded conv of random_network(3) on the device, and the raw C entries."""

    def __init__(self, blk_i=5, which=1):
        import torch
        from uttt_amd import _lib
        from uttt_amd.model import fold_bn, random_network
        from uttt_amd.nnfast import wino3h_weights
        blk = random_network(3).residual_blocks[blk_i]
        self.w, self.b = fold_bn(*((blk.conv1, blk.bn1) if which == 1 else (blk.conv2, blk.bn2)))
        u, self.su = wino3h_weights(self.w)
        self.u, self.bd = u.cuda(), self.b.cuda()
        self.lib = _lib.load()
        self.torch = torch

    def scaled(self, k):
        """The same conv with weights and bias times 2^k (exact)."""
        from uttt_amd.nnfast import wino3h_weights
        c = copy.copy(self)
        c.w, c.b = self.w * 2.0 ** k, self.b * 2.0 ** k
        u, c.su = wino3h_weights(c.w)
        c.u, c.bd = u.cuda(), c.b.cuda()
        return c

    def with_bias(self, b):
        c = copy.copy(self)
        c.b, c.bd = b, b.cuda()
        return c

    def ref(self, x, res=None):
        """relu(conv3x3(x) + b (+ res)) in f64 on the CPU; x, res (n,81,128) f32 (any device)."""
        import torch.nn.functional as F
        n = x.shape[0]
        xn = x.detach().cpu().double().reshape(n, 9, 9, 128).permute(0, 3, 1, 2)
        y = F.conv2d(xn, self.w.double(), self.b.double(), padding=1).permute(0, 2, 3, 1).reshape(n, 81, 128)
        return y if res is None else y + res.detach().cpu().double()

    def raw(self, x, res, y, x_amax, per_board, y_amax, clear=None, clear_count=0, n=None, n_dev=None, max_boards=None,
            precision="f32"):
        """The C entry's return code (host count n, or device count n_dev with max_boards)."""
        torch = self.torch
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        head = (p(x), p(self.u), ctypes.c_float(self.su), p(self.bd), p(res), p(y), p(x_amax), per_board, p(y_amax),
                p(clear), clear_count)
        if n_dev is not None:
            fn = self.lib.uttt_nn_conv3x3_wino3h_f16_dev if precision == "f16" else self.lib.uttt_nn_conv3x3_wino3h_dev
            return fn(*head, p(n_dev), max_boards, st)
        fn = self.lib.uttt_nn_conv3x3_wino3h_f16 if precision == "f16" else self.lib.uttt_nn_conv3x3_wino3h
        return fn(*head, x.shape[0] if n is None else n, st)

    def run(self, x, res=None, x_amax=None, per_board=1, precision="f32"):
        """(y, y_amax row as f32) of the host-count entry; x_amax defaults to board_amax(x)."""
        from uttt_amd.nnfast import board_amax
        torch = self.torch
        y = torch.full_like(x, float("nan"))
        ya = torch.zeros(x.shape[0], dtype=torch.int32, device="cuda")
        xa = board_amax(x) if x_amax is None else x_amax
        assert self.raw(x, res, y, xa, per_board, ya, precision=precision) == 0
        return y, ya.view(torch.float32)


@pytest.fixture(scope="module")
def conv(gpu):
    return Conv()


@pytest.fixture(scope="module")
def conv2(gpu):
    """Another conv, for the second of two chained ones."""
    return Conv(7, 2)


def within_bar(y, ya, want64, what, bar=1e-5):
    """Every output finite, within `bar` of its board's output maximum, and the max row exact."""
    import torch
    n = y.shape[0]
    want = torch.relu(want64)
    assert torch.isfinite(y).all(), what
    err = (y.cpu().double() - want).abs().reshape(n, -1).amax(dim=1)
    scale = want.reshape(n, -1).amax(dim=1).clamp_min(1e-300)
    worst = float((err / scale).max())
    print(f"{what}: worst error / board max = {worst:.3e}")
    assert worst <= bar, (what, worst)
    assert torch.equal(ya, y.reshape(n, -1).amax(dim=1)), what


def plain_and_residual(n, res):
    return ((None, "plain"), (res[:n].contiguous(), "residual"))


# ---- 1. the growth bound -------------------------------------------------------------------------------------

def saturating_boards(amax, seed=0):
    """(NMAX, 81, 128) f32 boards of maximum `amax` whose centre tile (window rows and columns 2..6, all
    interior) reaches |V| = 36 amax at several of the 25 points at once: on three channels per board the
    window is amax sign(B^T[i][a]) sign(B^T[j][b]) for three different row pairs (i, j) of absolute row sum 6;
    everything else is 0.1 amax randn."""
    import torch
    BT = toom_cook_bt()
    six = [i for i in range(5) if np.abs(BT[i]).sum() == 6.0]
    assert six == [0, 2, 4]
    pairs = [(i, j) for i in six for j in six]
    g = torch.Generator().manual_seed(seed)
    amax = np.float32(amax)
    x = (torch.randn(NMAX, 9, 9, 128, generator=g) * 0.1).numpy() * amax
    used = []
    for b in range(NMAX):
        pts = []
        for k in range(3):
            i, j = pairs[(b + 4 * k) % 9]
            ch = (37 * b + 43 * k + 5) % 128  # all three differ (43k mod 128 distinct), spread over the chunks
            x[b, 2:7, 2:7, ch] = amax * np.outer(np.sign(BT[i]), np.sign(BT[j])).astype(np.float32)
            pts.append(5 * i + j)
        used.append(pts)
    assert x.dtype == np.float32 and np.isfinite(x).all() and np.abs(x).max() == amax
    # the premise, in f64: the centre tile's V attains 36 amax at those points, and nothing exceeds it
    V = np.einsum("ia,nabc,jb->nijc", BT, x[:, 2:7, 2:7, :].astype(np.float64), BT)
    for b in range(NMAX):
        for k, pt in enumerate(used[b]):
            v = np.abs(V[b, pt // 5, pt % 5]).max()
            assert abs(v - 36.0 * float(amax)) <= 1e-12 * 36.0 * float(amax), (b, pt, v)
        assert len(set(used[b])) == 3
    assert np.abs(V).max() <= 36.0 * float(amax) * (1 + 1e-12)
    return torch.from_numpy(x.reshape(NMAX, 81, 128))


def switch_point(k):
    """The two neighbouring f32 maxima between which 36.0f * amax (f32, as pow2_scale forms it) crosses 2^k."""
    f36 = np.float32(36.0)
    a = np.float32(2.0 ** k / 36.0)
    while f36 * a >= np.float32(2.0 ** k):
        a = np.nextafter(a, np.float32(0))
    while f36 * np.nextafter(a, np.float32(np.inf)) < np.float32(2.0 ** k):
        a = np.nextafter(a, np.float32(np.inf))
    below, above = a, np.nextafter(a, np.float32(np.inf))
    assert np.frexp(f36 * below)[1] == k and np.frexp(f36 * above)[1] == k + 1  # different scale exponents
    return float(below), float(above)


GROWTH = [("1.0", 1.0), ("1e30", 1e30)] + [(f"2^{k}{side}", switch_point(k)[i]) for k in (-3, 0, 10)
                                            for i, side in enumerate(("-", "+"))]


@pytest.mark.parametrize("amax", [a for _, a in GROWTH], ids=[i for i, _ in GROWTH])
def test_growth_bound_is_reached(conv, amax):
    """Signed inputs that attain max|V| = 36 max|x| (asserted in f64 on the CPU first): V then fills the f16
    range the scale was chosen for, at unit scale, at 1e30, and on both sides of three points where the scale
    steps. Outputs finite and within the bar."""
    import torch
    x = saturating_boards(amax)
    g = torch.Generator().manual_seed(11)
    res = torch.randn(NMAX, 81, 128, generator=g) * float(np.float32(amax))
    want = conv.ref(x), conv.ref(x, res)
    xd, rd = x.cuda(), res.cuda()
    for n in NS:
        for i, (r, name) in enumerate(plain_and_residual(n, rd)):
            y, ya = conv.run(xd[:n].contiguous(), r)
            within_bar(y, ya, want[i][:n], f"growth amax={amax!r} n={n} {name}")


# ---- 2. zero maxima ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ordinary(gpu):
    """(x, residual) of NMAX ordinary boards: relu(randn), randn."""
    import torch
    g = torch.Generator().manual_seed(5)
    return torch.relu(torch.randn(NMAX, 81, 128, generator=g)), torch.randn(NMAX, 81, 128, generator=g)


def test_zero_board_among_ordinary_boards(conv, ordinary):
    """A board of zeros has x_amax 0 and scale 1; its output is relu(bias (+ residual)) bit for bit
    (fmaf(0, inv, b) is b) and its y_amax entry that maximum; the other boards meet the bar."""
    import torch
    x, res = ordinary
    for n in NS:
        z = n // 2
        xz = x[:n].clone()
        xz[z] = 0.0
        want = conv.ref(xz), conv.ref(xz, res[:n])
        xd = xz.cuda()
        for i, (r, name) in enumerate(plain_and_residual(n, res.cuda())):
            y, ya = conv.run(xd, r)
            within_bar(y, ya, want[i], f"zero board n={n} {name}")
            exact = torch.relu(conv.bd.expand(81, 128) + (r[z] if r is not None else 0.0))
            assert torch.equal(y[z], exact), (n, name)
            assert ya[z].item() == exact.max().item()


def test_all_zero_output_rotates_into_the_next_conv(conv, conv2, ordinary):
    """A conv with bias -1e3 on every channel and no residual: the ordinary boards' whole output is 0 and their
    y_amax entries stay 0 (every third board is scaled up until it has outputs, so both kinds share a batch).
    The next conv, chained on y with that row as its x_amax as the evaluator's rotation does, meets the bar."""
    import torch
    x, res = ordinary
    x = x.clone()
    x[2::3] *= 3e4
    first = conv.with_bias(torch.full((128,), -1e3))
    second = conv2
    want1 = first.ref(x)
    for n in NS:
        xd = x[:n].cuda()
        y1, ya1 = first.run(xd)
        within_bar(y1, ya1, want1[:n], f"bias -1e3 n={n}", bar=1e-5)
        dead = [b for b in range(n) if b % 3 != 2]
        assert not y1[dead].any() and not ya1[dead].view(torch.int32).any()
        live = [b for b in range(n) if b % 3 == 2]
        assert all(ya1[b].item() > 0 for b in live)
        want2 = second.ref(y1), second.ref(y1, res[:n])
        for i, (r, name) in enumerate(plain_and_residual(n, res.cuda())):
            y2, ya2 = second.run(y1, r, x_amax=ya1.view(torch.int32))
            within_bar(y2, ya2, want2[i], f"chained on zero boards n={n} {name}")
            if r is None and dead:
                assert torch.equal(y2[dead[0]], torch.relu(second.bd).expand(81, 128))


# ---- 3. one bound for all boards -----------------------------------------------------------------------------

def bracket_top(bound):
    """The largest f32 bound whose 36.0f * bound has the same binary exponent as 36.0f * `bound`."""
    f36, b = np.float32(36.0), np.float32(bound)
    e = np.frexp(f36 * b)[1]
    t = np.float32(2.0 ** e / 36.0)
    while np.frexp(f36 * t)[1] > e:
        t = np.nextafter(t, np.float32(0))
    while np.frexp(f36 * np.nextafter(t, np.float32(np.inf)))[1] == e:
        t = np.nextafter(t, np.float32(np.inf))
    assert t >= b and np.frexp(f36 * t)[1] == e
    return float(t)


def test_one_bound_for_all_boards(conv, ordinary):
    """x_amax_per_board = 0 (the stem's form): one bound of 1x, 7.3x and 1000x the true maximum. Every run is
    within the bar, and two bounds of one power-of-two bracket (the bound and its bracket's top) give the same
    bits; the three factors themselves fall in three different brackets."""
    import torch
    x, res = ordinary
    want = conv.ref(x), conv.ref(x, res)
    f36 = np.float32(36.0)
    for n in NS:
        xd = x[:n].cuda()
        true_max = float(xd.abs().max())
        bounds = [float(np.float32(f * true_max)) for f in (1.0, 7.3, 1000.0)]
        assert len({int(np.frexp(f36 * np.float32(b))[1]) for b in bounds}) == 3
        for i, (r, name) in enumerate(plain_and_residual(n, res.cuda())):
            for b in bounds:
                ys = []
                for bound in (b, bracket_top(b)):
                    xa = torch.tensor([bound], dtype=torch.float32, device="cuda").view(torch.int32)
                    y, ya = conv.run(xd, r, x_amax=xa, per_board=0)
                    within_bar(y, ya, want[i][:n], f"one bound {bound!r} n={n} {name}")
                    ys.append(y)
                assert torch.equal(ys[0], ys[1]), (n, name, b)


# ---- 4. amax_clear -------------------------------------------------------------------------------------------

def test_amax_clear(conv, ordinary):
    """clear_count = m < the row's length zeroes entries [0, m) and leaves the rest, for any board count, 0
    included (the early return needs both counts 0); the cleared row may not be x_amax or y_amax."""
    import torch
    from uttt_amd.nnfast import board_amax
    x, _ = ordinary
    L, m = 700, 613  # more entries than one workgroup has threads
    for n in (0,) + NS:
        xd = x[:max(n, 1)].cuda()
        y = torch.empty_like(xd)
        ya = torch.zeros(NMAX, dtype=torch.int32, device="cuda")
        row = torch.full((L,), SENTINEL, dtype=torch.int32, device="cuda")
        assert conv.raw(xd, None, y, board_amax(xd), 1, ya, clear=row, clear_count=m, n=n) == 0
        assert not row[:m].any() and (row[m:] == SENTINEL).all(), n
        if n == 0:
            assert not ya.any()
    xa = board_amax(xd)
    ya = torch.zeros(NMAX, dtype=torch.int32, device="cuda")
    for alias in (xa, ya):
        assert conv.raw(xd, None, y, xa, 1, ya, clear=alias, clear_count=1, n=xd.shape[0]) == -1  # UTTT_ERR_ARG
    assert conv.raw(xd, None, y, xa, 1, ya, clear=None, clear_count=1, n=xd.shape[0]) == -1


# ---- 5. the device-resident count ----------------------------------------------------------------------------

def test_device_count(conv, ordinary):
    """uttt_nn_conv3x3_wino3h_dev with max_boards = 29: rows of y and y_amax past min(*n_dev, 29) keep a sentinel
    bit pattern; the rows before it are the host-count call's bits."""
    import torch
    from uttt_amd.nnfast import board_amax
    x, res = ordinary
    xd, rd = x.cuda(), res.cuda()
    xa = board_amax(xd)
    for nd in (0, 1, 8, 29, 40):
        cnt = min(nd, NMAX)
        n_dev = torch.tensor([nd], dtype=torch.int32, device="cuda")
        for r in (None, rd):
            y = torch.full((NMAX, 81, 128), SENTINEL, dtype=torch.int32, device="cuda")
            ya = torch.full((NMAX,), SENTINEL, dtype=torch.int32, device="cuda")
            ya[:cnt] = 0
            assert conv.raw(xd, r, y.view(torch.float32), xa, 1, ya, n_dev=n_dev, max_boards=NMAX) == 0
            assert (y[cnt:] == SENTINEL).all() and (ya[cnt:] == SENTINEL).all(), nd
            if cnt:
                yh, yah = conv.run(xd[:cnt].contiguous(), r[:cnt].contiguous() if r is not None else None)
                assert torch.equal(y[:cnt], yh.view(torch.int32)), nd
                assert torch.equal(ya[:cnt], yah.view(torch.int32)), nd


# ---- 6. weight scale -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [-40, 40])
def test_weight_scale_is_an_exact_power_of_two(conv, ordinary, k):
    """Weights, bias and residual times 2^k: the same U bits with u_scale times 2^-k (the host test's
    invariance), so every output is the unscaled run's times 2^k exactly."""
    import torch
    x, res = ordinary
    sc = conv.scaled(k)
    assert torch.equal(sc.u, conv.u) and sc.su == conv.su * 2.0 ** -k
    for n in NS:
        xd = x[:n].cuda()
        for r, name in plain_and_residual(n, res.cuda()):
            y0, ya0 = conv.run(xd, r)
            y1, ya1 = sc.run(xd, r * 2.0 ** k if r is not None else None)
            assert torch.equal(y1, y0 * 2.0 ** k), (n, name)
            assert torch.equal(ya1, ya0 * 2.0 ** k), (n, name)


# ---- 7. non-finite values ------------------------------------------------------------------------------------

BAD = (3, 6, 9)  # batch rows of the three bad boards (row 3 lies in both sets of its group)


def boards_with_bad_values(ordinary):
    import torch
    x, res = ordinary
    good = [b for b in range(11) if b not in BAD]
    xb = x[:11].clone()
    xb[BAD[0], 4 * 9 + 4, 17] = float("inf")  # one +Inf at an interior position
    xb[BAD[1], 2 * 9 + 7, 90] = float("nan")  # one NaN
    xb[BAD[2]] *= 1e37 / float(xb[BAD[2]].max())  # finite, maximum 1e37: 36 max|x| >= 3e38
    assert torch.isfinite(xb[BAD[2]]).all() and abs(float(xb[BAD[2]].max()) / 1e37 - 1) < 1e-6
    return xb, res[:11].clone(), good


def run_bad_boards(conv, second, ordinary, precision, split):
    """First conv on 8 ordinary + 3 bad boards, then a second chained on it with y_amax as its x_amax; the
    same two convs on the 8 ordinary boards alone. Returns per stage (y of all, y of the ordinary alone)."""
    import torch
    from uttt_amd.nnfast import set_conv_split
    xb, res, good = boards_with_bad_values(ordinary)
    out = {}
    set_conv_split(split)
    try:
        for r, name in ((None, "plain"), (res.cuda(), "residual")):
            rg = r[good].contiguous() if r is not None else None
            y1, ya1 = conv.run(xb.cuda(), r, precision=precision)
            g1, ga1 = conv.run(xb[good].cuda(), rg, precision=precision)
            y2, _ = second.run(y1, r, x_amax=ya1.view(torch.int32), precision=precision)
            g2, _ = second.run(g1, rg, x_amax=ga1.view(torch.int32), precision=precision)
            out[name] = ((y1, g1), (y2, g2))
    finally:
        set_conv_split(-1)
    return out, good


KERNELS = [("f32", -1), ("f32", 1), ("f16", -1), ("f16", 1)]  # split -1: the channel-split kernel; 1: the persistent one


@pytest.mark.parametrize("precision,split", KERNELS)
def test_bad_boards_leave_the_others_alone(conv, conv2, ordinary, precision, split):
    """An Inf, a NaN or a maximum of 1e37 on three boards: the 8 ordinary boards' outputs are bit-equal to a
    run without those boards, through two chained convs."""
    import torch
    out, good = run_bad_boards(conv, conv2, ordinary, precision, split)
    for name, stages in out.items():
        for s, (y, g) in enumerate(stages):
            assert torch.isfinite(g).all()
            assert torch.equal(y[good], g), (name, s)


@pytest.mark.parametrize("precision,split", KERNELS)
def test_nonfinite_values_pass_through(conv, conv2, ordinary, precision, split):
    """The same three boards each leave the conv with at least one non-finite output (the ReLU keeps NaN), and
    still do after a second conv chained on the result with y_amax as its x_amax."""
    import torch
    out, _ = run_bad_boards(conv, conv2, ordinary, precision, split)
    for name, stages in out.items():
        for s, (y, _) in enumerate(stages):
            for b in BAD:
                assert not torch.isfinite(y[b]).all(), (name, "conv", s + 1, "board", b)


def test_evaluator_returns_nonfinite_rows_outside_the_tower_domain(gpu):
    """End to end: the calibrated network with one tower weight (of a deep copy) so large that the tower's
    activations leave the conv's domain 36 max|x| < 3e38. The evaluator must return non-finite policy or value
    rows (what the engine refuses, test_nonfinite_evaluator_output_is_refused), not finite ones from zeros.
    The weight is 1e37: with 1e30 the activations stay near 5e30 through the whole tower (measured on the
    PyTorch network on the CPU), inside the domain, where the PyTorch network's outputs are finite too."""
    import torch
    from uttt_amd._lib import STATE_DTYPE
    from uttt_amd.model import calibrated_network
    from uttt_amd.nnfast import FusedNetworkEvaluator
    d, r = golden("netcal.npz"), golden("rules.npz")
    idx = d["rules_index"][:8]
    states = np.zeros(len(idx), STATE_DTYPE)
    for j, i in enumerate(idx):
        p, e = r["pieces"][i].astype(np.uint32), r["enemy"][i].astype(np.uint32)
        for a in range(81):
            states["own"][j, a // 27] |= p[a] << (a % 27)
            states["opp"][j, a // 27] |= e[a] << (a % 27)
        states["mains"][j] = sum(int(r["main_p"][i][b]) << b for b in range(9)) | \
            sum(int(r["main_e"][i][b]) << (16 + b) for b in range(9))
        states["active"][j] = r["active"][i]
    net = copy.deepcopy(calibrated_network(GOLDEN + "/netcal.npz", "cpu"))
    with torch.no_grad():
        net.residual_blocks[0].conv1.weight[5, 7, 1, 1] = 1e37
        # the premise, on the PyTorch network: the first conv's output is finite, and on some boards (those
        # whose stem output is not zero all over the weight's input channel) outside the next conv's domain
        x = torch.from_numpy(d["x"][:8].astype(np.float32))
        blk = net.residual_blocks[0]
        t = torch.relu(blk.bn1(blk.conv1(torch.relu(net.bn_input(net.conv_input(x))))))
        outside = (t.reshape(8, -1).amax(dim=1) * 36.0 >= 3e38)
        assert torch.isfinite(t).all() and outside.any()
    fe = FusedNetworkEvaluator(net.cuda().eval(), None, max_batch=8)
    p, v = fe.forward_states(states)
    bad = ~(torch.isfinite(p).all(dim=1) & torch.isfinite(v)).cpu()
    print("boards outside the domain:", outside.tolist(), "non-finite rows:", bad.tolist())
    assert bad[outside].all(), (outside, bad)
