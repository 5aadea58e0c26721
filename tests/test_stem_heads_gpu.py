"""The network's three small kernels alone, through the raw C entries: k_stem and k_heads (csrc/nn_kernels.hip)
and k_amax (csrc/wino3h_conv.hip). The whole-network comparisons of test_engine_gpu.py put 32 convs' rounding
between the stem and the heads; here each kernel meets an exact model or an f64 reference of its own.

Stem: its inputs are 0/1 planes, so its output is a sum of weight rows in a stated order: a numpy float32 loop
in that order gives the same bits (S2), a 0/1 weight matrix decodes the tap mask it built (S1), and an f64 conv
bounds it by gamma_28 (S3). The reference planes are rules.npz's `tensor` rows, the reference program's own;
they never pass through legal_mask or action_at.

Heads: f64 numpy from the module's tensors (not from the packed block: a packing error is a numerical
failure), with a running error bound derived from the operation counts, u = 2^-24 and
gamma_k = k u / (1 - k u) (H1, H2); no tolerance here is a chosen number.
The two terms that cover the library functions, L_tanh and L_soft, assume 4 ulp for tanhf and 4 ulp for expf:
the HIP math accuracy tables are not part of the ROCm installation this was written against, so the figure is
ASSUMED, NOT MEASURED, and not taken from the kernel's observed error. With ulp <= 2^-23 for a result <= 1:
  L_tanh = 4 * 2^-23;
  L_soft = gamma_K, K = 16 (expf of the numerator and of the sum's terms, 4 ulp = 8 u each)
           + 2 (rounding of z - m in both: |d| e^d u <= u / e on a ratio <= 1) + 80 (the 81-term sum, any order)
           + 1 (the division).

Outputs are pre-filled with a NaN bit pattern and every call's rows past its count must still hold it."""
import copy
import ctypes

import numpy as np
import pytest

from conftest import GOLDEN, golden
from test_engine_gpu import _random_positions, _rules_states

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC5A5A5  # a NaN bit pattern, as int32
U = 2.0 ** -24
ULP1 = 2.0 ** -23  # no result <= 1 has a larger ulp
TANHF_ULP = 4  # assumed (see the module docstring)
EXPF_ULP = 4  # assumed
ERR_ARG = -1


def gamma(k):
    return k * U / (1.0 - k * U)


L_TANH = TANHF_ULP * ULP1
L_SOFT = gamma(2 * EXPF_ULP * 2 + 2 + 80 + 1)


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import uttt_amd
    return uttt_amd


@pytest.fixture(scope="module")
def lib(gpu):
    from uttt_amd import _lib
    return _lib.load()


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(a):
    """float32 numpy array -> its int32 bit patterns."""
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def sentinel(*shape):
    import torch
    return torch.full(shape, SENTINEL, dtype=torch.int32, device="cuda")


# ---- stem: states, planes, weights, model --------------------------------------------------------------------

def choose_rows():
    """About 40 rows of rules.npz chosen by property from the fixture alone -> (row indices, {class: rows})."""
    r = golden("rules.npz")
    hwc = r["tensor"].reshape(-1, 9, 9, 3)
    piece, legal = (hwc[..., 0] | hwc[..., 1]).astype(bool), hwc[..., 2].astype(bool)
    n_legal, active = r["n_legal"], r["active"]
    cls = {"terminal": np.flatnonzero(n_legal == 0)[:2],
           "most legal": np.flatnonzero(n_legal == n_legal.max())[:1],
           "active fixed": np.flatnonzero((active >= 0) & (n_legal > 0))[:2],
           "active free": np.flatnonzero((active < 0) & (n_legal > 0) & (n_legal < n_legal.max()))[:2]}
    where = {"corner 0,0": (slice(0, 1), slice(0, 1)), "corner 0,8": (slice(0, 1), slice(8, 9)),
             "corner 8,0": (slice(8, 9), slice(0, 1)), "corner 8,8": (slice(8, 9), slice(8, 9)),
             "edge top": (slice(0, 1), slice(1, 8)), "edge bottom": (slice(8, 9), slice(1, 8)),
             "edge left": (slice(1, 8), slice(0, 1)), "edge right": (slice(1, 8), slice(8, 9))}
    for name, (rs, cs) in where.items():
        cls["piece " + name] = np.flatnonzero(piece[:, rs, cs].any(axis=(1, 2)))[:1]
        cls["legal " + name] = np.flatnonzero(legal[:, rs, cs].any(axis=(1, 2)) & (n_legal < n_legal.max()))[:1]
    for name, rows in cls.items():
        assert len(rows) > 0, name  # every class is present in the fixture
    idx = list(dict.fromkeys(int(i) for rows in cls.values() for i in rows))
    rng = np.random.default_rng(40)
    for i in rng.permutation(len(n_legal)):
        if len(idx) >= 40:
            break
        if int(i) not in idx:
            idx.append(int(i))
    assert len(idx) == 40
    assert not hwc[cls["terminal"], :, :, 2].any()  # a terminal state's legal plane is empty
    return np.array(idx), cls


def taps_of(planes):
    """(n,9,9,3) 0/1 planes -> (n,9,9,27) bool: tap t = ch*9 + ky*3 + kx of output (R,C) is plane ch at
    (R+ky-1, C+kx-1), 0 outside the board (zero padding and shifting; no conv code)."""
    n = len(planes)
    pad = np.zeros((n, 11, 11, 3), bool)
    pad[:, 1:10, 1:10] = planes.astype(bool)
    out = np.zeros((n, 9, 9, 27), bool)
    for ch in range(3):
        for ky in range(3):
            for kx in range(3):
                out[..., ch * 9 + ky * 3 + kx] = pad[:, ky:ky + 9, kx:kx + 9, ch]
    return out


def stem_model(taps, w, b):
    """The kernel's arithmetic in numpy float32: start from the bias, add the weight rows of the set taps in
    ascending tap order (additions only, no contraction), then a ReLU that keeps NaN. -> (n,81,128) f32."""
    w, b = np.asarray(w, np.float32), np.asarray(b, np.float32)
    acc = np.broadcast_to(b, taps.shape[:3] + (128,)).astype(np.float32).copy()
    with np.errstate(invalid="ignore"):
        for t in range(27):
            acc[taps[..., t]] += w[t]
        out = np.where(~(acc <= 0), acc, np.float32(0))
    assert out.dtype == np.float32
    return out.reshape(len(taps), 81, 128)


def stem_network(kind):
    """random_network(3) as it is initialised ("init": its folded stem bias is 0), or with the input
    BatchNorm's statistics, weight and bias drawn at random ("bn": mixed-sign scales and a bias that matters)."""
    import torch
    from uttt_amd.model import random_network
    net = random_network(3)
    if kind == "bn":
        g = torch.Generator().manual_seed(31)
        bn = net.bn_input
        with torch.no_grad():
            bn.running_mean.copy_(torch.randn(128, generator=g) * 0.5)
            bn.running_var.copy_(torch.rand(128, generator=g) + 0.5)
            bn.weight.copy_(torch.randn(128, generator=g))
            bn.bias.copy_(torch.randn(128, generator=g) * 0.5)
    return net


def stem_weights(net):
    """(w[27][128], b[128]) as nnfast._prepared_weights permutes the folded conv_input."""
    from uttt_amd.model import fold_bn
    sw, sb = fold_bn(net.conv_input, net.bn_input)
    return sw.permute(1, 2, 3, 0).reshape(27, 128).contiguous(), sb.contiguous()


def dev_states(states):
    import torch
    a = np.ascontiguousarray(states).view(np.int32).reshape(len(states), 8).copy()
    return torch.from_numpy(a).cuda()


def run_stem(lib, st_dev, n, w, b):
    """uttt_nn_stem_states on the first n states -> (n,81,128) int32 bits; two more rows keep the sentinel."""
    out = sentinel(n + 2, 81, 128)
    assert lib.uttt_nn_stem_states(P(st_dev), n, P(w), P(b), P(out), stream()) == 0
    assert (out[n:] == SENTINEL).all(), n
    return out[:n].cpu().numpy()


class StemCase:
    def __init__(self, kind):
        idx, self.classes = choose_rows()
        self.planes = golden("rules.npz")["tensor"][idx].reshape(-1, 9, 9, 3)
        self.taps = taps_of(self.planes)
        self.states = dev_states(_rules_states(idx))
        self.net = stem_network(kind)
        self.w, self.b = stem_weights(self.net)
        self.wd, self.bd = self.w.cuda(), self.b.cuda()
        self.model = stem_model(self.taps, self.w.numpy(), self.b.numpy())  # computed once, never changed
        self.model.setflags(write=False)
        self.n = len(idx)


@pytest.fixture(scope="module", params=["init", "bn"])
def stem(request, gpu):
    return StemCase(request.param)


@pytest.fixture(scope="module")
def stem_bn(gpu):
    return StemCase("bn")


# ---- S1 ------------------------------------------------------------------------------------------------------

def test_stem_mask_decode(lib, stem_bn):
    """S1: w[t][c] = (c == t), bias 0: channel t < 27 of every output is exactly the 0/1 value of plane t // 9
    at the tap's shifted position, channels 27..127 exactly 0."""
    import torch
    s = stem_bn
    w = torch.zeros(27, 128)
    w[torch.arange(27), torch.arange(27)] = 1.0
    out = run_stem(lib, s.states, s.n, w.cuda(), torch.zeros(128).cuda()).view(np.float32).reshape(s.n, 9, 9, 128)
    want = np.zeros((s.n, 9, 9, 128), np.float32)
    want[..., :27] = s.taps
    bad = np.argwhere(bits(out) != bits(want))
    assert len(bad) == 0, f"first mismatches (state, R, C, channel = ch*9+ky*3+kx): {bad[:8].tolist()}"


# ---- S2 ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 5, 40])
def test_stem_equals_the_f32_model_bit_for_bit(lib, stem, n):
    """S2: the full and the partial last workgroup (2 states each)."""
    out = run_stem(lib, stem.states, n, stem.wd, stem.bd)
    assert np.isfinite(stem.model).all()
    bad = np.argwhere(out != bits(stem.model[:n]))
    assert len(bad) == 0, f"{len(bad)} outputs differ from the stated summation order; first: {bad[:8].tolist()}"


# ---- S3 ------------------------------------------------------------------------------------------------------

def test_stem_within_gamma28_of_f64_conv(lib, stem):
    """S3: |out - relu(conv2d in f64)| <= gamma_28 (|b_c| + sum over the set taps of |w_tc|); the right side is
    the same conv of |w|, |b|."""
    import torch
    import torch.nn.functional as F
    x = torch.from_numpy(stem.planes.astype(np.float64)).permute(0, 3, 1, 2)
    w4 = stem.w.double().reshape(3, 3, 3, 128).permute(3, 0, 1, 2)  # [co][ch][ky][kx]
    ref = torch.relu(F.conv2d(x, w4, stem.b.double(), padding=1)).permute(0, 2, 3, 1).reshape(stem.n, 81, 128)
    mag = F.conv2d(x, w4.abs(), stem.b.double().abs(), padding=1).permute(0, 2, 3, 1).reshape(stem.n, 81, 128)
    out = run_stem(lib, stem.states, stem.n, stem.wd, stem.bd).view(np.float32).astype(np.float64)
    err = np.abs(out - ref.numpy())
    bound = gamma(28) * mag.numpy()
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"S3 stem: worst |error| / gamma_28 bound = {worst:.3f} (max |error| {err.max():.3e})")
    assert (err <= bound).all(), worst


# ---- S4 ------------------------------------------------------------------------------------------------------

def test_stem_bound_holds(lib, stem):
    """S4: every output <= stem_bound (1 + gamma_28), stem_bound as nnfast._prepared_weights computes it (the
    tower's first conv scales by it): on the network's own weights, and on all-positive weights, where the
    bound is the sum of every row and only f32 rounding can pass the f64 figure."""
    import torch
    from uttt_amd.nnfast import _prepared_weights
    positive = copy.deepcopy(stem.net)
    with torch.no_grad():
        positive.conv_input.weight.abs_()
        positive.bn_input.weight.abs_().add_(0.25)
        positive.bn_input.bias.abs_()
        positive.bn_input.running_mean.abs_().neg_()
    for name, net in (("own weights", stem.net), ("all-positive weights", positive)):
        w, b = stem_weights(net)
        if name != "own weights":
            assert (w > 0).all() and (b >= 0).all()
        bound = _prepared_weights(net, torch.device("cuda"), "wino3h")["stem_bound"]
        out = run_stem(lib, stem.states, stem.n, w.cuda(), b.cuda()).view(np.float32)
        assert np.array_equal(bits(out), bits(stem_model(stem.taps, w.numpy(), b.numpy())))
        print(f"S4 {name}: max output / stem_bound = {float(out.max()) / bound:.6f}")
        assert (out >= 0).all() and float(out.max()) <= bound * (1 + gamma(28)), name
    # the bound attained: no game state sets all 27 taps (a legal cell is empty), so the legal plane's rows
    # are zeroed and one synthetic state has both players on every cell (legal_mask is bit operations only;
    # its legal plane is empty): every interior output is the f32 sum of all 18 positive rows and the bias
    from uttt_amd._lib import STATE_DTYPE
    with torch.no_grad():
        positive.conv_input.weight[:, 2] = 0.0
    full = np.zeros(1, STATE_DTYPE)
    full["own"], full["opp"], full["active"] = 0x7FFFFFF, 0x7FFFFFF, -1
    planes = np.zeros((1, 9, 9, 3), np.uint8)
    planes[..., :2] = 1
    w, b = stem_weights(positive)
    bound = _prepared_weights(positive, torch.device("cuda"), "wino3h")["stem_bound"]
    out = run_stem(lib, dev_states(full), 1, w.cuda(), b.cuda()).view(np.float32)
    assert np.array_equal(bits(out), bits(stem_model(taps_of(planes), w.numpy(), b.numpy())))
    print(f"S4 every tap set: max output / stem_bound = 1 {float(out.max()) / bound - 1:+.3e}")
    assert bound * (1 - gamma(28)) <= float(out.max()) <= bound * (1 + gamma(28))


# ---- S5 ------------------------------------------------------------------------------------------------------

def test_stem_device_count(lib, stem):
    """S5: uttt_nn_stem_states_dev, max_n = 5: rows below min(*n_dev, 5) are S2's bits, later rows untouched."""
    import torch
    for nd in (0, 1, 2, 3, 5, 9):
        cnt = min(nd, 5)
        n_dev = torch.tensor([nd], dtype=torch.int32, device="cuda")
        out = sentinel(7, 81, 128)
        assert lib.uttt_nn_stem_states_dev(P(stem.states), P(n_dev), 5, P(stem.wd), P(stem.bd), P(out), stream()) == 0
        out = out.cpu().numpy()
        assert (out[cnt:] == SENTINEL).all(), nd
        assert np.array_equal(out[:cnt], bits(stem.model[:cnt])), nd


# ---- S6 ------------------------------------------------------------------------------------------------------

def test_stem_from_engine_leaves(gpu, lib, oracle_lib, stem_bn):
    """S6: uttt_nn_stem on an engine's pending leaves (the tree_of indirection) equals, bit for bit, the S2 model
    on the planes k_encode wrote for the same leaves, and uttt_nn_stem_states on the leaves read back."""
    import torch
    s = stem_bn
    roots, _ = _random_positions(oracle_lib, 16, seed=29)
    bs = gpu.BatchedSearch(16, 50)
    e = bs.engine
    e.use_stream()
    e.search_begin(roots, 50, 8)
    uniform, zeros = torch.full((16, 81), 1.0 / 81, device="cuda"), torch.zeros(16, device="cuda")
    for rnd in range(3):  # leaves at depth 0, 1 and 2
        n = e.select(bs.x)
        assert 0 < n <= 16
        out = sentinel(16, 81, 128)
        assert lib.uttt_nn_stem(e.h, P(s.wd), P(s.bd), P(out)) == 0
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        assert (out[n:] == SENTINEL).all(), rnd
        planes = bs.x[:n].cpu().numpy()
        assert np.isin(planes, (0.0, 1.0)).all()
        want = stem_model(taps_of(planes.transpose(0, 2, 3, 1)), s.w.numpy(), s.b.numpy())
        assert np.array_equal(out[:n], bits(want)), rnd
        leaves, _ = e.pending()
        assert len(leaves) == n
        assert np.array_equal(run_stem(lib, dev_states(leaves), n, s.wd, s.bd), out[:n]), rnd
        e.apply(uniform, zeros)


# ---- S7 ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("t,c", [(0, 0), (4, 5), (13, 77), (26, 127)])
def test_stem_keeps_nonfinite_weights(lib, stem_bn, t, c):
    """S7: a NaN in w[t][c] makes out[s][pos][c] NaN exactly where tap t is set (the S1 mask) and changes no
    other bit; a +Inf there gives +Inf on the same outputs. (With fmaxf(acc, 0) the NaN became 0.)"""
    s = stem_bn
    hit = s.taps[..., t].reshape(s.n, 81)
    assert hit.any() and not hit.all()
    clean = bits(s.model)
    for bad in (np.float32("nan"), np.float32("inf")):
        w = s.w.clone()
        w[t, c] = float(bad)
        out = run_stem(lib, s.states, s.n, w.cuda(), s.bd)
        got = out.view(np.float32)[..., c]
        if np.isnan(bad):
            assert np.array_equal(np.isnan(got), hit), "NaN outputs are not the set-tap outputs"
        else:
            assert np.array_equal(got == np.inf, hit) and not np.isnan(got).any()
        keep = np.ones(out.shape, bool)
        keep[..., c] = ~hit
        assert np.array_equal(out[keep], clean[keep])


def test_stem_keeps_a_nan_bias(lib, stem_bn):
    """S7: a NaN bias in channel c makes all of channel c NaN and changes no other channel."""
    s = stem_bn
    for c in (0, 6, 127):
        b = s.b.clone()
        b[c] = float("nan")
        out = run_stem(lib, s.states, s.n, s.wd, b.cuda())
        assert np.isnan(out.view(np.float32)[..., c]).all(), c
        others = np.arange(128) != c
        assert np.array_equal(out[..., others], bits(s.model)[..., others]), c


# ---- heads: f64 reference with a running error bound ---------------------------------------------------------

class HeadRef:
    """The heads in f64 numpy from the module's own tensors, and the bound on an f32 evaluation of them:
    e1 = gamma_129 (|c| + sum |w x|) on the three 1x1-conv planes (128 products and the bias; ReLU is
    1-Lipschitz), carried through each FC as sum |W| e_in + gamma_(terms + 1) (|b| + sum |W| (|h| + e_in))."""

    def __init__(self, net):
        from uttt_amd.model import fold_bn
        d = lambda t: t.detach().cpu().double().numpy()  # noqa: E731
        pw, pb = fold_bn(net.policy_conv, net.policy_bn)
        vw, vb = fold_bn(net.value_conv, net.value_bn)
        self.cw = np.concatenate([d(pw).reshape(2, 128), d(vw).reshape(1, 128)])
        self.cb = np.concatenate([d(pb), d(vb)])
        self.W, self.b = d(net.policy_fc.weight), d(net.policy_fc.bias)
        self.W1, self.b1 = d(net.value_fc1.weight), d(net.value_fc1.bias)
        self.W2, self.b2 = d(net.value_fc2.weight).reshape(256), float(d(net.value_fc2.bias)[0])

    def __call__(self, act):
        """act (n,81,128) f32 -> dict of z (n,81), ez, s (n,), es, p = softmax(z), v = tanh(s)."""
        x = np.asarray(act, np.float32).astype(np.float64)
        n = len(x)
        with np.errstate(invalid="ignore", over="ignore"):
            pre = np.einsum("npc,jc->njp", x, self.cw) + self.cb[None, :, None]
            e1 = gamma(129) * (np.abs(self.cb)[None, :, None] + np.einsum("npc,jc->njp", np.abs(x), np.abs(self.cw)))
            h = np.where(~(pre <= 0), pre, 0.0)
            hp, ep = h[:, :2].reshape(n, 162), e1[:, :2].reshape(n, 162)  # input j = plane * 81 + position
            z = hp @ self.W.T + self.b
            ez = ep @ np.abs(self.W).T + gamma(163) * (np.abs(self.b) + (np.abs(hp) + ep) @ np.abs(self.W).T)
            hv, ev = h[:, 2], e1[:, 2]
            a = hv @ self.W1.T + self.b1
            ea = ev @ np.abs(self.W1).T + gamma(82) * (np.abs(self.b1) + (np.abs(hv) + ev) @ np.abs(self.W1).T)
            r = np.where(~(a <= 0), a, 0.0)
            s = r @ self.W2 + self.b2
            es = ea @ np.abs(self.W2) + gamma(257) * (abs(self.b2) + (np.abs(r) + ea) @ np.abs(self.W2))
            zs = z - z.max(axis=1, keepdims=True)
            p = np.exp(zs) / np.exp(zs).sum(axis=1, keepdims=True)
        return {"z": z, "ez": ez, "s": s, "es": es, "p": p, "v": np.tanh(s)}


def run_heads(lib, act, hw, n, softmax):
    """uttt_nn_heads on the first n boards -> (policy (n,81), value (n,)) int32 bits."""
    pol, val = sentinel(n + 2, 81), sentinel(n + 2)
    assert lib.uttt_nn_heads(P(act), P(hw), n, P(pol), P(val), softmax, stream()) == 0
    assert (pol[n:] == SENTINEL).all() and (val[n:] == SENTINEL).all(), n
    return pol[:n].cpu().numpy(), val[:n].cpu().numpy()


NS = (1, 7, 8, 9, 17)  # nb < HB = 8, nb = HB, two and three workgroups with a partial last one
NMAX = max(NS)


@pytest.fixture(scope="module")
def rnet(gpu):
    from uttt_amd.model import random_network
    return random_network(3)


@pytest.fixture(scope="module")
def base_act(gpu):
    """(17,81,128) relu(randn), fixed generator."""
    import torch
    return torch.relu(torch.randn(NMAX, 81, 128, generator=torch.Generator().manual_seed(7)))


@pytest.fixture(scope="module")
def head_cases(gpu, rnet, base_act):
    """{name: (packed weights on the device, activation on the device, reference dict of the 17 boards)}: (a)
    relu(randn) s, s in {1e-3, 1, 1e3}, on random_network(3); (b) the calibrated network's own final activation
    on the first 17 netcal.npz positions. The weights are packed from the CPU module whose tensors the
    reference reads."""
    from uttt_amd.model import calibrated_network
    from uttt_amd.nnfast import FusedNetworkEvaluator, pack_heads
    cases = {}
    hw, ref = pack_heads(rnet, "cuda"), HeadRef(rnet)
    for s in (1e-3, 1.0, 1e3):
        act = (base_act * s).contiguous()
        cases[f"a{s:g}"] = (hw, act.cuda(), ref(act.numpy()))
    cal = calibrated_network(GOLDEN + "/netcal.npz", "cpu")
    fe = FusedNetworkEvaluator(copy.deepcopy(cal).cuda(), None, max_batch=NMAX)
    fe.forward_states(_rules_states(golden("netcal.npz")["rules_index"][:NMAX]))
    act = fe.buf[0][:NMAX].clone()
    cases["b"] = (pack_heads(cal, "cuda"), act, HeadRef(cal)(act.cpu().numpy()))
    return cases


CASES = ["a0.001", "a1", "a1000", "b"]


@pytest.mark.parametrize("case", CASES)
def test_heads_logits_within_the_derived_bound(lib, head_cases, case):
    """H1: |z - z64| <= e_z elementwise, at every batch size."""
    hw, act, ref = head_cases[case]
    assert np.isfinite(ref["z"]).all() and (ref["ez"] > 0).all()
    for n in NS:
        z, _ = run_heads(lib, act, hw, n, 0)
        z = z.view(np.float32).astype(np.float64)
        assert np.isfinite(z).all()
        ratio = np.abs(z - ref["z"][:n]) / ref["ez"][:n]
        print(f"H1 {case} n={n}: worst |z - z64| / e_z = {ratio.max():.3e}")
        assert (ratio <= 1.0).all(), (n, float(ratio.max()))


@pytest.mark.parametrize("case", CASES)
def test_heads_value_and_policy_within_the_derived_bound(lib, head_cases, case):
    """H2: |v - tanh(s64)| <= e_s + L_tanh; |p_i - p64_i| <= p64_i (exp(2E) - 1) + L_soft, E = max_o e_z(o) of
    the board (logits within E move every ratio by a factor within e^(+-2E)). On the calibrated network's
    activation also the project's bar, 1e-5 absolute."""
    hw, act, ref = head_cases[case]
    E = ref["ez"].max(axis=1, keepdims=True)
    pb = ref["p"] * np.expm1(2 * E) + L_SOFT
    vb = ref["es"] + L_TANH
    for n in NS:
        p, v = run_heads(lib, act, hw, n, 1)
        p, v = p.view(np.float32).astype(np.float64), v.view(np.float32).astype(np.float64)
        assert np.isfinite(p).all() and np.isfinite(v).all()
        perr, verr = np.abs(p - ref["p"][:n]), np.abs(v - ref["v"][:n])
        print(f"H2 {case} n={n}: worst policy error / bound = {(perr / pb[:n]).max():.3e} (max {perr.max():.3e}), "
              f"value error / bound = {(verr / vb[:n]).max():.3e} (max {verr.max():.3e})")
        assert (perr <= pb[:n]).all(), (n, float((perr / pb[:n]).max()))
        assert (verr <= vb[:n]).all(), (n, float((verr / vb[:n]).max()))
        if case == "b":
            assert perr.max() <= 1e-5 and verr.max() <= 1e-5, (n, perr.max(), verr.max())


# ---- H3 ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("softmax", [0, 1])
def test_heads_board_independence(lib, rnet, base_act, softmax):
    """H3: a board's policy row and value do not depend on its row or on the other boards: every (q, r) slot of
    the value path, both workgroup roles, and the unused s_h rows of a partial workgroup."""
    import torch
    from uttt_amd.nnfast import pack_heads
    hw = pack_heads(rnet, "cuda")
    act = base_act.cuda()
    p, v = run_heads(lib, act, hw, NMAX, softmax)
    assert len({p[i].tobytes() for i in range(NMAX)}) == NMAX  # 17 distinct boards give 17 distinct rows
    # one board in all 17 rows
    same = base_act[5:6].expand(NMAX, 81, 128).contiguous().cuda()
    ps, vs = run_heads(lib, same, hw, NMAX, softmax)
    assert (ps == ps[0]).all() and (vs == vs[0]).all()
    assert np.array_equal(ps[0], p[5]) and vs[0] == v[5]
    # a permutation of the boards permutes the rows
    perm = torch.randperm(NMAX, generator=torch.Generator().manual_seed(3))
    assert (perm != torch.arange(NMAX)).any()
    pp, vp = run_heads(lib, act[perm.cuda()].contiguous(), hw, NMAX, softmax)
    assert np.array_equal(pp, p[perm.numpy()]) and np.array_equal(vp, v[perm.numpy()])
    # one board alone, and as row 0, 3, 7, 8, 16 of 17
    p1, v1 = run_heads(lib, act[5:6].contiguous(), hw, 1, softmax)
    assert np.array_equal(p1[0], p[5]) and v1[0] == v[5]
    for row in (0, 3, 7, 8, 16):
        batch = act.clone()
        batch[row] = act[5]
        pr, vr = run_heads(lib, batch, hw, NMAX, softmax)
        assert np.array_equal(pr[row], p1[0]) and vr[row] == v1[0], row


# ---- H4 ------------------------------------------------------------------------------------------------------

def test_heads_at_saturation(lib, rnet, base_act):
    """H4: a logit 1e3 above the rest gives an exact one-hot row; zero policy FC gives 1/81 everywhere (within 2
    ulp, row sum 1 within 81 u); value FC2 times 2^20 gives exactly +-1 with the reference's sign."""
    import torch
    from uttt_amd.nnfast import pack_heads
    act = base_act.cuda()
    ref = HeadRef(rnet)(base_act.numpy())
    # one logit far above
    hot = 37
    net = copy.deepcopy(rnet)
    spread = float(ref["z"].max() - ref["z"].min())
    with torch.no_grad():
        net.policy_fc.bias[hot] += 1e3 + spread
    z = HeadRef(net)(base_act.numpy())
    others = np.arange(81) != hot
    assert ((z["z"][:, hot:hot + 1] - z["z"][:, others]) - 2 * z["ez"].max() >= 1e3).all()  # the premise, in f64
    p, _ = run_heads(lib, act, pack_heads(net, "cuda"), NMAX, 1)
    want = np.zeros((NMAX, 81), np.float32)
    want[:, hot] = 1.0
    assert np.array_equal(p, bits(want))
    # all logits equal
    net = copy.deepcopy(rnet)
    with torch.no_grad():
        net.policy_fc.weight.zero_()
        net.policy_fc.bias.zero_()
    p, _ = run_heads(lib, act, pack_heads(net, "cuda"), NMAX, 1)
    p = p.view(np.float32).astype(np.float64)
    ulp = float(np.spacing(np.float32(1.0 / 81)))
    print(f"H4 uniform: worst |p - 1/81| = {np.abs(p - 1.0 / 81).max() / ulp:.3f} ulp, "
          f"worst |row sum - 1| = {np.abs(p.sum(axis=1) - 1).max() / U:.3f} u")
    assert (np.abs(p - 1.0 / 81) <= 2 * ulp).all()
    assert (np.abs(p.sum(axis=1) - 1.0) <= 81 * U).all()
    # a saturated tanh
    net = copy.deepcopy(rnet)
    with torch.no_grad():
        net.value_fc2.weight.mul_(2.0 ** 20)
        net.value_fc2.bias.mul_(2.0 ** 20)
    big = HeadRef(net)(base_act.numpy())
    # the premise, from the reference alone: on these boards any f32 sum within e_s of s64 has s64's sign and a
    # magnitude above 100, whose tanh is +-1 in f32 whatever tanhf's ulp (a board whose sum is below its own
    # bound proves nothing about the sign)
    sure = np.abs(big["s"]) - big["es"] > 100.0
    assert sure.sum() >= NMAX - 2 and (big["s"][sure] > 0).any() and (big["s"][sure] < 0).any()
    _, v = run_heads(lib, act, pack_heads(net, "cuda"), NMAX, 1)
    assert np.array_equal(v[sure], bits(np.sign(big["s"][sure]).astype(np.float32)))


# ---- H5 ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,k", [(1, 0), (17, 0), (17, 9)])
@pytest.mark.parametrize("bad", ["nan", "inf"])
def test_heads_keep_nonfinite_activations(lib, rnet, base_act, n, k, bad):
    """H5: a NaN or a +Inf in one channel of one position of board k: the board's 81 policy entries (logits and
    softmax) and its value are all non-finite, every other board is bit-identical to the clean run. The +Inf
    goes into a channel whose value-conv and first policy-conv weights are positive, where the f64 reference
    is non-finite too (through a negative weight relu(-Inf) = 0 is the right, finite, answer)."""
    from uttt_amd.nnfast import pack_heads
    ref = HeadRef(rnet)
    ch = int(np.flatnonzero((ref.cw[0] > 0) & (ref.cw[2] > 0))[0])
    x = base_act[:n].clone()
    x[k, 40, ch] = float(bad)
    want = ref(x.numpy())
    assert not np.isfinite(want["z"][k]).any() and not np.isfinite(want["s"][k])  # the premise
    hw = pack_heads(rnet, "cuda")
    others = np.arange(n) != k
    for softmax in (0, 1):
        p0, v0 = run_heads(lib, base_act[:n].cuda(), hw, n, softmax)
        p, v = run_heads(lib, x.cuda(), hw, n, softmax)
        assert not np.isfinite(p[k].view(np.float32)).any(), softmax
        assert not np.isfinite(v[k:k + 1].view(np.float32)).any(), softmax
        assert np.array_equal(p[others], p0[others]) and np.array_equal(v[others], v0[others]), softmax


# ---- H6 ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("softmax", [0, 1])
def test_heads_device_count(lib, rnet, base_act, softmax):
    """H6: uttt_nn_heads_dev, max_n = 17: rows below min(*n_dev, 17) are uttt_nn_heads' bits, later policy and
    value rows untouched."""
    import torch
    from uttt_amd.nnfast import pack_heads
    hw, act = pack_heads(rnet, "cuda"), base_act.cuda()
    ph, vh = run_heads(lib, act, hw, NMAX, softmax)
    for nd in (0, 1, 8, 9, 17, 40):
        cnt = min(nd, NMAX)
        n_dev = torch.tensor([nd], dtype=torch.int32, device="cuda")
        pol, val = sentinel(NMAX + 2, 81), sentinel(NMAX + 2)
        assert lib.uttt_nn_heads_dev(P(act), P(hw), P(n_dev), NMAX, P(pol), P(val), softmax, stream()) == 0
        pol, val = pol.cpu().numpy(), val.cpu().numpy()
        assert (pol[cnt:] == SENTINEL).all() and (val[cnt:] == SENTINEL).all(), nd
        assert np.array_equal(pol[:cnt], ph[:cnt]) and np.array_equal(val[:cnt], vh[:cnt]), nd


# ---- H7 ------------------------------------------------------------------------------------------------------

def test_heads_and_stem_refuse_bad_arguments(gpu, lib, oracle_lib, rnet, base_act, stem_bn):
    """H7: n < 0 or a null pointer in any position is UTTT_ERR_ARG, and nothing is written."""
    import torch
    from uttt_amd.nnfast import pack_heads
    hw, act = pack_heads(rnet, "cuda"), base_act.cuda()
    n_dev = torch.tensor([3], dtype=torch.int32, device="cuda")
    pol, val = sentinel(NMAX, 81), sentinel(NMAX)
    good = [P(act), P(hw), 3, P(pol), P(val), 1, stream()]
    assert lib.uttt_nn_heads(*good[:2], -1, *good[3:]) == ERR_ARG
    for i in (0, 1, 3, 4):
        assert lib.uttt_nn_heads(*[None if j == i else a for j, a in enumerate(good)]) == ERR_ARG, i
    good = [P(act), P(hw), P(n_dev), NMAX, P(pol), P(val), 1, stream()]
    assert lib.uttt_nn_heads_dev(*good[:3], -1, *good[4:]) == ERR_ARG
    for i in (0, 1, 2, 4, 5):
        assert lib.uttt_nn_heads_dev(*[None if j == i else a for j, a in enumerate(good)]) == ERR_ARG, i
    s = stem_bn
    out = sentinel(5, 81, 128)
    good = [P(s.states), 3, P(s.wd), P(s.bd), P(out), stream()]
    assert lib.uttt_nn_stem_states(good[0], -1, *good[2:]) == ERR_ARG
    for i in (0, 2, 3, 4):
        assert lib.uttt_nn_stem_states(*[None if j == i else a for j, a in enumerate(good)]) == ERR_ARG, i
    good = [P(s.states), P(n_dev), 5, P(s.wd), P(s.bd), P(out), stream()]
    assert lib.uttt_nn_stem_states_dev(*good[:2], -1, *good[3:]) == ERR_ARG
    for i in (0, 1, 3, 4, 5):
        assert lib.uttt_nn_stem_states_dev(*[None if j == i else a for j, a in enumerate(good)]) == ERR_ARG, i
    # the engine's stem: a null engine, and null weights, bias or output with leaves pending
    assert lib.uttt_nn_stem(None, P(s.wd), P(s.bd), P(out)) == ERR_ARG
    roots, _ = _random_positions(oracle_lib, 4, seed=5)
    bs = gpu.BatchedSearch(4, 50)
    bs.engine.use_stream()
    bs.engine.search_begin(roots, 50, 8)
    assert bs.engine.select(bs.x) > 0
    good = [bs.engine.h, P(s.wd), P(s.bd), P(out)]
    for i in (1, 2, 3):
        assert lib.uttt_nn_stem(*[None if j == i else a for j, a in enumerate(good)]) == ERR_ARG, i
    torch.cuda.synchronize()
    assert (pol == SENTINEL).all() and (val == SENTINEL).all() and (out == SENTINEL).all()


# ---- amax ----------------------------------------------------------------------------------------------------

COUNTS = (1, 63, 64, 65, 255, 256, 257, 1024 * 256 + 3)  # the last exceeds the grid cap: the stride loop runs


def amax_bits(x, preload=0):
    """nnfast.amax on a preloaded result -> the result's u32 bits as an int."""
    import torch
    from uttt_amd.nnfast import amax
    out = torch.tensor([preload], dtype=torch.int32, device="cuda")
    return int(amax(x, out=out).cpu().numpy().view(np.uint32)[0])


def max_abs_bits(a):
    return int(np.abs(a).max().astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("count", COUNTS)
def test_amax_is_the_exact_maximum(gpu, count):
    """A1: max |x| as bits, the maximum first, in the middle and last, positive and negative."""
    import torch
    rng = np.random.default_rng(count)
    base = rng.standard_normal(count).astype(np.float32)
    for pos in sorted({0, count // 2, count - 1}):
        for top in (7.5, -7.5):
            a = base.copy()
            a[pos] = top
            assert np.abs(a).argmax() == pos
            assert amax_bits(torch.from_numpy(a).cuda()) == max_abs_bits(a) == 0x40F00000, (pos, top)
    assert amax_bits(torch.from_numpy(base).cuda()) == max_abs_bits(base)


@pytest.mark.parametrize("count", (1, 65, 257, 1024 * 256 + 3))
def test_amax_special_values(gpu, count):
    """A1: only -0.0 gives bits 0; a subnormal maximum is kept; +Inf or -Inf present gives +Inf."""
    import torch
    a = np.full(count, -0.0, np.float32)
    assert amax_bits(torch.from_numpy(a).cuda()) == 0
    tiny = np.float32(2.0 ** -140)
    a[count // 2] = -tiny
    assert amax_bits(torch.from_numpy(a).cuda()) == int(tiny.view(np.uint32)) == 1 << 9
    a = np.random.default_rng(1).standard_normal(count).astype(np.float32)
    for inf in (np.inf, -np.inf):
        b = a.copy()
        b[count - 1] = inf
        assert amax_bits(torch.from_numpy(b).cuda()) == 0x7F800000


def test_amax_preloaded_result_and_zero_count(gpu, lib):
    """A2: a larger *amax on entry is kept, a smaller one replaced; count = 0 leaves it untouched."""
    import torch
    a = np.random.default_rng(2).standard_normal(300).astype(np.float32)
    x = torch.from_numpy(a).cuda()
    m = max_abs_bits(a)
    larger, smaller = int(np.float32(100.0).view(np.uint32)), int(np.float32(0.001).view(np.uint32))
    assert amax_bits(x, preload=larger) == larger
    assert amax_bits(x, preload=smaller) == m
    out = torch.tensor([smaller], dtype=torch.int32, device="cuda")
    assert lib.uttt_nn_amax(P(x), 0, P(out), stream()) == 0
    assert int(out.cpu()[0]) == smaller


@pytest.mark.parametrize("count", (1, 64, 257, 1024 * 256 + 3))
def test_amax_ignores_nan(gpu, count):
    """A3: a NaN among the values is ignored (fmaxf drops it, as the header says of y_amax): the result is the
    maximum of the others, 0 when there are none."""
    import torch
    a = np.random.default_rng(3).standard_normal(count).astype(np.float32)
    for pos in sorted({0, count // 2, count - 1}):
        b = a.copy()
        b[pos] = np.nan
        rest = np.delete(b, pos)
        want = max_abs_bits(rest) if len(rest) else 0
        assert amax_bits(torch.from_numpy(b).cuda()) == want, pos


def test_amax_refuses_bad_arguments(gpu, lib):
    import torch
    x = torch.ones(8, device="cuda")
    out = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert lib.uttt_nn_amax(None, 8, P(out), stream()) == ERR_ARG
    assert lib.uttt_nn_amax(P(x), 8, None, stream()) == ERR_ARG
    assert lib.uttt_nn_amax(P(x), -1, P(out), stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert int(out.cpu()[0]) == 0
