"""CPU tests of the board symmetries' host side (csrc/uttt_sym.h, uttt_amd/symmetry.py): the state
transform against numpy's rot90 / fliplr of the network input (the independent ground truth), its commutation with
the rules, the group tables, the hashed choice against a Python restatement on oracle/hashnp.py's mix64, the tensor
gathers, history augmentation, and train_network(augment=True) on the CPU."""
import ctypes
import random

import numpy as np
import pytest

from test_playout_host import pack

GOLD = 0x9E3779B97F4A7C15
N_POS = 64  # enough positions for the hashed choice to take every symmetry (checked below)


@pytest.fixture(scope="module")
def sym(engine_lib):
    from uttt_amd import symmetry
    return symmetry


@pytest.fixture(scope="module")
def positions(oracle_lib):
    """The initial position, then positions at mixed depths along random games (final ones included), some of them
    with a free move (active == -1)."""
    rng = random.Random(2024)
    out = [oracle_lib.OrState.initial()]
    while len(out) < N_POS:
        s = oracle_lib.OrState.initial()
        while not s.is_done() and len(out) < N_POS:
            s = s.next(rng.choice(s.legal_actions()))
            if rng.random() < 0.12 or s.is_done():
                out.append(s)
    packed = pack(out)
    assert (packed["active"][1:] == -1).any() and (packed["active"] >= 0).any()
    assert any(s.is_done() for s in out) and sum(not s.is_done() for s in out) > 40
    return packed, out


def _sp(a):
    from uttt_amd._lib import UtttState
    return a.ctypes.data_as(ctypes.POINTER(UtttState))


def _hwc(lib, states):
    out = np.zeros((len(states), 9, 9, 3), np.float32)
    assert lib.uttt_states_input_hwc(_sp(states), len(states), out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))) == 0
    return out


def _image(img, g):
    """The definition: np.rot90(np.fliplr(img) if f else img, k=r) on axes (0, 1)."""
    f, r = divmod(g, 4)
    return np.rot90(np.flip(img, axis=1) if f else img, k=r, axes=(0, 1))


def _legal(lib, st):
    out = np.zeros(81, np.int32)
    n = lib.uttt_state_legal_actions(_sp(st), out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    return out[:n].tolist()


def _next(lib, st, a):
    out = np.zeros(1, st.dtype)
    assert lib.uttt_state_next(_sp(st), int(a), _sp(out)) == 0
    return out


def test_action_perm_is_the_image_transform(sym):
    """pi_g from its definition: 9 beta_g(b) + beta_g(c), beta_g the image operation on a 3x3 index."""
    idx = np.arange(9).reshape(3, 3)
    for g in range(8):
        moved = _image(idx, g)  # moved[R', C'] = the index that landed there
        beta = np.zeros(9, np.int64)
        beta[moved.reshape(-1)] = np.arange(9)
        want = [9 * beta[a // 9] + beta[a % 9] for a in range(81)]
        assert sym.ACTION_PERM[g].tolist() == want, g
        assert sorted(want) == list(range(81))
    assert sym.ACTION_PERM[0].tolist() == list(range(81))
    assert len({tuple(p) for p in sym.ACTION_PERM.tolist()}) == 8


def test_input_of_transform_is_numpy_image(engine_lib, sym, positions):
    packed, _ = positions
    x = _hwc(engine_lib, packed)
    for g in range(8):
        t = sym.transform_states(packed, g)
        got = _hwc(engine_lib, t)
        want = np.stack([_image(img, g) for img in x])
        assert np.array_equal(got, want), g
    # one symmetry per state
    gs = np.arange(len(packed)) % 8
    got = _hwc(engine_lib, sym.transform_states(packed, gs))
    assert np.array_equal(got, np.stack([_image(img, g) for img, g in zip(x, gs)]))


def test_rules_commute(engine_lib, sym, positions):
    packed, _ = positions
    lib = engine_lib
    for i in range(len(packed)):
        s = packed[i:i + 1]
        legal = _legal(lib, s)
        for g in range(8):
            pi = sym.ACTION_PERM[g]
            t = sym.transform_states(s, g)
            assert _legal(lib, t) == sorted(pi[legal].tolist()), (i, g)
            for fn in (lib.uttt_state_is_lose, lib.uttt_state_is_draw, lib.uttt_state_is_done,
                       lib.uttt_state_is_first_player):
                assert fn(_sp(t)) == fn(_sp(s)), (i, g)
            for a in legal:
                assert _next(lib, t, pi[a]).tobytes() == sym.transform_states(_next(lib, s, a), g).tobytes(), (i, g, a)


def test_initial_is_fixed_and_group_tables(sym, positions):
    from uttt_amd import initial_states
    packed, _ = positions
    for g in range(8):
        assert sym.transform_states(initial_states(1), g).tobytes() == initial_states(1).tobytes()
        assert sym.transform_states(packed, 0).tobytes() == packed.tobytes()
        inv = sym.inverse(g)
        assert sym.compose(inv, g) == 0 and sym.compose(g, inv) == 0
        assert sym.transform_states(sym.transform_states(packed, g), inv).tobytes() == packed.tobytes(), g
        for h in range(8):
            k = sym.compose(g, h)  # h first, then g
            assert np.array_equal(sym.ACTION_PERM[k], sym.ACTION_PERM[g][sym.ACTION_PERM[h]]), (g, h)
            assert sym.transform_states(sym.transform_states(packed, h), g).tobytes() == \
                sym.transform_states(packed, k).tobytes(), (g, h)
    assert sorted(sym.INVERSE.tolist()) == list(range(8))


def _choice_py(ostate, seed):
    """playout_key(input words, seed) >> 61 restated on hashnp.mix64."""
    from oracle.hashnp import mix64
    x = ostate.tensor_nchw()
    h = GOLD
    for i in range(4):
        w = 0
        for j in range(64 * i, min(64 * i + 64, 243)):
            if x[j] != 0:
                w |= 1 << (j - 64 * i)
        h = mix64(h ^ w)
    return (h ^ mix64(seed)) >> 61


def test_hashed_choice(engine_lib, sym, positions):
    packed, ostates = positions
    for seed in (0, 0x1234567890ABCDEF):
        got = sym.hashed_symmetry(packed, seed)
        assert got.dtype == np.int8 and got.tolist() == [_choice_py(s, seed) for s in ostates], seed
    got = sym.hashed_symmetry(packed, 0)
    assert sorted(set(got.tolist())) == list(range(8))  # every symmetry occurs over the fixture positions
    assert not np.array_equal(got, sym.hashed_symmetry(packed, 1))
    # equal legal planes, different `active`: one board open, named or not (test_playout_host's position)
    from test_playout_host import _from_arrays
    z = np.zeros((9, 9), np.int32)
    p, e = z.copy(), z.copy()
    p[6, [0, 4]] = 1
    e[6, [1, 8]] = 1
    mp, me = [1, 0, 1, 1, 0, 0, 0, 1, 1], [0, 1, 0, 0, 1, 1, 0, 0, 0]
    both = np.concatenate([_from_arrays(engine_lib, p, e, mp, me, -1), _from_arrays(engine_lib, p, e, mp, me, 6)])
    for seed in range(8):
        c = sym.hashed_symmetry(both, seed)
        assert c[0] == c[1]


def test_argument_checks(engine_lib, sym, positions):
    packed, _ = positions
    with pytest.raises(ValueError):
        sym.transform_states(packed, 8)
    with pytest.raises(ValueError):
        sym.transform_states(packed, -1)
    s8 = np.full(len(packed), 8, np.int8)
    out = packed.copy()
    assert engine_lib.uttt_states_transform_host(_sp(packed), len(packed), s8.ctypes.data_as(
        ctypes.POINTER(ctypes.c_int8)), _sp(out)) == -1
    assert out.tobytes() == packed.tobytes()
    assert engine_lib.uttt_sym_compose(8, 0) == -1 and engine_lib.uttt_sym_inverse(-1) == -1
    bad = packed[:1].copy()
    bad["active"] = 9
    with pytest.raises(ValueError):
        sym.hashed_symmetry(bad)
    with pytest.raises(ValueError):
        sym.transform_states(bad, 1)


def test_tensor_gathers_agree_with_states(engine_lib, sym, positions):
    import torch
    packed, _ = positions
    x = np.ascontiguousarray(_hwc(engine_lib, packed).transpose(0, 3, 1, 2))
    rng = np.random.RandomState(3)
    p = rng.rand(len(packed), 81).astype(np.float32)
    gs = rng.randint(0, 8, len(packed))
    t = sym.transform_states(packed, gs)
    want_x = np.ascontiguousarray(_hwc(engine_lib, t).transpose(0, 3, 1, 2))
    assert np.array_equal(sym.transform_inputs(x, gs), want_x)
    tx = sym.transform_inputs(torch.from_numpy(x), torch.from_numpy(gs))
    assert np.array_equal(tx.numpy(), want_x)
    out = torch.zeros_like(tx)
    assert sym.transform_inputs(torch.from_numpy(x), gs, out=out) is out and np.array_equal(out.numpy(), want_x)
    tp = sym.transform_policy(p, gs)
    for i, g in enumerate(gs):
        assert np.array_equal(tp[i][sym.ACTION_PERM[g]], p[i])
    assert np.array_equal(sym.transform_policy(torch.from_numpy(p), gs).numpy(), tp)
    assert np.array_equal(sym.policy_from_image(tp, gs), p)
    assert np.array_equal(sym.policy_from_image(torch.from_numpy(tp), torch.from_numpy(gs)).numpy(), p)
    for g in range(8):  # a scalar symmetry for every row
        assert np.array_equal(sym.transform_inputs(x, g), sym.transform_inputs(x, np.full(len(x), g)))


def _history(engine_lib, packed, seed):
    """One sample per non-terminal position: a random policy on its legal moves."""
    rng = np.random.RandomState(seed)
    x = _hwc(engine_lib, packed)
    hist = []
    for i in range(len(packed)):
        legal = _legal(engine_lib, packed[i:i + 1])
        if not legal:
            continue
        pol = np.zeros(81, np.float64)
        pol[legal] = rng.dirichlet(np.ones(len(legal)))
        hist.append([x[i], pol, int(rng.randint(-1, 2))])
    return hist


def test_augment_history(engine_lib, sym, positions):
    packed, _ = positions
    hist = _history(engine_lib, packed, 4)
    aug = sym.augment_history(hist)
    assert len(aug) == 8 * len(hist)
    for i, (x, pol, val) in enumerate(hist):
        for g in range(8):
            ax, ap, av = aug[8 * i + g]
            assert av == val and ax.shape == (9, 9, 3) and ax.dtype == x.dtype and ap.dtype == pol.dtype
            assert np.array_equal(ax, _image(x, g))
            assert np.array_equal(ap[sym.ACTION_PERM[g]], pol)
            # the policy's support lies inside the image's legal plane
            legal_plane = ax[:, :, 2].reshape(81)
            pos_of = {a: pos for pos, a in enumerate(_action_at_table())}
            assert all(legal_plane[pos_of[a]] == 1 for a in np.nonzero(ap)[0]), (i, g)
    assert [len(sym.augment_history(hist[:3], 5)), len(sym.augment_history(hist[:3], [1, 2]))] == [3, 6]


def _action_at_table():
    out = []
    for pos in range(81):
        R, C = divmod(pos, 9)
        out.append((R // 3 * 3 + C // 3) * 9 + (R % 3) * 3 + C % 3)
    return out


def test_train_network_augment_cpu(engine_lib, sym, positions, monkeypatch):
    import torch
    from uttt_amd import train
    from uttt_amd.model import DualNetwork
    packed, _ = positions
    hist = _history(engine_lib, packed, 9)[:16]
    assert len(hist) == 16
    x0, p0, _ = train.history_arrays(hist)
    seen = []
    orig = train.EpochAugmenter.epoch

    def spy(self, epoch):
        orig(self, epoch)
        seen.append((epoch, self.sym.clone(), self.x.clone(), self.p.clone(), self.x0.clone(), self.p0.clone()))

    monkeypatch.setattr(train.EpochAugmenter, "epoch", spy)

    def run(augment, seed=5):
        torch.manual_seed(0)
        net = DualNetwork(filters=8, residual_num=1)
        losses = train.train_network(net, hist, epochs=2, batch_size=8, device=torch.device("cpu"), seed=seed,
                                     log=None, augment=augment)
        return losses, [t.clone() for t in net.state_dict().values()]

    la, wa = run(True)
    first = list(seen)
    lb, wb = run(True)
    assert la == lb and all(torch.equal(a, b) for a, b in zip(wa, wb))  # deterministic under its seed
    n_aug = len(seen)
    ln, wn = run(False)
    assert len(seen) == n_aug  # the hook is not entered without augment
    assert la != ln and not all(torch.equal(a, b) for a, b in zip(wa, wn))
    assert [e for e, *_ in first] == [0, 1]
    for epoch, s, x, p, xk, pk in first:
        assert np.array_equal(xk.numpy(), x0) and np.array_equal(pk.numpy(), p0)  # pristine
        assert s.shape == (16,) and 0 <= int(s.min()) and int(s.max()) <= 7
        assert np.array_equal(x.numpy(), sym.transform_inputs(x0, s.numpy()))
        assert np.array_equal(p.numpy(), sym.transform_policy(p0, s.numpy()))
    assert not torch.equal(first[0][1], first[1][1])  # a fresh draw per epoch
    assert not np.array_equal(first[0][2].numpy(), x0)
    _, w_other = run(True, seed=6)
    assert not all(torch.equal(a, b) for a, b in zip(wa, w_other))
