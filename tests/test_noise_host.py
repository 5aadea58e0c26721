"""Root noise on the CPU (uttt_root_noise_host, csrc/uttt_noise.h): argument checks, the shape of a
row for every root width and alpha at the ends of the range, what keys a row, the Dirichlet marginals' first three
moments (deterministic: the draws are counter-based), the mixed priors, and the two settings' parsers. No GPU."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

import wide_deep

ALPHAS = (1.0 / 32.0, 0.3, 1.0, 3.0, 32.0)


@pytest.fixture(scope="module")
def noise(engine_lib):
    from uttt_amd import noise
    return noise


@pytest.fixture(scope="module")
def roots(engine_lib, oracle_lib):
    """(packed states, L): the initial state (81), the states after its first 3 moves (9 each), 3 free-move roots
    (66-70)."""
    s0 = oracle_lib.OrState.initial()
    ost = [s0] + [s0.next(a) for a in (1, 41, 79)] + list(wide_deep.wide_roots(3, wide_deep.WIDE_SEED)[1])
    L = np.array([len(s.legal_actions()) for s in ost])
    assert L[0] == 81 and all(L[1:4] == 9) and all(66 <= x <= 70 for x in L[4:])
    return wide_deep.pack_states(ost), L


def call_raw(lib, states, stream, ply, eps, alpha, seed, eta, pri):
    from uttt_amd._lib import UtttState
    n = len(states)
    stream = np.ascontiguousarray(stream, np.int64)
    ply = np.ascontiguousarray(ply, np.int32)
    f32p = ctypes.POINTER(ctypes.c_float)
    return lib.uttt_root_noise_host(states.ctypes.data_as(ctypes.POINTER(UtttState)), n,
                                    stream.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                    ply.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), eps, alpha, seed,
                                    eta.ctypes.data_as(f32p) if eta is not None else None,
                                    pri.ctypes.data_as(f32p) if pri is not None else None)


def test_arguments_are_checked(engine_lib, roots):
    st = roots[0][:2]
    eta = np.zeros((2, 81), np.float32)
    ok = lambda eps, alpha: call_raw(engine_lib, st, [0, 1], [0, 0], eps, alpha, 0, eta, None)
    for eps in (-0.001, 1.001, float("nan"), float("inf")):
        assert ok(eps, 0.3) == -1, eps
    for alpha in (0.0, -1.0, 1.0 / 32.0 - 1e-4, 32.001, float("nan"), float("inf")):
        assert ok(0.25, alpha) == -1, alpha
    assert b"alpha" in engine_lib.uttt_last_error()
    for eps, alpha in ((0.0, 1.0 / 32.0), (1.0, 32.0), (0.25, 0.3)):
        assert ok(eps, alpha) == 0
    # either output may be NULL
    assert call_raw(engine_lib, st, [0, 1], [0, 0], 0.25, 0.3, 0, None, eta) == 0
    assert call_raw(engine_lib, st, [0, 1], [0, 0], 0.25, 0.3, 0, None, None) == 0


@pytest.mark.parametrize("alpha", ALPHAS)
def test_rows_are_distributions(engine_lib, roots, alpha):
    st, L = roots
    n = len(st)
    for seed in (0, 7, 2**64 - 1):
        eta = np.full((n, 81), -7.0, np.float32)
        pri = np.full((n, 81), -7.0, np.float32)
        assert call_raw(engine_lib, st, np.arange(n), np.arange(n) % 3, 0.25, alpha, seed, eta, pri) == 0
        for r in range(n):
            for row in (eta[r], pri[r]):
                assert np.all(np.isfinite(row[:L[r]])) and np.all(row[:L[r]] >= 0.0), (alpha, r)
                assert np.all(row[L[r]:] == -7.0), "entries at ranks >= L are untouched"
                # S is a sequential f32 sum of L terms and every entry one divide: L / 2 + 1 / 2 ulps at the most
                assert abs(row[:L[r]].astype(np.float64).sum() - 1.0) <= L[r] * 2.0 ** -23, (alpha, r)
            assert eta[r, :L[r]].max() > 0.0


def test_rows_are_keyed_by_seed_stream_ply_and_width(noise, roots):
    st, L = roots
    # two different positions with equal L and an equal key: the same row
    eta, pri = noise.root_noise_host(st[[1, 2, 3]], [5, 5, 5], [2, 2, 2], 0.25, 0.3, seed=9)
    assert np.array_equal(eta[0].view(np.uint32), eta[1].view(np.uint32))
    assert np.array_equal(eta[0].view(np.uint32), eta[2].view(np.uint32))
    assert np.array_equal(pri[0].view(np.uint32), pri[1].view(np.uint32))
    base = eta[0]
    # any one of seed, stream, ply changes it
    for kw in (dict(seed=10), dict(stream=6), dict(ply=3)):
        a = dict(stream=5, ply=2, seed=9)
        a.update(kw)
        other, _ = noise.root_noise_host(st[[1]], [a["stream"]], [a["ply"]], 0.25, 0.3, seed=a["seed"])
        assert not np.array_equal(other[0], base), kw
    # 64-bit streams and seeds are used whole
    hi, _ = noise.root_noise_host(st[[1]], [5 + 2**32], [2], 0.25, 0.3, seed=9)
    assert not np.array_equal(hi[0], base)
    hi, _ = noise.root_noise_host(st[[1]], [5], [2], 0.25, 0.3, seed=9 + 2**32)
    assert not np.array_equal(hi[0], base)
    # a permutation of the inputs permutes the rows
    n = len(st)
    stream, ply = np.arange(n) * 3 + 1, np.arange(n) % 4
    eta, pri = noise.root_noise_host(st, stream, ply, 0.25, 0.3, seed=1)
    perm = np.random.RandomState(0).permutation(n)
    eta_p, pri_p = noise.root_noise_host(st[perm], stream[perm], ply[perm], 0.25, 0.3, seed=1)
    assert np.array_equal(eta_p.view(np.uint32), eta[perm].view(np.uint32))
    assert np.array_equal(pri_p.view(np.uint32), pri[perm].view(np.uint32))


def beta_central_moments(a, b, orders):
    """Central moments of Beta(a, b) from its raw moments E x^k = prod_{j<k} (a + j) / (a + b + j)."""
    raw = [1.0]
    for k in range(max(orders)):
        raw.append(raw[-1] * (a + k) / (a + b + k))
    mu = raw[1]
    return {k: sum(math.comb(k, j) * raw[j] * (-mu) ** (k - j) for j in range(k + 1)) for k in orders}


@pytest.mark.parametrize("alpha", (0.3, 2.0))
def test_marginals_are_beta(noise, roots, alpha):
    """eta ~ Dirichlet(alpha, ..., alpha) over L = 9 moves: every component is Beta(alpha, (L - 1) alpha). 4,096
    keys; each sample moment within 5 standard errors, the standard errors from the Beta's own moments."""
    st, _ = roots
    L, N = 9, 4096
    eta, _ = noise.root_noise_host(np.repeat(st[1:2], N), np.arange(N), np.zeros(N), 0.25, alpha, seed=2024)
    x = eta[:, :L].astype(np.float64)
    c = beta_central_moments(alpha, (L - 1) * alpha, (2, 3, 4, 6))
    mu = 1.0 / L
    assert abs(c[2] - mu * (1.0 - mu) / (L * alpha + 1.0)) < 1e-15
    d = x - mu  # deviations from the true mean: sample means of d^k are unbiased for the central moments
    se1 = math.sqrt(c[2] / N)
    se2 = math.sqrt((c[4] - c[2] ** 2) / N)
    se3 = math.sqrt((c[6] - c[3] ** 2) / N)
    for i in range(L):
        m1, m2, m3 = d[:, i].mean(), (d[:, i] ** 2).mean(), (d[:, i] ** 3).mean()
        assert abs(m1) <= 5.0 * se1, (i, m1, se1)
        assert abs(m2 - c[2]) <= 5.0 * se2, (i, m2, c[2], se2)
        assert abs(m3 - c[3]) <= 5.0 * se3, (i, m3, c[3], se3)
    try:
        from scipy import stats
    except ImportError:
        return
    assert stats.kstest(x[:, 0], stats.beta(alpha, (L - 1) * alpha).cdf).pvalue > 1e-4


def round_f32(x):
    """The f32 nearest the Fraction x (ties to even): fmaf's one rounding, in exact arithmetic."""
    r = np.float32(float(x))  # within one f32 step of the answer (two roundings)
    cands = (np.nextafter(r, np.float32(-np.inf)), r, np.nextafter(r, np.float32(np.inf)))
    return min(cands, key=lambda c: (abs(Fraction(float(c)) - x), int(c.view(np.uint32)) & 1))


def test_mixed_priors(noise, roots):
    st, L = roots
    n = len(st)
    stream, ply = np.arange(n), np.arange(n)
    for alpha in (0.3, 32.0):
        eta, pri = noise.root_noise_host(st, stream, ply, 0.25, alpha, seed=3)
        eps = np.float32(0.25)
        for r in range(n):
            up = np.float32(1.0) / np.float32(L[r])
            c = np.float32(np.float32(1.0) - eps) * up  # one f32 multiply, then the fma: one rounding of the exact sum
            want = np.array([round_f32(Fraction(float(eps)) * Fraction(float(e)) + Fraction(float(c)))
                             for e in eta[r, :L[r]]], np.float32)
            assert np.array_equal(pri[r, :L[r]].view(np.uint32), want.view(np.uint32)), (alpha, r)
            assert np.all(pri[r, L[r]:] == 0.0)
        eta1, pri1 = noise.root_noise_host(st, stream, ply, 1.0, alpha, seed=3)
        assert np.array_equal(eta1.view(np.uint32), eta.view(np.uint32)), "eta does not depend on epsilon"
        assert np.array_equal(pri1.view(np.uint32), eta.view(np.uint32)), "epsilon 1 gives eta back"
        _, pri0 = noise.root_noise_host(st, stream, ply, 0.0, alpha, seed=3)
        for r in range(n):
            assert np.all(pri0[r, :L[r]].view(np.uint32) == (np.float32(1.0) / np.float32(L[r])).view(np.uint32))


def test_setting_parsers(noise, monkeypatch):
    assert noise.parse_root_noise(None) is None and noise.parse_root_noise("off") is None
    assert noise.parse_root_noise("0.25,0.3") == (0.25, 0.3, 0)
    assert noise.parse_root_noise("0.25, 0.3, 17") == (0.25, 0.3, 17)
    assert noise.parse_root_noise((0.25, 0.3, 5)) == (0.25, 0.3, 5)
    assert noise.parse_root_noise("0,0.3") is None
    for bad in ("0.25", "1.5,0.3", "0.25,0", "0.25,64", "a,b", "0.25,0.3,1,2"):
        with pytest.raises(ValueError):
            noise.parse_root_noise(bad)
    assert noise.parse_temperature_plies(None) == (None, 0.0)
    assert noise.parse_temperature_plies("8") == (8, 0.0)
    assert noise.parse_temperature_plies("8,0.5") == (8, 0.5)
    assert noise.parse_temperature_plies(8, 0.25) == (8, 0.25)
    for bad in ("-1", "8,-1", "x", "8,1,2", "8,inf"):
        with pytest.raises(ValueError):
            noise.parse_temperature_plies(bad)
    monkeypatch.delenv("UTTT_ROOT_NOISE", raising=False)
    monkeypatch.delenv("UTTT_TEMPERATURE_PLIES", raising=False)
    assert noise.root_noise_from_env() is None and noise.temperature_plies_from_env() == (None, 0.0)
    monkeypatch.setenv("UTTT_ROOT_NOISE", "0.25,0.3,4")
    monkeypatch.setenv("UTTT_TEMPERATURE_PLIES", "8")
    assert noise.root_noise_from_env() == (0.25, 0.3, 4) and noise.temperature_plies_from_env() == (8, 0.0)
