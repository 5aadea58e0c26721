"""uttt_nn_wino3h_weights (the tower conv's host weight transform, csrc/wino3h_conv.hip) against a numpy
f64 restatement of U = G g G^T: the documented fragment layout, the f16 hi/lo split, the power-of-two
scale, its invariance under power-of-two weight scalings, and the refusals (non-finite weights; weights so
small that the scale is no finite float). No GPU: the function runs on the host.

G is written here from the Toom-Cook points {0, 1, -1, 2, inf} (include/uttt_nn.h), not read from the
library: row i of a finite point p_i is [1, p_i, p_i^2] / prod_{j != i} (p_i - p_j), the point at
infinity's row is [0, 0, 1]."""
import ctypes

import numpy as np
import pytest

C, NP = 128, 25
POINTS = (0.0, 1.0, -1.0, 2.0)  # + the point at infinity
UTTT_OK, UTTT_ERR_ARG = 0, -1


def toom_cook_g():
    rows = []
    for i, p in enumerate(POINTS):
        n = np.prod([p - q for j, q in enumerate(POINTS) if j != i])
        rows.append([1.0 / n, p / n, p * p / n])
    rows.append([0.0, 0.0, 1.0])
    return np.array(rows, np.float64)


def reference_u(w):
    """U[xi = 5p + q][ci][co] = (G g G^T)[p][q] of w[co][ci][3][3], f64: (G g) G^T, every three-term sum
    taken left to right without fused multiply-adds. The order is part of the restatement: rows -1 and 2 of G
    are sixths, so U is not exact in f64, and where U su falls within an f64 rounding of the midpoint of two
    f16 values (2 of 409,600 elements of the folded set) its last bit decides which one hi is."""
    G = toom_cook_g()
    g = w.astype(np.float64)  # [co][ci][a][b]
    tg = sum_lr(G[:, 0, None] * g[:, :, None, 0, :], G[:, 1, None] * g[:, :, None, 1, :],
                G[:, 2, None] * g[:, :, None, 2, :])  # [co][ci][p][b]
    U = sum_lr(tg[..., None, 0] * G[:, 0], tg[..., None, 1] * G[:, 1], tg[..., None, 2] * G[:, 2])  # [co][ci][p][q]
    return np.ascontiguousarray(U.transpose(2, 3, 1, 0)).reshape(NP, C, C)


def sum_lr(a, b, c):
    return (a + b) + c


def decode(u):
    """(hi, lo) as f16 arrays [xi][ci][co] from the documented order
    U[xi][ci/32][hi|lo][co/16][(ci%32)/8][co%16][ci%8]."""
    a = u.view(np.float16).reshape(NP, C // 32, 2, C // 16, 4, 16, 8)
    a = a.transpose(2, 0, 1, 4, 6, 3, 5).reshape(2, NP, C, C)  # [h][xi][ci/32, (ci%32)/8, ci%8][co/16, co%16]
    return a[0], a[1]


def raw_weights(lib, w):
    """(return code, u, u_scale) of the C entry itself."""
    wc = np.ascontiguousarray(w, dtype=np.float32)
    assert wc.shape == (C, C, 3, 3)
    u = np.full(NP * C * C * 2, 0x7E00, np.uint16)  # f16 NaN: every element must be written
    su = ctypes.c_float(-1.0)
    rc = lib.uttt_nn_wino3h_weights(wc.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ctypes.c_void_p(u.ctypes.data),
                                    ctypes.byref(su))
    return rc, u, su.value


@pytest.fixture(scope="module")
def base_w():
    from uttt_amd.model import fold_bn, random_network
    blk = random_network(3).residual_blocks[5]
    w, _ = fold_bn(blk.conv1, blk.bn1)
    return w.numpy().copy()


def weight_sets(base_w):
    spike = base_w.copy()
    spike[77, 41, 2, 0] = 1e4 * np.abs(base_w).max()  # one entry 1e4 times the rest: most of U far below the scale
    return {"folded": base_w, "2^-40": base_w * np.float32(2.0 ** -40), "2^+40": base_w * np.float32(2.0 ** 40),
            "spike": spike, "zeros": np.zeros_like(base_w)}


def test_g_is_the_toom_cook_matrix_of_the_documented_points():
    """The restatement's own premise: with A^T the evaluation [1, p, p^2] at the points (inf: [0, 0, 1]) and
    B^T the rows of coefficients of prod_{j != i} (x - p_j) (inf: prod_j (x - p_j)), A^T [(G g) . (B^T d)] is
    the 1-D correlation of d (5) with g (3): F(3, 3) on these points."""
    G = toom_cook_g()
    AT = np.array([[1, p, p * p] for p in POINTS] + [[0, 0, 1]], np.float64).T
    BT = []
    for i in range(4):
        BT.append(np.concatenate([np.poly([q for j, q in enumerate(POINTS) if j != i])[::-1], [0.0]]))
    BT.append(np.poly(POINTS)[::-1])
    BT = np.array(BT)
    rng = np.random.default_rng(0)
    d, g = rng.standard_normal(5), rng.standard_normal(3)
    want = np.array([d[k:k + 3] @ g for k in range(3)])
    assert np.allclose(AT @ ((G @ g) * (BT @ d)), want, rtol=0, atol=1e-13)


@pytest.mark.parametrize("name", ["folded", "2^-40", "2^+40", "spike", "zeros"])
def test_layout_split_and_scale(engine_lib, base_w, name):
    w = weight_sets(base_w)[name]
    rc, u, su = raw_weights(engine_lib, w)
    assert rc == UTTT_OK
    U = reference_u(w)
    umax = np.abs(U).max()
    if name == "zeros":
        assert su == 1.0 and not (u & 0x7FFF).any()  # zeros of either sign (G has negative entries)
        return
    # the scale: a finite power of two that puts max |U| into [2^14, 2^15)
    assert np.isfinite(su) and su > 0 and np.frexp(su)[0] == 0.5
    assert 2.0 ** 14 <= umax * float(su) < 2.0 ** 15, (umax, su)
    hi, lo = decode(u)
    want = U * float(su)
    assert np.isfinite(hi).all() and np.isfinite(lo).all()
    # hi is the round-to-nearest f16 of the scaled f64 value, exactly
    assert np.array_equal(hi.view(np.uint16), want.astype(np.float16).view(np.uint16))
    # hi + lo: two round-to-nearest f16 roundings (2^-11 each), floored by half the f16 subnormal spacing
    err = np.abs(hi.astype(np.float64) + lo.astype(np.float64) - want)
    bound = np.maximum(2.0 ** -22 * np.abs(want), 2.0 ** -25)
    worst = (err / bound).max()
    assert worst <= 1.0, (name, worst)


def test_python_wrapper_returns_the_same_bits(engine_lib, base_w):
    import torch
    from uttt_amd.nnfast import wino3h_weights
    _, u, su = raw_weights(engine_lib, base_w)
    ut, sut = wino3h_weights(torch.from_numpy(base_w))
    assert sut == su and np.array_equal(ut.numpy().view(np.uint16), u)


@pytest.mark.parametrize("k", [-40, 40, 1, -97])
def test_power_of_two_invariance(engine_lib, base_w, k):
    """Weights times 2^k (exact in f32: nothing leaves the normal range): the same u bits, su times 2^-k."""
    scaled = base_w * np.float32(2.0 ** k)
    assert np.array_equal(scaled.astype(np.float64), base_w.astype(np.float64) * 2.0 ** k)
    for w in (base_w, weight_sets(base_w)["spike"]):
        rc0, u0, su0 = raw_weights(engine_lib, w)
        rc1, u1, su1 = raw_weights(engine_lib, w * np.float32(2.0 ** k))
        assert rc0 == UTTT_OK and rc1 == UTTT_OK
        assert np.array_equal(u0, u1)
        assert float(su1) == float(su0) * 2.0 ** -k


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_nonfinite_weights_are_refused(engine_lib, base_w, bad):
    from uttt_amd.nnfast import wino3h_weights
    import torch
    w = base_w.copy()
    w[3, 100, 1, 1] = bad
    rc, _, _ = raw_weights(engine_lib, w)
    assert rc == UTTT_ERR_ARG
    assert b"non-finite" in engine_lib.uttt_last_error()
    with pytest.raises(ValueError, match="non-finite"):
        wino3h_weights(torch.from_numpy(w))


def test_weights_too_small_for_a_float_scale_are_refused(engine_lib, base_w):
    """max |U| < 2^-113 needs su = 2^e with e > 127: the double su cast to float was +inf, the conv's
    u_scale > 0 check accepted it, and 1 / (sv su) = 0 made every output relu(bias). The function refuses
    such weights; the smallest it accepts (max |U| in [2^-113, 2^-112)) get su = 2^127."""
    umax = np.abs(reference_u(base_w)).max()
    e = int(np.frexp(umax)[1])  # 2^(e-1) <= umax < 2^e
    # the largest scaling the function must refuse, and the next one up, which it must accept
    for k, ok in ((-113 - e, False), (-112 - e, True)):
        w = base_w * np.float32(2.0 ** k)  # (the smallest weights round to f32 subnormals: U is taken of w itself)
        m = np.abs(reference_u(w)).max()
        assert (2.0 ** -113 <= m < 2.0 ** -112) if ok else (0 < m < 2.0 ** -113)
        rc, u, su = raw_weights(engine_lib, w)
        if ok:
            assert rc == UTTT_OK and su == 2.0 ** 127
            hi, _ = decode(u)
            assert np.array_equal(hi.view(np.uint16), (reference_u(w) * 2.0 ** 127).astype(np.float16).view(np.uint16))
        else:
            assert not (rc == UTTT_OK and not np.isfinite(su)), "a non-finite u_scale was returned"
            assert rc == UTTT_ERR_ARG
            assert b"too small" in engine_lib.uttt_last_error()
