"""CPU: the vertex-target oracle (tests/vertex_target_oracle.py) on cases worked by hand."""
import numpy as np

from tests.vertex_target_oracle import vertex_target_loss


def test_one_vertex_two_targets():
    V = np.array([[[1.0, 2.0, 3.0]]], np.float32)
    T = np.array([[[[0.0, 0.0, 0.0]], [[2.0, 2.0, 1.0]]]], np.float32)
    a = np.array([[0.5, 2.0]], np.float32)
    L, g = vertex_target_loss(V, T, a)
    # d_0 = (1, 2, 3), d_1 = (-1, 0, 2): L = 0.5 * 14 + 2 * 5 = 17; g = 2 * (0.5 d_0 + 2 d_1) = (-3, 2, 11)
    assert L.shape == (1,) and L[0] == 17.0
    assert g.dtype == np.float32 and np.array_equal(g, np.array([[[-3.0, 2.0, 11.0]]], np.float32))


def test_the_subtraction_is_fp32_and_the_sum_float64():
    # 1 + 2^-24 is not a float: the fp32 subtraction sees 1 exactly.  2^-30 survives beside 2^20 only in a float64 sum
    V = np.array([[[1.0, 0.0, 0.0]]], np.float32)
    T = np.array([[[[-2.0 ** -30, 0.0, 0.0]], [[1.0 - 2.0 ** 20, 0.0, 0.0]]]], np.float32)
    a = np.array([[1.0, 1.0]], np.float32)
    L, g = vertex_target_loss(V, T, a)
    d0 = np.float64(np.float32(np.float32(1.0) + np.float32(2.0 ** -30)))       # rounds to 1
    assert d0 == 1.0
    assert L[0] == 1.0 + 2.0 ** 40
    assert g[0, 0, 0] == np.float32(2.0 * (1.0 + 2.0 ** 20))


def test_a_zero_weight_row_is_never_read():
    rng = np.random.default_rng(0)
    V = rng.normal(size=(2, 5, 3)).astype(np.float32)
    T = rng.normal(size=(2, 3, 5, 3)).astype(np.float32)
    a = np.array([[1.5, 0.0, 0.25], [0.0, 2.0, 0.0]], np.float32)
    L, g = vertex_target_loss(V, T, a)
    T2 = T.copy()
    T2[0, 1] = np.nan
    T2[1, 0] = np.nan
    T2[1, 2] = np.inf
    L2, g2 = vertex_target_loss(V, T2, a)
    assert np.array_equal(L, L2) and np.array_equal(g, g2) and np.isfinite(L2).all() and np.isfinite(g2).all()
    d = V[1].astype(np.float64) - T[1, 1].astype(np.float64)
    assert abs(L[1] - 2.0 * (d * d).sum()) <= 1e-6 * L[1]


def test_all_weights_zero_give_zero_and_zeros():
    V = np.ones((1, 4, 3), np.float32)
    T = np.full((1, 2, 4, 3), np.nan, np.float32)
    L, g = vertex_target_loss(V, T, np.zeros((1, 2), np.float32))
    assert L[0] == 0.0 and g.dtype == np.float32 and not g.any() and not np.signbit(g).any()
