"""CPU: the NumPy restatement of the term mix's arithmetic (tests/term_mix_oracle.py) on hand-worked cases: values chosen so
that every rounding is visible and the expected bits can be written down."""
import numpy as np

from tests import term_mix_oracle as tm

f32, f64 = np.float32, np.float64
EPS = f32(2.0 ** -23)


def test_cotangent_two_rounded_products_and_one_rounded_add():
    # lam = 1 + 2^-23, g = 1 + 2^-23: the exact product 1 + 2^-22 + 2^-46 rounds to 1 + 2^-22; a fused multiply-add with
    # the second component -1 would keep the 2^-46 and return 2^-22 + 2^-46, the separately rounded form returns 2^-22
    lam = f32(1) + EPS
    g_sil = np.array([[[lam, 2.0, -3.0]]], f32)
    g_vt = np.array([[[-1.0, 0.5, 4.0]]], f32)
    g, L = tm.mix_cotangent(lam, g_sil, np.array([3.0], f32), 1.0, g_vt, np.array([0.25], f32))
    assert g.dtype == f32 and g[0, 0, 0] == f32(2.0 ** -22)
    assert g[0, 0, 1] == f32(2) * lam + f32(0.5) and g[0, 0, 2] == f32(f32(-3) * lam) + f32(4)
    # L_v: both products exact in float64, one float64 add, one rounding to float32
    assert L[0] == f32(f64(lam) * 3.0 + 0.25)
    assert L[0] == f32(3.25) + f32(2.0 ** -21)           # 3 * 2^-23 = 1.5 ulp of 3.25: the tie goes to the even 2 ulp


def test_cotangent_skips_a_component_with_share_zero():
    g_sil = np.array([[[1.5, -0.0, 2.0]]], f32)
    nan = np.full((1, 1, 3), np.nan, f32)
    g, L = tm.mix_cotangent(0.5, g_sil, np.array([2.0], f32), 0.0, nan, np.array([np.nan], f32))
    assert np.array_equal(g, np.array([[[0.75, -0.0, 1.0]]], f32)) and np.signbit(g[0, 0, 1])      # not added: -0 stays
    assert L[0] == f32(1.0)
    g, L = tm.mix_cotangent(0.0, None, None, 2.0, g_sil, np.array([2.0], f32))
    assert np.array_equal(g, np.array([[[3.0, -0.0, 4.0]]], f32)) and L[0] == f32(4.0)


def test_record_merge_by_hand():
    # S_sc = 3, S_v = 4, lam = 1: Q = 25, S = 5, entry = (3 a + 4 b) / 5
    sc = np.array([[3.0, 1.0, -2.0, 0.5]], f32)
    rv = np.array([[4.0, 0.5, 1.0, -0.25]], f32)
    out = tm.mix_record(1.0, sc, rv)
    assert np.array_equal(out, np.array([[5.0, 1.0, -0.4, 0.1]], f64).astype(f32))
    # lam = 4: Q = 4 * 9 + 16 = 52, entry = (12 a + 4 b) / sqrt(52)
    out = tm.mix_record(4.0, sc, rv)
    r = np.sqrt(f64(52))
    assert np.array_equal(out, np.array([[r, 14 / r, -20 / r, 5 / r]]).astype(f32))


def test_record_passes_the_scene_record_through_when_the_vertex_terms_pay_nothing():
    rng = np.random.default_rng(0)
    sc = rng.normal(0, 1, (3, 516)).astype(f32)
    sc[:, 0] = np.abs(sc[:, 0])
    rv = np.zeros_like(sc)
    assert np.array_equal(tm.mix_record(1.0, sc, rv).view(np.uint32), sc.view(np.uint32))
    assert not np.array_equal(tm.mix_record(0.5, sc, rv), sc)


def test_record_is_zero_below_flt_min():
    sc = np.array([[1e-20, 5.0, 6.0], [0.0, 7.0, 8.0]], f32)         # Q = 1e-40 < FLT_MIN, and 0
    rv = np.array([[0.0, 1.0, 1.0], [0.0, 2.0, 2.0]], f32)
    out = tm.mix_record(1.0, sc, rv)
    assert out.dtype == f32 and not out.any()
    sc[0, 0] = 2e-19                                                 # Q = 4e-38 >= FLT_MIN
    out = tm.mix_record(1.0, sc, rv)
    assert out[0, 0] == sc[0, 0] and out[0, 1] == 5.0


def test_parts_sum_and_scene_part():
    # (0.5 * 3 + 2 * 0.25) + 0.25 * 8 = 4
    s = tm.mix_parts_sum((0.5, 2.0, 0.25), np.array([[3.0, 0.25, 8.0], [0.0, 0.0, 0.0]], f32))
    assert s.dtype == f32 and np.array_equal(s, np.array([4.0, 0.0], f32))
    # S = 1 + 2^-23: S^2 = 1 + 2^-22 + 2^-46 in float64, 1 + 2^-22 in float32
    assert tm.scene_part(np.array([f32(1) + EPS]))[0] == f32(1) + f32(2.0 ** -22)
    # one rounding: float32(float64 sum), not a float32 sum of float32 products
    lam, p = f32(1) + EPS, f32(1) + EPS
    got = tm.mix_parts_sum((lam, lam, 0.0), np.array([[p, -p, 0.0]], f32))
    assert got[0] == 0.0
