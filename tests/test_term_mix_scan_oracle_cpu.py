"""The three-operand restatement of the term mix (tests/term_mix_scan_oracle.py) against the two-operand one it extends
(tests/term_mix_oracle.py): with a scan share of 0 it is that oracle bit for bit, the scan operand unread; with the share live
the order of the adds is silhouette, vertex targets, scan."""
import numpy as np
import pytest

from tests import term_mix_oracle as tm
from tests import term_mix_scan_oracle as tms

B, N = 5, 33


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope='module')
def data():
    rng = np.random.default_rng(3)
    g = [rng.normal(0, 10.0 ** e, (B, N)).astype(np.float32) for e in (0, -3, 2)]
    L = [np.abs(rng.normal(0, 10.0 ** e, B)).astype(np.float32) for e in (1, -2, 3)]
    return g, L


@pytest.mark.parametrize('lam', [(2.0, 0.25), (0.3, 0.0), (0.0, 1.7), (1.0, 1.0)])
def test_a_scan_share_of_zero_is_the_two_operand_oracle(data, lam):
    g, L = data
    nan_g, nan_L = np.full_like(g[2], np.nan), np.full_like(L[2], np.nan)
    got = tms.mix_cotangent3(lam[0], g[0], L[0], lam[1], g[1], L[1], 0.0, nan_g, nan_L)
    want = tm.mix_cotangent(lam[0], g[0], L[0], lam[1], g[1], L[1])
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1]))
    got = tms.mix_cotangent3(lam[0], g[0], L[0], lam[1], g[1], L[1], 0.0, None, None)
    assert np.array_equal(_bits(got[0]), _bits(want[0]))


def test_the_parts_sum_without_a_scan_share_is_the_three_part_sum(data):
    rng = np.random.default_rng(4)
    parts = np.abs(rng.normal(0, 5, (B, 4))).astype(np.float32)
    parts[:, 3] = np.nan                                               # (never added)
    for shares in ((0.5, 2.0, 0.25), (0.0, 2.0, 0.25), (0.5, 0.0, 0.25)):
        assert np.array_equal(_bits(tms.mix_parts_sum4(shares + (0.0,), parts)), _bits(tm.mix_parts_sum(shares, parts[:, :3])))


def test_the_order_of_the_adds(data):
    """written out once more by hand: ((a + b) + c) in float32, and in float64 for the loss"""
    g, L = data
    ls, lv, lc = np.float32(0.3), np.float32(1.7), np.float32(2.5)
    got_g, got_L = tms.mix_cotangent3(ls, g[0], L[0], lv, g[1], L[1], lc, g[2], L[2])
    want_g = ((ls * g[0]) + (lv * g[1])) + (lc * g[2])
    assert want_g.dtype == np.float32 and np.array_equal(_bits(got_g), _bits(want_g))
    f = np.float64
    want_L = ((f(ls) * L[0].astype(f) + f(lv) * L[1].astype(f)) + f(lc) * L[2].astype(f)).astype(np.float32)
    assert np.array_equal(_bits(got_L), _bits(want_L))
    # a skipped first component does not become "0 +": -0.0 stays -0.0
    neg = np.full((1, 4), -0.0, np.float32)
    out, _ = tms.mix_cotangent3(0.0, None, None, 0.0, None, None, 1.5, neg, np.zeros(1, np.float32))
    assert np.signbit(out).all()
    parts = np.array([[1.0, 2.0, 3.0, 4.0]], np.float32)
    assert tms.mix_parts_sum4((0.5, 2.0, 0.25, 1.5), parts)[0] == np.float32(0.5 + 4.0 + 0.75 + 6.0)
