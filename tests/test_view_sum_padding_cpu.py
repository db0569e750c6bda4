"""CPU: a sequential float32 sum from +0 does not change a bit when the terms behind the V-th are replaced by +0.

The closure's loss phase (csrc/closure_device.h: loss_and_keypoint_grad, view_sum) adds the views' parts of a keypoint
gradient word in ascending order.  It reads all the rows the array has, selects `vv < V ? value : 0.f` and adds every
selected value, where it used to add only the first V.  The argument that no word changes: the running sum starts at +0, and
in round-to-nearest a sum is -0 only when both addends are -0, so the running sum is never -0 and s + (+0) is s bit for bit;
the first add, 0.f + p0, is kept and turns a -0 part into +0 as before.  Here the two forms are evaluated in numpy float32 on
inputs chosen against that argument: -0 and +0 parts, denormals, a part that cancels its predecessor exactly, all parts -0.
Rows >= V hold anything at all on the device (NaN included) and are only selected away: the padded form here gets NaN there
before the select."""
import numpy as np
import pytest

N = 16                      # MVFIT_MAX_VIEWS
BATCHES = (8, 16)           # the kernel's uniform choice: a batch of 8 when V <= 8, of 16 otherwise


def _sum_first(parts, V):
    """the loop as it was: s = 0; for vv < V: s += parts[vv]"""
    s = np.float32(0.0)
    for vv in range(V):
        s = np.float32(s + parts[vv])
    return s


def _sum_selected(parts, V, batch):
    """the batched form: all rows read, rows >= V selected to +0, every selected value added in the same order"""
    rows = np.array(parts[:batch], np.float32)
    sel = [rows[vv] if vv < V else np.float32(0.0) for vv in range(batch)]
    s = np.float32(0.0)
    for vv in range(batch):
        s = np.float32(s + sel[vv])
    return s


def _bits(x):
    return np.asarray(x, np.float32).reshape(1).view(np.uint32)[0]


def _cases():
    f = np.float32
    tiny = np.finfo(np.float32).tiny                      # smallest normal
    den = f(1e-45)                                        # smallest denormal
    rng = np.random.RandomState(7)
    out = {
        'all_minus_zero': np.full(N, -0.0, f),
        'all_plus_zero': np.zeros(N, f),
        'mixed_zeros': np.array([-0.0, 0.0] * (N // 2), f),
        'minus_zero_first': np.concatenate([[f(-0.0)], rng.randn(N - 1)]).astype(f),
        'denormals': np.array([den * (k + 1) * (-1) ** k for k in range(N)], f),
        'denormal_steps': np.array([tiny, -den, den, -tiny] * (N // 4), f),
        # every odd part cancels its predecessor exactly: the running sum is +0 (never -0) at every even V
        'cancels': np.array([v for k in range(N // 2) for v in (f(1.5 + k), f(-(1.5 + k)))], f),
        'cancels_negative_first': np.array([v for k in range(N // 2) for v in (f(-(0.3 + k)), f(0.3 + k))], f),
        'cancel_then_minus_zero': np.array([2.5, -2.5, -0.0, -0.0, 1e-40, -1e-40, -0.0, 3.0] * 2, f),
        'random': rng.randn(N).astype(f),
        'random_wide': (rng.randn(N) * 10.0 ** rng.randint(-30, 30, N)).astype(f),
    }
    assert np.signbit(out['all_minus_zero']).all() and np.signbit(out['cancel_then_minus_zero'][2])
    assert out['denormals'].all() and (np.abs(out['denormals']) < tiny).all()
    return out


CASES = _cases()


@pytest.mark.parametrize('name', list(CASES))
def test_padding_with_plus_zero_changes_no_bit(name):
    parts = CASES[name]
    for V in range(1, N + 1):
        want = _sum_first(parts, V)
        for batch in BATCHES:
            if V > batch:
                continue
            garbage = parts.copy()
            garbage[V:] = np.nan                          # what lies behind the V-th row is never added
            got = _sum_selected(garbage, V, batch)
            assert _bits(got) == _bits(want), (name, V, batch, want, got)


@pytest.mark.parametrize('name', list(CASES))
def test_running_sum_is_never_minus_zero(name):
    """the premise: from +0, no prefix sum is -0 (so adding +0 to it is exact)"""
    parts = CASES[name]
    for V in range(1, N + 1):
        s = _sum_first(parts, V)
        assert not (s == 0 and np.signbit(s)), (name, V)


def test_first_add_turns_a_minus_zero_part_into_plus_zero():
    parts = CASES['all_minus_zero']
    for V in range(1, N + 1):
        for batch in BATCHES:
            if V <= batch:
                assert _bits(_sum_selected(parts, V, batch)) == 0
        assert _bits(_sum_first(parts, V)) == 0


def test_a_sum_started_at_minus_zero_would_change():
    """why the sum's start matters: started at -0 the all -0 sum is -0 and a selected +0 flips its sign"""
    s = np.float32(-0.0)
    s = np.float32(s + np.float32(-0.0))
    assert _bits(s) == 0x80000000
    assert _bits(np.float32(s + np.float32(0.0))) == 0
