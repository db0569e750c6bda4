"""GPU: the device L-BFGS (float64 instantiation, lbfgs_device.h) through every line-search branch, case for case of
tests/lbfgs_branch_cases.py, against the reference's own runs (tests/golden/lbfgs_kat_branches.npz) - both direction forms.

Per case: the reference's closure count; the first 40 trial points to the 1e-7 of
test_gpu_lbfgs.py::test_device_lbfgs_follows_reference (absolute in x like there; relative to |x|inf on the two unbounded
objectives, whose points reach 1e39);
the WHOLE device trace replayed by the oracle (tests/lbfgs_follow.py) stays within lbfgs_follow.TOL of what the oracle
proposes on the device's own iterates, and that replay takes the branch sequence recorded for the reference - the device
walked each branch at the same closure and agreed there; final loss and final point as in
test_gpu_lbfgs.py::test_device_gtd_exit_after_direction.  What these checks can tell apart is pinned on the CPU
(tests/test_lbfgs_branch_cases_cpu.py).  Measured worst replay deviation per case: DESIGN.md 4.3.
"""
import math

import numpy as np
import pytest

from mvsmplfitting_amd.engine import MvFitError, lbfgs_kat
from oracle import lbfgs_np as ln
from tests import lbfgs_branch_cases as bc
from tests import lbfgs_follow as lf

pytestmark = pytest.mark.gpu
GOLD = bc.load_golden()


def run_device(case, form, x0=None, **over):
    kind = bc.KIND[case['kind']] | (0x100 if form == 'compact' else 0)
    D = case['D']
    x0 = GOLD[case['name'] + '_x0'] if x0 is None else x0
    return lbfgs_kat(kind, D, [0, 10, 13, D], x0, max_trace=int(GOLD[case['name'] + '_n']) + 8, **dict(bc.device_opts(case), **over))


UNBOUNDED = ('steep', 'steep2')          # trial points reach 1e39: compared relative to |x|inf; every other objective absolutely


def dist(a, b, relative):
    """worst |a - b| over the entries where b is finite - relative: over max(1, |b|inf) there; the others have to be
    non-finite in the same way (inf for NaN otherwise)"""
    ok = np.isfinite(b)
    if not np.array_equal(a[~ok], b[~ok], equal_nan=True):
        return float('inf')
    d = float(np.abs(a[ok] - b[ok]).max(initial=0.0))
    return d / max(1.0, np.abs(b[ok]).max(initial=0.0)) if relative else d


@pytest.mark.parametrize('form', ['two_loop', 'compact'])
@pytest.mark.parametrize('case', bc.CASES, ids=lambda c: c['name'])
def test_device_walks_every_line_search_branch(case, form):
    name, D = case['name'], case['D']
    ref, n_ref = GOLD[name + '_trace'], int(GOLD[name + '_n'])
    xf, trace, ncl, final = run_device(case, form)
    assert ncl == n_ref == len(trace), (name, form, ncl, n_ref)
    unb = case['kind'] in UNBOUNDED
    for i in range(min(n_ref, 40)):
        assert dist(trace[i][:D], ref[i][:D], unb) < 1e-7, (name, form, i)
        assert dist(trace[i][D:], ref[i][D:], True) <= 1e-7, (name, form, i)
    with np.errstate(all='ignore'):
        fo = lf.replay(trace, D, kind=case['kind'], case=case)
    assert not fo.exhausted and len(fo.trace) == len(trace), (name, form, len(fo.trace), fo.exhausted)
    worst = max(fo.dev)
    print('%s %s: %d closures, worst replay deviation %.2g' % (name, form, ncl, worst))
    assert worst <= lf.TOL, (name, form, worst, int(np.argmax(fo.dev)))
    assert fo.branches == bc.tags_of(GOLD, name), (name, form)
    ref_final = float(GOLD[name + '_final'])
    if math.isnan(ref_final):
        assert math.isnan(final), (name, form, final)
    else:
        assert abs(final - ref_final) <= 1e-9 * max(1.0, abs(final)), (name, form, final, ref_final)
    assert dist(xf, GOLD[name + '_xf'], unb) < 1e-8, (name, form)
    if name == bc.NONFINITE:
        assert not np.isfinite(trace[0][D]) and fo.branches[-1][1] == 'fit_nonfinite'


@pytest.mark.parametrize('kind', sorted(bc.KIND, key=bc.KIND.get))
def test_device_objective_is_the_oracle_s(kind):
    """kat_eval against oracle/lbfgs_np.py:kat_objective at a point away from the start, value and gradient: the trace's
    first row holds the loss there, and its second row is the first trial point x - t g, t = min(1, 1 / sum |g|)
    (lbfgs_ls.py:313, :371)."""
    D = 49
    fn, x0 = ln.kat_objective(kind, D)
    x = x0 + 0.37 * np.cos(1.3 * np.arange(D) + 0.2) + 0.9
    f, g = fn(x)
    _, trace, ncl, _ = lbfgs_kat(bc.KIND[kind], D, [0, 10, 13, D], x, max_trace=4, max_iter=1, maxiters=1, tolerance_grad=1e-30)
    assert ncl >= 2
    # two summation orders of D terms: D 2^-52 sum |terms|, and sum |terms| < 500 max(1, |f|) at this point for every kind
    assert abs(trace[0][D] - f) <= 1e-11 * max(1.0, abs(f)), (kind, trace[0][D], f)
    t = min(1.0, 1.0 / np.abs(g).sum())
    assert np.abs((x - trace[1][:D]) / t - g).max() <= 1e-9 * np.abs(g).max(), kind


def test_unknown_objective_is_refused():
    x0 = np.zeros(49)
    for kind in (len(bc.KIND), 99, 0x100 | len(bc.KIND), -1):
        with pytest.raises(MvFitError, match='-1'):
            lbfgs_kat(kind, 49, [0, 10, 13, 49], x0)
