"""GPU: the two forms of the compact direction's triangular products (csrc/lbfgs_device.h) write the same words.

lb_direction_compact takes the no-wrap form of w = R^-1 p and a = R^-T z (lb_cmp_tri_nowrap: running addresses, a lane's
columns in batches of eight) while the live window does not wrap round the history ring (head + n <= 100), and the general
form (lb_cmp_tri: ring arithmetic per column) otherwise.  Both perform the same FMAs in the same order on the same lanes, so
a fit must not depend on which one ran.  The hooks build (-DMVFIT_DEBUG_HOOKS) reads MVFIT_DIR_GENERAL on the host: 1 forces
the general form in every direction call, of the fit kernels and of mvfit_lbfgs_kat.  Here: the same fits and the same
float64 run with the general form forced and with the automatic choice, compared word for word."""
import os

import numpy as np
import pytest

from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import MvFit, lbfgs_kat, stage_weights
from oracle import lbfgs_np as ln
from tests import lbfgs_follow as lf

pytestmark = pytest.mark.gpu

HOOKS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'mvsmplfitting_amd', 'libmvfit_hooks.so')
SWITCH = 'MVFIT_DIR_GENERAL'
TRACE_CAP = 2000                   # closures recorded per problem (the fits below take a few hundred to ~1000)


def _hooks():
    if not os.path.isfile(HOOKS):
        pytest.skip('libmvfit_hooks.so not built (make -C mvsmplfitting_amd/csrc hooks)')
    return HOOKS


def _forced_general(run):
    os.environ[SWITCH] = '1'
    try:
        return run()
    finally:
        del os.environ[SWITCH]


def _problems(eng, B, views=8, seed=5):
    cams = syn.make_camera_ring(views)
    fr = syn.make_frames(B, seed0=seed)
    x = np.zeros((B, 118), np.float32)
    for k, (a, b) in dict(betas=(0, 10), global_orient=(10, 13), body_pose=(13, 82), transl=(82, 85), scale=(85, 86)).items():
        x[:, a:b] = fr[k]
    eng.set_problems(cams, np.zeros((B, views, 17, 2), np.float32), np.ones((B, views, 17), np.float32))
    _, joints = eng.vertices(x)
    gt, conf = syn.make_observations(joints.cpu().numpy(), cams, seed=seed + 7)
    eng.set_problems(cams, gt, conf)
    x0 = np.zeros((B, 118), np.float32)
    x0[:, 85] = 1.0
    return x0


def _fit(eng, x0, history):
    tr = eng.fit_trace(TRACE_CAP)
    xf, st = eng.fit(x0, stage_weights(1536.0), history=history)
    out = dict(x=xf.cpu().numpy(), final=st['final_loss'].cpu().numpy(), ncl=st['n_closure'].cpu().numpy(),
               nit=st['n_iter'].cpu().numpy(), trace=tr.cpu().numpy())
    eng.fit_trace(0)
    return out


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


@pytest.mark.parametrize('history', [100, 4])
def test_fit_does_not_depend_on_the_form_of_the_triangular_products(history):
    """3 problems, 8 views, L2 prior, the four yaml stages; history 4 puts eviction on the path (the window then moves along
    the ring with every accepted pair)."""
    eng = MvFit(syn.make_body_model(0, skin_topk=4), library=_hooks())
    try:
        x0 = _problems(eng, 3)
        general = _forced_general(lambda: _fit(eng, x0, history))
        auto = _fit(eng, x0, history)
    finally:
        eng.close()
    print('history %d: closures %s, iterations %s, final losses %s' % (history, auto['ncl'], auto['nit'], auto['final']))
    assert auto['ncl'].max() <= TRACE_CAP, auto['ncl']                       # every closure of the fits was recorded
    assert np.all(np.isfinite(auto['final'])) and np.all(auto['ncl'] > 100)
    assert np.array_equal(auto['ncl'], general['ncl']) and np.array_equal(auto['nit'], general['nit'])
    for key in ('x', 'final', 'trace'):                                      # (the trace is NaN where nothing was written: words, not values)
        differing = int((_words(auto[key]) != _words(general[key])).sum())
        assert differing == 0, (history, key, differing)


def test_float64_run_through_a_ring_wrap_does_not_depend_on_the_form():
    """Chained Rosenbrock, D = 86, history 7: the run accepts 100 + 7 pairs or more (tests/lbfgs_follow.py: HEAD_WRAP), so the
    window passes from not wrapped (head + n <= 100) to wrapped and back, and the automatic choice changes form twice."""
    D, history = 86, 7
    assert (D, history) in lf.HEAD_WRAP
    hooks = _hooks()
    _, x0 = ln.kat_objective('rosen', D)

    def run():
        return lbfgs_kat(1 | 0x100, D, [0, 10, 13, D], x0, max_trace=400, library=hooks, history=history)
    xg, tg, ng, fg = _forced_general(run)
    xa, ta, na, fa = run()
    print('rosen D=%d history=%d: %d closures' % (D, history, na))
    assert na == ng and 100 + history < na == len(ta) < 400, (na, ng)         # (a pair takes at least one closure)
    assert int((_words(ta) != _words(tg)).sum()) == 0
    assert int((_words(xa) != _words(xg)).sum()) == 0 and np.float64(fa).tobytes() == np.float64(fg).tobytes()
