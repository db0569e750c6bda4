"""GPU: the two forms of the compact direction's mat-vecs (csrc/lbfgs_device.h) write the same words.

In the 512-thread fit kernels t = Y w - q and d = S a - gamma t meet their sums in registers (lb_cmp_matvec_row: the sixteen
row classes of a four-element chunk in the sixteen lanes of one DPP row, one pair add, a seven-step ordered chain, one
barrier); the form they replaced leaves eight per-wave partials in LDS and adds them in a combine loop between two barriers
(lb_cmp_matvec).  Same FMAs and adds in the same order, on other lanes - so a fit must not depend on which one ran.  The hooks
build (-DMVFIT_DEBUG_HOOKS) reads MVFIT_DIR_MATVEC_LDS on the host: 1 makes every direction call take the LDS form.  Here: the
same fits and the same float64 run with the switch on and off, compared word for word - every closure's trial point and
loss, the closure and iteration counts, the final parameters and losses.

Shapes: 2 problems x 2 views.  ld = 88 (plain L2 prior: 22 live chunks) and ld = 52 (synthetic VPoser decoder: 13 live chunks,
a partly filled wave, DPP rows whose chunk is dead); history 100 (the window grows through 1, 15, 16, 17, 32, 33 live pairs:
row class c holds rows c, c + 16, ...) and history 5 (the ring wraps and evicts within a few dozen closures: live rows
scattered over the classes, head != 0); the four default stages (a stage reset zero-fills the history: one live pair in the
next direction); MVFIT_F_REUSE_OUTER_VALUE (the other loop of lbfgs_round)."""
import os

import numpy as np
import pytest

from mvsmplfitting_amd import _lib
from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import MvFit, lbfgs_kat, stage_weights
from oracle import lbfgs_np as ln
from tests import lbfgs_follow as lf

pytestmark = pytest.mark.gpu

HOOKS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'mvsmplfitting_amd', 'libmvfit_hooks.so')
SWITCH = 'MVFIT_DIR_MATVEC_LDS'
TRACE_CAP = 2000                   # closures recorded per problem
B, VIEWS = 2, 2


def _hooks():
    if not os.path.isfile(HOOKS):
        pytest.skip('libmvfit_hooks.so not built (make -C mvsmplfitting_amd/csrc hooks)')
    return HOOKS


def _lds_form(run):
    os.environ[SWITCH] = '1'
    try:
        return run()
    finally:
        del os.environ[SWITCH]


def _problems(eng, seed=5):
    cams = syn.make_camera_ring(VIEWS)
    fr = syn.make_frames(B, seed0=seed)
    x = np.zeros((B, 118), np.float32)
    for k, (a, b) in dict(betas=(0, 10), global_orient=(10, 13), body_pose=(13, 82), transl=(82, 85), scale=(85, 86)).items():
        x[:, a:b] = fr[k]
    eng.set_problems(cams, np.zeros((B, VIEWS, 17, 2), np.float32), np.ones((B, VIEWS, 17), np.float32))
    _, joints = eng.vertices(x)
    gt, conf = syn.make_observations(joints.cpu().numpy(), cams, seed=seed + 7)
    eng.set_problems(cams, gt, conf)
    x0 = np.zeros((B, 118), np.float32)
    x0[:, 85] = 1.0
    return x0


def _fit(eng, x0, history, flags):
    tr = eng.fit_trace(TRACE_CAP)
    xf, st = eng.fit(x0, stage_weights(1536.0, flags=flags), history=history)
    out = dict(x=xf.cpu().numpy(), final=st['final_loss'].cpu().numpy(), ncl=st['n_closure'].cpu().numpy(),
               nit=st['n_iter'].cpu().numpy(), trace=tr.cpu().numpy())
    eng.fit_trace(0)
    return out


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _same_words(case, rows, lds):
    print('%s: closures %s, iterations %s, final losses %s' % (case, rows['ncl'], rows['nit'], rows['final']))
    assert rows['ncl'].max() <= TRACE_CAP, rows['ncl']                       # every closure of the fits was recorded
    assert np.all(np.isfinite(rows['final'])) and np.all(rows['ncl'] > 100)
    assert np.array_equal(rows['ncl'], lds['ncl']) and np.array_equal(rows['nit'], lds['nit'])
    for key in ('x', 'final', 'trace'):                                      # (the trace is NaN where nothing was written: words, not values)
        differing = int((_words(rows[key]) != _words(lds[key])).sum())
        assert differing == 0, (case, key, differing)


@pytest.fixture(scope='module')
def l2_engine():
    eng = MvFit(syn.make_body_model(0, skin_topk=4), library=_hooks())
    yield eng, _problems(eng)
    eng.close()


@pytest.mark.parametrize('history', [100, 5])
def test_l2_fit_does_not_depend_on_the_form_of_the_mat_vecs(l2_engine, history):
    """ld = 88, the four yaml stages.  history 100: a stage that runs more than 34 iterations has had 1 ... 33 live pairs in
    its window, and with four stages one of them does if the fit runs more than 4 x 34; history 5: head moves with every
    accepted pair from the sixth on."""
    eng, x0 = l2_engine
    lds = _lds_form(lambda: _fit(eng, x0, history, 0))
    rows = _fit(eng, x0, history, 0)
    _same_words('l2 history %d' % history, rows, lds)
    if history == 100:
        assert rows['nit'].max() > 4 * 34, rows['nit']


def test_l2_fit_with_reuse_of_the_step_start_value(l2_engine):
    """MVFIT_F_REUSE_OUTER_VALUE: lbfgs_round's bounded loop around direction() instead of the two-trip form."""
    eng, x0 = l2_engine
    lds = _lds_form(lambda: _fit(eng, x0, 100, _lib.F_REUSE_OUTER_VALUE))
    rows = _fit(eng, x0, 100, _lib.F_REUSE_OUTER_VALUE)
    _same_words('l2 reuse', rows, lds)


@pytest.mark.parametrize('history', [100, 5])
def test_vposer_fit_does_not_depend_on_the_form_of_the_mat_vecs(history):
    """ld = 52: 13 live chunks (six waves with two, one with one live and one dead chunk), the decoder in the fit's own
    workgroups (no helper answers that could time out: the two runs are deterministic)."""
    eng = MvFit(syn.make_body_model(0, skin_topk=4), vposer=syn.make_vposer_decoder(), library=_hooks())
    try:
        x0 = _problems(eng)
        eng.set_options(vposer_helpers=0)
        lds = _lds_form(lambda: _fit(eng, x0, history, _lib.F_VPOSER))
        rows = _fit(eng, x0, history, _lib.F_VPOSER)
    finally:
        eng.close()
    _same_words('vposer history %d' % history, rows, lds)


def test_float64_run_does_not_depend_on_the_switch():
    """lbfgs_kat in compact form (chained Rosenbrock, D = 86, history 7, through a ring wrap): the 64-thread float64
    instantiation keeps the LDS form (one wave, seven zero partials), so the switch must change nothing."""
    D, history = 86, 7
    assert (D, history) in lf.HEAD_WRAP
    hooks = _hooks()
    _, x0 = ln.kat_objective('rosen', D)

    def run():
        return lbfgs_kat(1 | 0x100, D, [0, 10, 13, D], x0, max_trace=400, library=hooks, history=history)
    xl, tl, nl, fl = _lds_form(run)
    xr, tr, nr, fr = run()
    print('rosen D=%d history=%d: %d closures' % (D, history, nr))
    assert nr == nl and 100 + history < nr == len(tr) < 400, (nr, nl)
    assert int((_words(tr) != _words(tl)).sum()) == 0
    assert int((_words(xr) != _words(xl)).sum()) == 0 and np.float64(fr).tobytes() == np.float64(fl).tobytes()
