"""GPU: the loss phase gives the same words whether its view sums read all rows and select, or loop over conditional reads.

E4 (csrc/closure_device.h: loss_and_keypoint_grad) ends with two sums over a run-time count: g_kp[k][a] over the V views'
parts (threads 64 .. 114) and g_tau over the data term's per-wave partials (threads 0 .. 2; with MVFIT_F_USE_3D both also
add the 3-D term's part).  They read every row the arrays have in one batch - 8 rows when V <= 8, all 16 otherwise -, select
`vv < V ? value : 0.f` and add in ascending order; tests/test_view_sum_padding_cpu.py holds the argument that a selected +0
changes no word.  The hooks build (-DMVFIT_DEBUG_HOOKS) reads MVFIT_VIEW_SUMS_SERIAL when a ctx is created: 1 sets bit 2
of ModelLds::stream_late in the uploaded image and that ctx's kernels take the loops of conditional reads they had before.
Here: two engines per case, one created with the switch on, compared word for word - loss and the 118 gradient words of
mvfit_closure at the four points of tests/closure_bits_cases.py in the L2, GMM and VPoser modes and with MVFIT_F_USE_3D,
and whole L2 fits at history 100 (parameters, final losses, closure and iteration counts, every trace row) on the
single-launch kernel and on the chained step kernel (round_mode = 1).

Shapes: 2 problems; views 1, 2, 7, 8, 9, 16 - the edges of the 8- and 16-wide batches (8 | 9) and of the data term's wave
counts (17 V threads: 1 wave up to 3 views, 3 waves at 7-11 views, 5 at 16).  One view of problem 0 has zero confidence: its
parts are +-0.  The four points are those of the recorded inputs; the observations are made here for each view count (the
float64 oracle's keypoints, once per count)."""
import functools
import os

import numpy as np
import pytest

from mvsmplfitting_amd import _lib
from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import MvFit, stage_weights
from tests import closure_bits_cases as cb

pytestmark = pytest.mark.gpu

HOOKS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'mvsmplfitting_amd', 'libmvfit_hooks.so')
SWITCH = 'MVFIT_VIEW_SUMS_SERIAL'
TRACE_CAP = 2000
B = 2
VIEWS = (1, 2, 7, 8, 9, 16)
MODES = cb.MODES + ('l2_3d',)


def _hooks():
    if not os.path.isfile(HOOKS):
        pytest.skip('libmvfit_hooks.so not built (make -C mvsmplfitting_amd/csrc hooks)')
    return HOOKS


@pytest.fixture(scope='module')
def points():
    return dict(np.load(cb.GOLDEN))['x'][:, :B]                           # [4, B, 118]


@functools.lru_cache(maxsize=None)
def _keypoints():
    from oracle import closure_np as cn
    orc = cn.ClosureOracle(cb.model(), np.float64)
    fr = syn.make_frames(B, seed0=3100)
    return np.stack([orc.body(dict({k: fr[k][b] for k in fr}, use_vposer=False), want_cache=False)['joints'] for b in range(B)])


@functools.lru_cache(maxsize=None)
def _problem(V):
    """cams, gt[B, V, 17, 2], conf[B, V, 17] with one view of problem 0 at zero confidence, gt3d[B, 17, 3], conf3d[B, 17]"""
    kp = _keypoints()
    cams = syn.make_camera_ring(V)
    gt, conf = syn.make_observations(kp, cams, seed=3107 + V)
    conf = conf.copy()
    conf[0, V // 2] = 0.0
    rng = np.random.RandomState(40 + V)
    gt3d = (kp + 0.02 * rng.randn(*kp.shape)).astype(np.float32)
    c3d = rng.uniform(0.3, 1.0, kp.shape[:2]).astype(np.float32)
    c3d[0, 5] = 0.0
    return cams, gt, conf, gt3d, c3d


def _flags(mode):
    return _lib.F_USE_3D if mode == 'l2_3d' else cb.mode_flags(mode)


def _engine(mode, V, serial, round_mode=0):
    """an engine of the hooks build on B problems of V views; serial: created with the switch on"""
    if serial:
        os.environ[SWITCH] = '1'
    try:
        eng = MvFit(cb.model(), vposer=syn.make_vposer_decoder() if mode == 'vposer' else None,
                    gmm=syn.gmm_constants(syn.make_gmm()) if mode == 'gmm' else None, library=_hooks())
    finally:
        os.environ.pop(SWITCH, None)
    if round_mode:
        eng.set_options(round_mode=round_mode)
    cams, gt, conf, gt3d, c3d = _problem(V)
    eng.set_problems(cams, gt, conf)
    if mode == 'l2_3d':
        eng.set_joints3d(gt3d, c3d)
    return eng


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _closures(eng, x, mode):
    """loss[4, B], grad[4, B, 118]"""
    stages = stage_weights(cb.IMAGE_HEIGHT, flags=_flags(mode))
    loss, grad = [], []
    for k in range(x.shape[0]):
        c = eng.closure(x[k], stages[cb.POINT_STAGE[k]])
        loss.append(c['loss'].cpu().numpy())
        grad.append(c['grad'].cpu().numpy())
    return np.stack(loss), np.stack(grad)


@pytest.mark.parametrize('V', VIEWS)
@pytest.mark.parametrize('mode', MODES)
def test_closure_words_do_not_depend_on_the_form_of_the_view_sums(points, mode, V):
    out = []
    for serial in (True, False):
        eng = _engine(mode, V, serial)
        try:
            out.append(_closures(eng, points, mode))
        finally:
            eng.close()
    (ls, gs), (lb, gb) = out
    assert gs.shape == (4, B, 118) and ls.shape == (4, B)
    assert np.isfinite(ls).all() and np.isfinite(gs).all()
    # (the sums carry the whole data term's gradient: translation = g_tau, pose through g_kp; problem 1 has every view)
    assert gs[:, 1, 82:85].any(axis=1).all()
    assert (gs[:, 1, 86:118] if mode == 'vposer' else gs[:, 1, 13:82]).any(axis=1).all()
    differing = [int((_words(a) != _words(b)).sum()) for a, b in ((ls, lb), (gs, gb))]
    print('%s %d views: words differing of loss / gradient: %s of %s' % (mode, V, differing, [ls.size, gs.size]))
    assert differing == [0, 0]


def _fit(eng, x0, history):
    tr = eng.fit_trace(TRACE_CAP)
    xf, st = eng.fit(x0, cb.mode_stages('l2'), history=history)
    out = dict(x=xf.cpu().numpy(), final=st['final_loss'].cpu().numpy(), ncl=st['n_closure'].cpu().numpy(),
               nit=st['n_iter'].cpu().numpy(), trace=tr.cpu().numpy())
    eng.fit_trace(0)
    return out


@pytest.mark.parametrize('round_mode', [0, 1])
@pytest.mark.parametrize('V', [8, 16])
def test_l2_fit_does_not_depend_on_the_form_of_the_view_sums(points, V, round_mode):
    runs = []
    for serial in (True, False):
        eng = _engine('l2', V, serial, round_mode)
        try:
            runs.append(_fit(eng, points[0], 100))
        finally:
            eng.close()
    s, b = runs
    print('%d views round_mode %d: closures %s, iterations %s, final losses %s' % (V, round_mode, b['ncl'], b['nit'], b['final']))
    assert np.isfinite(b['final']).all() and (b['ncl'] > 20).all() and b['ncl'].max() <= TRACE_CAP
    assert np.array_equal(s['ncl'], b['ncl']) and np.array_equal(s['nit'], b['nit'])
    for key in ('x', 'final', 'trace'):                                   # (the trace is NaN where nothing was written: words, not values)
        differing = int((_words(s[key]) != _words(b[key])).sum())
        assert differing == 0, (V, round_mode, key, differing)
