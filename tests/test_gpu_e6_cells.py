"""GPU: E6 of the closure's adjoint writes the same words from its lane cells as from the dense rows of wT.

E6 (csrc/closure_device.h: closure_backward) sums g_A_j = sum_s W[s][j] [g_x v_posed^T | g_x] on sixteen lanes per joint.  With
ModelLds::e6_cells set a lane adds only the vertices of its cell - the non-zero weights, in the dense loop's order - and the
products it leaves out are fma(+-0, v, acc): no word may change.  The hooks build (-DMVFIT_DEBUG_HOOKS) reads MVFIT_E6_DENSE when a
ctx is created: 1 clears the flag in the uploaded image, every kernel of that ctx takes the dense loop.  Here: two engines per
model, one created with the switch on, compared word for word - loss and the 118 gradient words of mvfit_closure at the four
points of tests/closure_bits_cases.py (the start, a small step, both priors dropped, joints at exactly zero) in the L2, GMM and
VPoser modes, and one whole L2 fit at history 100 and 5 (parameters, final losses, closure and iteration counts, every
closure's trial point and loss).

Shapes: 2 problems x 2 views.  Models: top4 (ns = 88: eight lanes have a sixth dense trip), the LSP regressor (ns = 69), the
skeleton model with top-4 weights (ns = 5, the n_skel path of E6's tail), one cell of exactly E6_NZ entries, and one cell of
E6_NZ + 1 entries - the builder clears the flag there and both engines take the dense loop."""
import functools
import os

import numpy as np
import pytest

from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import MvFit
from tests import closure_bits_cases as cb
from tests import test_e6_cells_cpu as cells

pytestmark = pytest.mark.gpu

HOOKS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'mvsmplfitting_amd', 'libmvfit_hooks.so')
SWITCH = 'MVFIT_E6_DENSE'
E6_NZ = 4
TRACE_CAP = 2000
B = 2
MODELS = ('top4', 'lsp', 'smpl4', 'full', 'overlong')


def _hooks():
    if not os.path.isfile(HOOKS):
        pytest.skip('libmvfit_hooks.so not built (make -C mvsmplfitting_amd/csrc hooks)')
    return HOOKS


@functools.lru_cache(maxsize=None)
def _model(name):
    if name in ('full', 'overlong'):
        return cells.cell_model(E6_NZ + (name == 'overlong'))
    return cells._model(name)


@pytest.fixture(scope='module')
def inputs():
    return dict(np.load(cb.GOLDEN))


def _engine(name, mode, dense, inp):
    """an engine of the hooks build on the first B problems of the recorded inputs; dense: created with the switch on"""
    if dense:
        os.environ[SWITCH] = '1'
    try:
        eng = MvFit(_model(name), vposer=syn.make_vposer_decoder() if mode == 'vposer' else None,
                    gmm=syn.gmm_constants(syn.make_gmm()) if mode == 'gmm' else None, library=_hooks())
    finally:
        os.environ.pop(SWITCH, None)
    eng.set_problems(tuple(inp[k] for k in ('cam_R', 'cam_t', 'cam_f', 'cam_c')), inp['gt'][:B], inp['conf'][:B])
    return eng


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _closures(eng, inp, mode):
    stages = cb.mode_stages(mode)
    loss, grad = [], []
    for k in range(inp['x'].shape[0]):
        c = eng.closure(inp['x'][k, :B], stages[cb.POINT_STAGE[k]])
        loss.append(c['loss'].cpu().numpy())
        grad.append(c['grad'].cpu().numpy())
    return np.stack(loss), np.stack(grad)


@pytest.mark.parametrize('mode', cb.MODES)
@pytest.mark.parametrize('name', MODELS)
def test_closure_words_do_not_depend_on_the_form_of_e6(inputs, name, mode):
    out = []
    for dense in (True, False):
        eng = _engine(name, mode, dense, inputs)
        try:
            out.append(_closures(eng, inputs, mode))
        finally:
            eng.close()
    (ld, gd), (lc, gc) = out
    assert gd.shape == (4, B, 118) and np.isfinite(ld).all() and np.isfinite(gd).all()
    assert (gd[:, :, 10:82] != 0).any(axis=2).all()                       # (the pose gradient runs through E6)
    dl, dg = int((_words(ld) != _words(lc)).sum()), int((_words(gd) != _words(gc)).sum())
    print('%s %s: loss words differing %d of %d, gradient words differing %d of %d' % (name, mode, dl, ld.size, dg, gd.size))
    assert dl == 0 and dg == 0


def _fit(eng, x0, history):
    tr = eng.fit_trace(TRACE_CAP)
    xf, st = eng.fit(x0, cb.mode_stages('l2'), history=history)
    out = dict(x=xf.cpu().numpy(), final=st['final_loss'].cpu().numpy(), ncl=st['n_closure'].cpu().numpy(),
               nit=st['n_iter'].cpu().numpy(), trace=tr.cpu().numpy())
    eng.fit_trace(0)
    return out


@pytest.mark.parametrize('name', MODELS)
def test_l2_fit_does_not_depend_on_the_form_of_e6(inputs, name):
    runs = []
    for dense in (True, False):
        eng = _engine(name, 'l2', dense, inputs)
        try:
            runs.append([_fit(eng, inputs['x'][0, :B], history) for history in (100, 5)])
        finally:
            eng.close()
    for history, d, c in zip((100, 5), *runs):
        print('%s history %d: closures %s, iterations %s, final losses %s' % (name, history, c['ncl'], c['nit'], c['final']))
        assert np.isfinite(c['final']).all() and (c['ncl'] > 20).all() and c['ncl'].max() <= TRACE_CAP
        assert np.array_equal(d['ncl'], c['ncl']) and np.array_equal(d['nit'], c['nit'])
        for key in ('x', 'final', 'trace'):                               # (the trace is NaN where nothing was written: words, not values)
            differing = int((_words(d[key]) != _words(c[key])).sum())
            assert differing == 0, (name, history, key, differing)
