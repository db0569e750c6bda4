"""GPU: the adjoint's transposed basis stream gives the same words whether waves 6-7 load their items in E6 or in E7.

E7 (csrc/closure_device.h: closure_backward) streams pd_subT on waves 1-7, one item (a k-slice of one float4 row group) per
thread.  Waves 6 and 7 have no work in E6, the phase in front of it, and issue their item's loads there, one barrier ahead of
the FMAs; no item changes its owner, its addresses, its FMAs or their order, so no word may change.  The hooks build
(-DMVFIT_DEBUG_HOOKS) reads MVFIT_BWD_STREAM_LATE when a ctx is created: 1 sets ModelLds::stream_late in the uploaded image and
every wave of that ctx's kernels loads inside E7, the form without early loads.  Here: two engines per model, one created
with the switch on, compared word for word - loss and the 118 gradient words of mvfit_closure at the four points of
tests/closure_bits_cases.py in the L2, GMM and VPoser modes, and one whole L2 fit at history 100 and 5 (parameters, final
losses, closure and iteration counts, every trace row), once on the default fit path (the single-launch kernel) and once with
round_mode = 1 (the chained step kernel).

Shapes: 2 problems x 2 views.  Models: the LSP regressor (ns = 69: 28 columns per slice, the SMPL instantiation), top4
(ns = 88: 36 columns per slice, the general instantiation, whose last eight loads are conditional), the skeleton model with
top-4 weights (ns = 5: 4 columns per slice, every other column of the 28 loaded is clamped to the last one) and the body with
dense skinning weights (E6 on the dense rows of wT beside the early loads)."""
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
SWITCH = 'MVFIT_BWD_STREAM_LATE'
TRACE_CAP = 2000
B = 2
MODELS = {'lsp': 69, 'top4': 88, 'smpl4': 5, 'dense': 88}                 # name: selected vertices


def _hooks():
    if not os.path.isfile(HOOKS):
        pytest.skip('libmvfit_hooks.so not built (make -C mvsmplfitting_amd/csrc hooks)')
    return HOOKS


@functools.lru_cache(maxsize=None)
def _model(name):
    model = cells._model(name)
    assert len(cells.selected(model)) == MODELS[name]
    return model


@pytest.fixture(scope='module')
def inputs():
    return dict(np.load(cb.GOLDEN))


def _engine(name, mode, late, inp, round_mode=0):
    """an engine of the hooks build on the first B problems of the recorded inputs; late: created with the switch on"""
    if late:
        os.environ[SWITCH] = '1'
    try:
        eng = MvFit(_model(name), vposer=syn.make_vposer_decoder() if mode == 'vposer' else None,
                    gmm=syn.gmm_constants(syn.make_gmm()) if mode == 'gmm' else None, library=_hooks())
    finally:
        os.environ.pop(SWITCH, None)
    if round_mode:
        eng.set_options(round_mode=round_mode)
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
@pytest.mark.parametrize('name', list(MODELS))
def test_closure_words_do_not_depend_on_where_the_stream_loads(inputs, name, mode):
    out = []
    for late in (True, False):
        eng = _engine(name, mode, late, inputs)
        try:
            out.append(_closures(eng, inputs, mode))
        finally:
            eng.close()
    (ll, gl), (le, ge) = out
    assert gl.shape == (4, B, 118) and np.isfinite(ll).all() and np.isfinite(gl).all()
    # (the stream's g_coef goes into the body pose's gradient - with VPoser through the decoder into the embedding's)
    assert (gl[:, :, 86:118] if mode == 'vposer' else gl[:, :, 13:82]).any(axis=2).all()
    dl, dg = int((_words(ll) != _words(le)).sum()), int((_words(gl) != _words(ge)).sum())
    print('%s %s: loss words differing %d of %d, gradient words differing %d of %d' % (name, mode, dl, ll.size, dg, gl.size))
    assert dl == 0 and dg == 0


def _fit(eng, x0, history):
    tr = eng.fit_trace(TRACE_CAP)
    xf, st = eng.fit(x0, cb.mode_stages('l2'), history=history)
    out = dict(x=xf.cpu().numpy(), final=st['final_loss'].cpu().numpy(), ncl=st['n_closure'].cpu().numpy(),
               nit=st['n_iter'].cpu().numpy(), trace=tr.cpu().numpy())
    eng.fit_trace(0)
    return out


@pytest.mark.parametrize('round_mode', [0, 1])
@pytest.mark.parametrize('name', list(MODELS))
def test_l2_fit_does_not_depend_on_where_the_stream_loads(inputs, name, round_mode):
    runs = []
    for late in (True, False):
        eng = _engine(name, 'l2', late, inputs, round_mode)
        try:
            runs.append([_fit(eng, inputs['x'][0, :B], history) for history in (100, 5)])
        finally:
            eng.close()
    for history, l, e in zip((100, 5), *runs):
        print('%s round_mode %d history %d: closures %s, iterations %s, final losses %s'
              % (name, round_mode, history, e['ncl'], e['nit'], e['final']))
        assert np.isfinite(e['final']).all() and (e['ncl'] > 20).all() and e['ncl'].max() <= TRACE_CAP
        assert np.array_equal(l['ncl'], e['ncl']) and np.array_equal(l['nit'], e['nit'])
        for key in ('x', 'final', 'trace'):                               # (the trace is NaN where nothing was written: words, not values)
            differing = int((_words(l[key]) != _words(e[key])).sum())
            assert differing == 0, (name, round_mode, history, key, differing)
