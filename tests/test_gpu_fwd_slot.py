"""GPU: the closure's forward slot gives the same words whether waves 5-7 load their basis items in E1 or in E2.

E2 (csrc/closure_device.h: sparse_forward) streams pd_sub on waves 1-7, thread 64 + t owning the items t and t + 448 that
exist (csrc/model_layout.h: fwd_item_owner).  E1, the phase in front of it, computes one Rodrigues per element of R on waves
0-4; waves 5-7 have no work there and issue their item's loads, one barrier ahead of the FMAs.  No item changes its owner, its
addresses, its FMAs or their order, so no word may change.  The hooks build (-DMVFIT_DEBUG_HOOKS) reads MVFIT_FWD_STREAM_LATE
when a ctx is created: 1 sets bit 1 of ModelLds::stream_late in the uploaded image and every wave of that ctx's kernels loads
inside E2, the form without early loads.  Here: two engines per model, one created with the switch on, compared word for word
- loss, the 118 gradient words and the joints of mvfit_closure at the four points of tests/closure_bits_cases.py in the L2,
GMM and VPoser modes, the vertices and joints of mvfit_vertices at those points, and one whole L2 fit at history 100 and 5
(parameters, final losses, closure and iteration counts, every trace row), once on the default fit path (the single-launch
kernel) and once with round_mode = 1 (the chained step kernel, which has no forward stream).

Shapes: 2 problems x 2 views.  Models: the LSP regressor (ns = 69, 416 items: 160 early, half of wave 6 without one), top4
(ns = 88, 528 items: 192 early, 80 threads with two in-slot items), the skeleton model with top-4 weights (ns = 5, 32 items:
no early item at all) and the body with dense skinning weights."""
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
SWITCH = 'MVFIT_FWD_STREAM_LATE'
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
    """loss[4, B], grad[4, B, 118], closure joints[4, B, 17, 3], vertices[4, B, nv, 3], joints of the vertices call"""
    stages = cb.mode_stages(mode)
    out = [[] for _ in range(5)]
    for k in range(inp['x'].shape[0]):
        c = eng.closure(inp['x'][k, :B], stages[cb.POINT_STAGE[k]], want_joints=True)
        v, j = eng.vertices(inp['x'][k, :B], flags=cb.mode_flags(mode))
        for o, t in zip(out, (c['loss'], c['grad'], c['joints'], v, j)):
            o.append(t.cpu().numpy())
    return [np.stack(o) for o in out]


@pytest.mark.parametrize('mode', cb.MODES)
@pytest.mark.parametrize('name', list(MODELS))
def test_closure_words_do_not_depend_on_where_the_forward_stream_loads(inputs, name, mode):
    out = []
    for late in (True, False):
        eng = _engine(name, mode, late, inputs)
        try:
            out.append(_closures(eng, inputs, mode))
        finally:
            eng.close()
    late, early = out
    ll, gl = late[0], late[1]
    assert gl.shape == (4, B, 118) and late[2].shape == (4, B, 17, 3) and late[4].shape == (4, B, 17, 3)
    assert all(np.isfinite(a).all() for a in late)
    # (the stream's v_posed reaches every keypoint, and through them the gradient of the pose)
    assert (gl[:, :, 86:118] if mode == 'vposer' else gl[:, :, 13:82]).any(axis=2).all()
    differing = [int((_words(a) != _words(b)).sum()) for a, b in zip(late, early)]
    print('%s %s: words differing of loss / gradient / closure joints / vertices / joints: %s of %s'
          % (name, mode, differing, [a.size for a in late]))
    assert differing == [0, 0, 0, 0, 0]


def _fit(eng, x0, history):
    tr = eng.fit_trace(TRACE_CAP)
    xf, st = eng.fit(x0, cb.mode_stages('l2'), history=history)
    out = dict(x=xf.cpu().numpy(), final=st['final_loss'].cpu().numpy(), ncl=st['n_closure'].cpu().numpy(),
               nit=st['n_iter'].cpu().numpy(), trace=tr.cpu().numpy())
    eng.fit_trace(0)
    return out


@pytest.mark.parametrize('round_mode', [0, 1])
@pytest.mark.parametrize('name', list(MODELS))
def test_l2_fit_does_not_depend_on_where_the_forward_stream_loads(inputs, name, round_mode):
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
