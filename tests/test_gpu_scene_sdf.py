"""GPU: the scene collision loss mvfit_scene_sdf_loss (scene_sdf.hip; MvFit.scene_sdf_loss) against the reference's own
SDFLoss, float32 + autograd, recorded in tests/golden/scene_sdf_ref.npz (tools/make_golden_scene_sdf.py).  Bounds: the fields
bit for bit, the loss 1e-5 relative, the gradients 2e-4 of max |g_ref| elementwise with no row left out (the bounds of
tests/test_gpu_sdf_term.py); the reference's own float32-vs-float64 gap on each case, stored with it, must stay below a
quarter of each bound.  Batching: a scene's numbers do not depend on the call it is part of."""
import ctypes as C

import numpy as np
import pytest
import torch

from mvsmplfitting_amd.engine import MvFitError
from tests import scene_sdf_cases as sc
from tests.gpu_helpers import make_engine
from tests.helpers import body_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    e = make_engine(body_model())
    yield e
    e.close()


def _np(t):
    return t.detach().cpu().numpy()


def _run(eng, c, **kw):
    return eng.scene_sdf_loss(c['translated'], c['faces'], grid_size=c['grid_size'], scale_factor=c['scale_factor'],
                              robustifier=c['robustifier'], **kw)


@pytest.mark.parametrize('name', ['a', 'c'])
def test_fields_are_bit_identical_and_loss_and_gradients_match_the_reference(eng, name):
    c = sc.case(name)
    sc.check_gap(c)
    loss, g, phi = _run(eng, c, return_phi=True)
    assert np.array_equal(_np(phi), c['phi']), np.count_nonzero(_np(phi) != c['phi'])
    sc.check(c, float(loss[0]), _np(g))
    assert eng.sdf_info()['op'] == 'walk'                  # 160 faces: the staged walk


@pytest.mark.parametrize('robust', [False, True])
def test_far_body_counts_in_the_divisor_and_gets_exactly_zero_and_the_face_lists_ran(eng, robust):
    c = sc.case('b', robust)
    sc.check_gap(c)
    loss, g, phi = _run(eng, c, return_phi=True)
    assert eng.sdf_info()['op'] == 'face_lists'
    assert np.array_equal(_np(phi), c['phi'])
    sc.check(c, float(loss[0]), _np(g))
    assert not np.any(_np(g)[2]), 'far body'
    pair, _, _ = eng.scene_sdf_loss(c['translated'][:2], c['faces'], grid_size=32, robustifier=c['robustifier'], need_grad=False)
    assert float(pair[0]) * 4.0 == pytest.approx(float(loss[0]) * 9.0, rel=1e-6), 'the divisor is P^2 with the far body counted'


def test_two_full_bodies_on_the_rows_the_golden_holds(eng):
    c = sc.case('d')
    sc.check_gap(c)
    loss, g, phi = _run(eng, c, return_phi=True)
    assert eng.sdf_info()['op'] == 'face_lists'
    assert np.array_equal(_np(phi), c['phi'])
    sc.check(c, float(loss[0]), _np(g))


def _scenes():
    """Scenes of sizes [1, 3, 2, 3] from case a's bodies (the last: reversed and moved)."""
    a = sc.case('a')['translated']
    last = (a[::-1] + np.array([5.0, -1.0, 2.0], np.float32)).astype(np.float32)
    return [a[:1], a, a[:2], last]


@pytest.mark.parametrize('scale_factor,robustifier', [(0.2, None), (0.02, 0.05)])
def test_a_scenes_numbers_do_not_depend_on_the_call(eng, scale_factor, robustifier):
    c = sc.case('a')
    scenes = _scenes()
    kw = dict(grid_size=16, scale_factor=scale_factor, robustifier=robustifier)

    def call(order, **extra):
        v = np.concatenate([scenes[k] for k in order])
        loss, g, _ = eng.scene_sdf_loss(v, c['faces'], scene_sizes=[len(scenes[k]) for k in order], **kw, **extra)
        first = np.concatenate([[0], np.cumsum([len(scenes[k]) for k in order])])
        return {k: (_np(loss)[n], None if g is None else _np(g)[first[n]:first[n + 1]]) for n, k in enumerate(order)}
    whole = call([0, 1, 2, 3])
    assert whole[0][0] == 0.0 and not np.any(whole[0][1]), 'one body: loss 0, gradient 0'
    assert whole[1][0] > 0 and whole[2][0] > 0 and whole[3][0] > 0
    if robustifier is None:
        sc.check(c, whole[1][0], whole[1][1])
    again, perm, nograd = call([0, 1, 2, 3]), call([3, 1, 0, 2]), call([0, 1, 2, 3], need_grad=False)
    for k in range(4):
        alone = call([k])
        for other in (alone, again, perm):
            assert whole[k][0] == other[k][0] and np.array_equal(whole[k][1], other[k][1]), k
        assert whole[k][0] == nograd[k][0] and nograd[k][1] is None


def test_scenes_on_both_sides_of_a_group_boundary_are_bit_identical_to_themselves_alone(eng):
    """G = 128: a field is 8 MB, the cap of 256 MB holds 32 - eleven scenes of three bodies go as groups of ten and one."""
    c = sc.case('a')
    a = c['translated']
    v = np.concatenate([a] * 11)
    loss, g, _ = eng.scene_sdf_loss(v, c['faces'], scene_sizes=[3] * 11, grid_size=128)
    one, g1, _ = eng.scene_sdf_loss(a, c['faces'], grid_size=128)
    loss, g = _np(loss), _np(g)
    assert loss[0] > 0
    for s in (0, 9, 10):
        assert loss[s] == _np(one)[0] and np.array_equal(g[3 * s:3 * s + 3], _np(g1)), s


def test_scenes_on_both_sides_of_a_face_list_run_boundary_are_bit_identical_to_themselves_alone(eng):
    """576 faces: 3.1 MB of face lists per body, a run of the face-list kernels takes at most 2 GB of them = 718 bodies -
    241 scenes of three bodies are voxelised in two runs, the boundary inside scene 239.  G = 16 keeps it cheap."""
    c = sc.case('b')
    a = c['translated']
    v = np.concatenate([a] * 241)
    loss, g, _ = eng.scene_sdf_loss(v, c['faces'], scene_sizes=[3] * 241, grid_size=16)
    assert eng.sdf_info()['op'] == 'face_lists'
    one, g1, _ = eng.scene_sdf_loss(a, c['faces'], grid_size=16)
    loss, g = _np(loss), _np(g)
    assert loss[0] > 0
    for s in (0, 238, 239, 240):
        assert loss[s] == _np(one)[0] and np.array_equal(g[3 * s:3 * s + 3], _np(g1)), s


def test_bad_arguments_are_refused_with_a_message_that_names_the_function(eng):
    c = sc.case('a')
    v, f = c['translated'], c['faces']

    def refused(*a, **kw):
        with pytest.raises(MvFitError, match='error -1: mvfit_scene_sdf_loss') as ei:
            eng.scene_sdf_loss(*a, **kw)
        return str(ei.value)
    assert 'empty' in refused(v, f, scene_sizes=[3, 0])
    assert 'decreases' in refused(np.concatenate([v, v[:1]]), f, scene_sizes=[3, -1, 2])
    assert 'at most 256' in refused(np.zeros((257, 4, 3), np.float32), np.array([[0, 1, 2]]), scene_sizes=[257])
    assert 'grid_size 1 ' in refused(v, f, grid_size=1)
    assert 'grid_size 129 ' in refused(v, f, grid_size=129)
    bad = f.copy()
    bad[7, 1] = v.shape[1]
    assert 'face vertex index 82 outside [0, 82)' in refused(v, bad)
    bad[7, 1] = -1
    assert 'face vertex index -1' in refused(v, bad)
    # the raw C ABI: null pointers, scene_first[0] != 0
    lib, ctx = eng._lib, eng._ctx
    vt = torch.tensor(v, device=eng.device)
    ft = torch.tensor(f, device=eng.device, dtype=torch.int32)
    loss = torch.zeros(1, device=eng.device)
    first = (C.c_int32 * 2)(0, 3)

    def raw(vp, fp, sp, lp):
        rc = lib.mvfit_scene_sdf_loss(ctx, vp, 82, fp, int(ft.shape[0]), sp, 1, 16, 0.2, 0.0, lp, None, None)
        return rc, lib.mvfit_last_error(ctx).decode()
    for args in ((None, ft.data_ptr(), first, loss.data_ptr()), (vt.data_ptr(), None, first, loss.data_ptr()),
                 (vt.data_ptr(), ft.data_ptr(), None, loss.data_ptr()), (vt.data_ptr(), ft.data_ptr(), first, None)):
        rc, msg = raw(*args)
        assert rc == -1 and msg.startswith('mvfit_scene_sdf_loss: null'), (rc, msg)
    rc, msg = raw(vt.data_ptr(), ft.data_ptr(), (C.c_int32 * 2)(1, 3), loss.data_ptr())
    assert rc == -1 and 'scene_first[0] = 1' in msg and msg.startswith('mvfit_scene_sdf_loss')
    rc, msg = raw(vt.data_ptr(), ft.data_ptr(), first, loss.data_ptr())
    assert rc == 0, msg
    assert float(loss[0]) == pytest.approx(c['loss'], rel=1e-5)
