"""GPU: scan.refine_fit - one fit with the scan term inside the engine's rounds, per-body acceptance on the closure's objective
(the contract of silhouette.refine_fit).

Three bodies (syn.make_frames), 4 views, keypoints observed at the truth; scans of 257 points on the true surface, body 1 with
count 0.  The start is the truth with pose and translation perturbed as tests/test_gpu_vertex_target.py's _perturbed does,
shape and scale moved too, plus 3 cm in the translation; w is chosen so that w^2 L is ten times the data term of body 0 at the
start.  The scan pulls the body back towards the truth's surface, where the keypoint term agrees: for the bodies with points
the objective and the scan loss itself must both fall.  Zero iterations: the engine takes no max_iter = 0, a tolerance_grad
above every gradient makes L-BFGS return from its first closure - nothing moved, nothing is accepted, the rows come back
exactly."""
import numpy as np
import pytest
import torch

from mvsmplfitting_amd import scan
from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import MvFitError, pack_params
from tests.gpu_helpers import make_engine
from tests.helpers import body_model
from tests.test_gpu_scan_loss import surface_samples
from tests.test_gpu_vertex_target import _perturbed, _stage

pytestmark = pytest.mark.gpu

V, B, PMAX = 4, 3, 257
EMPTY = 1


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope='module')
def world():
    model = body_model()
    faces = np.asarray(model['faces'], np.int64)
    eng = make_engine(model)
    cams = syn.make_camera_ring(V)
    x_true = pack_params(B=B, **syn.make_frames(B, seed0=6400))
    eng.set_problems(cams, np.zeros((B, V, 17, 2), np.float32), np.zeros((B, V, 17), np.float32))
    verts, joints = eng.vertices(x_true)
    gt, conf = syn.make_observations(_np(joints), cams, seed=3, noise_px=0.0)
    eng.set_problems(cams, gt, conf)
    rng = np.random.default_rng(11)
    v = _np(verts).astype(np.float64)
    points = np.stack([surface_samples(v[n], faces, PMAX, 0.0, rng) for n in range(B)]).astype(np.float32)
    count = np.full(B, PMAX, np.int32)
    count[EMPTY] = 0
    eng.set_scans(points, count=count)
    x0 = _perturbed(x_true, 1)
    x0[:, 0:10] += rng.normal(0, 0.3, (B, 10)).astype(np.float32)
    x0[:, 85] *= np.float32(1.03)
    x0[:, 82:85] += np.array([0.03, 0.0, 0.0], np.float32)
    data = float(eng.closure(x0, _stage(0.0), want_grad=False)['loss'][0])
    L = float(eng.scan_loss(eng.vertices(x0)[0], need_grad=False)[0][0])
    assert data > 0 and L > 0
    w = float(np.sqrt(10.0 * data / L))
    print('w %.6g (body 0 at the start: data term %.6g, scan loss %.6g)' % (w, data, L))
    yield dict(eng=eng, x0=x0, w=w, points=points, count=count)
    eng.close()


def _term_is_off_and_the_set_is_there(eng, x0):
    with pytest.raises(MvFitError, match='error -3'):        # no term: a weight > 0 is refused
        eng.closure(x0, _stage(1.0))
    assert eng.scan_loss(eng.vertices(x0)[0], need_grad=False)[0].shape == (B,)


def test_refine_fit_lowers_the_objective_and_the_scan_loss(world):
    eng, x0, w = world['eng'], world['x0'], world['w']
    x1, rep = scan.refine_fit(eng, x0, _stage(w))
    for k in ('before', 'after', 'accepted', 'scan_before', 'scan_after', 'n_closure', 'loss'):
        assert len(rep[k]) == B, k
    print('before %s\nafter %s\naccepted %s\nscan before %s\nscan after %s\nclosures %s'
          % (rep['before'], rep['after'], rep['accepted'], rep['scan_before'], rep['scan_after'], rep['n_closure']))
    for j in range(B):
        if j == EMPTY:
            continue
        assert rep['accepted'][j], j
        assert rep['after'][j] < rep['before'][j], j
        assert rep['scan_after'][j] < rep['scan_before'][j], j
    assert rep['scan_before'][EMPTY] == 0.0 and rep['scan_after'][EMPTY] == 0.0
    assert np.array_equal(rep['loss'], rep['after'])
    x1 = _np(x1)
    for j in range(B):
        if rep['accepted'][j]:
            assert rep['after'][j] < rep['before'][j] and not np.array_equal(x1[j], x0[j])
        else:
            assert np.array_equal(x1[j], x0[j]) and rep['after'][j] == rep['before'][j]
    # the returned rows have the reported objective and scan loss
    eng.set_scan_term()
    try:
        J = _np(eng.closure(x1, _stage(w), want_grad=False)['loss']).astype(np.float64)
        S = _np(eng.sdf_term_read()[1]).astype(np.float64)
    finally:
        eng.clear_scan_term()
    assert np.array_equal(J, rep['after']) and np.array_equal(S, rep['scan_after'])
    _term_is_off_and_the_set_is_there(eng, x0)


def test_rows_that_are_not_accepted_come_back_exactly(world):
    eng, x0, w = world['eng'], world['x0'], world['w']
    x1, rep = scan.refine_fit(eng, x0, _stage(w), tolerance_grad=1e30)       # L-BFGS returns from its first closure
    assert not np.asarray(rep['accepted']).any()
    assert np.array_equal(_np(x1), x0)
    assert np.array_equal(rep['after'], rep['before']) and np.array_equal(rep['scan_after'], rep['scan_before'])
    assert (np.asarray(rep['n_closure']) <= 2).all()
    _term_is_off_and_the_set_is_there(eng, x0)


def test_the_term_is_cleared_when_something_raises(world):
    eng, x0 = world['eng'], world['x0']
    with pytest.raises(ValueError):
        scan.refine_fit(eng, x0, _stage(0.0))
    with pytest.raises(MvFitError):
        scan.refine_fit(eng, x0, _stage(1.0), max_iter=0)
    _term_is_off_and_the_set_is_there(eng, x0)
