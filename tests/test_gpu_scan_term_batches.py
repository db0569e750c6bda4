"""GPU: the scan term (round_term.h: TERM_SCAN) outside the batch shapes of tests/test_gpu_scan_term.py (closures at B = 34, fits
at B = 3), in the shape of tests/test_gpu_round_term_batches.py, whose helpers and docstring this file borrows.

B = 131 = 128 + 3 problems on the model with sparse skinning (body_model(0, 4)): five 32-problem chunks of the gated pull-back,
the last one with three live problems; the lead phase of the fit [stage(0), stage(w)] is a single launch, the second phase the
captured round graph over all 131 bodies of the scan set.  Chunk 1 (rows 32..63) is built dead as that file's docstring
describes - zero shape, the priors' rest pose as truth, the start at the truth, observations at confidence 0 - and has scan
count 0; rows 1, 65, 97 and 129 have count 0 too.  Every other row has Pmax = 257 rows of points on the surface of a perturbed
copy of its start, between 1 and 257 of them counted.  _assert_dead_chunk holds: scan_round's gated kernels skipped a dead
chunk beside live ones, whose partials, accumulators and gradient rows a later round finds stale.

References, none of them new: the same 37 problems (SUB there) fitted in a batch of 37 with re-indexed scans, bit for bit in
parameters, closure counts and final losses; the second fit on the engine replays the captured graph behind a lead phase (the
memset-node case of DESIGN §4a) and returns the same bits; the closure against the stand-alone op and MvFit.vertices_backward
within LOSS_RTOL / GRAD_TOL (tests/scene_sdf_cases.py)."""
import numpy as np
import pytest
import torch

from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import pack_params
from tests.gpu_helpers import make_engine
from tests.helpers import body_model
from tests.scene_sdf_cases import GRAD_TOL, LOSS_RTOL
from tests.test_gpu_round_term_batches import B, CONF_DEAD, DEAD, SUB, W_ROW, _assert_dead_chunk, _rest_pose, _take
from tests.test_gpu_scan_loss import surface_samples
from tests.test_gpu_sdf_batches import NSMALL, _checked_fit, _same
from tests.test_gpu_silhouette_term import BETAS, SCALE, _cams, _observe
from tests.test_gpu_vertex_target import FIT_KW, _perturbed, _stage

pytestmark = pytest.mark.gpu

PMAX = 257
NO_POINTS = (1, 65, 97, 129)                               # (and all of chunk 1)
SCALARS = (1.0, 0.5, 0.05)
ROW = W_ROW[B]                                             # 128: the row whose data term and penalty set the weight


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope='module')
def world():
    model = body_model(0, 4)
    faces = np.asarray(model['faces'], np.int64)
    eng = make_engine(model)
    cams, _, _ = _cams(1)
    fr = syn.make_frames(B, seed0=7300, betas=BETAS)
    fr['scale'][:] = SCALE
    fr['betas'][DEAD] = 0.0
    fr['body_pose'][DEAD] = _rest_pose()
    x_true = pack_params(B=B, **fr)
    gt, conf = _observe(eng, cams, x_true)
    clean, _ = syn.make_observations(_np(eng.vertices(x_true)[1]), cams, seed=3, noise_px=0.0)
    gt[DEAD] = clean[DEAD]
    conf[DEAD] = CONF_DEAD
    eng.set_problems(cams, gt, conf)
    x0 = _perturbed(x_true, 1)
    x0[DEAD] = x_true[DEAD]
    v = _np(eng.vertices(_perturbed(x0, 10))[0]).astype(np.float64)
    rng = np.random.default_rng(10)
    points = np.stack([surface_samples(v[n], faces, PMAX, 0.005, rng) for n in range(B)]).astype(np.float32)
    count = np.random.default_rng(8).integers(1, PMAX + 1, B).astype(np.int32)
    count[[0, 31, 64, 127, ROW, 130]] = [PMAX, 64, 1, 256, PMAX, PMAX]
    count[list(NO_POINTS)] = 0
    count[DEAD] = 0
    weights = np.random.default_rng(9).uniform(0.5, 2.0, (B, PMAX)).astype(np.float32)
    weights[:, 5::41] = 0.0
    # the weight: w^2 = data term / L of one row at the start (the term files' rule)
    eng.set_scans(points, count=count, weights=weights)
    data = float(eng.closure(x0, _stage(0.0), want_grad=False)['loss'][ROW])
    L = float(eng.scan_loss(eng.vertices(x0)[0], *SCALARS, need_grad=False)[0][ROW])
    eng.close()
    assert data > 0 and L > 0
    w = float(np.sqrt(data / L))
    print('weight %.6g (row %d: data term %.6g, L %.6g)' % (w, ROW, data, L))
    return dict(model=model, cams=cams, gt=gt, conf=conf, x0=x0, points=points, count=count, weights=weights, w=w)


def _engine(world, rows=None, **options):
    """the problems ``rows`` (None: all), their scans re-indexed, the term on"""
    rows = np.arange(B) if rows is None else np.asarray(rows)
    eng = make_engine(world['model'], **options)
    eng.set_problems(world['cams'], world['gt'][rows], world['conf'][rows])
    eng.set_scans(world['points'][rows], count=world['count'][rows], weights=world['weights'][rows])
    eng.set_scan_term(*SCALARS)
    return eng, world['x0'][rows].copy()


def test_the_world_reaches_the_shapes_it_is_built_for(world):
    c = world['count']
    assert len(SUB) == NSMALL and {0, 31, 32, 127, 128, 130} <= set(SUB) and {r // 32 for r in SUB} == {0, 1, 2, 3, 4}
    assert not c[DEAD].any() and not c[list(NO_POINTS)].any() and {0, 1, 64, 256, 257} <= set(c.tolist())
    assert {r // 32 for r in np.flatnonzero(c)} == {0, 2, 3, 4} and c[ROW] == PMAX
    assert set(NO_POINTS) & set(SUB) and (c[SUB] > 0).sum() >= 20


def test_two_stage_fit_at_131_equals_the_fit_of_37_and_its_own_replay(world):
    stages = [_stage(0.0), _stage(world['w'])]
    eng, x = _engine(world)
    try:
        big = _checked_fit(eng, x, stages, **FIT_KW)
        builds = eng.round_graph_info()['builds']
        again = _checked_fit(eng, x, stages, **FIT_KW)
        assert eng.round_graph_info()['builds'] == builds      # the replay of the graph the first fit captured
    finally:
        eng.close()
    _assert_dead_chunk(big[1], 'scan, two stages')
    _same(again, big, 'scan: second fit on the engine')
    eng, xs = _engine(world, SUB)
    try:
        ref = _checked_fit(eng, xs, stages, **FIT_KW)
    finally:
        eng.close()
    _same(_take(big, SUB), ref, 'scan: 131 against 37, two stages')
    moved = np.flatnonzero(world['count'] > 0)
    assert not np.array_equal(big[0][moved], world['x0'][moved])


def test_closure_at_131(world):
    w = world['w']
    eng, x = _engine(world)
    try:
        o1 = eng.closure(x, _stage(w), want_grad=True, want_verts=True)
        S = _np(eng.sdf_term_read()[1])
        L_at, g_at = eng.scan_loss(o1['verts'], *SCALARS)
        g_ref = _np(eng.vertices_backward(x, grad_verts=g_at)).astype(np.float64)
        eng.clear_scan_term()
        o0 = eng.closure(x, _stage(0.0), want_grad=True)
    finally:
        eng.close()
    loss, grad, loss0, grad0 = _np(o1['loss']), _np(o1['grad']), _np(o0['loss']), _np(o0['grad'])
    assert np.array_equal(S, _np(L_at))                         # L_j is exactly the op at the trial point's vertices
    L_ref = _np(L_at).astype(np.float64)
    paying = np.flatnonzero(world['count'] > 0)
    free = np.flatnonzero(world['count'] == 0)
    assert {int(r) // 32 for r in paying} == {0, 2, 3, 4}
    worst = 0.0
    for j in paying:
        pen, pen_ref = float(loss[j]) - float(loss0[j]), w * w * L_ref[j]
        gp = grad[j].astype(np.float64) - grad0[j].astype(np.float64)
        gp_ref = w * w * g_ref[j]
        e_g = np.abs(gp - gp_ref).max() / np.abs(gp_ref).max()
        worst = max(worst, e_g)
        if j in (0, 31, 64, 127, 128, 130):
            print('problem %d: L %.7g | pen %.7g ref %.7g (loss %.7g) | grad err/max %.2e (max %.4g)'
                  % (j, S[j], pen, pen_ref, loss[j], e_g, np.abs(gp_ref).max()))
        assert L_ref[j] > 0
        assert abs(pen - pen_ref) <= LOSS_RTOL * float(loss[j]), j
        assert e_g <= GRAD_TOL, j
    print('%d paying rows, worst gradient error / max %.2e' % (paying.size, worst))
    # no points: the bits of the closure without the term
    assert not S[free].any()
    assert np.array_equal(loss[free], loss0[free]) and np.array_equal(grad[free], grad0[free])
    assert not np.array_equal(loss[paying], loss0[paying])
