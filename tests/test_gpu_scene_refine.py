"""GPU: the joint refinement of the persons of a scene (scene_fit.refine_scenes, fit_folder(scene_collision=...)) on two
frames of two full bodies, 4 views, keypoints projected exactly from a ground truth in which scene A's bodies stand 0.13 m
apart (they interpenetrate) and scene B's 1 m apart (they do not).  The persons are fitted independently first, then refined.

The weight of the collision term is the smallest power of ten at which scene A's penalty at the independent result is at
least scene A's summed loss without the term; test_the_weight_is_the_smallest_power_of_ten_that_matters prints both numbers
and asserts that WEIGHT is that power.  Measured on an MI355X: sum_j S_j^2 = 466327.6 (S = 481.56, 484.18) and a summed loss
of 814.58 without the term, so the penalty is 46.6 at 0.01 and 4663 at 0.1: WEIGHT = 0.1."""
import os
import json
import pickle

import numpy as np
import pytest

from mvsmplfitting_amd import batch
from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import MvFit, stage_weights
from mvsmplfitting_amd.scene_fit import refine_scenes
from tests.helpers import body_model
from tests.scene_sdf_cases import LOSS_RTOL

pytestmark = pytest.mark.gpu

V, F, P = 4, 2, 2
SIZES = [2, 2]
OFFSET = np.array([[[0.0, 0.0, 0.0], [0.13, 0.02, 0.07]],          # scene A (frame 0): case d's translation apart
                   [[-0.5, 0.0, 0.0], [0.5, 0.0, 0.0]]], np.float32)  # scene B (frame 1): a metre apart
KW = dict(sweeps=3, grid_size=32, scale_factor=0.2, robustifier=0.05)
WEIGHT = 0.1


def _truth():
    x = np.zeros((F, P, 118), np.float32)
    for p in range(P):
        betas = np.random.default_rng(400 + p).normal(0, 0.3, 10).astype(np.float32)
        fr = syn.make_frames(F, seed0=70 + 100 * p, betas=betas)
        for k, (a, b) in dict(betas=(0, 10), global_orient=(10, 13), body_pose=(13, 82), scale=(85, 86)).items():
            x[:, p, a:b] = fr[k]
        x[:, p, 82:85] = OFFSET[:, p]
    return x


def _stage(weight):
    return dict(stage_weights(1536.0)[-1], coll_loss_weight=weight)


@pytest.fixture(scope='module')
def scene(tmp_path_factory):
    root = tmp_path_factory.mktemp('scene_refine')
    model = body_model()
    cams = syn.make_camera_ring(V)
    xgt = _truth()
    eng = MvFit(model)
    eng.set_problems(cams, np.zeros((F * P, V, 17, 2), np.float32), np.zeros((F * P, V, 17), np.float32))
    _, joints = eng.vertices(xgt.reshape(F * P, 118))
    uv = syn.project_points(joints.cpu().numpy(), *cams).reshape(F, P, V, 17, 2)
    cam_R, cam_t, cam_f, cam_c = (np.asarray(a, np.float64) for a in cams)
    with open(root / 'cams.txt', 'w') as fh:
        for v in range(V):
            fh.write('%d\n' % v)
            K = np.array([[cam_f[v], 0, cam_c[v, 0]], [0, cam_f[v], cam_c[v, 1]], [0, 0, 1]])
            for r in K:
                fh.write(' '.join('%.10f' % x for x in r) + '\n')
            fh.write('0 0\n')
            for r in np.hstack([cam_R[v], cam_t[v][:, None]]):
                fh.write(' '.join('%.10f' % x for x in r) + '\n')
    for v in range(V):
        d = root / 'keypoints' / 's0' / ('Camera%02d' % v)
        d.mkdir(parents=True)
        for f in range(F):
            people = [dict(pose_keypoints_2d=[float(x) for x in np.concatenate([uv[f, p, v], np.ones((17, 1))], 1).reshape(-1)])
                      for p in range(P)]
            with open(d / ('%05d_keypoints.json' % f), 'w') as fh:
                json.dump(dict(version=1.0, people=people), fh)
    sc = dict(root=root, keyp=str(root / 'keypoints'), cams=str(root / 'cams.txt'), model=model, rig=cams, eng=eng)
    # the independent fit, then the problems as fit_folder sets them (frame-major, ascending id)
    sc['ind'] = _fit(sc, 'independent', persons='all')
    _set_all(sc)
    sc['refined'] = refine_scenes(eng, sc['ind']['params'], SIZES, _stage(WEIGHT), **KW)
    yield sc
    eng.close()


def _set_all(sc):
    """All four problems, keypoints and cameras read back from the files as fit_folder reads them."""
    frames = next(iter(batch.list_frames(sc['keyp'])))[2]
    _, kpp, _ = batch.load_serial_people(frames, V)
    kp = kpp.reshape(F * P, V, 17, 3)
    sc['gt'], sc['conf'] = kp[..., :2].copy(), kp[..., 2].copy()
    ex, it = batch.iof.load_camera_para(sc['cams'])
    ex, it = np.asarray(ex[:V], np.float64), np.asarray(it[:V], np.float64)
    sc['rig32'] = (ex[:, :3, :3].astype(np.float32), ex[:, :3, 3].astype(np.float32), it[:, 0, 0].astype(np.float32),
                   it[:, :2, 2].astype(np.float32))
    sc['eng'].set_problems(sc['rig32'], sc['gt'], sc['conf'])


def _fit(sc, name, **kw):
    return batch.fit_folder(sc['model'], sc['keyp'], sc['cams'], str(sc['root'] / name), engine=sc['eng'], **kw)['s0']


def _tree(folder):
    return sorted(os.path.relpath(os.path.join(d, f), folder) for d, _, fs in os.walk(folder) for f in fs)


def test_the_weight_is_the_smallest_power_of_ten_that_matters(scene):
    eng, x = scene['eng'], scene['ind']['params']
    _set_all(scene)
    v, _ = eng.vertices(x)
    eng.set_scene_obstacles(v, SIZES, **{k: KW[k] for k in ('grid_size', 'scale_factor', 'robustifier')})
    try:
        eng.closure(x, _stage(1.0), want_grad=False)
        S = eng.sdf_term_read()[1].cpu().numpy().astype(np.float64)
        loss0 = eng.closure(x, _stage(0.0), want_grad=False)['loss'].cpu().numpy().astype(np.float64)
    finally:
        eng.clear_scene_obstacles()
    s2, l0 = float((S[:2] ** 2).sum()), float(loss0[:2].sum())
    print('scene A at the independent result: sum S_j^2 = %.7g (S = %s), summed loss without the term = %.7g; pen at WEIGHT '
          '%g = %.7g, at WEIGHT / 10 = %.7g; scene B: S = %s' % (s2, S[:2], l0, WEIGHT, WEIGHT ** 2 * s2, (WEIGHT / 10) ** 2 * s2, S[2:]))
    assert s2 > 0 and not np.any(S[2:])
    assert WEIGHT ** 2 * s2 >= l0 > (WEIGHT / 10) ** 2 * s2


def test_J_is_monotone_and_rejected_rows_are_kept_exactly(scene):
    x, rep = scene['refined']
    J = np.stack([rep['J0']] + [s['J'] for s in rep['sweeps']])
    prev = rep['params0']
    print('J per sweep:\n%s\ncollision per sweep:\n%s\naccepted: %s' % (
        J, np.stack([rep['collision0']] + [s['collision'] for s in rep['sweeps']]), [s['accepted'].tolist() for s in rep['sweeps']]))
    assert 1 <= len(rep['sweeps']) <= KW['sweeps']
    assert np.all(np.diff(J, axis=0) <= 0)
    for s in rep['sweeps']:
        for k in range(2):
            rows = slice(2 * k, 2 * k + 2)
            assert s['accepted'][k] or np.array_equal(s['params'][rows], prev[rows])
            assert not s['accepted'][k] or not np.array_equal(s['params'][rows], prev[rows])
        prev = s['params']
    assert np.array_equal(x.cpu().numpy(), prev)


def test_the_interpenetrating_scene_gets_strictly_better(scene):
    _, rep = scene['refined']
    last = rep['sweeps'][-1]
    print('scene A: collision %.7g -> %.7g, J %.7g -> %.7g' % (rep['collision0'][0], last['collision'][0], rep['J0'][0], last['J'][0]))
    assert rep['collision0'][0] > 0
    assert last['collision'][0] < rep['collision0'][0]
    assert last['J'][0] < rep['J0'][0]
    assert rep['collision0'][1] == 0.0 and last['collision'][1] == 0.0


def test_a_fit_with_the_term_reports_its_own_closure_and_runs_no_asynchronous_pass(scene):
    eng, x = scene['eng'], scene['ind']['params']
    _set_all(scene)
    v, _ = eng.vertices(x)
    eng.set_scene_obstacles(v, SIZES, **{k: KW[k] for k in ('grid_size', 'scale_factor', 'robustifier')})
    try:
        xf, st = eng.fit(x, [_stage(WEIGHT)])
        loss = eng.closure(xf, _stage(WEIGHT), want_grad=False)['loss'].cpu().numpy().astype(np.float64)
    finally:
        eng.clear_scene_obstacles()
    final = st['final_loss'].cpu().numpy().astype(np.float64)
    print('final_loss %s\nclosure    %s\npasses %s' % (final, loss, st['passes']))
    assert np.all(np.abs(final - loss) <= LOSS_RTOL * np.abs(loss))
    assert st['passes'] == dict(run=0, skipped=0, missed=0, timed_out=0)


def test_a_scene_refined_alone_is_the_scene_refined_in_the_batch(scene):
    eng = scene['eng']
    x, rep = scene['refined']
    try:
        eng.set_problems(scene['rig32'], scene['gt'][:2], scene['conf'][:2])
        xa, ra = refine_scenes(eng, scene['ind']['params'][:2], [2], _stage(WEIGHT), **KW)
    finally:
        _set_all(scene)
    assert np.array_equal(xa.cpu().numpy(), x.cpu().numpy()[:2])
    # (the batch may run a sweep more for scene B's sake: scene A's rows are then kept or moved exactly as alone)
    for sa, sb in zip(ra['sweeps'], rep['sweeps']):
        assert sa['J'][0] == sb['J'][0] and sa['accepted'][0] == sb['accepted'][0] and sa['collision'][0] == sb['collision'][0]


def test_fit_folder_refines_writes_and_reports(scene):
    x, rep = scene['refined']
    timing = {}
    out = _fit(scene, 'refined', persons='all', scene_collision=dict(weight=WEIGHT, **KW), timing=timing)
    assert _tree(scene['root'] / 'refined') == _tree(scene['root'] / 'independent') == sorted(
        os.path.join('s0', '%05d' % f, '%03d.pkl' % p) for f in range(F) for p in range(P))
    assert 'refine' in timing and timing['refine'] > 0
    assert 'scene_report' in out and 'scene_report' not in scene['ind']
    assert np.array_equal(out['scene_report']['sweeps'][-1]['J'], rep['sweeps'][-1]['J'])
    assert np.array_equal(out['params'], x.cpu().numpy())
    assert not np.array_equal(out['params'][:2], scene['ind']['params'][:2])
    for n, path in enumerate(out['files']):
        with open(path, 'rb') as fh:
            saved = pickle.load(fh)
        assert np.array_equal(saved['transl'][0], out['params'][n, 82:85]) and np.array_equal(saved['betas'][0], out['params'][n, 0:10])
        assert saved['loss'] == float(out['final_loss'][n])


def test_without_the_argument_nothing_changes(scene):
    a, b = scene['ind'], _fit(scene, 'none', persons='all', scene_collision=None)
    assert sorted(a) == sorted(b)
    for k in ('params', 'final_loss', 'n_closure', 'init'):
        assert np.array_equal(a[k], b[k]), k
    for p, q in zip(a['files'], b['files']):
        with open(p, 'rb') as fa, open(q, 'rb') as fb:
            assert fa.read() == fb.read()
