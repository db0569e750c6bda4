"""GPU: fit_folder(landmarks=dict(table=..., weight=...)) on a serial the test writes: three frames, a ring of four cameras, one
synthetic body per frame whose ankles are rotated.  The keypoint files carry 26 rows per person - the 17 keypoints with 2 px of
noise, three empty rows, and in rows 20-25 the projections of the six vertices the ankles move most (the table of the test; the
synthetic model's feet are not SMPL's, so the golden table's vertex numbers would name arbitrary vertices here).  No threshold on
how far the foot error falls: it is printed, and only the direction is asserted.  Files with 17 rows: the results of the run
without the option, bit for bit."""
import json
import os
import pickle

import numpy as np
import pytest

from mvsmplfitting_amd import batch
from mvsmplfitting_amd import io_formats as iof
from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import MvFit, pack_params
from tests.helpers import body_model

pytestmark = pytest.mark.gpu
F, V = 3, 4
WEIGHT = 0.5


def _write(root, kp17, feet):
    """<root>/0000/Camera0v/0000f_keypoints.json; feet None: 17-row files"""
    for v in range(V):
        d = os.path.join(root, '0000', 'Camera%02d' % v)
        os.makedirs(d)
        for f in range(F):
            rows = [kp17[f, v]]
            if feet is not None:
                rows += [np.zeros((3, 3), np.float32), feet[f, v]]
            kp = np.concatenate(rows).astype(np.float64)
            with open(os.path.join(d, '%05d_keypoints.json' % (f + 1)), 'w') as fh:
                json.dump(dict(version=1.0, people=[dict(pose_keypoints_2d=[float(a) for a in kp.reshape(-1)])]), fh)


@pytest.fixture(scope='module')
def world(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('landmark_folder')
    model = body_model()
    cams = syn.make_camera_ring(V)
    ex = np.tile(np.eye(4), (V, 1, 1))
    ex[:, :3, :3], ex[:, :3, 3] = cams[0], cams[1]
    K = np.tile(np.eye(3), (V, 1, 1))
    K[:, 0, 0] = K[:, 1, 1] = cams[2]
    K[:, :2, 2] = cams[3]
    cam_file = str(tmp / 'cams.txt')
    iof.save_camera_para(cam_file, ex, K)
    lbs = np.asarray(model['lbs_weights'])
    ids = np.concatenate([np.argsort(-lbs[:, j])[:3] for j in (7, 8)])
    table = dict(names=['foot_%d' % i for i in range(6)], keypoint_index=list(range(20, 26)), vertex_ids=[[int(i)] for i in ids],
                 weights=[[1.0]] * 6)
    x_true = pack_params(B=F, **syn.make_frames(F, seed0=900))
    x_true[:, 13 + 18:13 + 24] = np.random.default_rng(5).normal(0.0, 0.5, (F, 6)).astype(np.float32)
    eng = MvFit(model)
    eng.set_problems(cams, np.zeros((F, V, 17, 2), np.float32), np.zeros((F, V, 17), np.float32))
    verts, joints = eng.vertices(x_true)
    gt, conf = syn.make_observations(joints.cpu().numpy(), cams, seed=9)
    kp17 = np.concatenate([gt, conf[..., None]], axis=-1)
    feet_xy = syn.project_points(verts.cpu().numpy()[:, ids], *cams).astype(np.float32)
    feet = np.concatenate([feet_xy, np.full(feet_xy.shape[:-1] + (1,), 0.9, np.float32)], axis=-1)
    _write(str(tmp / 'kp26'), kp17, feet)
    _write(str(tmp / 'kp17'), kp17, None)

    def foot_error(params):
        eng.set_problems(cams, gt, conf)
        p = eng.vertices(params)[0].cpu().numpy()[:, ids]
        return np.linalg.norm(syn.project_points(p, *cams) - feet_xy, axis=-1).mean(axis=(1, 2))
    yield dict(tmp=tmp, model=model, eng=eng, cam_file=cam_file, table=table, foot_error=foot_error)
    eng.close()


def _run(world, keyp, out, **kw):
    return batch.fit_folder(world['model'], str(world['tmp'] / keyp), world['cam_file'], str(world['tmp'] / out), engine=world['eng'],
                            **kw)['0000']


def test_a_serial_is_refined_against_its_foot_points(world):
    base = _run(world, 'kp26', 'plain')
    timing = {}
    r = _run(world, 'kp26', 'feet', landmarks=dict(table=world['table'], weight=WEIGHT), timing=timing)
    rep = r['landmark_report']
    e0, e1 = world['foot_error'](base['params']), world['foot_error'](r['params'])
    print('foot reprojection error, px: without the option %s, with it %s | objective before %s after %s | accepted %s | %.3f s'
          % (e0.tolist(), e1.tolist(), rep['before'].tolist(), rep['after'].tolist(), rep['accepted'].tolist(), timing['landmark']))
    assert rep['targets'].tolist() == [V * 6] * F and timing['landmark'] > 0
    assert r['params'].shape == (F, 118) and np.array_equal(r['final_loss'], np.asarray(rep['loss'], np.float32))
    for t in range(F):
        path = world['tmp'] / 'feet' / '0000' / ('%05d' % (t + 1)) / '000.pkl'
        assert str(path) == r['files'][t] and path.exists()
        with open(path, 'rb') as f:
            res = pickle.load(f)
        assert np.array_equal(res['betas'][0], r['params'][t, :10]) and float(res['loss']) == float(r['final_loss'][t])
    acc = rep['accepted']
    assert acc.any() and (rep['after'][acc] < rep['before'][acc]).all() and np.array_equal(rep['after'][~acc], rep['before'][~acc])
    assert np.array_equal(r['params'][~acc], base['params'][~acc])                   # a rejected row: the keypoint fit's bits
    assert e1.mean() < e0.mean() and (e1[acc] < e0[acc]).all()
    eng = world['eng']                                                               # handed back without table, targets and term
    assert eng._lm_L == 0 and not eng._lm_term
    with pytest.raises(Exception, match='error -3'):
        eng.landmark_loss(eng.vertices(r['params'])[0])


def test_files_with_17_rows_give_the_unchanged_result(world):
    base = _run(world, 'kp17', 'plain17')
    r = _run(world, 'kp17', 'feet17', landmarks=dict(table=world['table'], weight=WEIGHT))
    assert np.array_equal(r['params'].view(np.uint32), base['params'].view(np.uint32))
    assert np.array_equal(r['final_loss'].view(np.uint32), base['final_loss'].view(np.uint32))
    assert np.array_equal(r['n_closure'], base['n_closure'])
    rep = r['landmark_report']
    assert rep['loss'] is None and not rep['accepted'].any() and not rep['targets'].any()
    for t in range(F):
        with open(r['files'][t], 'rb') as f, open(base['files'][t], 'rb') as g:
            a, b = pickle.load(f), pickle.load(g)
        assert sorted(a) == sorted(b) and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a)
