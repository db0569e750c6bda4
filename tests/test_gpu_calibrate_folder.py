"""GPU: fit_folder(refine_cameras=...) on a temporary serial of three frames made from the demo inputs (tests/golden/demo_data),
with a camera file whose view 1 is turned by one degree: the usual files and cameras_refined.txt are written, the file loads
back to the result's cameras, the energy did not rise; the combinations that are not built are refused."""
import json
import os

import numpy as np
import pytest

from mvsmplfitting_amd import batch, io_formats
from mvsmplfitting_amd.engine import MvFit
from tests import camera_refine_oracle as co
from tests.helpers import GOLD, body_model

pytestmark = pytest.mark.gpu
DATA = os.path.join(GOLD, 'demo_data')
FRAMES = 3


def _vposer():
    d = dict(np.load(os.path.join(GOLD, 'vposer_poser_epoch091_decoder.npz')))
    return {k: d[k] for k in ('fc1_w', 'fc1_b', 'fc2_w', 'fc2_b', 'out_w', 'out_b')}


def _make_serial(root):
    rng = np.random.default_rng(5)
    src = os.path.join(DATA, 'keypoints', '0000')
    for cam in sorted(os.listdir(src)):
        os.makedirs(os.path.join(root, '0000', cam))
        with open(os.path.join(src, cam, '00001_keypoints.json')) as f:
            doc = json.load(f)
        kp = np.asarray(doc['people'][0]['pose_keypoints_2d'], np.float64).reshape(-1, 3)
        for t in range(FRAMES):
            moved = kp.copy()
            moved[:, :2] += 4.0 * t + rng.normal(0, 1.5, (kp.shape[0], 2))
            out = dict(doc, people=[dict(doc['people'][0], pose_keypoints_2d=moved.reshape(-1).tolist())])
            with open(os.path.join(root, '0000', cam, '%05d_keypoints.json' % (t + 1)), 'w') as f:
                json.dump(out, f)


def _turned_camera_file(path):
    ex, K = io_formats.load_camera_para(os.path.join(DATA, '3DOH50K_Parameters.txt'))
    cam = co.pack(ex[1, :3, :3], ex[1, :3, 3], 1.0, (0.0, 0.0))
    cam = co.step(cam, np.concatenate([np.deg2rad(1.0) * np.array([0.6, 0.0, 0.8]), np.zeros(6)]))
    ex[1, :3, :3], ex[1, :3, 3] = cam[:9].reshape(3, 3), cam[9:12]
    io_formats.save_camera_para(path, ex, K)
    return ex, K


@pytest.mark.parametrize('persons', [0, 'all'])
def test_a_serial_is_refitted_under_the_refined_rig(tmp_path, persons):
    keyp, cam_file = str(tmp_path / 'keypoints'), str(tmp_path / 'cams.txt')
    _make_serial(keyp)
    ex0, K0 = _turned_camera_file(cam_file)
    eng = MvFit(body_model(), vposer=_vposer())
    try:
        timing = {}
        out = batch.fit_folder(body_model(), keyp, cam_file, str(tmp_path / 'results'), vposer=_vposer(), image_height=1536.0,
                               engine=eng, timing=timing, persons=persons, refine_cameras=dict(sweeps=2, anchor=0))
        r = out['0000']
        rep = r['camera_report']
        E = [rep['E0']] + [s['E'] for s in rep['sweeps']]
        print('persons %r: E %s, accepted %s, statuses %s, %.3f s' % (persons, E, [s['accepted'] for s in rep['sweeps']],
                                                                  rep['sweeps'][0]['report'][:, 4], timing['cameras']))
        assert 1 <= len(rep['sweeps']) <= 2 and E[-1] <= E[0] and timing['cameras'] > 0
        assert np.array_equal(r['params'], rep['sweeps'][-1]['params'])
        assert np.array_equal(r['final_loss'], rep['loss'].astype(np.float32))
        for t in range(FRAMES):
            path = tmp_path / 'results' / '0000' / ('%05d' % (t + 1)) / '000.pkl'
            assert str(path) == r['files'][t] and path.exists()
        refined = tmp_path / 'results' / '0000' / 'cameras_refined.txt'
        assert refined.exists()
        ex, K = io_formats.load_camera_para(str(refined))
        V = ex.shape[0]
        assert np.array_equal(ex.view(np.uint64), r['cameras'][0].view(np.uint64))
        assert np.array_equal(K.view(np.uint64), r['cameras'][1].view(np.uint64))
        # the anchor is the camera file's view 0 as the engine takes it (float32); free='extrinsics' leaves the intrinsics
        assert np.array_equal(ex[0, :3], ex0[0, :3].astype(np.float32).astype(np.float64))
        assert np.array_equal(K[:, 0, 0], K0[:V, 0, 0].astype(np.float32).astype(np.float64)) and np.array_equal(K[:, 2], K0[:V, 2])
        # the camera file itself is untouched: the next serial starts from it
        ex1, K1 = io_formats.load_camera_para(cam_file)
        assert np.array_equal(ex1, ex0) and np.array_equal(K1, K0)
    finally:
        eng.close()


def test_combinations_that_are_not_built_are_refused(tmp_path):
    keyp, cam_file = str(tmp_path / 'keypoints'), str(tmp_path / 'missing.txt')     # refused before any file is read
    args = (body_model(), keyp, cam_file, str(tmp_path / 'results'))
    rc = dict(sweeps=1)
    for kw in (dict(is_seq=True), dict(use_3d=True), dict(persons='all', scene_collision=dict(weight=1.0)),
               dict(silhouettes=dict(mask_root='m', weight=1.0)), dict(temporal=dict(weight=1.0)),
               dict(joint=dict(weight=1.0, silhouettes=dict(share=1.0, mask_root='m'), temporal=dict(share=1.0)))):
        with pytest.raises(ValueError, match='refine_cameras with %s is not built' % [k for k in kw if k != 'persons'][0]):
            batch.fit_folder(*args, refine_cameras=rc, **kw)
    with pytest.raises(ValueError, match='unknown keys'):
        batch.fit_folder(*args, refine_cameras=dict(sweep=1))
    assert not os.path.exists(str(tmp_path / 'results'))
