"""GPU: fit_folder(joint=dict(silhouettes=..., temporal=...)) on a temporary serial of four frames made from the demo inputs
(tests/golden/demo_data), as tests/test_gpu_temporal_folder.py builds it.  Masks: the keypoint fit's own bodies with the
parameters averaged over each frame's neighbours (a smoother motion than the keypoints give), rendered into two cameras per
frame at 1536 x 2048, written as PNG and fitted against at downscale=4.  The usual files are written, the result carries
joint_report, and both components end below the keypoint fit's values.  Weights: the silhouette term as
tests/test_gpu_silhouette_folder.py weighs it (1), the temporal term as tests/test_gpu_temporal_folder.py does (20^2 = 400)."""
import json
import os
import pickle
import shutil

import numpy as np
import pytest

from mvsmplfitting_amd import _lib, batch
from mvsmplfitting_amd.engine import MvFit
from tests.helpers import GOLD, body_model

pytestmark = pytest.mark.gpu
DATA = os.path.join(GOLD, 'demo_data')
FRAMES, H, W, K = 4, 1536, 2048, 4
MASK_VIEWS = (0, 2)


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


def test_a_serial_is_refined_jointly_and_written(tmp_path):
    from PIL import Image
    keyp, cam_file = str(tmp_path / 'keypoints'), str(tmp_path / 'cams.txt')
    _make_serial(keyp)
    shutil.copy(os.path.join(DATA, '3DOH50K_Parameters.txt'), cam_file)
    eng = MvFit(body_model(), vposer=_vposer())
    try:
        base = batch.fit_folder(body_model(), keyp, cam_file, str(tmp_path / 'plain'), vposer=_vposer(), image_height=float(H),
                                engine=eng)['0000']
        serial, cams, frames = batch.list_frames(keyp)[0]
        x = base['params']
        smooth = np.stack([x[max(t - 1, 0):t + 2].mean(axis=0) for t in range(FRAMES)]).astype(np.float32)
        v, _ = eng.vertices(smooth, flags=_lib.F_VPOSER)              # (the serial's problems are still set)
        prob = np.repeat(np.arange(FRAMES), len(MASK_VIEWS)).astype(np.int32)
        view = np.tile(np.array(MASK_VIEWS, np.int32), FRAMES)
        _, fid = eng.render_overlay(v, None, np.zeros((len(prob), H, W, 3), np.uint8), prob, view, face_id=True)
        on = (fid >= 0).cpu().numpy()
        assert on.reshape(len(prob), -1).any(axis=1).all()
        root = tmp_path / 'masks'
        for i, (t, c) in enumerate(zip(prob, view)):
            os.makedirs(root / serial / cams[c], exist_ok=True)
            Image.fromarray(on[i].astype(np.uint8) * 255, 'L').save(batch.mask_path(str(root), serial, cams[c], frames[t][0]))
        timing = {}
        out = batch.fit_folder(body_model(), keyp, cam_file, str(tmp_path / 'results'), vposer=_vposer(), image_height=float(H),
                               engine=eng, timing=timing,
                               joint=dict(weight=1.0, sweeps=2, silhouettes=dict(share=1.0, mask_root=str(root), downscale=K),
                                          temporal=dict(share=400.0)))
        r = out['0000']
        rep = r['joint_report']
        last = rep['sweeps'][-1]
        print('E %s -> %s, accepted %s, parts (S_sc^2, L_sil, L_vt) %s -> %s, %.3f s'
              % (rep['E0'], last['E'], [sw['accepted'].tolist() for sw in rep['sweeps']], rep['parts0'].tolist(), last['parts'].tolist(),
                 timing['joint']))
        assert rep['group'].tolist() == [0] * FRAMES and rep['shares'] == dict(scene=0.0, silhouette=1.0, temporal=400.0)
        assert rep['images'] == [(int(t), int(c)) for t, c in zip(prob, view)] and rep['mask_size'] == (H // K, W // K)
        assert 1 <= len(rep['sweeps']) <= 2 and timing['joint'] > 0
        assert r['frames'] == ['%05d' % (t + 1) for t in range(FRAMES)]
        assert r['params'].shape == (FRAMES, 118) and np.array_equal(r['params'], last['params'])
        assert np.array_equal(r['final_loss'], rep['loss'].astype(np.float32))
        for t in range(FRAMES):
            path = tmp_path / 'results' / '0000' / ('%05d' % (t + 1)) / '000.pkl'
            assert str(path) == r['files'][t] and path.exists()
            with open(path, 'rb') as f:
                res = pickle.load(f)
            assert np.array_equal(res['betas'][0], r['params'][t, :10])
            assert float(res['loss']) == float(r['final_loss'][t]) == float(np.float32(rep['loss'][t]))
        # both components fell from the keypoint fit's values, and the energy with them
        assert last['E'][0] < rep['E0'][0]
        assert rep['parts0'][0, 0] == 0 and last['parts'][0, 1] < rep['parts0'][0, 1] and last['parts'][0, 2] < rep['parts0'][0, 2]
        # the engine is handed back without mix, targets and mask set
        assert eng._mix is None
        with pytest.raises(Exception, match='error -3'):
            eng.silhouette_loss(v)
    finally:
        eng.close()
