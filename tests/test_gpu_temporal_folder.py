"""GPU: fit_folder(temporal=...) on a temporary serial of four frames made from the demo inputs (tests/golden/demo_data): the
demo frame's keypoints, drifting a few pixels per frame with a little independent noise.  With and without is_seq the usual
files are written, the result carries temporal_report, and the loss in the result files is the report's."""
import json
import os
import pickle
import shutil

import numpy as np
import pytest

from mvsmplfitting_amd import batch
from mvsmplfitting_amd.engine import MvFit
from tests.helpers import GOLD, body_model

pytestmark = pytest.mark.gpu
DATA = os.path.join(GOLD, 'demo_data')
FRAMES, WEIGHT = 4, 20.0


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


@pytest.mark.parametrize('is_seq', [False, True])
def test_a_serial_is_smoothed_and_written(tmp_path, is_seq):
    keyp, cam_file = str(tmp_path / 'keypoints'), str(tmp_path / 'cams.txt')
    _make_serial(keyp)
    shutil.copy(os.path.join(DATA, '3DOH50K_Parameters.txt'), cam_file)
    eng = MvFit(body_model(), vposer=_vposer())
    try:
        timing = {}
        out = batch.fit_folder(body_model(), keyp, cam_file, str(tmp_path / 'results'), vposer=_vposer(), image_height=1536.0,
                               engine=eng, is_seq=is_seq, timing=timing, temporal=dict(weight=WEIGHT, sweeps=2))
        r = out['0000']
        rep = r['temporal_report']
        print('is_seq %s: E %s -> %s, smooth %s -> %s, accepted %s, %.3f s'
              % (is_seq, rep['E0'], rep['sweeps'][-1]['E'], rep['smooth0'], rep['sweeps'][-1]['smooth'],
                 [sw['accepted'].tolist() for sw in rep['sweeps']], timing['temporal']))
        pairs = FRAMES - 1
        print('  rms vertex displacement between consecutive frames %.4f -> %.4f (world units); translation per frame %s, scale %s, restarted %s'
              % (np.sqrt(rep['smooth0'][0] / (pairs * eng.nv)), np.sqrt(rep['sweeps'][-1]['smooth'][0] / (pairs * eng.nv)),
                 np.round(r['params'][:, 82:85], 3).tolist(), np.round(r['params'][:, 85], 3).tolist(), np.asarray(r['restarted']).tolist()))
        assert r['frames'] == ['%05d' % (t + 1) for t in range(FRAMES)]
        assert rep['E0'].shape == (1,) and 1 <= len(rep['sweeps']) <= 2 and timing['temporal'] > 0
        assert r['params'].shape == (FRAMES, 118) and np.array_equal(r['params'], rep['sweeps'][-1]['params'])
        assert np.array_equal(r['final_loss'], rep['loss'].astype(np.float32))
        for t in range(FRAMES):
            path = tmp_path / 'results' / '0000' / ('%05d' % (t + 1)) / '000.pkl'
            assert str(path) == r['files'][t] and path.exists()
            with open(path, 'rb') as f:
                res = pickle.load(f)
            assert np.array_equal(res['betas'][0], r['params'][t, :10])
            assert float(res['loss']) == float(r['final_loss'][t]) == float(np.float32(rep['loss'][t]))
        assert (rep['sweeps'][-1]['E'] <= rep['E0']).all()            # (the accept rule: never above the start)
        # the engine is handed back without the term
        assert not eng._vt_term
    finally:
        eng.close()
