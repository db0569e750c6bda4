"""GPU: fit_folder(silhouettes=...) on the demo inputs (tests/golden/demo_data): the keypoint fit's own result rendered into
one 1536 x 2048 mask per camera, written as PNG under a temporary mask_root and fitted against at downscale=4."""
import os
import pickle

import numpy as np
import pytest
import torch

from mvsmplfitting_amd import _lib, batch
from mvsmplfitting_amd import io_formats as iof
from mvsmplfitting_amd.engine import MvFit, stage_weights
from tests.helpers import GOLD, body_model

pytestmark = pytest.mark.gpu
DATA = os.path.join(GOLD, 'demo_data')
H, W, K, WEIGHT = 1536, 2048, 4, 1.0


def _vposer():
    d = dict(np.load(os.path.join(GOLD, 'vposer_poser_epoch091_decoder.npz')))
    return {k: d[k] for k in ('fc1_w', 'fc1_b', 'fc2_w', 'fc2_b', 'out_w', 'out_b')}


def test_demo_folder_refined_against_its_own_masks(tmp_path):
    from PIL import Image
    keyp, cam_file = os.path.join(DATA, 'keypoints'), os.path.join(DATA, '3DOH50K_Parameters.txt')
    eng = MvFit(body_model(), vposer=_vposer())
    try:
        base = batch.fit_folder(body_model(), keyp, cam_file, str(tmp_path / 'plain'), vposer=_vposer(), image_height=float(H),
                                engine=eng)['0000']
        serial, cams, frames = batch.list_frames(keyp)[0]
        V = len(cams)
        v, _ = eng.vertices(base['params'], flags=_lib.F_VPOSER)          # (the serial's problems are still set)
        _, fid = eng.render_overlay(v, None, np.zeros((V, H, W, 3), np.uint8), np.zeros(V, np.int32), np.arange(V, dtype=np.int32),
                                    face_id=True)
        on = (fid >= 0).cpu().numpy()
        assert on.reshape(V, -1).any(axis=1).all()
        root = tmp_path / 'masks'
        for i, cam in enumerate(cams):
            os.makedirs(root / serial / cam)
            Image.fromarray(on[i].astype(np.uint8) * 255, 'L').save(batch.mask_path(str(root), serial, cam, frames[0][0]))
        timing = {}
        out = batch.fit_folder(body_model(), keyp, cam_file, str(tmp_path / 'results'), vposer=_vposer(), image_height=float(H),
                               engine=eng, timing=timing, silhouettes=dict(mask_root=str(root), weight=WEIGHT, downscale=K))
        r = out['0000']
        rep = r['silhouette_report']
        print('objective %s -> %s, accepted %s, silhouette loss %s -> %s, %s closures, %.3f s'
              % (rep['before'], rep['after'], rep['accepted'], rep['silhouette_before'], rep['silhouette_after'], rep['n_closure'],
                 timing['silhouette']))
        assert rep['images'] == [(0, i) for i in range(V)] and rep['mask_size'] == (H // K, W // K)
        assert timing['silhouette'] > 0
        path = tmp_path / 'results' / '0000' / '00001' / '000.pkl'
        assert str(path) == r['files'][0] and path.exists()
        with open(path, 'rb') as f:
            res = pickle.load(f)
        assert np.array_equal(res['betas'][0], r['params'][0, :10]) and float(res['loss']) == float(r['final_loss'][0])
        if not rep['accepted'][0]:
            assert np.array_equal(r['params'], base['params'])
        # final_loss is the closure with the term at the written parameters
        ex, it = (np.asarray(a[:V], np.float64) for a in iof.load_camera_para(cam_file))
        view = np.arange(V)
        per_image = (ex[view, :3, :3].astype(np.float32), ex[view, :3, 3].astype(np.float32),
                     (it[view, 0, 0] / K).astype(np.float32), (it[view, :2, 2] / K).astype(np.float32))
        masks = np.stack([iof.downscale_mask(iof.read_mask(batch.mask_path(str(root), serial, cam, frames[0][0])), K)
                          for cam in cams])
        eng.set_silhouettes(masks, np.zeros(V, np.int32), per_image)
        eng.set_silhouette_term()
        stage = dict(stage_weights(float(H), flags=_lib.F_VPOSER)[-1], coll_loss_weight=WEIGHT)
        L = float(eng.closure(torch.as_tensor(r['params']), stage, want_grad=False)['loss'][0])
        assert abs(L - float(r['final_loss'][0])) <= 1e-6 * abs(L), (L, r['final_loss'])
    finally:
        eng.close()
