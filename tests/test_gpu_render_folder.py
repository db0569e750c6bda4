"""GPU: fit_folder(save_images=True) on the reference's demo inputs (tests/golden/demo_data) with synthetic 2048 x 1536
JPEGs: one overlay per view that has keypoints, each the render_overlay of the saved parameters within JPEG tolerance;
the fit's own outputs unchanged; a missing image is a ValueError."""
import os
import pickle
import shutil

import numpy as np
import pytest

from mvsmplfitting_amd import batch
from mvsmplfitting_amd import io_formats as iof
from mvsmplfitting_amd.engine import MvFit
from tests.helpers import GOLD, body_model

pytestmark = pytest.mark.gpu
PIL = pytest.importorskip('PIL')
DATA = os.path.join(GOLD, 'demo_data')
CAMS = os.path.join(DATA, '3DOH50K_Parameters.txt')


def _images(root, keyp):
    """A smooth synthetic 2048 x 1536 picture per camera folder and frame of the keypoint tree."""
    yy, xx = np.mgrid[0:1536, 0:2048]
    for serial, cams, frames in batch.list_frames(keyp):
        for v, cam in enumerate(cams):
            d = os.path.join(root, serial, cam)
            os.makedirs(d, exist_ok=True)
            base = np.stack([(xx * 255 // 2047), (yy * 255 // 1535), np.full_like(xx, 40 * v)], -1).astype(np.uint8)
            for fn, _ in frames:
                iof.save_image(os.path.join(d, fn + '.jpg'), base)


def test_demo_folder_save_images(tmp_path):
    keyp = str(tmp_path / 'data' / 'keypoints')
    shutil.copytree(os.path.join(DATA, 'keypoints'), keyp)
    # camera 05 has no keypoint file in this frame: no image is read or written for it
    os.remove(os.path.join(keyp, '0000', 'Camera05', '00001_keypoints.json'))
    _images(str(tmp_path / 'data' / 'images'), keyp)
    model = body_model()
    timing = {}
    with MvFit(model) as eng:
        plain = batch.fit_folder(model, keyp, CAMS, str(tmp_path / 'plain'), engine=eng)
        out = batch.fit_folder(model, keyp, CAMS, str(tmp_path / 'res'), engine=eng, save_images=True, timing=timing)
        assert 'render' in timing and timing['render'] > 0
        r, p = out['0000'], plain['0000']
        assert np.array_equal(r['params'], p['params']) and np.array_equal(r['final_loss'], p['final_loss'])
        for a, b in zip(r['files'], p['files']):
            with open(a, 'rb') as fa, open(b, 'rb') as fb:
                assert fa.read() == fb.read()
        written = sorted(os.listdir(tmp_path / 'res' / 'images' / '0000' / '00001'))
        assert written == ['Camera%02d.jpg' % v for v in range(5)], written
        assert r['images'] == [str(tmp_path / 'res' / 'images' / '0000' / '00001' / w) for w in written]
        # each overlay: the renderer on the saved parameters (feet / hands zeroed), within JPEG tolerance
        with open(r['files'][0], 'rb') as f:
            res = pickle.load(f)
        x = r['params'].copy()
        x[0, 13:82] = res['body_pose'][0]
        verts, joints = eng.vertices(x, flags=0)
        imgs = np.stack([iof.read_image(str(tmp_path / 'data' / 'images' / '0000' / ('Camera%02d' % v) / '00001.jpg'))
                         for v in range(5)])
        want, fid = eng.render_overlay(verts, joints, imgs, [0] * 5, list(range(5)), face_id=True)
        want = want.cpu().numpy()
        fid = fid.cpu().numpy()
        for v in range(5):
            got = iof.read_image(r['images'][v])
            assert got.shape == (1536, 2048, 3)
            assert (fid[v] >= 0).sum() > 1000, 'the fitted body should be in view %d' % v
            mad = np.abs(got.astype(np.int16) - want[v].astype(np.int16)).mean()
            assert mad < 2.0, (v, mad)
        # a view with keypoints but no image
        os.remove(str(tmp_path / 'data' / 'images' / '0000' / 'Camera02' / '00001.jpg'))
        with pytest.raises(ValueError, match='Camera02'):
            batch.fit_folder(model, keyp, CAMS, str(tmp_path / 'res2'), engine=eng, save_images=True)


def test_render_serial_images_in_chunks(tmp_path, monkeypatch):
    """More jobs than one GPU call takes (RENDER_BATCH lowered to 2), two image sizes: every overlay is the
    render_overlay of its own problem and view."""
    monkeypatch.setattr(batch, 'RENDER_BATCH', 2)
    from concurrent.futures import ThreadPoolExecutor
    from mvsmplfitting_amd import synthetic as syn
    from mvsmplfitting_amd.engine import pack_params
    model = body_model()
    R, t, f, c = syn.make_camera_ring(4)
    cams = (R, t, f * np.float32(320 / 2048.0), np.tile(np.array([160.0, 120.0], np.float32), (4, 1)))
    jobs = []
    for n in range(7):
        H, W = (240, 320) if n % 3 else (200, 300)
        path = str(tmp_path / ('in%d.png' % n))
        yy, xx = np.mgrid[0:H, 0:W]
        iof.save_image(path, np.stack([xx * 255 // W, yy * 255 // H, np.full_like(xx, 30 * n)], -1).astype(np.uint8))
        jobs.append((n % 2, n % 4, path, ('S', 'f%d' % (n % 2), 'Cam%d' % n)))
    with MvFit(model) as eng:
        eng.set_problems(cams, np.zeros((2, 4, 17, 2), np.float32), np.zeros((2, 4, 17), np.float32))
        verts, joints = eng.vertices(pack_params(B=2, **syn.make_frames(2)))
        with ThreadPoolExecutor(4) as pool:
            paths = batch.render_serial_images(eng, verts, joints, jobs, str(tmp_path / 'out'), pool)
        for j, p in zip(jobs, paths):
            assert p == str(tmp_path / 'out' / 'S' / j[3][1] / (j[3][2] + '.jpg'))
            want = eng.render_overlay(verts, joints, iof.read_image(j[2])[None], [j[0]], [j[1]])[0].cpu().numpy()
            got = iof.read_image(p)
            assert got.shape == want.shape
            assert np.abs(got.astype(np.int16) - want.astype(np.int16)).mean() < 2.0
