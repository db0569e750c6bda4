"""GPU: fit_folder(scans=dict(root=...)) and fit_folder(joint=dict(silhouettes=..., scans=...)) on a temporary serial of four
frames made from the demo inputs (tests/golden/demo_data), as tests/test_gpu_joint_folder.py builds it.  Point files: 2000
samples, 1 mm of noise, of the surface of the keypoint fit's bodies with other betas and a 3 % larger scale; the last frame has
no file.  Masks (the joint run): those bodies rendered into two cameras per frame, fitted against at downscale=4.  The scan
weight is sqrt(mean keypoint objective / mean scan loss) at the keypoint fit: neither term drowns the other.  No threshold on
how far the scan loss falls: it is printed."""
import os
import pickle
import shutil

import numpy as np
import pytest

from mvsmplfitting_amd import _lib, batch
from mvsmplfitting_amd.engine import MvFit
from tests.helpers import body_model
from tests.test_gpu_joint_folder import DATA, FRAMES, H, K, MASK_VIEWS, W, _make_serial, _vposer
from tests.test_gpu_scan_loss import surface_samples

pytestmark = pytest.mark.gpu
P = 2000
NOISE = 0.001
WITH_FILE = (0, 1, 2)                   # frame 3 has no point file
D_BETAS = np.array([0.8, -0.6, 0.5, -0.4, 0.3, 0.0, 0.0, 0.0, 0.0, 0.0], np.float32)
SCAN_KW = dict(w_s2m=1.0, w_m2s=0.0, sigma=0.05)


@pytest.fixture(scope='module')
def world(tmp_path_factory):
    from PIL import Image
    tmp = tmp_path_factory.mktemp('scan_folder')
    keyp, cam_file = str(tmp / 'keypoints'), str(tmp / 'cams.txt')
    _make_serial(keyp)
    shutil.copy(os.path.join(DATA, '3DOH50K_Parameters.txt'), cam_file)
    model = body_model()
    faces = np.asarray(model['faces'], np.int64)
    eng = MvFit(model, vposer=_vposer())
    base = batch.fit_folder(model, keyp, cam_file, str(tmp / 'plain'), vposer=_vposer(), image_height=float(H), engine=eng)['0000']
    serial, cams, frames = batch.list_frames(keyp)[0]
    x = base['params']
    other = x.copy()
    other[:, :10] += D_BETAS
    other[:, 85] *= np.float32(1.03)
    v, _ = eng.vertices(other, flags=_lib.F_VPOSER)                   # (the serial's problems are still set)
    vh = v.cpu().numpy().astype(np.float64)
    rng = np.random.default_rng(11)
    root = tmp / 'scans'
    points = np.zeros((FRAMES, P, 3), np.float32)
    for t in WITH_FILE:
        points[t] = surface_samples(vh[t], faces, P, NOISE, rng)
        path = batch.scan_path(str(root), serial, frames[t][0])
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.save(path, points[t])
    count = np.array([P if t in WITH_FILE else 0 for t in range(FRAMES)], np.int32)
    # the weight: the keypoint objective against the scan loss, both at the keypoint fit
    eng.set_scans(points, count=count)
    L0 = eng.scan_loss(eng.vertices(x, flags=_lib.F_VPOSER)[0], need_grad=False, **SCAN_KW)[0].cpu().numpy().astype(np.float64)
    eng.clear_scans()
    weight = float(np.sqrt(base['final_loss'].astype(np.float64).mean() / L0[list(WITH_FILE)].mean()))
    # the masks of the joint run
    prob = np.repeat(np.arange(FRAMES), len(MASK_VIEWS)).astype(np.int32)
    view = np.tile(np.array(MASK_VIEWS, np.int32), FRAMES)
    _, fid = eng.render_overlay(v, None, np.zeros((len(prob), H, W, 3), np.uint8), prob, view, face_id=True)
    on = (fid >= 0).cpu().numpy()
    mroot = tmp / 'masks'
    for i, (t, c) in enumerate(zip(prob, view)):
        os.makedirs(mroot / serial / cams[c], exist_ok=True)
        Image.fromarray(on[i].astype(np.uint8) * 255, 'L').save(batch.mask_path(str(mroot), serial, cams[c], frames[t][0]))
    yield dict(tmp=tmp, keyp=keyp, cam_file=cam_file, model=model, eng=eng, base=base, root=str(root), mroot=str(mroot), L0=L0,
               weight=weight, count=count, v=v)
    eng.close()


def _files(world, folder, r):
    for t in range(FRAMES):
        path = world['tmp'] / folder / '0000' / ('%05d' % (t + 1)) / '000.pkl'
        assert str(path) == r['files'][t] and path.exists()
        with open(path, 'rb') as f:
            res = pickle.load(f)
        assert np.array_equal(res['betas'][0], r['params'][t, :10])
        assert float(res['loss']) == float(r['final_loss'][t])


def _clean(world):
    """the engine is handed back without scan set, mix and term"""
    eng = world['eng']
    assert eng._scan_shape is None and eng._mix is None and not eng._scan_term
    with pytest.raises(Exception, match='error -3'):
        eng.scan_loss(world['v'], need_grad=False)
    with pytest.raises(Exception, match='error -3'):
        eng.term_mix_read()


def test_a_serial_is_refined_against_its_point_files(world):
    eng, base, w = world['eng'], world['base'], world['weight']
    timing = {}
    out = batch.fit_folder(world['model'], world['keyp'], world['cam_file'], str(world['tmp'] / 'results'), vposer=_vposer(),
                           image_height=float(H), engine=eng, timing=timing, scans=dict(weight=w, root=world['root'], **SCAN_KW))
    r = out['0000']
    rep = r['scan_report']
    acc = rep['accepted']
    print('weight %.4g | scan loss (m^2) before %s after %s | objective before %s after %s | accepted %s | %.3f s'
          % (w, rep['scan_before'].tolist(), rep['scan_after'].tolist(), rep['before'].tolist(), rep['after'].tolist(), acc.tolist(),
             timing['scan']))
    fell = 1.0 - rep['scan_after'][list(WITH_FILE)].sum() / rep['scan_before'][list(WITH_FILE)].sum()
    print('scan loss over the frames with a file: fell by %.1f %%' % (100.0 * fell))
    assert rep['points'].tolist() == world['count'].tolist() and timing['scan'] > 0
    # (the op at the keypoint fit's bodies through MvFit.vertices; the closure's vertex pass may differ from it in the last bits)
    assert np.allclose(rep['scan_before'], world['L0'], rtol=1e-3, atol=0)
    assert r['params'].shape == (FRAMES, 118) and np.array_equal(r['final_loss'], np.asarray(rep['loss'], np.float32))
    _files(world, 'results', r)
    assert (rep['scan_after'] <= rep['scan_before']).all()
    assert rep['scan_before'][3] == 0 and rep['scan_after'][3] == 0                 # the frame without a file pays nothing
    assert acc[list(WITH_FILE)].any()
    assert (rep['after'][acc] < rep['before'][acc]).all()
    assert np.array_equal(rep['after'][~acc], rep['before'][~acc])
    assert np.array_equal(r['params'][~acc], base['params'][~acc])                   # a rejected row: the keypoint fit's bits
    assert not np.array_equal(r['params'][acc], base['params'][acc])
    _clean(world)


def test_a_serial_is_refined_jointly_against_masks_and_point_files(world):
    eng, base, w = world['eng'], world['base'], world['weight']
    timing = {}
    joint = dict(weight=1.0, sweeps=2, silhouettes=dict(share=1.0, mask_root=world['mroot'], downscale=K),
                 scans=dict(share=w * w, root=world['root'], **SCAN_KW))
    out = batch.fit_folder(world['model'], world['keyp'], world['cam_file'], str(world['tmp'] / 'joint'), vposer=_vposer(),
                           image_height=float(H), engine=eng, timing=timing, joint=joint)
    r = out['0000']
    rep = r['joint_report']
    last = rep['sweeps'][-1]
    print('E %s -> %s, accepted %s, parts (S_sc^2, L_sil, L_vt, L_scan) %s -> %s, %.3f s'
          % (rep['E0'].tolist(), last['E'].tolist(), [sw['accepted'].tolist() for sw in rep['sweeps']], rep['parts0'].tolist(),
             last['parts'].tolist(), timing['joint']))
    # every problem is a group of its own: neither part links problems
    assert rep['group'].tolist() == list(range(FRAMES))
    assert rep['shares'] == dict(scene=0.0, silhouette=1.0, temporal=0.0, scan=float(w * w))
    assert rep['parts0'].shape == (FRAMES, 4) and last['parts'].shape == (FRAMES, 4) and rep['parts_problem'].shape == (FRAMES, 4)
    assert rep['points'].tolist() == world['count'].tolist() and rep['mask_size'] == (H // K, W // K)
    assert np.allclose(rep['parts0'][:, 3], world['L0'], rtol=1e-3, atol=0)
    assert not rep['parts0'][:, 0].any() and not rep['parts0'][:, 2].any() and (rep['parts0'][:, 1] > 0).all()
    assert np.array_equal(r['params'], last['params']) and np.array_equal(r['final_loss'], rep['loss'].astype(np.float32))
    _files(world, 'joint', r)
    ever = np.zeros(FRAMES, bool)
    prev = rep['E0']
    for sw in rep['sweeps']:
        assert (sw['E'] <= prev).all() and (sw['E'][sw['accepted']] < prev[sw['accepted']]).all()
        ever |= sw['accepted']
        prev = sw['E']
    assert ever.any()
    assert np.array_equal(r['params'][~ever], base['params'][~ever])                 # a rejected row: the keypoint fit's bits
    assert (last['parts'][list(WITH_FILE), 3] <= rep['parts0'][list(WITH_FILE), 3]).all()
    assert eng._mix is None
    with pytest.raises(Exception, match='error -3'):
        eng.silhouette_loss(world['v'])
    _clean(world)
