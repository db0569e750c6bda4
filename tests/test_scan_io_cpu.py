"""CPU: fit_folder(scans=...) and joint=dict(scans=...) up to the engine - the option checks (every ValueError is raised before
any engine is created: engine=None and no GPU here), the file layout, and the two loaders on files under tmp_path: point files
with and without weights, the subsample rule one past max_points, problems without a file, the multi-person file name, and
depth maps against scan.points_from_depth called directly."""
import os

import numpy as np
import pytest

from mvsmplfitting_amd import batch
from mvsmplfitting_amd import io_formats as iof
from mvsmplfitting_amd.scan import points_from_depth
from tests.helpers import body_model

FRAMES = [('000000',), ('000001',), ('000002',)]
CAMS = ['camA', 'camB']
H, W = 6, 8
RIG = (np.stack([np.eye(3), np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]])]).astype(np.float32),
       np.array([[0.0, 0.0, 2.0], [0.1, -0.2, 3.0]], np.float32), np.array([10.0, 12.0], np.float32),
       np.array([[4.0, 3.0], [3.5, 2.5]], np.float32))


def _save(path, a):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.save(path, a)


def _cfg(**kw):
    return dict(batch.SCAN_DEFAULTS, **kw)


# ------------------------------------------------------------------------------------------------ the option
def test_check_scans_fills_the_defaults():
    cfg = batch.check_scans(dict(weight=30.0, root='r'))
    assert cfg == dict(weight=30.0, root='r', depth_root=None, w_s2m=1.0, w_m2s=0.0, sigma=0.05, max_points=8192, stride=1,
                       mask_root=None)
    cfg = batch.check_scans(dict(weight=1.0, depth_root='d', mask_root='m', stride=2, w_m2s=0.5), multi=True)
    assert (cfg['depth_root'], cfg['mask_root'], cfg['stride'], cfg['w_m2s'], cfg['root']) == ('d', 'm', 2, 0.5, None)


def test_fit_folder_scans_argument_errors(tmp_path):
    model = body_model()
    run = lambda **kw: batch.fit_folder(model, str(tmp_path / 'none'), str(tmp_path / 'none.txt'), str(tmp_path / 'out'), **kw)
    ok = dict(weight=1.0, root=str(tmp_path))
    with pytest.raises(ValueError, match="scans: a dict with at least 'weight'"):
        run(scans=True)
    with pytest.raises(ValueError, match="scans: a dict with at least 'weight'"):
        run(scans=dict(root='r'))
    with pytest.raises(ValueError, match='scans: unknown keys .*rooot'):
        run(scans=dict(weight=1.0, rooot='r'))
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='scans: weight must be > 0'):
            run(scans=dict(ok, weight=bad))
    # exactly one source
    with pytest.raises(ValueError, match='scans: exactly one of root'):
        run(scans=dict(weight=1.0))
    with pytest.raises(ValueError, match='scans: exactly one of root'):
        run(scans=dict(ok, depth_root='d'))
    for bad in (dict(w_s2m=-1.0), dict(sigma=float('nan')), dict(w_m2s=float('inf'))):
        with pytest.raises(ValueError, match='scans: w_s2m, w_m2s and sigma must be finite and >= 0'):
            run(scans=dict(ok, **bad))
    with pytest.raises(ValueError, match='scans: w_s2m and w_m2s are both 0'):
        run(scans=dict(ok, w_s2m=0.0))
    for bad in (dict(max_points=0), dict(stride=0)):
        with pytest.raises(ValueError, match='scans: max_points and stride must be >= 1'):
            run(scans=dict(ok, **bad))
    # depth maps of several persons need masks
    with pytest.raises(ValueError, match='scans: depth maps of more than one person need mask_root'):
        run(scans=dict(weight=1.0, depth_root='d'), persons='all')
    # what it does not go with, in the wording of the existing pairs
    with pytest.raises(ValueError, match='scans is not available with is_seq=True'):
        run(scans=ok, is_seq=True)
    with pytest.raises(ValueError, match='refine_cameras with scans is not built'):
        run(scans=ok, refine_cameras=dict())
    with pytest.raises(ValueError, match="scans and silhouettes both use the fit's one term slot"):
        run(scans=ok, silhouettes=dict(mask_root='m', weight=1.0))
    with pytest.raises(ValueError, match="scans and temporal both use the fit's one term slot"):
        run(scans=ok, temporal=dict(weight=1.0))
    with pytest.raises(ValueError, match="scans and scene_collision both use the fit's one term slot"):
        run(scans=ok, scene_collision=dict(weight=1.0), persons='all')
    with pytest.raises(ValueError, match='joint and scans'):
        run(scans=ok, joint=dict(weight=1.0, temporal=dict(share=1.0), silhouettes=dict(share=1.0, mask_root='m')))
    assert not (tmp_path / 'out').exists()


def test_check_joint_with_a_scans_part(tmp_path):
    sc = dict(share=1.5, root=str(tmp_path))
    cfg = batch.check_joint(dict(weight=2.0, temporal=dict(share=0.25), scans=sc))
    assert cfg['scans'] == dict(share=1.5, root=str(tmp_path), depth_root=None, w_s2m=1.0, w_m2s=0.0, sigma=0.05, max_points=8192,
                                stride=1, mask_root=None)
    assert cfg['temporal'] == dict(share=0.25) and 'silhouettes' not in cfg
    # "at least two" counts four parts
    with pytest.raises(ValueError, match='joint: at least two of'):
        batch.check_joint(dict(weight=1.0, scans=sc))
    cfg = batch.check_joint(dict(weight=1.0, scans=sc, scene_collision=dict(share=1.0), silhouettes=dict(share=1.0, mask_root='m'),
                                 temporal=dict(share=1.0)), multi=True)
    assert set(cfg) == {'weight', 'sweeps', 'scene_collision', 'silhouettes', 'temporal', 'scans'}
    # the part's own checks
    t = dict(share=1.0)
    with pytest.raises(ValueError, match="joint: scans: a dict with at least 'share'"):
        batch.check_joint(dict(weight=1.0, temporal=t, scans=dict(root='r')))
    with pytest.raises(ValueError, match='joint: scans: unknown keys .*weight'):
        batch.check_joint(dict(weight=1.0, temporal=t, scans=dict(sc, weight=1.0)))
    for bad in (0.0, -2.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='joint: scans: share must be > 0'):
            batch.check_joint(dict(weight=1.0, temporal=t, scans=dict(sc, share=bad)))
    with pytest.raises(ValueError, match='joint: scans: exactly one of root'):
        batch.check_joint(dict(weight=1.0, temporal=t, scans=dict(share=1.0)))
    with pytest.raises(ValueError, match='joint: scans: w_s2m and w_m2s are both 0'):
        batch.check_joint(dict(weight=1.0, temporal=t, scans=dict(sc, w_s2m=0.0)))
    with pytest.raises(ValueError, match='joint: scans: depth maps of more than one person need mask_root'):
        batch.check_joint(dict(weight=1.0, temporal=t, scans=dict(share=1.0, depth_root='d')), multi=True)
    with pytest.raises(ValueError, match='joint and scans'):
        batch.check_joint(dict(weight=1.0, temporal=t, scans=sc), scans=dict(weight=1.0, root='r'))


# ------------------------------------------------------------------------------------------------ the files
def test_scan_path():
    assert batch.scan_path('r', 's1', '000007') == os.path.join('r', 's1', '000007.npy')
    assert batch.scan_path('r', 's1', '000007', 12) == os.path.join('r', 's1', '000007_012.npy')
    assert batch.scan_path('d', 's1', '000007', camera='camB') == os.path.join('d', 's1', 'camB', '000007.npy')
    assert batch.scan_path('d', 's1', '000007', 3, camera='camB') == os.path.join('d', 's1', 'camB', '000007.npy')


def test_point_files_weights_and_problems_without_a_file(tmp_path):
    root = str(tmp_path)
    rng = np.random.default_rng(0)
    a = rng.normal(size=(5, 3)).astype(np.float32)
    b = np.concatenate([rng.normal(size=(9, 3)), rng.uniform(0, 2, (9, 1))], axis=1)          # float64 [P,4]
    b[4, 3] = 0.0
    _save(batch.scan_path(root, 's1', '000000'), a)
    _save(batch.scan_path(root, 's1', '000002'), b)
    pts, count, w, found = batch.load_serial_scans(_cfg(root=root), 's1', CAMS, FRAMES, [(0, None), (1, None), (2, None)], RIG)
    assert pts.shape == (3, 9, 3) and pts.dtype == np.float32 and count.dtype == np.int32
    assert count.tolist() == [5, 0, 9]                                  # the frame without a file: no points
    assert np.array_equal(pts[0, :5], a) and np.array_equal(pts[2], b[:, :3].astype(np.float32))
    assert w.shape == (3, 9) and w.dtype == np.float32
    assert np.array_equal(w[2], b[:, 3].astype(np.float32)) and (w[0] == 1).all()         # a [P,3] file beside a [P,4] one: weight 1
    assert [n for n, _ in found] == [0, 2]
    # no weights anywhere: None
    pts, count, w, _ = batch.load_serial_scans(_cfg(root=root), 's1', CAMS, FRAMES, [(0, None), (1, None)], RIG)
    assert w is None and pts.shape == (2, 5, 3) and count.tolist() == [5, 0]
    # a serial without any file names an example path
    with pytest.raises(ValueError, match='scans: serial s2 has no scan file under .*000001.npy'):
        batch.load_serial_scans(_cfg(root=root), 's2', CAMS, FRAMES, [(1, None), (2, None)], RIG)


def test_point_file_refusals(tmp_path):
    root = str(tmp_path)
    bad = {'shape': np.zeros((4, 2), np.float32), 'rank': np.zeros((4, 3, 1), np.float32), 'dtype': np.zeros((4, 3), np.int32)}
    for name, arr in bad.items():
        _save(batch.scan_path(root, name, '000000'), arr)
        with pytest.raises(ValueError, match='a point file holds a float array'):
            batch.load_serial_scans(_cfg(root=root), name, CAMS, FRAMES, [(0, None)], RIG)
    for k, v in enumerate((-0.5, float('nan'), float('inf'))):
        a = np.ones((3, 4), np.float32)
        a[1, 3] = v
        _save(batch.scan_path(root, 'w%d' % k, '000000'), a)
        with pytest.raises(ValueError, match='weights .* must be finite and >= 0'):
            batch.load_serial_scans(_cfg(root=root), 'w%d' % k, CAMS, FRAMES, [(0, None)], RIG)


def test_the_subsample_rule_one_past_max_points(tmp_path):
    root = str(tmp_path)
    cap = 16
    P = cap + 1
    a = np.concatenate([np.arange(P * 3, dtype=np.float64).reshape(P, 3), np.linspace(0.5, 1.5, P)[:, None]], axis=1)
    _save(batch.scan_path(root, 's1', '000000'), a)
    _save(batch.scan_path(root, 's1', '000001'), a[:cap])
    pts, count, w, _ = batch.load_serial_scans(_cfg(root=root, max_points=cap), 's1', CAMS, FRAMES, [(0, None), (1, None)], RIG)
    rows = [int(np.floor(i * P / cap)) for i in range(cap)]
    assert rows == list(range(cap)) and rows != list(range(1, P))        # (at P = cap + 1 the last row is the one left out)
    assert count.tolist() == [cap, cap] and pts.shape == (2, cap, 3)
    assert np.array_equal(pts[0], a[rows, :3].astype(np.float32)) and np.array_equal(w[0], a[rows, 3].astype(np.float32))
    assert np.array_equal(pts[1], a[:cap, :3].astype(np.float32))       # exactly max_points: every row
    assert batch.subsample_rows(40, 16).tolist() == [int(np.floor(i * 40 / 16)) for i in range(16)]


def test_the_multi_person_file_name(tmp_path):
    root = str(tmp_path)
    a, b = np.full((2, 3), 1.0, np.float32), np.full((3, 3), 2.0, np.float32)
    _save(batch.scan_path(root, 's1', '000001', 0), a)
    _save(batch.scan_path(root, 's1', '000001', 7), b)
    _save(batch.scan_path(root, 's1', '000001'), np.full((4, 3), 9.0, np.float32))       # (the single-person name: not a person's)
    problems = [(0, 0), (1, 0), (1, 7), (2, 7)]
    pts, count, w, found = batch.load_serial_scans(_cfg(root=root), 's1', CAMS, FRAMES, problems, RIG)
    assert count.tolist() == [0, 2, 3, 0] and w is None
    assert (pts[1, :2] == 1.0).all() and (pts[2] == 2.0).all()
    assert [os.path.basename(p) for _, p in found] == ['000001_000.npy', '000001_007.npy']


def _depth(seed):
    d = np.random.default_rng(seed).uniform(1.0, 3.0, (H, W)).astype(np.float32)
    d[0, :3] = 0.0
    d[1, 1] = np.nan
    return d


def test_depth_maps_against_points_from_depth(tmp_path):
    droot, mroot = str(tmp_path / 'depth'), str(tmp_path / 'masks')
    from PIL import Image
    dA, dB, dA2 = _depth(1), _depth(2), _depth(3)
    _save(batch.scan_path(droot, 's1', '000000', camera='camA'), dA)
    _save(batch.scan_path(droot, 's1', '000000', camera='camB'), dB)
    _save(batch.scan_path(droot, 's1', '000002', camera='camB'), dA2)
    cfg = _cfg(depth_root=droot, stride=2)
    pts, count, w, found = batch.load_serial_scans(cfg, 's1', CAMS, FRAMES, [(0, None), (1, None), (2, None)], RIG)
    ref0 = points_from_depth(np.stack([dA, dB]), RIG, stride=2)
    ref2 = points_from_depth(dA2[None], tuple(a[1:] for a in RIG), stride=2)               # its one view is rig row 1
    assert w is None and count.tolist() == [len(ref0), 0, len(ref2)] and len(ref0) > len(ref2) > 0
    assert np.array_equal(pts[0, :len(ref0)], ref0) and np.array_equal(pts[2, :len(ref2)], ref2)
    assert [n for n, _ in found] == [0, 0, 2]
    # max_points is points_from_depth's
    few, count_few, _, _ = batch.load_serial_scans(dict(cfg, max_points=7), 's1', CAMS, FRAMES, [(0, None)], RIG)
    assert count_few.tolist() == [7] and np.array_equal(few[0], points_from_depth(np.stack([dA, dB]), RIG, stride=2, max_points=7))
    # masks: the person's own file where it exists, every pixel of a view without one; two persons share the depth maps
    mA = np.zeros((H, W), np.uint8)
    mA[2:5, 2:6] = 255
    path = batch.mask_path(mroot, 's1', 'camA', '000000', 4)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(mA).save(path)
    cfg_m = _cfg(depth_root=droot, mask_root=mroot)
    pts, count, _, _ = batch.load_serial_scans(cfg_m, 's1', CAMS, FRAMES, [(0, 4), (0, 5)], RIG)
    ref4 = points_from_depth(np.stack([dA, dB]), RIG, mask=np.stack([mA, np.ones((H, W), np.uint8)]))
    ref5 = points_from_depth(np.stack([dA, dB]), RIG)
    assert count.tolist() == [len(ref4), len(ref5)] and len(ref4) < len(ref5)
    assert np.array_equal(pts[0, :len(ref4)], ref4) and np.array_equal(pts[1, :len(ref5)], ref5)
    # refusals
    with pytest.raises(ValueError, match='scans: serial s9 has no scan file under .*camA.*000000.npy'):
        batch.load_serial_scans(cfg, 's9', CAMS, FRAMES, [(0, None)], RIG)
    _save(batch.scan_path(droot, 's3', '000000', camera='camA'), np.zeros((H, W, 1), np.float32))
    with pytest.raises(ValueError, match='a depth map holds a float array'):
        batch.load_serial_scans(cfg, 's3', CAMS, FRAMES, [(0, None)], RIG)
    _save(batch.scan_path(droot, 's4', '000000', camera='camA'), np.zeros((H, W), np.uint16))
    with pytest.raises(ValueError, match='a depth map holds a float array'):
        batch.load_serial_scans(cfg, 's4', CAMS, FRAMES, [(0, None)], RIG)
    _save(batch.scan_path(droot, 's5', '000000', camera='camA'), dA)
    _save(batch.scan_path(droot, 's5', '000000', camera='camB'), dB[:, :4])
    with pytest.raises(ValueError, match='differ in size'):
        batch.load_serial_scans(cfg, 's5', CAMS, FRAMES, [(0, None)], RIG)


def test_the_readers(tmp_path):
    p = str(tmp_path / 'a.npy')
    np.save(p, np.arange(12, dtype=np.float64).reshape(4, 3))
    pts, w = iof.read_points(p)
    assert pts.dtype == np.float32 and pts.shape == (4, 3) and w is None and pts.flags['C_CONTIGUOUS']
    np.save(p, np.ones((4, 4), np.float16))
    pts, w = iof.read_points(p)
    assert pts.dtype == np.float32 and w.dtype == np.float32 and w.tolist() == [1.0] * 4
    np.save(p, np.ones((3, 5), np.float64))
    assert iof.read_depth(p).dtype == np.float32 and iof.read_depth(p).shape == (3, 5)
