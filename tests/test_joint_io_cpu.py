"""CPU: the argument checks of fit_folder(joint=...) - every ValueError is raised before any engine is created (engine=None
and no GPU here) and before any file is read - and the mask loading both silhouette paths share."""
import os

import numpy as np
import pytest

from mvsmplfitting_amd import batch
from mvsmplfitting_amd import io_formats as iof
from tests.helpers import body_model


def _parts(tmp_path, **over):
    parts = dict(scene_collision=dict(share=0.5), silhouettes=dict(share=2.0, mask_root=str(tmp_path)), temporal=dict(share=0.25))
    parts.update(over)
    return {k: v for k, v in parts.items() if v is not None}


def test_fit_folder_joint_argument_errors(tmp_path):
    model = body_model()
    run = lambda **kw: batch.fit_folder(model, str(tmp_path / 'none'), str(tmp_path / 'none.txt'), str(tmp_path / 'out'), **kw)
    sil_t = _parts(tmp_path, scene_collision=None)
    with pytest.raises(ValueError, match="joint: a dict with at least 'weight'"):
        run(joint=True)
    with pytest.raises(ValueError, match="joint: a dict with at least 'weight'"):
        run(joint=dict(sweeps=2, **sil_t))
    with pytest.raises(ValueError, match='joint: unknown keys .*wieght'):
        run(joint=dict(weight=1.0, wieght=2.0, **sil_t))
    for bad in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError, match='joint: weight must be > 0'):
            run(joint=dict(weight=bad, **sil_t))
    with pytest.raises(ValueError, match='joint: sweeps must be >= 1'):
        run(joint=dict(weight=1.0, sweeps=0, **sil_t))
    # at least two parts
    with pytest.raises(ValueError, match='joint: at least two of'):
        run(joint=dict(weight=1.0))
    with pytest.raises(ValueError, match='joint: at least two of'):
        run(joint=dict(weight=1.0, temporal=dict(share=1.0)))
    with pytest.raises(ValueError, match='joint: at least two of'):
        run(joint=dict(weight=1.0, temporal=dict(share=1.0), silhouettes=None))
    # together with a single option
    with pytest.raises(ValueError, match='joint and temporal'):
        run(joint=dict(weight=1.0, **sil_t), temporal=dict(weight=1.0))
    with pytest.raises(ValueError, match='joint and silhouettes'):
        run(joint=dict(weight=1.0, **sil_t), silhouettes=dict(mask_root=str(tmp_path), weight=1.0))
    with pytest.raises(ValueError, match='joint and scene_collision'):
        run(joint=dict(weight=1.0, **sil_t), scene_collision=dict(weight=1.0), persons='all')
    with pytest.raises(ValueError, match='joint is not available with is_seq=True'):
        run(joint=dict(weight=1.0, **sil_t), is_seq=True)
    # the scene part needs the multi-person path
    with pytest.raises(ValueError, match='joint: scene_collision refines the persons of a frame together'):
        run(joint=dict(weight=1.0, **_parts(tmp_path)))
    with pytest.raises(ValueError, match='joint: scene_collision refines the persons of a frame together'):
        run(joint=dict(weight=1.0, **_parts(tmp_path, silhouettes=None)), persons=0)
    # the parts
    with pytest.raises(ValueError, match="joint: temporal: a dict with at least 'share'"):
        run(joint=dict(weight=1.0, **_parts(tmp_path, scene_collision=None, temporal=dict())))
    with pytest.raises(ValueError, match="joint: temporal: a dict with at least 'share'"):
        run(joint=dict(weight=1.0, **_parts(tmp_path, scene_collision=None, temporal=True)))
    with pytest.raises(ValueError, match="joint: silhouettes: a dict with at least 'share' and 'mask_root'"):
        run(joint=dict(weight=1.0, **_parts(tmp_path, scene_collision=None, silhouettes=dict(share=1.0))))
    with pytest.raises(ValueError, match='joint: temporal: unknown keys .*weight'):
        run(joint=dict(weight=1.0, **_parts(tmp_path, scene_collision=None, temporal=dict(share=1.0, weight=2.0))))
    with pytest.raises(ValueError, match='joint: silhouettes: unknown keys .*w_inn'):
        run(joint=dict(weight=1.0, **_parts(tmp_path, scene_collision=None, silhouettes=dict(share=1.0, mask_root='m', w_inn=1.0))))
    with pytest.raises(ValueError, match='joint: scene_collision: unknown keys .*sweeps'):
        run(joint=dict(weight=1.0, **_parts(tmp_path, scene_collision=dict(share=1.0, sweeps=2))), persons='all')
    for part in ('scene_collision', 'silhouettes', 'temporal'):
        for bad in (0.0, -2.0, float('nan'), float('inf')):
            p = _parts(tmp_path)
            p[part] = dict(p[part], share=bad)
            with pytest.raises(ValueError, match='joint: %s: share must be > 0' % part):
                run(joint=dict(weight=1.0, **p), persons='all')
    for bad in (dict(grid_size=1), dict(robustifier=0.0), dict(scale_factor=-0.2)):
        with pytest.raises(ValueError, match='joint: scene_collision: grid_size must be >= 2'):
            run(joint=dict(weight=1.0, **_parts(tmp_path, scene_collision=dict(share=1.0, **bad))), persons='all')
    for bad in (dict(downscale=0), dict(contour_stride=0)):
        with pytest.raises(ValueError, match='joint: silhouettes: downscale and contour_stride must be >= 1'):
            run(joint=dict(weight=1.0, **_parts(tmp_path, silhouettes=dict(share=1.0, mask_root='m', **bad))), persons='all')


def test_check_joint_fills_the_defaults(tmp_path):
    cfg = batch.check_joint(dict(weight=2.0, **_parts(tmp_path)), multi=True)
    assert cfg['weight'] == 2.0 and cfg['sweeps'] == 3
    assert cfg['scene_collision'] == dict(share=0.5, grid_size=32, robustifier=0.05, scale_factor=0.2)
    assert cfg['temporal'] == dict(share=0.25)
    assert cfg['silhouettes'] == dict(share=2.0, mask_root=str(tmp_path), w_in=1.0, w_out=1.0, sigma=0.0, contour_stride=1,
                                      downscale=1, max_mask_bytes=2 ** 31)
    cfg = batch.check_joint(dict(weight=1.0, sweeps=5, **_parts(tmp_path, scene_collision=None)))
    assert cfg['sweeps'] == 5 and 'scene_collision' not in cfg
    # the existing options' own mutual exclusions are what they were
    with pytest.raises(ValueError, match='temporal and silhouettes'):
        batch.check_temporal(dict(weight=1.0), None, dict(mask_root='m', weight=1.0))
    with pytest.raises(ValueError, match='silhouettes and scene_collision'):
        batch.check_silhouettes(dict(mask_root='m', weight=1.0), False, dict(weight=1.0))


def test_load_serial_masks(tmp_path):
    """Two frames, two cameras, three mask files: the images, their bodies and their per-image cameras at downscale 2."""
    frames = [('000000',), ('000001',)]
    cams = ['camA', 'camB']
    m = np.zeros((8, 12), np.uint8)
    m[2:6, 3:9] = 255
    for cam, frame in (('camA', '000000'), ('camB', '000000'), ('camB', '000001')):
        path = batch.mask_path(str(tmp_path), 's1', cam, frame)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        from PIL import Image
        Image.fromarray(m).save(path)
    rig = (np.stack([np.eye(3)] * 2).astype(np.float32), np.zeros((2, 3), np.float32), np.array([100.0, 200.0], np.float32),
           np.array([[6.0, 4.0], [8.0, 2.0]], np.float32))
    cfg = dict(batch.SILHOUETTE_DEFAULTS, mask_root=str(tmp_path), downscale=2)
    masks, body, per_image, found = batch.load_serial_masks(cfg, 's1', cams, frames, [(0, None), (1, None)], rig, 6890)
    assert masks.shape == (3, 4, 6) and masks.dtype == np.uint8
    assert np.array_equal(masks[0], iof.downscale_mask(iof.read_mask(found[0][2]), 2))
    assert body.tolist() == [0, 0, 1] and [(n, v) for n, v, _ in found] == [(0, 0), (0, 1), (1, 1)]
    assert per_image[2].tolist() == [50.0, 100.0, 100.0] and per_image[3].tolist() == [[3.0, 2.0], [4.0, 1.0], [4.0, 1.0]]
    with pytest.raises(ValueError, match='silhouettes: serial s2 has no mask file'):
        batch.load_serial_masks(cfg, 's2', cams, frames, [(0, None)], rig, 6890)
    with pytest.raises(ValueError, match='the smallest downscale that fits is'):
        batch.load_serial_masks(dict(cfg, max_mask_bytes=1000), 's1', cams, frames, [(0, None), (1, None)], rig, 6890)
