"""GPU: scan.refine_to_scan on the real engine - bodies with known betas and scale, scans sampled from the float64 oracle's
vertices of those bodies, a start with both perturbed.  The objective must fall for every accepted body, every body must be
accepted here, and the mean point-to-surface distance (float64, tests/scan_oracle.py) must end below half of where it began."""
import numpy as np
import pytest
import torch

from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import pack_params
from mvsmplfitting_amd.layer import BodyLayer
from mvsmplfitting_amd.scan import refine_to_scan
from tests import scan_oracle as so
from tests.helpers import oracle_for
from tests.small_models import sub_model

pytestmark = pytest.mark.gpu


def mean_distance(orc, x, faces, points):
    out = []
    for b in range(len(x)):
        p = dict(betas=x[b, 0:10], global_orient=x[b, 10:13], body_pose=x[b, 13:82], transl=x[b, 82:85], scale=x[b, 85])
        v = orc.body(p, want_cache=False)['vertices']
        out.append(np.sqrt(so.scan_to_mesh(points[b].astype(np.float64), v, faces)['m']).mean())
    return np.array(out)


def test_refine_to_scan_recovers_shape_and_scale():
    model = sub_model(syn.make_body_model(skin_topk=4), 1001)
    faces = np.asarray(model['faces'], np.int64)
    orc = oracle_for(model, None, None)
    B, P = 2, 600
    x_true = pack_params(B=B, **syn.make_frames(B, seed0=6200))
    x_true[:, 85] = [1.05, 0.93]
    rng = np.random.default_rng(9)
    points = np.zeros((B, P, 3), np.float32)
    for b in range(B):
        p = dict(betas=x_true[b, 0:10], global_orient=x_true[b, 10:13], body_pose=x_true[b, 13:82], transl=x_true[b, 82:85],
                 scale=x_true[b, 85])
        v = orc.body(p, want_cache=False)['vertices']
        f = faces[rng.integers(0, len(faces), P)]
        u = rng.random((P, 2))
        flip = u.sum(axis=1) > 1
        u[flip] = 1.0 - u[flip]
        points[b] = v[f[:, 0]] + u[:, :1] * (v[f[:, 1]] - v[f[:, 0]]) + u[:, 1:] * (v[f[:, 2]] - v[f[:, 0]]) + rng.normal(0, 0.001, (P, 3))
    x0 = x_true.copy()
    x0[:, 0:10] += rng.normal(0, 0.6, (B, 10)).astype(np.float32)
    x0[:, 85] *= [0.93, 1.08]
    layer = BodyLayer(model)
    out, rep = refine_to_scan(layer, x0, points, free=('betas', 'scale', 'transl'), weight=1.0, sigma=0.0, shape_weight=0.01,
                              max_iter=40)
    out = out.cpu().numpy()
    d0, d1 = mean_distance(orc, x0, faces, points), mean_distance(orc, out, faces, points)
    print('objective', rep['before'], '->', rep['after'], 'accepted', rep['accepted'], 'iterations', rep['iterations'])
    print('mean distance', d0, '->', d1, 'scale', out[:, 85], 'true', x_true[:, 85])
    assert all(rep['accepted'])
    assert all(a < b for a, b, ok in zip(rep['after'], rep['before'], rep['accepted']) if ok)
    assert (d1 < 0.5 * d0).all()
    assert np.array_equal(out[:, 10:82], x0[:, 10:82])                            # the pose was not free
    assert np.abs(out[:, 85] - x_true[:, 85]).max() < 0.5 * np.abs(x0[:, 85] - x_true[:, 85]).min()
    with pytest.raises(Exception, match='no scan set'):                           # the driver leaves the engine without scans
        layer.engine.scan_loss(torch.zeros(B, 1001, 3))
