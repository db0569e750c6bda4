"""GPU: silhouette.refine_shape on BodyLayer - one synthetic person in 3 frames x 4 views whose masks (192 x 256, rendered
from the truth: betas up to |3|, scale 1.08) pull betas and scale, shared over the frames, from (0, 1) towards the truth.
The sizes of the improvements are not fixed in advance (DESIGN section 7 records the measured ones); their direction is."""
import functools

import numpy as np
import pytest
import torch

from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import pack_params
from mvsmplfitting_amd.layer import BodyLayer
from mvsmplfitting_amd.silhouette import refine_shape
from tests.helpers import body_model

pytestmark = pytest.mark.gpu

H, W, FRAMES, VIEWS = 192, 256, 3, 4
BETAS = np.array([3.0, -2.0, 1.5, -1.0, 2.5, 0.5, -3.0, 1.0, -0.5, 2.0], np.float32)
SCALE = 1.08
IMAGE_BODY = np.repeat(np.arange(FRAMES), VIEWS).astype(np.int32)
IMAGE_VIEW = np.tile(np.arange(VIEWS), FRAMES).astype(np.int32)


@functools.lru_cache(maxsize=None)
def truth():
    R, t, f, c = syn.make_camera_ring(VIEWS, radius=4.0)
    f = (f * np.float32(W / 2048.0)).astype(np.float32)
    c = np.tile(np.array([W / 2.0, H / 2.0], np.float32), (VIEWS, 1))
    fr = syn.make_frames(FRAMES, seed0=5200, betas=BETAS)
    fr['scale'][:] = SCALE
    return (R, t, f, c), pack_params(B=FRAMES, **fr)


def render_masks(eng, cams, x):
    eng.set_problems(cams, np.zeros((FRAMES, VIEWS, 17, 2), np.float32), np.zeros((FRAMES, VIEWS, 17), np.float32))
    v, _ = eng.vertices(x)
    _, fid = eng.render_overlay(v, None, np.zeros((FRAMES * VIEWS, H, W, 3), np.uint8), IMAGE_BODY, IMAGE_VIEW, face_id=True)
    return fid >= 0


def iou(a, b):
    return ((a & b).sum(dim=(1, 2)).double() / (a | b).sum(dim=(1, 2)).double()).cpu().numpy()


def test_masks_pull_shared_betas_and_scale_towards_the_truth():
    cams, x_true = truth()
    layer = BodyLayer(body_model())
    eng = layer.engine
    masks = render_masks(eng, cams, x_true)
    assert masks.flatten(1).any(dim=1).all()
    x0 = x_true.copy()
    x0[:, 0:10] = 0.0
    x0[:, 85] = 1.0
    per_image = tuple(a[IMAGE_VIEW] for a in cams)
    out, rep = refine_shape(layer, x0, masks.to(torch.uint8), IMAGE_BODY, per_image, free=('betas', 'scale'), share=[0, 0, 0],
                            weight=1e-3, sigma=0.0, shape_weight=0.1, max_iter=30)
    iou0, iou1 = iou(render_masks(eng, cams, x0), masks), iou(render_masks(eng, cams, out), masks)
    s1 = float(out[0, 85])
    print('objective %.6g -> %.6g, silhouette loss %.6g -> %.6g, %d iterations' %
          (rep['before'][0], rep['after'][0], rep['silhouette_before'][0], rep['silhouette_after'][0], rep['iterations']))
    print('IoU per image before %s' % np.round(iou0, 4))
    print('IoU per image after  %s' % np.round(iou1, 4))
    print('scale 1 -> %.5f (truth %.2f); betas -> %s' % (s1, SCALE, np.round(out[0, 0:10].cpu().numpy(), 3)))
    assert rep['accepted'] == [True]
    assert rep['silhouette_after'][0] < rep['silhouette_before'][0]
    assert (iou1 > iou0).all()
    assert abs(s1 - SCALE) < abs(1.0 - SCALE)
    assert torch.equal(out[0, 0:10], out[1, 0:10]) and torch.equal(out[0, 0:10], out[2, 0:10])
    assert torch.equal(out[0, 85], out[1, 85]) and torch.equal(out[0, 85], out[2, 85])
    x0t = torch.from_numpy(x0).to(out.device)
    assert torch.equal(out[:, 10:85], x0t[:, 10:85]) and torch.equal(out[:, 86:], x0t[:, 86:])
    eng.close()


def test_a_mask_set_that_already_matches_is_not_made_worse():
    cams, x_true = truth()
    layer = BodyLayer(body_model())
    eng = layer.engine
    masks = render_masks(eng, cams, x_true)
    per_image = tuple(a[IMAGE_VIEW] for a in cams)
    out, rep = refine_shape(layer, x_true, masks.to(torch.uint8), IMAGE_BODY, per_image, free=('betas', 'scale'),
                            share=[0, 0, 0], weight=1e-3, sigma=0.0, shape_weight=0.1, max_iter=10)
    print('objective %.6g -> %.6g, accepted %s' % (rep['before'][0], rep['after'][0], rep['accepted']))
    if rep['accepted'][0]:
        assert rep['after'][0] <= rep['before'][0]
    else:
        assert torch.equal(out, torch.from_numpy(x_true).to(out.device))
    eng.close()
