"""GPU: the silhouette term (csrc/silhouette.hip; include/mvfit.h:mvfit_set_silhouettes / mvfit_silhouette_loss) against its
NumPy restatement (tests/silhouette_oracle.py): fields bit for bit and contour lists exactly, winners exactly, loss within
1e-5 relative and gradient within 2e-4 of max |g_ref| elementwise (the project's bounds for the SDF terms), batch
independence bit for bit, the autograd module through BodyLayer, error codes.

Chunk widths of the kernels, all exceeded by the 333 x 517 masks in both dimensions: 256 columns per workgroup in the column
pass, 256 threads striding over a row in the row pass (the whole row in LDS), 64 pixels per ballot and 4 rows per workgroup
in the contour kernels, 256 row segments in the per-image prefix (two rows each at H = 333)."""
import functools

import numpy as np
import pytest
import torch

from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import MvFit, MvFitError, pack_params
from mvsmplfitting_amd.layer import BodyLayer
from mvsmplfitting_amd.silhouette import SilhouetteLoss
from tests import silhouette_oracle as so
from tests.helpers import body_model

pytestmark = pytest.mark.gpu

LOSS_RTOL, GRAD_TOL = 1e-5, 2e-4
H, W = 96, 128
IMAGE_BODY = np.array([0, 2, 0, 2, 2], np.int32)        # image lists of sizes 2, 0 and 3, interleaved


def mask_cases(h, w, seed):
    """[6,h,w]: random speckle, a single on pixel in a corner, a blob with a hole, a mask touching all four borders, an
    empty image, an all-on image."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    r2 = ((yy - h / 2.0) / (0.35 * h + 0.5)) ** 2 + ((xx - w / 2.1) / (0.3 * w + 0.5)) ** 2
    speckle = rng.random((h, w)) < 0.03
    corner = np.zeros((h, w), bool)
    corner[h - 1, 0] = True
    blob = (r2 <= 1.0) & (r2 > 0.08)
    cross = (np.abs(yy - h // 2) <= h // 6) | (np.abs(xx - w // 3) <= w // 7)
    return np.stack([speckle, corner, blob, cross, np.zeros((h, w), bool), np.ones((h, w), bool)]).astype(np.uint8) * 200


def dummy_cams(M):
    return (np.tile(np.eye(3, dtype=np.float32), (M, 1, 1)), np.tile(np.float32([[0, 0, 5]]), (M, 1)),
            np.full(M, 100.0, np.float32), np.zeros((M, 2), np.float32))


@pytest.fixture(scope='module')
def eng():
    with MvFit(body_model()) as e:
        yield e


@pytest.mark.parametrize('stride', [1, 3])
@pytest.mark.parametrize('size', [(2, 2), (37, 53), (333, 517)])
def test_field_bit_for_bit_and_contour_lists_exactly(eng, size, stride):
    masks = mask_cases(size[0], size[1], seed=size[0])
    M = len(masks)
    eng.set_silhouettes(masks, np.zeros(M, np.int32), dummy_cams(M), contour_stride=stride)
    field, first, xy = (t.cpu().numpy() for t in eng.silhouettes())
    want = so.prepare(masks, stride)
    assert np.array_equal(field.view(np.uint32), want['fields'].view(np.uint32)), int((field != want['fields']).sum())
    assert np.array_equal(first, want['first']) and np.array_equal(xy, want['xy'])
    assert not field[4].any() and not field[5].any() and first[4] == first[5] == first[6]
    if size[0] > 2:
        assert first[-1] > 20 and field.max() > 5
    # a second set of the same size reuses the work areas and gives the same answer
    eng.set_silhouettes(torch.from_numpy(masks).to(eng.device), np.zeros(M, np.int32), dummy_cams(M), contour_stride=stride)
    field2, first2, xy2 = eng.silhouettes()
    assert np.array_equal(field2.cpu().numpy(), field) and np.array_equal(xy2.cpu().numpy(), xy)


@functools.lru_cache(maxsize=None)
def world():
    """Three bodies, five images (IMAGE_BODY) at 96 x 128 with masks rendered from displaced copies of the bodies; camera 3
    stands so close that some vertices have pz <= 0.05, camera 4's principal point is shifted so that some project outside
    the image.  The oracle's answers are computed once per setting and shared."""
    model = body_model()
    R, t, f, c = syn.make_camera_ring(5, radius=4.0)
    f = (f * np.float32(W / 2048.0)).astype(np.float32)
    c = np.tile(np.array([W / 2.0, H / 2.0], np.float32), (5, 1))
    fr = syn.make_frames(3, seed0=4100)
    fr['transl'][:] = [[0.0, 0.0, 0.0], [0.3, 0.0, 0.2], [-0.1, 0.05, 0.1]]
    x = pack_params(B=3, **fr)
    c[4] = (W / 2.0 + 40.0, H / 2.0 - 30.0)
    xd = x.copy()
    xd[:, 0:10] += np.random.default_rng(8).normal(0, 0.8, (3, 10)).astype(np.float32)
    xd[:, 82:85] += np.float32([0.04, -0.03, 0.02])
    xd[:, 85] = 1.06
    with MvFit(model) as e:
        e.set_problems((R, t, f, c), np.zeros((3, 5, 17, 2), np.float32), np.zeros((3, 5, 17), np.float32))
        verts = e.vertices(x)[0].cpu().numpy()
        # camera 3 stands beside body 2 at mid height and looks up along it: the legs lie behind its near plane
        cen = verts[2].mean(axis=0).astype(np.float64)
        eye = cen + np.array([0.6, 0.0, 0.0])
        R[3] = syn.look_at_rotation(eye, target=cen + np.array([0.0, 0.6, 0.0]), up=(0.0, 0.0, 1.0))
        t[3] = -R[3].astype(np.float64) @ eye
        f[3] = 60.0
        cams = (R.astype(np.float32), t.astype(np.float32), f, c)
        e.set_problems(cams, np.zeros((3, 5, 17, 2), np.float32), np.zeros((3, 5, 17), np.float32))
        vd, _ = e.vertices(xd)
        _, fid = e.render_overlay(vd, None, np.zeros((5, H, W, 3), np.uint8), IMAGE_BODY, np.arange(5), face_id=True)
        masks = (fid >= 0).to(torch.uint8).cpu().numpy()
    return dict(x=x, verts=verts, masks=masks, cams=cams, prep=so.prepare(masks, 1), ref={})


def reference(w, **kw):
    key = tuple(sorted(kw.items()))
    if key not in w['ref']:
        w['ref'][key] = so.evaluate(w['prep'], w['verts'], IMAGE_BODY, w['cams'], **kw)
    return w['ref'][key]


def test_world_exercises_every_path():
    w = world()
    r = reference(w, w_in=1.0, w_out=1.0, sigma=0.0)
    assert all(m.any() for m in w['masks'][:3]) and len(w['prep']['xy']) > 200
    valid3 = r['cells'][3][0]
    assert 0 < valid3.sum() < len(valid3), 'camera 3 should cut the body with its near plane'
    _, u, v = so._project(w['verts'][2], *(a[4] for a in w['cams']), False)
    assert ((u < 0) | (u > W) | (v < 0) | (v > H)).any(), 'camera 4 should see vertices outside the image'
    assert (reference(w, w_in=1.0, w_out=0.0, sigma=0.0)['loss'][[0, 2]] > 0).all()
    assert (reference(w, w_in=0.0, w_out=1.0, sigma=0.0)['loss'][[0, 2]] > 0).all()


@pytest.mark.parametrize('kw', [dict(w_in=1.0, w_out=1.0, sigma=0.0), dict(w_in=1.0, w_out=1.0, sigma=20.0),
                                dict(w_in=0.0, w_out=1.0, sigma=0.0), dict(w_in=1.0, w_out=0.0, sigma=0.0)],
                         ids=['both', 'sigma20', 'termB', 'termA'])
def test_loss_gradient_and_winners_against_the_oracle(eng, kw):
    w = world()
    ref = reference(w, **kw)
    eng.set_silhouettes(w['masks'], IMAGE_BODY, w['cams'])
    loss, g, win = eng.silhouette_loss(w['verts'], return_winner=True, **kw)
    loss, g, win = loss.cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64), win.cpu().numpy()
    assert np.array_equal(win, ref['winner']), int((win != ref['winner']).sum())
    scale = np.abs(ref['g']).max()
    lerr = np.abs(loss - ref['loss']) / np.maximum(np.abs(ref['loss']), 1e-30)
    gerr = np.abs(g - ref['g']).max() / scale
    print('%s: loss %s rel err %s, grad err / max %.3g (max |g| %.4g)' % (kw, loss, lerr, gerr, scale))
    assert loss[1] == 0 and not g[1].any()              # the image-less body
    assert ref['loss'][0] > 0 and ref['loss'][2] > 0 and scale > 0
    assert (np.abs(loss - ref['loss']) <= LOSS_RTOL * np.abs(ref['loss'])).all()
    assert (np.abs(g - ref['g']) <= GRAD_TOL * scale).all()
    loss_only, none = eng.silhouette_loss(w['verts'], need_grad=False, **kw)
    assert none is None and np.array_equal(loss_only.cpu().numpy().astype(np.float64), loss)


def test_a_body_alone_and_a_second_run_give_the_same_words(eng):
    w = world()
    v = torch.from_numpy(w['verts']).to(eng.device)
    eng.set_silhouettes(w['masks'], IMAGE_BODY, w['cams'])
    loss, g = eng.silhouette_loss(v, sigma=20.0)
    loss_b, g_b = eng.silhouette_loss(v, sigma=20.0)
    assert torch.equal(loss, loss_b) and torch.equal(g, g_b)
    pick = np.flatnonzero(IMAGE_BODY == 2)
    eng.set_silhouettes(w['masks'][pick], np.zeros(len(pick), np.int32), tuple(a[pick] for a in w['cams']))
    loss_1, g_1 = eng.silhouette_loss(v[2:3], sigma=20.0)
    assert torch.equal(loss_1[0], loss[2]) and torch.equal(g_1[0], g[2]) and g_1.abs().max() > 0
    # at another position of a larger batch
    eng.set_silhouettes(w['masks'][pick], np.full(len(pick), 3, np.int32), tuple(a[pick] for a in w['cams']))
    loss_4, g_4 = eng.silhouette_loss(torch.cat([v[:1], v[:1], v[1:2], v[2:3]]), sigma=20.0)
    assert torch.equal(loss_4[3], loss[2]) and torch.equal(g_4[3], g[2]) and not g_4[:3].any() and not loss_4[:3].any()


def test_through_autograd_with_the_body_layer():
    w = world()
    layer = BodyLayer(body_model())
    e, dev = layer.engine, layer.engine.device
    sil = SilhouetteLoss(engine=e, masks=w['masks'], image_body=IMAGE_BODY, cams=w['cams'], sigma=20.0)
    x = torch.from_numpy(w['x']).to(dev)
    leaf = lambda a: a.clone().requires_grad_(True)
    betas, orient, pose, transl = leaf(x[:, 0:10]), leaf(x[:, 10:13]), leaf(x[:, 13:82]), leaf(x[:, 82:85])
    out = layer(betas, orient, pose, transl=transl)
    loss = sil(out.vertices)
    loss.sum().backward()
    l_op, g_op = e.silhouette_loss(out.vertices.detach(), sigma=20.0)
    assert torch.equal(l_op, loss.detach()) and g_op.abs().max() > 0
    gx = e.vertices_backward(x, g_op)
    assert torch.equal(betas.grad, gx[:, 0:10]) and betas.grad.abs().max() > 0
    assert torch.equal(transl.grad, gx[:, 82:85]) and transl.grad.abs().max() > 0
    assert torch.equal(pose.grad, gx[:, 13:82])
    e.close()


def test_errors(eng):
    w = world()
    v = torch.from_numpy(w['verts']).to(eng.device)
    eng.clear_silhouettes()
    with pytest.raises(MvFitError, match='error -3: mvfit_silhouette_loss'):
        eng.silhouette_loss(v)
    with pytest.raises(MvFitError, match='error -1: mvfit_set_silhouettes'):
        eng.set_silhouettes(w['masks'], IMAGE_BODY, w['cams'], contour_stride=0)
    with pytest.raises(MvFitError, match='error -1: mvfit_set_silhouettes'):
        eng.set_silhouettes(np.ones((1, 1, 8), np.uint8), [0], dummy_cams(1))
    eng.set_silhouettes(w['masks'], IMAGE_BODY, w['cams'])
    with pytest.raises(MvFitError, match='error -1: mvfit_silhouette_loss'):
        eng.silhouette_loss(v[:2])                      # image_body holds body 2
    eng.silhouette_loss(v)
    eng.clear_silhouettes()
    with pytest.raises(MvFitError, match='error -3: mvfit_silhouette_loss'):
        eng.silhouette_loss(v)
