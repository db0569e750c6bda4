"""CPU: the silhouette term's NumPy restatement (tests/silhouette_oracle.py) against its own definition - field, contour
rules, analytic gradient against central differences - and the plumbing of SilhouetteLoss / refine_shape against stand-in
engines (tests/silhouette_stub_engine.py)."""
import numpy as np
import pytest
import torch

from mvsmplfitting_amd.silhouette import SilhouetteLoss, keypoint_term, refine_shape
from tests import silhouette_oracle as so
from tests.silhouette_stub_engine import QuadEngine, StubLayer


def look_at(eye, target=(0.0, 0.0, 0.0)):
    """World -> camera (R, t) of a camera at eye looking at target, y down."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross([0.0, -1.0, 0.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return R.astype(np.float32), (-R @ eye).astype(np.float32)


def blob_world(seed=5, nv=48, H=40, W=52):
    """Two random blob "bodies", three images (bodies 0, 1, 0); the masks are discs around the projections of displaced
    copies, one inflated and two shrunk, so vertices lie outside the masks (term A) and contour points away from the
    vertices (term B)."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(2, nv, 3))
    V = 0.35 * d / np.linalg.norm(d, axis=2, keepdims=True) * rng.uniform(0.6, 1.0, (2, nv, 1))
    eyes = [(0.2, -0.1, -3.0), (2.4, 0.3, -1.8), (-2.0, -0.4, -2.2)]
    Rt = [look_at(e) for e in eyes]
    cams = (np.stack([r for r, _ in Rt]), np.stack([t for _, t in Rt]), np.full(3, 55.0, np.float32),
            np.tile(np.array([[W / 2.0, H / 2.0]], np.float32), (3, 1)))
    image_body = np.array([0, 1, 0], np.int32)
    masks = np.zeros((3, H, W), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for i in range(3):
        src = (1.25, 0.7, 0.75)[i] * V[image_body[i]] + np.array([0.07, -0.05, 0.03])
        _, u, w = so._project(src, cams[0][i], cams[1][i], cams[2][i], cams[3][i], True)
        for a, b in zip(u, w):
            masks[i][(xx + 0.5 - a) ** 2 + (yy + 0.5 - b) ** 2 <= 2.2 ** 2] = 1
    return V, masks, image_body, cams


def test_scipy_field_is_the_bruteforce_integer_minimum_bit_for_bit():
    rng = np.random.default_rng(0)
    mask = (rng.random((37, 53)) < 0.02).astype(np.uint8)
    assert mask.any()
    assert np.array_equal(so.field(mask).view(np.uint32), so.field_bruteforce(mask).view(np.uint32))
    assert not so.field(np.zeros((5, 7), np.uint8)).any()                 # no on pixel: zeros, not scipy's answer
    assert not so.field(np.ones((5, 7), np.uint8)).any()


@pytest.mark.parametrize('sigma', [0.0, 5.0])
def test_analytic_gradient_against_central_differences(sigma):
    """Pure float64 mode.  A coordinate is left out only when a bilinear cell or a contour point's winner differs between
    its two probe points (at most 2 % of them); the rest agrees to 1e-6 of the largest gradient entry."""
    V, masks, image_body, cams = blob_world()
    prep = so.prepare(masks, 2)
    kw = dict(w_in=0.7, w_out=1.3, sigma=sigma, pure64=True)
    r = so.evaluate(prep, V, image_body, cams, **kw)
    assert r['loss'].min() > 0 and (r['winner'] >= 0).all() and len(r['winner']) > 20
    for valid, x0, _ in r['cells']:                                       # both terms are active and nothing is clamped
        assert valid.all() and x0.min() >= 0
    # term A is active: some vertex lies outside its mask
    assert so.evaluate(prep, V, image_body, cams, w_in=1.0, w_out=0.0, sigma=sigma, pure64=True)['loss'].min() > 0
    h = 1e-5
    scale = np.abs(r['g']).max()
    skipped, worst, total = 0, 0.0, 0

    def state(e):
        return np.concatenate([e['winner']] + [np.concatenate([c[1], c[2]]) for c in e['cells']])
    for n in range(V.shape[0]):
        for j in range(V.shape[1]):
            for c in range(3):
                Vp, Vm = V.copy(), V.copy()
                Vp[n, j, c] += h
                Vm[n, j, c] -= h
                ep, em = so.evaluate(prep, Vp, image_body, cams, **kw), so.evaluate(prep, Vm, image_body, cams, **kw)
                total += 1
                if not np.array_equal(state(ep), state(em)):
                    skipped += 1
                    continue
                fd = (ep['loss'].sum() - em['loss'].sum()) / (2 * h)
                worst = max(worst, abs(fd - r['g'][n, j, c]))
    print('sigma %g: %d of %d coordinates left out, worst |fd - g| / max|g| = %.3g' % (sigma, skipped, total, worst / scale))
    assert skipped <= 0.02 * total
    assert worst <= 1e-6 * scale


def test_contour_rules():
    m = np.zeros((6, 7), np.uint8)
    m[0:4, 0:5] = 1                                    # touches the top and left borders
    c = so.contour(m)
    # the border does not make a contour: only the pixels next to an off pixel inside the image, in raster order
    assert c.tolist() == [[4, 0], [4, 1], [4, 2], [0, 3], [1, 3], [2, 3], [3, 3], [4, 3]]
    assert so.contour(m, 3).tolist() == [[4, 0], [0, 3], [3, 3]]           # the k-th point is kept iff k % 3 == 0
    full = np.ones((4, 5), np.uint8)
    assert len(so.contour(full)) == 0 and len(so.contour(np.zeros((4, 5), np.uint8))) == 0
    hole = np.ones((5, 5), np.uint8)
    hole[2, 2] = 0
    assert so.contour(hole).tolist() == [[2, 1], [1, 2], [3, 2], [2, 3]]
    prep = so.prepare(np.stack([np.zeros((5, 5), np.uint8), hole, np.ones((5, 5), np.uint8)]), 2)
    assert prep['first'].tolist() == [0, 0, 2, 2] and prep['xy'].tolist() == [[2, 1], [3, 2]]
    assert prep['nonempty'].tolist() == [False, True, True] and not prep['fields'][0].any() and not prep['fields'][2].any()


def test_empty_and_all_on_images_and_imageless_bodies_contribute_nothing():
    V, masks, image_body, cams = blob_world()
    masks = masks.copy()
    masks[1] = 0                                       # body 1's only image is empty
    masks[2] = 1                                       # all on: field 0, no contour
    r = so.evaluate(so.prepare(masks), V.astype(np.float32), image_body, cams)
    r0 = so.evaluate(so.prepare(masks[:1]), V.astype(np.float32), image_body[:1], tuple(a[:1] for a in cams))
    assert r['loss'][1] == 0 and not r['g'][1].any()
    assert r['loss'][0] == r0['loss'][0] and np.array_equal(r['g'][0], r0['g'][0])


def test_module_backward_scales_the_kept_gradient_per_body():
    V, masks, image_body, cams = blob_world()
    eng = so.OracleEngine()
    sil = SilhouetteLoss(engine=eng, masks=masks, image_body=image_body, cams=cams, contour_stride=2, sigma=4.0)
    v = torch.tensor(V, dtype=torch.float32, requires_grad=True)
    loss = sil(v)
    assert loss.shape == (2,) and eng.calls == ['set', 'loss']
    (loss * torch.tensor([2.0, -3.0])).sum().backward()
    _, g = eng.silhouette_loss(v.detach(), sigma=4.0)
    assert g.abs().max() > 0
    assert torch.equal(v.grad[0], 2.0 * g[0]) and torch.equal(v.grad[1], -3.0 * g[1])
    with pytest.raises(ValueError):
        SilhouetteLoss(engine=eng, masks=masks)


def _stub_problem():
    """Four problems in groups [0, 0, 1, 1].  Group 0 starts away from its target (scale 1 -> 1.2 lowers its loss); the rows
    of group 1 differ from one another and each sits exactly on its own target, so any shared shape is worse."""
    rng = np.random.default_rng(1)
    T = rng.normal(size=(4, 3)).astype(np.float32)
    x = np.zeros((4, 118), np.float32)
    x[:, 85] = 1.0
    x[2, 0:3], x[3, 0:3] = [0.3, -0.2, 0.1], [-0.4, 0.5, 0.2]
    x[2, 85], x[3, 85] = 0.9, 1.1
    x[:, 82:85] = rng.normal(size=(4, 3))
    target = np.stack([x[b, 85] * T + x[b, 0:3] + x[b, 82:85] for b in range(4)])
    target[0] = 1.2 * T + np.float32([0.1, 0.0, -0.1]) + x[0, 82:85]
    target[1] = 1.2 * T + np.float32([0.1, 0.0, -0.1]) + x[1, 82:85]
    eng = QuadEngine(target)
    return StubLayer(eng, T), eng, torch.tensor(x)


def test_refine_shape_shares_one_shape_per_group_and_reverts_a_rejected_group_exactly():
    layer, eng, x = _stub_problem()
    masks = np.ones((4, 4, 4), np.uint8)
    out, rep = refine_shape(layer, x, masks, np.arange(4), (None,) * 4, share=[7, 7, 9, 9], weight=2.0, sigma=0.0, shape_weight=0.1,
                            max_iter=40)
    assert rep['groups'] == [7, 9] and rep['accepted'] == [True, False] and rep['iterations'] > 0
    assert rep['after'][0] < rep['before'][0] and rep['silhouette_after'][0] < rep['silhouette_before'][0]
    assert rep['after'][1] >= rep['before'][1]
    # group 7: one betas and one scale for both rows, moved towards the target; nothing else moved
    assert torch.equal(out[0, 0:10], out[1, 0:10]) and torch.equal(out[0, 85], out[1, 85])
    assert abs(float(out[0, 85]) - 1.2) < 0.02 and abs(float(out[0, 0]) - 0.1) < 0.02
    assert torch.equal(out[:, 10:85], x[:, 10:85]) and torch.equal(out[:, 86:], x[:, 86:])
    # group 9: rejected, its differing rows come back bit for bit
    assert torch.equal(out[2:], x[2:])
    assert eng.calls[0] == 'set' and eng.calls[-1] == 'clear' and eng.masks is None
    # the objective: weight * sum of the group's losses + shape_weight^2 |betas|^2, once per group
    assert rep['before'][1] == pytest.approx(0.01 * float((x[2, 0:10] ** 2).sum()), rel=1e-5, abs=1e-9)


def test_refine_shape_without_sharing_and_with_a_per_problem_block_and_keypoints():
    layer, eng, x = _stub_problem()
    x = x[:2].clone()
    eng.target = eng.target[:2] + torch.tensor([[0.3, 0.0, 0.0]])          # a shift only transl can follow
    cams_fit = (np.eye(3, dtype=np.float32)[None], np.array([[0.0, 0.0, 6.0]], np.float32), np.array([50.0], np.float32),
                np.array([[20.0, 20.0]], np.float32))
    gt = np.full((2, 1, 17, 2), 20.0, np.float32)
    kp = (cams_fit, gt, np.ones((2, 1, 17), np.float32), 0.05, 100.0)
    out, rep = refine_shape(layer, x, np.ones((2, 4, 4), np.uint8), [0, 1], (None,) * 4, free=('scale', 'transl'), weight=1.0,
                            sigma=0.0, shape_weight=0.0, keypoints=kp)
    assert rep['groups'] == [0, 1] and rep['accepted'] == [True, True]
    assert torch.equal(out[:, 0:10], x[:, 0:10]) and not torch.equal(out[:, 82:85], x[:, 82:85])
    with torch.no_grad():
        o = layer(x[:, 0:10], None, None, transl=x[:, 82:85], scale=x[:, 85:86])
        k = keypoint_term(o.joints, *kp)
    r = o.vertices - eng.target
    assert rep['before'] == pytest.approx(((r * r).sum(dim=(1, 2)) + k).tolist(), rel=1e-5)
    assert k.min() > 0
    with pytest.raises(ValueError):
        refine_shape(layer, x, np.ones((2, 4, 4), np.uint8), [0, 1], (None,) * 4, free=('pose_embedding',), weight=1.0, sigma=0.0,
                     shape_weight=0.0)
