"""CPU: the scan loss's float64 oracle (tests/scan_oracle.py) against torch autograd, and the Python layer of the term
(mvsmplfitting_amd/scan.py) on stand-in engines: ScanLoss's argument checks and backward, points_from_depth, refine_to_scan."""
import numpy as np
import pytest
import torch

from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.scan import ScanLoss, points_from_depth, refine_to_scan
from tests import scan_oracle as so
from tests.scan_stub_engine import QuadScanEngine, StubLayer

# two triangles far apart: a right one in the plane z = 0 and a slanted one
VERTS = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 5], [3.2, 0.4, 5.5], [2.3, 1.5, 4.6]], np.float64)
FACES = np.array([[0, 1, 2], [3, 4, 5]], np.int64)
# barycentric coordinates (of b and c) of points whose nearest feature is, in REGIONS order: a, b, ab, c, ac, bc, interior
BARY = np.array([[-0.3, -0.2], [1.4, -0.2], [0.5, -0.3], [-0.2, 1.4], [-0.3, 0.5], [0.8, 0.8], [0.25, 0.25]])


def seven_region_points():
    """14 points: per face one point in each of the seven regions, lifted off the face's plane"""
    pts = []
    for f in FACES:
        a, ab, ac = VERTS[f[0]], VERTS[f[1]] - VERTS[f[0]], VERTS[f[2]] - VERTS[f[0]]
        nrm = np.cross(ab, ac)
        nrm /= np.linalg.norm(nrm)
        pts.append(a + BARY[:, :1] * ab + BARY[:, 1:] * ac + 0.15 * nrm)
    return np.concatenate(pts)


def test_the_points_cover_all_seven_regions_of_both_faces():
    r = so.scan_to_mesh(seven_region_points(), VERTS, FACES)
    assert r['face'].tolist() == [0] * 7 + [1] * 7
    assert r['region'].tolist() == list(range(7)) * 2, r['region']
    assert not r['ambiguous'].any()
    # by hand, face 0: the point over vertex a, and the one over the interior
    p = seven_region_points()
    assert r['m'][0] == pytest.approx(((p[0] - VERTS[0]) ** 2).sum())
    assert r['m'][6] == pytest.approx(0.15 ** 2) and (r['v'][6], r['w'][6]) == pytest.approx((0.25, 0.25))


@pytest.mark.parametrize('sigma', [0.0, 0.4])
@pytest.mark.parametrize('w_s2m,w_m2s', [(1.0, 0.0), (0.0, 1.0), (0.7, 1.3)])
def test_oracle_gradient_is_autograd_in_float64(w_s2m, w_m2s, sigma):
    pts = seven_region_points()
    points = np.stack([pts, pts[::-1] + 0.05])
    points = np.concatenate([points, np.full((2, 2, 3), np.nan)], axis=1)         # two rows beyond count
    count = [14, 13]
    weights = np.random.default_rng(0).uniform(0.5, 2.0, (2, 16))
    weights[1, 3] = 0.0                                                           # takes no part
    points[1, 3] = np.nan
    verts = np.stack([VERTS, VERTS + np.random.default_rng(1).normal(0, 0.05, VERTS.shape)])
    ref = so.evaluate(verts, FACES, points, count, weights, w_s2m=w_s2m, w_m2s=w_m2s, sigma=sigma)
    if w_s2m > 0:
        assert set(zip(ref['nearest_face'][0, :14].tolist(), ref['region'][0, :14].tolist())) == {(f, r) for f in (0, 1) for r in range(7)}
        assert ref['nearest_face'][1, 3] == -1 and (ref['nearest_face'][:, 14:] == -1).all()
    v = torch.tensor(verts, dtype=torch.float64, requires_grad=True)
    loss = so.torch_scan_loss(v, FACES, np.nan_to_num(points), count, weights, w_s2m=w_s2m, w_m2s=w_m2s, sigma=sigma, chunk=5)
    loss.sum().backward()
    assert np.allclose(loss.detach().numpy(), ref['loss'], rtol=1e-12, atol=0)
    assert np.abs(v.grad.numpy() - ref['grad']).max() <= 1e-12 * np.abs(ref['grad']).max()


def test_the_pruned_search_is_the_brute_force_one():
    from tests.small_models import sub_model
    m = sub_model(syn.make_body_model(skin_topk=4), 700)
    verts, faces = np.asarray(m['v_template'], np.float64), np.asarray(m['faces'], np.int64)
    rng = np.random.default_rng(2)
    f = faces[rng.integers(0, len(faces), 300)]
    pts = verts[f].mean(axis=1) + rng.normal(0, 0.03, (300, 3))
    pts[:40] = verts[f[:40, 0]] + rng.normal(0, 1e-9, (40, 3))                    # on shared vertices: many faces tie
    pts[40:60] += rng.normal(0, 0.5, (20, 3))                                      # far away
    a, b = so.scan_to_mesh(pts, verts, faces, prune=True), so.scan_to_mesh(pts, verts, faces, prune=False)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert set(a['region'].tolist()) == set(range(7))


def test_a_body_without_points_contributes_nothing():
    ref = so.evaluate(VERTS[None], FACES, np.full((1, 4, 3), np.nan), [0], None, w_s2m=1.0, w_m2s=1.0)
    assert ref['loss'][0] == 0 and not ref['grad'].any() and (ref['nearest_point'] == -1).all()


# ------------------------------------------------------------------------------------------------------------- ScanLoss
def test_scanloss_argument_errors():
    eng = QuadScanEngine(np.zeros((2, 5, 3)))
    pts = np.zeros((2, 7, 3), np.float32)
    with pytest.raises(ValueError, match='engine='):
        ScanLoss(points=pts)
    with pytest.raises(ValueError, match='points='):
        ScanLoss(engine=eng)
    with pytest.raises(ValueError, match=r'\[N, Pmax, 3\]'):
        ScanLoss(engine=eng, points=np.zeros((2, 7, 2)))
    with pytest.raises(ValueError, match='count'):
        ScanLoss(engine=eng, points=pts, count=[3])
    with pytest.raises(ValueError, match='count'):
        ScanLoss(engine=eng, points=pts, count=[3, 8])
    with pytest.raises(ValueError, match='weights'):
        ScanLoss(engine=eng, points=pts, weights=np.ones((2, 6)))
    for kw in (dict(w_s2m=-1.0), dict(w_m2s=float('nan')), dict(sigma=-0.1)):
        with pytest.raises(ValueError, match='finite'):
            ScanLoss(engine=eng, points=pts, **kw)
    assert eng.calls == []
    mod = ScanLoss(engine=eng, points=pts, count=[7, 0])
    assert eng.calls == ['set']
    with pytest.raises(ValueError, match=r'\[N, Nv, 3\]'):
        mod(torch.zeros(2, 5))
    with pytest.raises(ValueError, match='bodies'):
        mod(torch.zeros(3, 5, 3))
    mod.rebind()
    assert eng.calls == ['set', 'set']


def test_module_backward_scales_the_kept_gradient_per_body():
    rng = np.random.default_rng(3)
    target = rng.normal(size=(2, 5, 3)).astype(np.float32)
    eng = QuadScanEngine(target)
    mod = ScanLoss(engine=eng, points=np.zeros((2, 4, 3), np.float32))
    v = torch.tensor(rng.normal(size=(2, 5, 3)).astype(np.float32), requires_grad=True)
    loss = mod(v)
    assert torch.equal(loss, ((v.detach() - eng.target) ** 2).sum(dim=(1, 2)))
    (loss * torch.tensor([3.0, -0.5])).sum().backward()
    want = torch.tensor([3.0, -0.5])[:, None, None] * (2.0 * (v.detach() - eng.target))
    assert torch.equal(v.grad, want)
    assert eng.calls == ['set', 'loss']
    with pytest.raises(RuntimeError):                                             # once differentiable
        g, = torch.autograd.grad(mod(v).sum(), v, create_graph=True)
        g.sum().backward()


# ---------------------------------------------------------------------------------------------------- points_from_depth
def test_points_from_depth_round_trips_through_the_projection():
    R, t, f, c = syn.make_camera_ring(3, radius=4.0)
    H, W = 24, 40
    f = (f * np.float32(W / 2048.0)).astype(np.float32)
    c = np.tile(np.float32([W / 2.0 - 1.5, H / 2.0 + 2.25]), (3, 1))
    rng = np.random.default_rng(5)
    depth = rng.uniform(2.5, 5.5, (3, H, W)).astype(np.float32)
    depth[0, 3, 4] = 0.0
    depth[1, 5, 6] = -1.0
    depth[2, 7, 8] = np.nan
    depth[2, 9, 10] = np.inf
    pts = points_from_depth(depth, (R, t, f, c))
    assert pts.dtype == np.float32 and pts.shape == (3 * H * W - 4, 3)
    keep = np.isfinite(depth) & (depth > 0)
    first = 0
    for v in range(3):
        ys, xs = np.nonzero(keep[v])
        mine = pts[first:first + len(ys)].astype(np.float64)
        first += len(ys)
        uv = syn.project_points(mine[None], R[v:v + 1], t[v:v + 1], f[v:v + 1], c[v:v + 1])[0, 0]
        z = (mine @ R[v].astype(np.float64).T + t[v].astype(np.float64))[:, 2]
        # the points are rounded to fp32 once: 2^-24 relative on coordinates of size ~|camera distance|, seen through f / z
        tol_px = 4.0 * 2.0 ** -24 * 8.0 * float(f[v]) / 2.5
        assert np.abs(uv[:, 0] - (xs + 0.5)).max() <= tol_px and np.abs(uv[:, 1] - (ys + 0.5)).max() <= tol_px
        assert np.abs(z - depth[v, ys, xs]).max() <= 4.0 * 2.0 ** -24 * 8.0
    # mask, stride and max_points
    mask = np.zeros((3, H, W), np.uint8)
    mask[1, 4:12, 8:20] = 7
    sub = points_from_depth(torch.from_numpy(depth), (R, t, f, c), mask=mask, stride=2)
    assert len(sub) == 4 * 6 - 0 and np.array_equal(sub[0], pts[np.flatnonzero(keep[0].ravel()).size + 4 * W + 8 - 0])
    few = points_from_depth(depth, (R, t, f, c), max_points=100)
    assert few.shape == (100, 3) and np.array_equal(few[0], pts[0])
    with pytest.raises(ValueError, match='stride'):
        points_from_depth(depth, (R, t, f, c), stride=0)
    with pytest.raises(ValueError, match='mask'):
        points_from_depth(depth, (R, t, f, c), mask=mask[:, :5])


# ------------------------------------------------------------------------------------------------------- refine_to_scan
def stub_world():
    rng = np.random.default_rng(11)
    template = rng.normal(size=(6, 3)).astype(np.float32)
    x_true = np.zeros((3, 118), np.float32)
    x_true[:, 85] = [1.1, 0.9, 1.0]
    x_true[:, 82:85] = rng.normal(0, 0.1, (3, 3))
    target = x_true[:, 85, None, None] * template[None] + x_true[:, None, 82:85]
    eng = QuadScanEngine(target)
    return eng, StubLayer(eng, template), x_true


def test_refine_to_scan_keeps_what_fell_and_reverts_the_rest_exactly():
    eng, layer, x_true = stub_world()
    x0 = x_true.copy()
    x0[:2, 85] += [0.2, -0.15]
    x0[:2, 82:85] += 0.05
    # body 2 starts at its optimum: nothing can fall, its row must come back bit for bit
    out, rep = refine_to_scan(layer, x0, np.zeros((3, 4, 3), np.float32), free=('scale', 'transl'), weight=1.0, sigma=0.0,
                              shape_weight=0.0, max_iter=30)
    assert rep['accepted'] == [True, True, False]
    assert all(a < b for a, b in zip(rep['after'][:2], rep['before'][:2]))
    assert torch.equal(out[2], torch.from_numpy(x0[2]))
    assert np.abs(out[:2, 85].numpy() - x_true[:2, 85]).max() < 1e-3
    assert torch.equal(out[:, :82], torch.from_numpy(x0[:, :82]))                # the blocks that are not free
    assert eng.calls[0] == 'set' and eng.calls[-1] == 'clear' and eng.scans is None
    assert rep['iterations'] > 0 and len(rep['scan_before']) == 3


def test_refine_to_scan_argument_errors_and_cleanup():
    eng, layer, x_true = stub_world()
    with pytest.raises(ValueError, match='free block'):
        refine_to_scan(layer, x_true, np.zeros((3, 4, 3), np.float32), free=('pose_embedding',), weight=1.0, sigma=0.0, shape_weight=0.0)
    with pytest.raises(ValueError, match='118'):
        refine_to_scan(layer, x_true[:, :100], np.zeros((3, 4, 3), np.float32), weight=1.0, sigma=0.0, shape_weight=0.0)

    def boom(*a, **k):
        raise RuntimeError('boom')
    eng.scan_loss = boom
    with pytest.raises(RuntimeError, match='boom'):
        refine_to_scan(layer, x_true, np.zeros((3, 4, 3), np.float32), weight=1.0, sigma=0.0, shape_weight=0.0)
    assert eng.calls[-1] == 'clear'
