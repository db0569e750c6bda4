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


# ------------------------------------------------------------------- what tests/test_gpu_scan_edges.py builds its cases from
def template_mesh(nv):
    from tests.small_models import sub_model
    m = sub_model(syn.make_body_model(skin_topk=4), nv)
    return np.asarray(m['v_template'], np.float32).astype(np.float64), np.asarray(m['faces'], np.int64)


def samples(verts, faces, P, noise, seed):
    rng = np.random.default_rng(seed)
    f = faces[rng.integers(0, len(faces), P)]
    u = rng.random((P, 2))
    u[u.sum(axis=1) > 1] = 1.0 - u[u.sum(axis=1) > 1]
    a, b, c = verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]]
    return a + u[:, :1] * (b - a) + u[:, 1:] * (c - a) + rng.normal(0, noise, (P, 3))


def test_the_repeated_face_list_is_the_same_surface_and_not_ambiguous():
    verts, faces = template_mesh(1001)
    many = so.repeated_faces(faces, 13)
    assert many.shape == (13 * 1399, 3) and -(-len(many) // 8) > 2048
    nf = len(faces)
    for k in range(13):                                    # copy k: rotated by k mod 3, the odd copies in reverse order
        block = many[k * nf:(k + 1) * nf]
        block = block[::-1] if k % 2 else block
        assert np.array_equal(np.roll(block, k % 3, axis=1), faces)
    pts = samples(verts, faces, 321, 0.03, 5)
    one, all13 = so.scan_to_mesh(pts, verts, faces), so.scan_to_mesh(pts, verts, many)
    assert all13['ambiguous'].mean() <= 0.01 and one['ambiguous'].mean() <= 0.01
    assert np.abs(all13['m'] - one['m']).max() <= 1e-12 * one['m'].max()
    assert np.abs(all13['d'] - one['d']).max() <= 1e-9      # the copies share the closest point
    k, pos = np.divmod(all13['face'], nf)
    base = np.where(k % 2 == 1, nf - 1 - pos, pos)
    assert (np.sort(faces[base], axis=1) == np.sort(many[all13['face']], axis=1)).all()


def test_the_lowest_face_with_m_zero_is_the_lowest_face_at_the_vertex():
    verts, faces = template_mesh(700)
    assert len(np.unique(verts, axis=0)) == len(verts)     # distinct positions: only a vertex's own faces reach m = 0
    got = so.lowest_zero_face(verts, verts, faces)
    want = np.full(len(verts), -1)
    for f in range(len(faces) - 1, -1, -1):
        want[faces[f]] = f
    assert (want == -1).sum() == 88 and np.array_equal(got, want)
    # brute force over every pair agrees
    m = so.closest(verts[:, None, :], verts[faces[:, 0]][None], (verts[faces[:, 1]] - verts[faces[:, 0]])[None],
                   (verts[faces[:, 2]] - verts[faces[:, 0]])[None])[3]
    assert np.array_equal(np.where((m == 0).any(axis=1), (m == 0).argmax(axis=1), -1), want)


@pytest.mark.parametrize('shift,scale', [((512.0, -300.0, 40.0), 1.0), (None, 2.0 ** -6)])
def test_far_points_are_far_and_not_ambiguous(shift, scale):
    verts, faces = template_mesh(1001)
    verts = ((verts + (0.0 if shift is None else np.asarray(shift))) * scale).astype(np.float32).astype(np.float64)
    far, s, t = so.far_points(verts, faces, 8, lo=5.0 * scale, hi=50.0 * scale)
    assert (s > 1e-5 * t + 1e-7).all() and t.min() >= 5.0 * scale and t.max() <= 50.0 * scale and t.max() > 10 * scale
    pts = np.concatenate([far.astype(np.float32).astype(np.float64),
                          (samples(verts / scale, faces, 313, 0.03, 5) * scale).astype(np.float32).astype(np.float64)])
    r = so.scan_to_mesh(pts, verts, faces)
    dist = np.sqrt(r['m'][:8])
    assert np.abs(dist - t).max() <= 1e-5 * t.max() and (r['region'][:8] != 6).all()
    assert not r['ambiguous'][:8].any() and r['ambiguous'].mean() <= 0.01


def test_a_point_whose_every_face_gives_nan_has_no_winner_and_pays_nothing():
    verts, faces = template_mesh(700)
    a, c = faces[2, 0], faces[2, 2]
    line = np.array([[a, a, c], [a, a, c]])
    pts = samples(verts, faces, 200, 0.03, 7)
    d2 = ((pts - verts[a]) * (verts[c] - verts[a])).sum(axis=1)
    for prune in (True, False):
        r = so.scan_to_mesh(pts, verts, line, prune=prune)
        assert (d2 > 0).sum() > 20 and (d2 <= 0).sum() > 20
        assert (r['face'][d2 > 0] == -1).all() and (r['face'][d2 <= 0] == 0).all()
        assert not r['m'][d2 > 0].any() and not r['ambiguous'].any()
        assert np.allclose(r['m'][d2 <= 0], ((pts - verts[a]) ** 2).sum(axis=1)[d2 <= 0], rtol=1e-14)
    ref = so.evaluate(verts[None], line, pts[None], [200], None, w_s2m=1.0)
    only = so.evaluate(verts[None], line, pts[None][:, d2 <= 0], [(d2 <= 0).sum()], None, w_s2m=1.0)
    assert only['loss'][0] > 0 and abs(ref['loss'][0] - only['loss'][0]) <= 1e-13 * only['loss'][0]
    assert np.array_equal(ref['grad'], only['grad'])
    assert (ref['nearest_face'][0][d2 > 0] == -1).all()
    # among the model's other faces the two repeated-index faces never win where their m is NaN
    pair = np.concatenate([[[a, a, c], [a, a, a]], faces[2:]])
    r = so.scan_to_mesh(pts, verts, pair)
    brute = so.scan_to_mesh(pts, verts, pair, prune=False)
    assert all(np.array_equal(r[k], brute[k]) for k in r) and (r['face'] >= 0).all() and np.isfinite(r['m']).all()
    assert (r['face'][d2 > 0] >= 1).all()


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
