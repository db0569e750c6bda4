"""CPU: the restatement of the occlusion between bodies (tests/silhouette_occlusion_oracle.py) against hand-worked cases and
against tests/silhouette_oracle.py, the driver silhouette.refine_fit_occluded against a scripted engine, and fit_folder's
``occlusion`` key."""
import numpy as np
import pytest
import torch

from mvsmplfitting_amd.batch import check_silhouettes
from mvsmplfitting_amd.silhouette import refine_fit_occluded
from tests import silhouette_occlusion_oracle as oo
from tests import silhouette_oracle as so
from tests.silhouette_occlusion_stub_engine import ScriptedEngine

H, W = 6, 8
EYE = (np.eye(3, dtype=np.float32), np.zeros(3, np.float32), np.float32(1.0), np.zeros(2, np.float32))     # u = X / Z, v = Y / Z
INF = np.float32(np.inf)


def _at(u, v, z):
    """The world point that the camera EYE projects to (u, v) at depth z (exact for the values used here)."""
    return [u * z, v * z, z]


# the occluder: one triangle with corners at pixels (1, 1), (7, 1), (1, 5), everywhere at depth 2
TRI = np.array([_at(1, 1, 2), _at(7, 1, 2), _at(1, 5, 2)], np.float32)


def _tri_cover():
    """Worked by hand: pixel (x, y) is sampled at (x + .5, y + .5); inside iff x >= 1, y >= 1 and 2 x + 3 y <= 14."""
    c = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            c[y, x] = x >= 1 and y >= 1 and 2 * x + 3 * y <= 14
    return c


def test_a_single_triangle_over_a_6_by_8_image():
    bits = oo.depth_bits(TRI, np.array([[0, 1, 2]]), EYE, H, W)
    z = bits.view(np.float32)
    cover = _tri_cover()
    assert cover.sum() == 12 and cover[1, 1:6].all() and cover[4, 1] and not cover[4, 2] and not cover[5].any()
    assert np.array_equal(np.isfinite(z), cover)
    assert (z[cover] == np.float32(2.0)).all() and (bits[~cover] == oo.INF_BITS).all()
    # the other winding and a second, nearer triangle over part of it: minimum over the bits
    near = np.array([_at(1, 1, 1.5), _at(3, 1, 1.5), _at(1, 3, 1.5)], np.float32)
    verts = np.stack([np.zeros((3, 3), np.float32), TRI[[0, 2, 1]], near])          # bodies 0 (the image's own: nothing), 1, 2
    z_occ, z_own = oo.freeze(verts, np.array([[0, 1, 2]]), [0], tuple(np.asarray(a)[None] for a in EYE), [5, 5, 5], H, W)
    assert np.isinf(z_own).all()                                                    # a degenerate own body draws nothing
    assert z_occ[0, 1, 1] == np.float32(1.5) and z_occ[0, 1, 5] == np.float32(2.0) and np.isinf(z_occ[0, 0, 0])
    assert np.array_equal(np.isfinite(z_occ[0]), cover)
    # other scenes and scene -1 do not occlude
    z_occ, _ = oo.freeze(verts, np.array([[0, 1, 2]]), [0], tuple(np.asarray(a)[None] for a in EYE), [5, 4, -1], H, W)
    assert np.isinf(z_occ).all()
    z_occ, _ = oo.freeze(verts, np.array([[0, 1, 2]]), [0], tuple(np.asarray(a)[None] for a in EYE), [-1, -1, -1], H, W)
    assert np.isinf(z_occ).all()


def _block():
    """Mask: the block of columns 5..7, rows 1..3; its contour in raster order and the triangle's map."""
    mask = np.zeros((1, H, W), np.uint8)
    mask[0, 1:4, 5:8] = 1
    prep = so.prepare(mask, 1)
    assert prep['xy'].tolist() == [[5, 1], [6, 1], [7, 1], [5, 2], [5, 3], [6, 3], [7, 3]]
    z_occ = oo.depth_bits(TRI, np.array([[0, 1, 2]]), EYE, H, W).view(np.float32)[None]
    return mask, prep, z_occ


def test_point_flags_by_hand():
    mask, prep, z_occ = _block()
    own = np.full((1, H, W), INF, np.float32)
    # own depth +inf: "not known to be in front".  (5, 1): the left neighbour (4, 1) is explained, the upper one (5, 0) is not
    # (nothing covers it) -> unflagged.  (5, 2): its only off neighbour (4, 2) is explained -> flagged.  (5, 3): (4, 3) and
    # (5, 4) lie outside the triangle -> unflagged.  (7, y): the right neighbour lies outside the image and does not count.
    assert np.isfinite(z_occ[0, 1, 4]) and np.isfinite(z_occ[0, 2, 4]) and np.isinf(z_occ[0, 3, 4]) and np.isinf(z_occ[0, 0, 5])
    assert oo.point_flags(mask, prep['first'], prep['xy'], z_occ, own).tolist() == [0, 0, 0, 1, 0, 0, 0]
    # the body in front of the occluder at the point (1.0 <= 2.0): the off pixel is its own outline
    own[0, 2, 5] = 1.0
    assert oo.point_flags(mask, prep['first'], prep['xy'], z_occ, own).tolist() == [0, 0, 0, 0, 0, 0, 0]
    own[0, 2, 5] = 2.0                           # equal depths: in front
    assert oo.point_flags(mask, prep['first'], prep['xy'], z_occ, own).tolist() == [0, 0, 0, 0, 0, 0, 0]
    own[0, 2, 5] = 3.0                           # behind
    assert oo.point_flags(mask, prep['first'], prep['xy'], z_occ, own).tolist() == [0, 0, 0, 1, 0, 0, 0]
    # everything covered: every point whose off neighbours are inside the image is flagged
    allz = np.full((1, H, W), 2.0, np.float32)
    assert oo.point_flags(mask, prep['first'], prep['xy'], allz, np.full((1, H, W), INF, np.float32)).tolist() == [1] * 7


def test_hidden_bytes_margin_and_image_border():
    cams = tuple(np.asarray(a)[None] for a in EYE)
    z_occ = np.full((1, H, W), 2.0, np.float32)
    up = np.nextafter(np.float32(2.5), INF)
    pts = [_at(2.5, 1.5, 2.5),                   # z_occ + margin = 2.5 < 2.5: no
           _at(2.5, 1.5, up),                    # one ulp behind the threshold: hidden
           _at(2.5, 1.5, 1.0),                   # in front
           [0.0, 0.0, 4.0],                      # u == 0, v == 0: inside
           [-0.004, 0.0, 4.0],                   # u < 0
           [32.0, 0.0, 4.0],                     # u == W exactly: outside
           [31.0, 0.0, 4.0],                     # u = 7.75: the last column
           [0.0, 24.0, 4.0],                     # v == H exactly
           [0.0, 23.0, 4.0],
           [2.0, 2.0, 0.05],                     # pz <= 0.05: invalid, never hidden
           [2.0, 2.0, -4.0]]
    v = np.array(pts, np.float32)[None]
    got = oo.hidden_bytes(v, [0], cams, z_occ, 0.5)[0].tolist()
    assert got == [0, 1, 0, 1, 0, 0, 1, 0, 1, 0, 0]
    assert oo.hidden_bytes(v, [0], cams, z_occ, 0.0)[0].tolist() == [1, 1, 0, 1, 0, 0, 1, 0, 1, 0, 0]
    assert not oo.hidden_bytes(v, [0], cams, np.full((1, H, W), INF, np.float32), 0.5).any()
    # the map is read at [(int)v][(int)u]
    z_occ[0, 1, 2] = INF
    assert oo.hidden_bytes(v, [0], cams, z_occ, 0.0)[0].tolist()[:3] == [0, 0, 0]


def _cloud(seed=0, nv=60):
    """Two bodies of nv points in front of two 24 x 32 images, a blob mask each."""
    rng = np.random.default_rng(seed)
    Hh, Ww = 24, 32
    R = np.stack([np.eye(3), np.eye(3)]).astype(np.float32)
    t = np.array([[0, 0, 0], [0.1, -0.1, 0.2]], np.float32)
    f = np.array([20.0, 22.0], np.float32)
    c = np.array([[16, 12], [15, 13]], np.float32)
    V = np.concatenate([rng.uniform(-1.0, 1.0, (2, nv, 2)), rng.uniform(1.5, 3.0, (2, nv, 1))], axis=2).astype(np.float32)
    yy, xx = np.mgrid[0:Hh, 0:Ww]
    masks = np.stack([((yy - 12) ** 2 + (xx - 15) ** 2 < 60), ((yy - 10) ** 2 / 2 + (xx - 18) ** 2 < 50)]).astype(np.uint8)
    return masks, V, np.array([0, 1]), (R, t, f, c)


@pytest.mark.parametrize('sigma', [0.0, 3.0])
def test_nothing_hidden_and_nothing_flagged_is_the_plain_oracle(sigma):
    masks, V, body, cams = _cloud()
    prep = so.prepare(masks, 2)
    a = so.evaluate(prep, V, body, cams, 0.7, 1.3, sigma)
    b = oo.evaluate(prep, V, body, cams, 0.7, 1.3, sigma)
    c = oo.evaluate(prep, V, body, cams, 0.7, 1.3, sigma, hidden=np.zeros((2, V.shape[1]), np.uint8), flags=np.zeros(len(prep['xy']), np.uint8))
    for r in (b, c):
        assert np.array_equal(r['loss'], a['loss']) and np.array_equal(r['g'], a['g']) and np.array_equal(r['winner'], a['winner'])
    assert a['loss'].min() > 0 and np.abs(a['g']).max() > 0


def test_hidden_vertices_and_flagged_points_drop_out():
    masks, V, body, cams = _cloud()
    prep = so.prepare(masks, 1)
    plain = so.evaluate(prep, V, body, cams)
    hidden = np.zeros((2, V.shape[1]), np.uint8)
    hidden[0, plain['winner'][0]] = 1            # the winner of point 0 is hidden: another vertex wins
    flags = np.zeros(len(prep['xy']), np.uint8)
    flags[3] = 1
    r = oo.evaluate(prep, V, body, cams, hidden=hidden, flags=flags)
    assert r['winner'][3] == -2 and r['winner'][0] not in (plain['winner'][0], -1, -2)
    assert r['rho_a'][0, plain['winner'][0]] == 0 and not r['g'][0, plain['winner'][0]].any()
    # a hidden vertex is an invalid vertex: the same numbers as with the vertex behind the camera
    V2 = V.copy()
    V2[0, plain['winner'][0]] = [0, 0, -1]
    r2 = oo.evaluate(prep, V2, body, cams, flags=flags)
    assert np.array_equal(r2['loss'], r['loss']) and np.array_equal(r2['g'], r['g']) and np.array_equal(r2['winner'], r['winner'])
    # B_i sums the unflagged points only: flagging the point removes exactly its rho_B
    r3 = oo.evaluate(prep, V, body, cams, w_in=0.0, hidden=hidden)
    r4 = oo.evaluate(prep, V, body, cams, w_in=0.0, hidden=hidden, flags=flags)
    p3 = prep['xy'][3].astype(np.float64) + 0.5
    from tests import render_oracle as ro
    _, u, w = ro.transform(V[0], cams[0][0], cams[1][0], cams[2][0], cams[3][0])
    j = r3['winner'][3]
    m = np.float32(np.float32(u[j] - np.float32(p3[0])) ** 2 + np.float32(w[j] - np.float32(p3[1])) ** 2)
    assert abs((r3['loss'][0] - r4['loss'][0]) - float(m)) <= 1e-9 * r3['loss'][0]


def test_gradient_against_central_differences():
    masks, V, body, cams = _cloud(seed=3)
    prep = so.prepare(masks, 1)
    hidden = np.zeros((2, V.shape[1]), np.uint8)
    hidden[:, ::5] = 1
    flags = np.zeros(len(prep['xy']), np.uint8)
    flags[::4] = 1
    V = V.astype(np.float64)
    kw = dict(w_in=0.8, w_out=1.1, sigma=4.0, hidden=hidden, flags=flags, pure64=True)
    r = oo.evaluate(prep, V, body, cams, **kw)
    eps, checked = 1e-6, 0
    for n in range(2):
        for j in range(V.shape[1]):
            # away from the discontinuities: the projection keeps its field cell and the winners stay under the step
            p, u, w = so._project(V[n], cams[0][n], cams[1][n], cams[2][n], cams[3][n], True)
            fx, fy = (u[j] - 0.5) % 1.0, (w[j] - 0.5) % 1.0
            if min(fx, 1 - fx, fy, 1 - fy) < 1e-3:
                continue
            for k in range(3):
                Vp, Vm = V.copy(), V.copy()
                Vp[n, j, k] += eps
                Vm[n, j, k] -= eps
                rp, rm = oo.evaluate(prep, Vp, body, cams, **kw), oo.evaluate(prep, Vm, body, cams, **kw)
                if not (np.array_equal(rp['winner'], r['winner']) and np.array_equal(rm['winner'], r['winner'])):
                    continue
                fd = (rp['loss'][n] - rm['loss'][n]) / (2 * eps)
                assert abs(fd - r['g'][n, j, k]) <= 1e-5 * max(1.0, np.abs(r['g'][n]).max()), (n, j, k, fd, r['g'][n, j, k])
                checked += 1
            if hidden[n, j]:
                assert not r['g'][n, j].any()
        assert checked > 30
    assert np.abs(r['g']).max() > 0


# ---- the driver
def _moves(B, rows, towards=True):
    m = np.zeros((B, 118), np.float32)
    m[rows, 0] = -0.5 if towards else 0.5        # x starts at 2 on coordinate 0, the goal is 0
    return m


def _start(B):
    x = np.zeros((B, 118), np.float32)
    x[:, 0] = 2.0
    return x


def test_driver_sweeps_freeze_at_the_current_rows_and_stop_when_nothing_is_accepted():
    B = 3
    eng = ScriptedEngine(np.zeros((B, 118)), [_moves(B, [0, 2]), _moves(B, [1], towards=False), _moves(B, [0])])
    out, rep = refine_fit_occluded(eng, _start(B), dict(coll_loss_weight=1.0), [0, 0, -1], margin=0.03, sweeps=5)
    assert eng.calls == ['freeze', 'term_on', 'fit', 'term_off', 'freeze', 'drop_graph', 'term_on', 'fit', 'term_off', 'clear_occluders']
    assert len(rep['sweeps']) == 2                                                   # the second sweep accepted nothing
    assert rep['sweeps'][0]['accepted'].tolist() == [True, False, True] and not rep['sweeps'][1]['accepted'].any()
    assert out[:, 0].tolist() == [1.5, 2.0, 1.5]                                     # the rejected row went back
    # frozen at the current rows' vertices, with the caller's scene labels and margin
    assert torch.equal(eng.frozen[0][0], eng.vertices(torch.as_tensor(_start(B)))[0])
    assert torch.equal(eng.frozen[1][0], eng.vertices(out)[0])
    assert eng.frozen[0][1].tolist() == [0, 0, -1] and eng.frozen[1][2] == 0.03
    # per sweep and image: hidden vertices and flagged points
    assert rep['sweeps'][0]['hidden'].tolist() == [1] * 6 and rep['sweeps'][1]['hidden'].tolist() == [2] * 6
    assert rep['sweeps'][0]['flagged'].tolist() == [2, 1, 2, 1, 2, 1]
    assert rep['accepted'].tolist() == [False] * 3 and not eng.occluders and not eng.term


def test_driver_runs_the_sweeps_it_is_given():
    B = 2
    eng = ScriptedEngine(np.zeros((B, 118)), [_moves(B, [0, 1])] * 3)
    out, rep = refine_fit_occluded(eng, _start(B), dict(coll_loss_weight=1.0), [0, 0], sweeps=2)
    assert eng.calls.count('fit') == 2 and len(rep['sweeps']) == 2 and out[:, 0].tolist() == [1.0, 1.0]
    assert rep['before'].tolist() == [2.25, 2.25] and rep['after'].tolist() == [1.0, 1.0]
    with pytest.raises(ValueError):
        refine_fit_occluded(eng, _start(B), dict(coll_loss_weight=1.0), [0, 0], sweeps=0)
    with pytest.raises(ValueError):
        refine_fit_occluded(eng, _start(B), dict(coll_loss_weight=1.0), [0, 0, 0])


def test_driver_cleans_up_on_an_exception():
    B = 2
    eng = ScriptedEngine(np.zeros((B, 118)), [_moves(B, [0]), None])
    with pytest.raises(RuntimeError, match='scripted failure'):
        refine_fit_occluded(eng, _start(B), dict(coll_loss_weight=1.0), [0, 0], sweeps=3)
    assert eng.calls[-2:] == ['term_off', 'clear_occluders'] and not eng.occluders and not eng.term


# ---- fit_folder's option
def test_check_silhouettes_occlusion_key():
    base = dict(mask_root='m', weight=2.0)
    assert check_silhouettes(base)['occlusion'] is None
    assert check_silhouettes(dict(base, occlusion={}))['occlusion'] == dict(margin=0.02, sweeps=2)
    assert check_silhouettes(dict(base, occlusion=dict(margin=0.05)))['occlusion'] == dict(margin=0.05, sweeps=2)
    assert check_silhouettes(dict(base, occlusion=dict(sweeps=4)), multi=True)['occlusion']['sweeps'] == 4
    with pytest.raises(ValueError, match='persons='):
        check_silhouettes(dict(base, occlusion={}), multi=False)
    check_silhouettes(base, multi=False)
    for bad in (dict(depth=1), dict(margin=-0.1), dict(margin=float('nan')), dict(sweeps=0), True, [0.02, 2]):
        with pytest.raises(ValueError, match='occlusion'):
            check_silhouettes(dict(base, occlusion=bad))
    with pytest.raises(ValueError, match='unknown keys'):
        check_silhouettes(dict(base, occluders={}))
