"""CPU: the NumPy restatement of the overlay renderer (tests/render_oracle.py, include/mvfit.h:mvfit_render_overlay)
against hand-worked cases: coverage counts, shared edges, a sphere's silhouette, the depth test and the shade formula."""
import numpy as np

from mvsmplfitting_amd import synthetic as syn
from tests import render_oracle as ro

# identity camera with f = 1, c = 0: a vertex at (u, v, 1) lands on pixel coordinates (u, v)
IDENT = (np.eye(3, dtype=np.float32), np.zeros(3, np.float32), 1.0, np.zeros(2, np.float32))


def _flat(uv, z=1.0):
    uv = np.asarray(uv, np.float64)
    return np.concatenate([uv * z, np.full((uv.shape[0], 1), z)], axis=1).astype(np.float32)


def test_single_triangle_pixel_counts():
    # legs of 10 px from a pixel corner: centres (x + .5, y + .5) with x + y <= 9 -> 55 pixels
    _, fid = ro.render(_flat([[0, 0], [10, 0], [0, 10]]), [[0, 1, 2]], IDENT, 16, 16)
    assert (fid == 0).sum() == 55
    ys, xs = np.nonzero(fid == 0)
    assert np.all(xs + ys <= 9)
    # the same triangle through pixel centres: the edges are inclusive -> x + y <= 10, 66 pixels; either winding
    for tri in ([0, 1, 2], [0, 2, 1]):
        _, fid = ro.render(_flat([[0.5, 0.5], [10.5, 0.5], [0.5, 10.5]]), [tri], IDENT, 16, 16)
        assert (fid == 0).sum() == 66
    # degenerate (zero area): nothing
    _, fid = ro.render(_flat([[0.5, 0.5], [5.5, 5.5], [10.5, 10.5]]), [[0, 1, 2]], IDENT, 16, 16)
    assert (fid < 0).all()


def test_shared_edges_leave_no_hole():
    # a hexagon with irregular (non-lattice) vertices split into a fan of six triangles around an off-centre point
    ang = np.arange(6) * np.pi / 3 + 0.1234
    rim = np.stack([40.3 + 27.7 * np.cos(ang), 30.9 + 23.1 * np.sin(ang)], 1)
    uv = np.concatenate([[[41.17, 29.61]], rim])
    faces = [[0, 1 + k, 1 + (k + 1) % 6] for k in range(6)]
    _, fid = ro.render(_flat(uv), faces, IDENT, 64, 80)
    # every pixel centre strictly inside the hexagon (exact integer test on the snapped rim) is covered
    XY = np.rint(rim * 256).astype(np.int64)
    ys, xs = np.mgrid[0:64, 0:80]
    sx, sy = 256 * xs + 128, 256 * ys + 128
    inside = np.ones_like(sx, bool)
    for k in range(6):
        a, b = XY[k], XY[(k + 1) % 6]
        inside &= (b[0] - a[0]) * (sy - a[1]) - (b[1] - a[1]) * (sx - a[0]) > 0
    assert inside.sum() > 1000
    assert np.all(fid[inside] >= 0)
    # and nothing outside the closed hexagon is drawn
    closed = np.ones_like(sx, bool)
    for k in range(6):
        a, b = XY[k], XY[(k + 1) % 6]
        closed &= (b[0] - a[0]) * (sy - a[1]) - (b[1] - a[1]) * (sx - a[0]) >= 0
    assert np.all(fid[~closed] < 0)


def test_sphere_silhouette_is_the_analytic_disc():
    v, f = syn._uv_sphere()
    R, d, focal = 1.0, 4.0, 300.0
    verts = (v * R + np.array([0.0, 0.0, d])).astype(np.float32)
    cam = (np.eye(3, dtype=np.float32), np.zeros(3, np.float32), focal, np.array([160.0, 120.0], np.float32))
    _, fid = ro.render(verts, f, cam, 240, 320)
    r = focal * R / np.sqrt(d * d - R * R)
    area = np.pi * r * r
    assert abs((fid >= 0).sum() - area) < 0.01 * area, ((fid >= 0).sum(), area)
    # centred on the principal point
    ys, xs = np.nonzero(fid >= 0)
    assert abs(xs.mean() + 0.5 - 160.0) < 0.5 and abs(ys.mean() + 0.5 - 120.0) < 0.5


def test_nearer_face_wins():
    uv = [[2, 2], [30, 3], [5, 28]]
    far, near = _flat(uv, z=3.0), _flat(uv, z=2.0)
    verts = np.concatenate([near, far])
    for faces, nearer in (([[0, 1, 2], [3, 4, 5]], 0), ([[3, 4, 5], [0, 1, 2]], 1)):
        _, fid = ro.render(verts, faces, IDENT, 32, 32)
        assert (fid >= 0).sum() > 300
        assert np.all(fid[fid >= 0] == nearer)
    # equal depth: the lower face id
    _, fid = ro.render(np.concatenate([near, near]), [[0, 1, 2], [3, 4, 5]], IDENT, 32, 32)
    assert np.all(fid[fid >= 0] == 0)


def test_flat_facet_shade_by_hand():
    # one facet in the plane z = 2 facing the camera; f = 100, c = (32, 24)
    f_, cx, cy, z = 100.0, 32.0, 24.0, 2.0
    corners = np.array([[-0.5, -0.4], [0.6, -0.3], [-0.2, 0.5]])
    verts = np.concatenate([corners, np.full((3, 1), z)], 1).astype(np.float32)
    cam = (np.eye(3, dtype=np.float32), np.zeros(3, np.float32), f_, np.array([cx, cy], np.float32))
    img = np.full((48, 64, 3), 7, np.uint8)
    out, fid = ro.render(verts, [[0, 1, 2]], cam, 48, 64, image=img)
    assert np.all(out[fid < 0] == 7)                     # background keeps the input bytes
    # by hand at a few covered pixels: q on the ray through the pixel centre, n = -z towards the camera
    mn, mx = verts.min(0).astype(np.float64), verts.max(0).astype(np.float64)
    c, h = (mn + mx) / 2, (mx - mn) / 2
    r = np.linalg.norm(h)
    ys, xs = np.nonzero(fid == 0)
    for k in np.linspace(0, len(xs) - 1, 7).astype(int):
        x, y = xs[k], ys[k]
        q = np.array([(x + 0.5 - cx) * z / f_, (y + 0.5 - cy) * z / f_, z])
        n = np.array([0.0, 0.0, -1.0])
        s = 0.5 * 0.3
        for th in np.pi * np.array([1, 3, 5]) / 6:
            for ph in np.pi * np.array([0, 2, 4]) / 3:
                L = c + r * np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
                d = L - q
                s += 0.5 / np.pi * r * r * max(0.0, n @ d / np.linalg.norm(d)) / (d @ d)
        want = round(255 * min(1.0, s) ** (1 / 2.2))
        assert np.all(out[y, x] == out[y, x, 0]) and abs(int(out[y, x, 0]) - want) <= 1, (out[y, x], want)


def test_dots_are_red_discs_drawn_last():
    verts = _flat([[0, 0], [40, 0], [0, 40]])
    pts = np.array([[10.7, 9.2, 1.0], [-0.5, 30.9, 1.0], [5.0, 5.0, -1.0]], np.float32)   # the last is behind the camera
    out, fid = ro.render(verts, [[0, 1, 2]], IDENT, 48, 48, points=pts)
    red = np.all(out == (255, 0, 0), axis=-1)
    disc = lambda cx, cy: (np.mgrid[0:48, 0:48][1] - cx) ** 2 + (np.mgrid[0:48, 0:48][0] - cy) ** 2 <= 64
    assert np.array_equal(red, disc(10, 9) | disc(0, 30))     # truncation toward zero: -0.5 -> 0
    assert fid[9, 10] == 0                                    # the face id is the mesh's
