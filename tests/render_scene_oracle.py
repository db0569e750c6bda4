"""NumPy restatement of include/mvfit.h:mvfit_render_scene on top of tests/render_oracle.py: the bodies of an image are
concatenated into one mesh (body k: vertices k Nv + j, faces k Nf + f), which goes through render_oracle's transform /
raster / vertex_normals / lights unchanged; the only new arithmetic is the shading per channel with the body's colour."""
import numpy as np

from tests import render_oracle as ro

# code/utils/utils.py:904-912 Renderer.colors in dictionary order
PALETTE = np.array([(.8, .1, .1), (.1, .1, .8), (.1, .8, .1), (.7, .7, .9), (.9, .9, .8), (.7, .75, .5), (.5, .7, .75)],
                   np.float32)


def light_sum(n, q, L, r2):
    """render_oracle.shade_value's accumulator: sum_k r^2 max(0, n.l_k) / |L_k - q|^2, float64 [M]."""
    acc = np.zeros(n.shape[0])
    for k in range(L.shape[0]):
        lx, ly, lz = L[k, 0] - q[:, 0], L[k, 1] - q[:, 1], L[k, 2] - q[:, 2]
        d2 = (lx * lx + ly * ly) + lz * lz
        ndl = ((n[:, 0] * lx + n[:, 1] * ly) + n[:, 2] * lz) / np.sqrt(d2)
        acc = np.where(ndl > 0.0, acc + r2 * ndl / d2, acc)
    return acc


def shade_bytes(acc, col):
    """acc float64 [M], col float32 [M, 3] -> uint8 [M, 3]: s = c * 0.3 + (c / pi) * acc per channel."""
    c = np.asarray(col, np.float32).astype(np.float64)
    s = c * 0.3 + (c / np.pi) * acc[:, None]
    return np.floor(255.0 * np.power(np.minimum(1.0, s), 1.0 / 2.2) + 0.5).astype(np.uint8)


def render_scene(bodies, faces, cam, H, W, image=None, points=None, colors=None, normals=None):
    """One image: bodies = list of [Nv,3] float32 world vertices (all of one topology ``faces`` [Nf,3]) in slot order,
    cam = (R, t, f, c), points = list of [P,3] per body or None, colors [n,3] float32 or None (the palette), normals =
    list of per-body world normals or None.  Returns (out uint8 [H,W,3], face_id int32 [H,W], body_id int32 [H,W])."""
    R, t, f, c = cam
    F1 = np.asarray(faces, np.int64)
    n, Nf = len(bodies), F1.shape[0]
    out = np.zeros((H, W, 3), np.uint8) if image is None else np.array(image, np.uint8, copy=True)
    fid = np.full(H * W, -1, np.int32)
    bid = np.full(H * W, -1, np.int32)
    if n:
        Nv = np.asarray(bodies[0]).shape[0]
        verts = np.concatenate([np.asarray(b, np.float32) for b in bodies])
        F = np.concatenate([F1 + k * Nv for k in range(n)])
        col = PALETTE[np.arange(n) % 7] if colors is None else np.asarray(colors, np.float32).reshape(n, 3)
        p, u, w = ro.transform(verts, R, t, f, c)
        pz = p[:, 2]
        with np.errstate(invalid='ignore'):
            ok = ((pz > ro.ZNEAR) & (u >= -ro.GUARD) & (u <= np.float32(W) + ro.GUARD) & (w >= -ro.GUARD)
                  & (w <= np.float32(H) + ro.GUARD))
        X = np.where(ok, np.rint(np.where(ok, u, 0) * np.float32(256)), 0).astype(np.int64)
        Y = np.where(ok, np.rint(np.where(ok, w, 0) * np.float32(256)), 0).astype(np.int64)
        vis = ro.raster(X, Y, pz, ok, F, H, W)
        hit = np.flatnonzero(vis != ro.EMPTY)
        if hit.size:
            fi = (vis[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)
            fid[hit] = fi % Nf
            bid[hit] = fi // Nf
            ys, xs = hit // W, hit % W
            sx, sy = 256 * xs + 128, 256 * ys + 128
            i0, i1, i2 = F[fi, 0], F[fi, 1], F[fi, 2]
            sgn = np.where(ro._edge(X[i0], Y[i0], X[i1], Y[i1], X[i2], Y[i2]) > 0, 1, -1)
            e0 = (ro._edge(X[i1], Y[i1], X[i2], Y[i2], sx, sy) * sgn).astype(np.float64)
            e1 = (ro._edge(X[i2], Y[i2], X[i0], Y[i0], sx, sy) * sgn).astype(np.float64)
            e2 = (ro._edge(X[i0], Y[i0], X[i1], Y[i1], sx, sy) * sgn).astype(np.float64)
            pz64 = pz.astype(np.float64)
            w0, w1, w2 = e0 * (1.0 / pz64[i0]), e1 * (1.0 / pz64[i1]), e2 * (1.0 / pz64[i2])
            ws = (w0 + w1) + w2
            b0, b1, b2 = (w0 / ws)[:, None], (w1 / ws)[:, None], (w2 / ws)[:, None]
            p64 = p.astype(np.float64)
            q = (b0 * p64[i0] + b1 * p64[i1]) + b2 * p64[i2]
            nw = np.concatenate([ro.vertex_normals(bodies[k], F1) if normals is None else normals[k] for k in range(n)])
            R64 = np.asarray(R, np.float32).astype(np.float64)
            nc = np.stack([(R64[k, 0] * nw[:, 0] + R64[k, 1] * nw[:, 1]) + R64[k, 2] * nw[:, 2] for k in range(3)], axis=1)
            nn = (b0 * nc[i0] + b1 * nc[i1]) + b2 * nc[i2]
            ln = np.sqrt((nn[:, 0] * nn[:, 0] + nn[:, 1] * nn[:, 1]) + nn[:, 2] * nn[:, 2])
            nn = np.where(ln[:, None] > 0, nn / np.where(ln > 0, ln, 1.0)[:, None], nn)
            away = ((nn[:, 0] * q[:, 0] + nn[:, 1] * q[:, 1]) + nn[:, 2] * q[:, 2]) > 0.0
            nn = np.where(away[:, None], -nn, nn)
            L, r2 = ro.lights(p)
            out.reshape(-1, 3)[hit] = shade_bytes(light_sum(nn, q, L, r2), col[fi // Nf])
    if points is not None:
        for k in range(n):
            ro.draw_dots(out, points[k], cam)
    return out, fid.reshape(H, W), bid.reshape(H, W)
