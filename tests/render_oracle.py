"""NumPy restatement of include/mvfit.h:mvfit_render_overlay (csrc/render.hip): float32 transform in the stated order,
int64 edge functions, float64 depth and shading.  The raster is vectorised over the pixel boxes of faces grouped by box
size; every covered sample goes through one unbuffered ``np.minimum.at``, so the visibility key (fp32 depth bits << 32 |
face id) is the same order-independent minimum the kernel takes with its 64-bit atomics."""
import numpy as np

ZNEAR = np.float32(0.05)
ZFAR = np.float32(8000.0)
GUARD = np.float32(16384.0)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def transform(verts, R, t, f, c):
    """Camera-space p (float32) and pixel u, v (float32): p = ((R0 X + R1 Y) + R2 Z) + t, u = f (px / pz) + cx."""
    v = np.asarray(verts, np.float32)
    R = np.asarray(R, np.float32)
    t = np.asarray(t, np.float32)
    X, Y, Z = v[:, 0], v[:, 1], v[:, 2]
    p = np.stack([((R[k, 0] * X + R[k, 1] * Y) + R[k, 2] * Z) + t[k] for k in range(3)], axis=1)
    f = np.float32(f)
    c = np.asarray(c, np.float32)
    with np.errstate(divide='ignore', invalid='ignore'):
        u = f * (p[:, 0] / p[:, 2]) + c[0]
        w = f * (p[:, 1] / p[:, 2]) + c[1]
    return p, u, w


def vertex_normals(verts, faces):
    """World-space unit normals, float64: per vertex the sum of (p1 - p0) x (p2 - p0) over its faces in ascending id."""
    P = np.asarray(verts, np.float32).astype(np.float64)
    F = np.asarray(faces, np.int64)
    a, b, c = P[F[:, 0]], P[F[:, 1]], P[F[:, 2]]
    e1, e2 = b - a, c - a
    fn = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                   e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                   e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    vid = F.reshape(-1)
    fid = np.repeat(np.arange(F.shape[0]), 3)
    order = np.lexsort((fid, vid))                     # by vertex, then ascending face id
    s = np.zeros_like(P)
    np.add.at(s, vid[order], fn[fid[order]])           # unbuffered: sequential in that order
    ln = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
    out = np.zeros_like(s)
    nz = ln > 0
    out[nz] = s[nz] / ln[nz, None]
    return out


def _edge(xa, ya, xb, yb, sx, sy):
    return (xb - xa) * (sy - ya) - (yb - ya) * (sx - xa)


def lights(p):
    """The nine point lights (camera space) and r^2 from the box of the camera-space vertices."""
    mn, mx = p.min(0).astype(np.float64), p.max(0).astype(np.float64)
    cen = 0.5 * (mn + mx)
    h = 0.5 * (mx - mn)
    r = np.sqrt((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2])
    L = []
    for a in range(3):
        for q in range(3):
            th, ph = np.pi * (2 * a + 1) / 6.0, 2.0 * np.pi * q / 3.0
            d = np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
            L.append(cen + r * d)
    return np.asarray(L), r * r


def shade_value(n, q, L, r2):
    """Pixel byte of unit normals n [M,3] (already flipped to face the camera) at camera-space points q [M,3]."""
    acc = np.zeros(n.shape[0])
    for k in range(L.shape[0]):
        lx, ly, lz = L[k, 0] - q[:, 0], L[k, 1] - q[:, 1], L[k, 2] - q[:, 2]
        d2 = (lx * lx + ly * ly) + lz * lz
        ndl = ((n[:, 0] * lx + n[:, 1] * ly) + n[:, 2] * lz) / np.sqrt(d2)
        acc = np.where(ndl > 0.0, acc + r2 * ndl / d2, acc)
    s = 0.5 * 0.3 + (0.5 / np.pi) * acc
    return np.floor(255.0 * np.power(np.minimum(1.0, s), 1.0 / 2.2) + 0.5).astype(np.uint8)


def raster(X, Y, pz, ok, faces, H, W, max_elems=1 << 22):
    """Visibility keys [H*W] uint64 (EMPTY where nothing is drawn)."""
    F = np.asarray(faces, np.int64)
    vis = np.full(H * W, EMPTY, np.uint64)
    i0, i1, i2 = F[:, 0], F[:, 1], F[:, 2]
    keep = ok[i0] & ok[i1] & ok[i2]
    X0, X1, X2, Y0, Y1, Y2 = X[i0], X[i1], X[i2], Y[i0], Y[i1], Y[i2]
    area = _edge(X0, Y0, X1, Y1, X2, Y2)
    keep &= area != 0
    sgn = np.where(area > 0, 1, -1).astype(np.int64)
    minX, maxX = np.minimum(np.minimum(X0, X1), X2), np.maximum(np.maximum(X0, X1), X2)
    minY, maxY = np.minimum(np.minimum(Y0, Y1), Y2), np.maximum(np.maximum(Y0, Y1), Y2)
    x0 = np.maximum(0, (minX - 128 + 255) >> 8)
    x1 = np.minimum(W - 1, (maxX - 128) >> 8)
    y0 = np.maximum(0, (minY - 128 + 255) >> 8)
    y1 = np.minimum(H - 1, (maxY - 128) >> 8)
    keep &= (x0 <= x1) & (y0 <= y1)
    idx = np.flatnonzero(keep)
    if idx.size == 0:
        return vis
    bw = (x1 - x0 + 1)[idx]
    bh = (y1 - y0 + 1)[idx]
    kw = np.ceil(np.log2(bw)).astype(np.int64)
    kh = np.ceil(np.log2(bh)).astype(np.int64)
    iz = 1.0 / pz.astype(np.float64)
    for key_w, key_h in sorted(set(zip(kw.tolist(), kh.tolist()))):
        sel = idx[(kw == key_w) & (kh == key_h)]
        gw, gh = 1 << key_w, 1 << key_h
        step = max(1, max_elems // (gw * gh))
        dy, dx = np.meshgrid(np.arange(gh), np.arange(gw), indexing='ij')
        for s0 in range(0, sel.size, step):
            fs = sel[s0:s0 + step]
            xs = x0[fs][:, None, None] + dx[None]
            ys = y0[fs][:, None, None] + dy[None]
            valid = (xs <= x1[fs][:, None, None]) & (ys <= y1[fs][:, None, None])
            sx, sy = 256 * xs + 128, 256 * ys + 128
            g = sgn[fs][:, None, None]

            def e(a, b):
                return _edge(X[a][fs][:, None, None], Y[a][fs][:, None, None], X[b][fs][:, None, None],
                             Y[b][fs][:, None, None], sx, sy) * g
            e0, e1, e2 = e(i1, i2), e(i2, i0), e(i0, i1)
            cov = valid & (e0 >= 0) & (e1 >= 0) & (e2 >= 0)
            if not cov.any():
                continue
            fi = np.broadcast_to(fs[:, None, None], cov.shape)[cov]
            w = ((e0[cov].astype(np.float64) * iz[i0[fi]] + e1[cov].astype(np.float64) * iz[i1[fi]])
                 + e2[cov].astype(np.float64) * iz[i2[fi]])
            z = ((area[fi] * sgn[fi]).astype(np.float64) / w).astype(np.float32)
            zok = (z >= ZNEAR) & (z <= ZFAR)
            key = (z[zok].view(np.uint32).astype(np.uint64) << np.uint64(32)) | fi[zok].astype(np.uint64)
            np.minimum.at(vis, (ys[cov][zok] * W + xs[cov][zok]), key)
    return vis


def render(verts, faces, cam, H, W, image=None, points=None, normals=None):
    """One image: verts [Nv,3] float32 (world), faces [Nf,3], cam = (R[3,3], t[3], f, c[2]) of this view, image uint8
    [H,W,3] (None: zeros), points [P,3] or None.  Returns (out uint8 [H,W,3], face_id int32 [H,W])."""
    R, t, f, c = cam
    p, u, w = transform(verts, R, t, f, c)
    pz = p[:, 2]
    with np.errstate(invalid='ignore'):
        ok = (pz > ZNEAR) & (u >= -GUARD) & (u <= np.float32(W) + GUARD) & (w >= -GUARD) & (w <= np.float32(H) + GUARD)
    X = np.where(ok, np.rint(np.where(ok, u, 0) * np.float32(256)), 0).astype(np.int64)
    Y = np.where(ok, np.rint(np.where(ok, w, 0) * np.float32(256)), 0).astype(np.int64)
    F = np.asarray(faces, np.int64)
    vis = raster(X, Y, pz, ok, F, H, W)
    out = np.zeros((H, W, 3), np.uint8) if image is None else np.array(image, np.uint8, copy=True)
    fid = np.full(H * W, -1, np.int32)
    hit = np.flatnonzero(vis != EMPTY)
    if hit.size:
        fi = (vis[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        fid[hit] = fi
        ys, xs = hit // W, hit % W
        sx, sy = 256 * xs + 128, 256 * ys + 128
        i0, i1, i2 = F[fi, 0], F[fi, 1], F[fi, 2]
        sgn = np.where(_edge(X[i0], Y[i0], X[i1], Y[i1], X[i2], Y[i2]) > 0, 1, -1)
        e0 = (_edge(X[i1], Y[i1], X[i2], Y[i2], sx, sy) * sgn).astype(np.float64)
        e1 = (_edge(X[i2], Y[i2], X[i0], Y[i0], sx, sy) * sgn).astype(np.float64)
        e2 = (_edge(X[i0], Y[i0], X[i1], Y[i1], sx, sy) * sgn).astype(np.float64)
        pz64 = pz.astype(np.float64)
        w0, w1, w2 = e0 * (1.0 / pz64[i0]), e1 * (1.0 / pz64[i1]), e2 * (1.0 / pz64[i2])
        ws = (w0 + w1) + w2
        b0, b1, b2 = (w0 / ws)[:, None], (w1 / ws)[:, None], (w2 / ws)[:, None]
        p64 = p.astype(np.float64)
        q = (b0 * p64[i0] + b1 * p64[i1]) + b2 * p64[i2]
        nw = vertex_normals(verts, F) if normals is None else normals
        R64 = np.asarray(R, np.float32).astype(np.float64)
        nc = np.stack([(R64[k, 0] * nw[:, 0] + R64[k, 1] * nw[:, 1]) + R64[k, 2] * nw[:, 2] for k in range(3)], axis=1)
        n = (b0 * nc[i0] + b1 * nc[i1]) + b2 * nc[i2]
        ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        n = np.where(ln[:, None] > 0, n / np.where(ln > 0, ln, 1.0)[:, None], n)
        away = ((n[:, 0] * q[:, 0] + n[:, 1] * q[:, 1]) + n[:, 2] * q[:, 2]) > 0.0
        n = np.where(away[:, None], -n, n)
        L, r2 = lights(p)
        val = shade_value(n, q, L, r2)
        out.reshape(-1, 3)[hit] = val[:, None]
    if points is not None:
        draw_dots(out, points, cam)
    return out, fid.reshape(H, W)


def dot_centres(points, cam, H, W):
    """Truncated pixel centres (cx, cy) of the points that draw a dot."""
    R, t, f, c = cam
    p, u, w = transform(points, R, t, f, c)
    with np.errstate(invalid='ignore'):
        ok = (p[:, 2] > ZNEAR) & (u >= -GUARD) & (u <= np.float32(W) + GUARD) & (w >= -GUARD) & (w <= np.float32(H) + GUARD)
    return [(int(np.trunc(u[k])), int(np.trunc(w[k]))) for k in np.flatnonzero(ok)]


def draw_dots(out, points, cam):
    H, W = out.shape[:2]
    for cx, cy in dot_centres(points, cam, H, W):
        for dy in range(-8, 9):
            for dx in range(-8, 9):
                x, y = cx + dx, cy + dy
                if dx * dx + dy * dy <= 64 and 0 <= x < W and 0 <= y < H:
                    out[y, x] = (255, 0, 0)
    return out
