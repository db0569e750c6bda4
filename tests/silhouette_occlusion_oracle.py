"""TESTS ONLY - NumPy restatement of the occlusion between the bodies of a scene in the silhouette term
(include/mvfit.h:mvfit_set_silhouette_occluders).

Depth maps from tests/render_oracle.py's ``transform`` and ``raster`` (the visibility key's upper 32 bits, minimum over the
bodies), point flags and hidden bytes restated from the contract, and the evaluation of tests/silhouette_oracle.py with a
per-(image, vertex) mask and per-point flags: with nothing hidden and nothing flagged it is that evaluation, operation for
operation."""
import numpy as np

from tests import render_oracle as ro
from tests import silhouette_oracle as so

INF_BITS = np.uint32(0x7F800000)


def depth_bits(verts, faces, cam, H, W):
    """uint32 [H,W]: the fp32 bits of the smallest depth of any face of one body covering the pixel sample, +inf's bits where
    nothing does.  The steps of render_oracle.render up to the visibility buffer."""
    R, t, f, c = cam
    p, u, w = ro.transform(verts, R, t, f, c)
    pz = p[:, 2]
    with np.errstate(invalid='ignore'):
        ok = (pz > ro.ZNEAR) & (u >= -ro.GUARD) & (u <= np.float32(W) + ro.GUARD) & (w >= -ro.GUARD) & (w <= np.float32(H) + ro.GUARD)
    X = np.where(ok, np.rint(np.where(ok, u, 0) * np.float32(256)), 0).astype(np.int64)
    Y = np.where(ok, np.rint(np.where(ok, w, 0) * np.float32(256)), 0).astype(np.int64)
    vis = ro.raster(X, Y, pz, ok, np.asarray(faces, np.int64), H, W)
    bits = (vis >> np.uint64(32)).astype(np.uint32)
    bits[vis == ro.EMPTY] = INF_BITS
    return bits.reshape(H, W)


def occluders_of(image_body, body_scene):
    """Per image the list of occluding bodies (ascending)."""
    scene = np.asarray(body_scene).reshape(-1)
    out = []
    for n in np.asarray(image_body).reshape(-1):
        s = scene[int(n)]
        out.append([] if s < 0 else [int(m) for m in np.flatnonzero(scene == s) if m != int(n)])
    return out


def freeze(vertices, faces, image_body, cams, body_scene, H, W):
    """z_occ, z_own float32 [M,H,W]."""
    V = np.asarray(vertices, np.float32)
    cam_R, cam_t, cam_f, cam_c = cams
    M = len(image_body)
    z_occ = np.full((M, H, W), INF_BITS, np.uint32)
    z_own = np.full((M, H, W), INF_BITS, np.uint32)
    cache = {}

    def bits(body, i):
        cam = (cam_R[i], cam_t[i], cam_f[i], cam_c[i])
        key = (body, np.asarray(cam_R[i], np.float32).tobytes(), np.asarray(cam_t[i], np.float32).tobytes(), float(cam_f[i]),
               np.asarray(cam_c[i], np.float32).tobytes())
        if key not in cache:
            cache[key] = depth_bits(V[body], faces, cam, H, W)
        return cache[key]

    for i, occ in enumerate(occluders_of(image_body, body_scene)):
        z_own[i] = bits(int(image_body[i]), i)
        for m in occ:
            z_occ[i] = np.minimum(z_occ[i], bits(m, i))          # positive floats order like their bits
    return z_occ.view(np.float32), z_own.view(np.float32)


def point_flags(masks, first, xy, z_occ, z_own):
    """uint8 [C]: 1 iff every off 4-neighbour inside the image is explained."""
    masks = np.asarray(masks)
    M, H, W = masks.shape
    flag = np.zeros(len(xy), np.uint8)
    for i in range(M):
        for k in range(int(first[i]), int(first[i + 1])):
            x, y = int(xy[k, 0]), int(xy[k, 1])
            own = z_own[i, y, x]
            ok = True
            for qx, qy in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)):
                if qx < 0 or qx >= W or qy < 0 or qy >= H or masks[i, qy, qx] != 0:
                    continue
                zq = z_occ[i, qy, qx]
                explained = bool(zq < np.float32(np.inf)) and not bool(own <= zq)
                ok = ok and explained
            flag[k] = 1 if ok else 0
    return flag


def hidden_bytes(vertices, image_body, cams, z_occ, margin):
    """uint8 [M,Nv]: valid, inside the image (fp32 compares) and z_occ[(int)v][(int)u] + margin < pz (fp32 add)."""
    V = np.asarray(vertices, np.float32)
    cam_R, cam_t, cam_f, cam_c = cams
    M, H, W = z_occ.shape
    out = np.zeros((M, V.shape[1]), np.uint8)
    mg = np.float32(margin)
    for i in range(M):
        p, u, w = ro.transform(V[int(image_body[i])], cam_R[i], cam_t[i], cam_f[i], cam_c[i])
        with np.errstate(invalid='ignore'):
            inside = (p[:, 2] > np.float32(so.ZNEAR)) & (u >= 0) & (u < np.float32(W)) & (w >= 0) & (w < np.float32(H))
        idx = np.flatnonzero(inside)
        z = z_occ[i, w[idx].astype(np.int32), u[idx].astype(np.int32)]
        out[i, idx] = ((z + mg).astype(np.float32) < p[idx, 2]).astype(np.uint8)
    return out


def evaluate(prep, vertices, image_body, cams, w_in=1.0, w_out=1.0, sigma=0.0, hidden=None, flags=None, pure64=False):
    """silhouette_oracle.evaluate with ``hidden`` [M,Nv] (a hidden vertex is treated like an invalid one) and ``flags`` [C] (a
    flagged point contributes nothing, winner -2).  Also returns rho_a [M,Nv] float64: term A's share per (image, vertex)."""
    dt = np.float64 if pure64 else np.float32
    V = np.asarray(vertices, dt)
    N, nv = V.shape[0], V.shape[1]
    cam_R, cam_t, cam_f, cam_c = cams
    fields, first, xy, stride = prep['fields'], prep['first'], prep['xy'], prep['stride']
    M, H, W = fields.shape
    hidden = np.zeros((M, nv), bool) if hidden is None else np.asarray(hidden).astype(bool)
    flags = np.zeros(len(xy), bool) if flags is None else np.asarray(flags).astype(bool)
    loss = np.zeros(N)
    g = np.zeros((N, nv, 3))
    winner = np.full(len(xy), -1, np.int32)
    winner[flags] = -2
    rho_a = np.zeros((M, nv))
    s2 = float(sigma) ** 2
    for i in range(M):                                  # ascending image index: the order of every body's sums
        n = int(image_body[i])
        p, u, w = so._project(V[n], cam_R[i], cam_t[i], cam_f[i], cam_c[i], pure64)
        valid = (p[:, 2] > dt(so.ZNEAR)) & ~hidden[i]
        idx = np.flatnonzero(valid)
        if not prep['nonempty'][i]:
            continue
        gu, gv = np.zeros(nv), np.zeros(nv)
        # term A
        x, y = u[idx] - dt(0.5), w[idx] - dt(0.5)
        xc = np.minimum(np.maximum(x, dt(0)), dt(W - 1))
        yc = np.minimum(np.maximum(y, dt(0)), dt(H - 1))
        x0 = np.minimum(np.floor(xc).astype(np.int64), W - 2)
        y0 = np.minimum(np.floor(yc).astype(np.int64), H - 2)
        a, b = (xc - x0.astype(dt)).astype(np.float64), (yc - y0.astype(dt)).astype(np.float64)
        D = fields[i].astype(np.float64)
        D00, D01, D10, D11 = D[y0, x0], D[y0, x0 + 1], D[y0 + 1, x0], D[y0 + 1, x0 + 1]
        d = (1 - b) * ((1 - a) * D00 + a * D01) + b * ((1 - a) * D10 + a * D11)
        ddx = np.where(x == xc, (1 - b) * (D01 - D00) + b * (D11 - D10), 0.0)
        ddy = np.where(y == yc, (1 - a) * (D10 - D00) + a * (D11 - D01), 0.0)
        if sigma > 0:
            den = s2 + d * d
            rho, drdd = s2 * d * d / den, 2 * d * (s2 / den) ** 2
        else:
            rho, drdd = d * d, 2 * d
        A = rho.sum()
        rho_a[i, idx] = rho
        gu[idx] += w_in * drdd * ddx
        gv[idx] += w_in * drdd * ddy
        # term B
        Bsum = 0.0
        k_all = np.arange(int(first[i]), int(first[i + 1]))
        k_all = k_all[~flags[k_all]]
        if len(k_all) and len(idx):
            uu, ww = u[idx], w[idx]
            for k0 in range(0, len(k_all), 256):
                ks = k_all[k0:k0 + 256]
                q = xy[ks]
                cx, cy = q[:, 0].astype(dt) + dt(0.5), q[:, 1].astype(dt) + dt(0.5)
                dx, dy = uu[None, :] - cx[:, None], ww[None, :] - cy[:, None]
                m = dx * dx + dy * dy                   # products and sum each rounded to dt
                kk = np.argmin(m, axis=1)               # first minimum = lowest j
                rr = np.arange(len(q))
                winner[ks] = idx[kk]
                mw = m[rr, kk].astype(np.float64)
                if sigma > 0:
                    den = s2 + mw
                    rb, drb = s2 * mw / den, (s2 / den) ** 2
                else:
                    rb, drb = mw, np.ones_like(mw)
                Bsum += rb.sum()
                np.add.at(gu, idx[kk], w_out * stride * drb * 2 * dx[rr, kk].astype(np.float64))
                np.add.at(gv, idx[kk], w_out * stride * drb * 2 * dy[rr, kk].astype(np.float64))
        loss[n] += w_in * A + w_out * (stride * Bsum)
        # pull-back through the projection
        P = p[idx].astype(np.float64)
        k = float(dt(cam_f[i])) / P[:, 2]
        gp = np.stack([k * gu[idx], k * gv[idx], -k * (gu[idx] * P[:, 0] + gv[idx] * P[:, 1]) / P[:, 2]], axis=1)
        g[n, idx] += gp @ np.asarray(cam_R[i], dt).astype(np.float64)          # R^T applied to a row vector
    return dict(loss=loss, g=g, winner=winner, rho_a=rho_a)


def occluded(masks, stride, vertices, faces, image_body, cams, body_scene, margin, eval_vertices=None, **kw):
    """The whole chain: prepare -> freeze at ``vertices`` -> flags -> hidden and evaluation at ``eval_vertices`` (default: the
    frozen ones).  Returns evaluate's dict plus prep, z_occ, z_own, flags, hidden."""
    masks = np.asarray(masks)
    prep = so.prepare(masks, stride)
    H, W = masks.shape[1:]
    z_occ, z_own = freeze(vertices, faces, image_body, cams, body_scene, H, W)
    flags = point_flags(masks, prep['first'], prep['xy'], z_occ, z_own)
    ev = vertices if eval_vertices is None else eval_vertices
    hidden = hidden_bytes(ev, image_body, cams, z_occ, margin)
    r = evaluate(prep, ev, image_body, cams, hidden=hidden, flags=flags, **kw)
    r.update(prep=prep, z_occ=z_occ, z_own=z_own, flags=flags, hidden=hidden)
    return r
