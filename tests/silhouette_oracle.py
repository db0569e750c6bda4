"""TESTS ONLY - NumPy restatement of the silhouette term (include/mvfit.h:mvfit_set_silhouettes / mvfit_silhouette_loss).

Field from scipy's exact Euclidean distance transform, contour by array slicing, projection by tests/render_oracle.transform's
fp32 sequence, cell indices and winners in float32 exactly as the contract orders the operations, everything after that in
float64.  ``pure64=True`` runs the whole evaluation in float64 (for finite differences of the restatement itself)."""
import numpy as np
import torch
from scipy import ndimage

from tests import render_oracle as ro

ZNEAR = 0.05


def field(mask):
    """D[H,W] float32; zeros for a mask without an on pixel."""
    on = np.asarray(mask) != 0
    if not on.any():
        return np.zeros(on.shape, np.float32)
    return ndimage.distance_transform_edt(~on).astype(np.float32)


def field_bruteforce(mask):
    """The definition itself: integer minimum over all on pixels (small masks only)."""
    on = np.asarray(mask) != 0
    H, W = on.shape
    if not on.any():
        return np.zeros((H, W), np.float32)
    ys, xs = np.nonzero(on)
    yy, xx = np.mgrid[0:H, 0:W]
    d2 = ((yy[..., None] - ys) ** 2 + (xx[..., None] - xs) ** 2).min(axis=2)
    return np.sqrt(d2.astype(np.float64)).astype(np.float32)


def contour(mask, stride=1):
    """(x, y) int32 [C,2]: on pixels with an off 4-neighbour inside the image, raster order, every stride-th."""
    on = np.asarray(mask) != 0
    off = ~on
    nb = np.zeros_like(on)
    nb[:, 1:] |= off[:, :-1]
    nb[:, :-1] |= off[:, 1:]
    nb[1:, :] |= off[:-1, :]
    nb[:-1, :] |= off[1:, :]
    ys, xs = np.nonzero(on & nb)                       # row-major = raster order
    return np.stack([xs, ys], axis=1).astype(np.int32)[::stride]


def prepare(masks, stride=1):
    """fields [M,H,W] float32, contour_first [M+1] int32, contour_xy [C,2] int32, nonempty [M] bool."""
    masks = np.asarray(masks)
    fields = np.stack([field(m) for m in masks])
    cs = [contour(m, stride) for m in masks]
    first = np.concatenate([[0], np.cumsum([len(c) for c in cs])]).astype(np.int32)
    xy = np.concatenate(cs, axis=0) if len(cs) else np.zeros((0, 2), np.int32)
    return dict(fields=fields, first=first, xy=xy.reshape(-1, 2), nonempty=np.array([(m != 0).any() for m in masks]),
                stride=int(stride))


def _project(verts, R, t, f, c, pure64):
    if not pure64:
        return ro.transform(verts, R, t, f, c)
    v, R, t, c = (np.asarray(a, np.float64) for a in (verts, R, t, c))
    p = np.stack([((R[k, 0] * v[:, 0] + R[k, 1] * v[:, 1]) + R[k, 2] * v[:, 2]) + t[k] for k in range(3)], axis=1)
    with np.errstate(divide='ignore', invalid='ignore'):
        return p, float(f) * (p[:, 0] / p[:, 2]) + c[0], float(f) * (p[:, 1] / p[:, 2]) + c[1]


def evaluate(prep, vertices, image_body, cams, w_in=1.0, w_out=1.0, sigma=0.0, pure64=False):
    """loss [N] float64, g [N,Nv,3] float64, winner [C] int32, cells: per image (valid [Nv], x0 [Nv], y0 [Nv])."""
    dt = np.float64 if pure64 else np.float32
    V = np.asarray(vertices, dt)
    N, nv = V.shape[0], V.shape[1]
    cam_R, cam_t, cam_f, cam_c = cams
    fields, first, xy, stride = prep['fields'], prep['first'], prep['xy'], prep['stride']
    M, H, W = fields.shape
    loss = np.zeros(N)
    g = np.zeros((N, nv, 3))
    winner = np.full(len(xy), -1, np.int32)
    cells = []
    s2 = float(sigma) ** 2
    for i in range(M):                                  # ascending image index: the order of every body's sums
        n = int(image_body[i])
        p, u, w = _project(V[n], cam_R[i], cam_t[i], cam_f[i], cam_c[i], pure64)
        valid = p[:, 2] > dt(ZNEAR)
        idx = np.flatnonzero(valid)
        x0a, y0a = np.full(nv, -1), np.full(nv, -1)
        cells.append((valid, x0a, y0a))
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
        x0a[idx], y0a[idx] = x0, y0
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
        gu[idx] += w_in * drdd * ddx
        gv[idx] += w_in * drdd * ddy
        # term B
        Bsum = 0.0
        pts = xy[first[i]:first[i + 1]]
        if len(pts) and len(idx):
            uu, ww = u[idx], w[idx]
            for k0 in range(0, len(pts), 256):
                q = pts[k0:k0 + 256]
                cx, cy = q[:, 0].astype(dt) + dt(0.5), q[:, 1].astype(dt) + dt(0.5)
                dx, dy = uu[None, :] - cx[:, None], ww[None, :] - cy[:, None]
                m = dx * dx + dy * dy                   # products and sum each rounded to dt
                kk = np.argmin(m, axis=1)               # first minimum = lowest j
                rr = np.arange(len(q))
                winner[first[i] + k0:first[i] + k0 + len(q)] = idx[kk]
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
    return dict(loss=loss, g=g, winner=winner, cells=cells)


class OracleEngine:
    """CPU stand-in for MvFit's silhouette entries (the engine SilhouetteLoss drives), on the restatement."""

    def __init__(self):
        self.device = torch.device('cpu')
        self.prep = None
        self.calls = []

    def set_silhouettes(self, masks, image_body, cams, contour_stride=1):
        m = masks.cpu().numpy() if isinstance(masks, torch.Tensor) else np.asarray(masks)
        self.prep = prepare(m, contour_stride)
        self.image_body = np.asarray(image_body).reshape(-1)
        self.cams = tuple(np.asarray(a, np.float32) for a in cams)
        self.calls.append('set')

    def clear_silhouettes(self):
        self.prep = None
        self.calls.append('clear')

    def silhouette_loss(self, vertices, w_in=1.0, w_out=1.0, sigma=0.0, need_grad=True, return_winner=False):
        assert self.prep is not None, 'no mask set'
        r = evaluate(self.prep, vertices.detach().cpu().numpy(), self.image_body, self.cams, w_in, w_out, sigma)
        self.calls.append('loss')
        out = (torch.tensor(r['loss'], dtype=torch.float32), torch.tensor(r['g'], dtype=torch.float32) if need_grad else None)
        return out + (torch.tensor(r['winner']),) if return_winner else out
