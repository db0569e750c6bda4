"""NumPy statement of the surface landmark term (include/mvfit.h: mvfit_landmark_loss), written once for a dtype: float64 is
the oracle, float32 - every product, quotient and sum in float32 - the yardstick of what float32 arithmetic costs on the same
inputs.

    p_l  = sum_k w_lk V[vid_lk]                                  (slots of weight 0 are never read)
    u    = f (R p + t)_xy / (R p + t)_z + c
    L_b  = sum_v sum_l conf^2 sum_{x,y} g(u - xy; rho) + w3d sum_l conf3^2 sum_{x,y,z} g(p - xyz; rho3d)
    g(r; s) = s^2 r^2 / (r^2 + s^2) for s > 0, r^2 for s == 0

Entries of confidence 0 are never read: they may hold NaN."""
import numpy as np


def gmof(r, s):
    """(g(r; s), dg/dr) in r's dtype."""
    dt = r.dtype.type
    r2 = r * r
    if s > 0:
        s2 = dt(s) * dt(s)
        den = r2 + s2
        return s2 * r2 / den, dt(2) * r * s2 * s2 / (den * den)
    return r2, dt(2) * r


def landmark_points(verts, vertex_ids, weights, dtype=np.float64):
    """p[B,L,3]: the slots in ascending order from 0."""
    V_ = np.asarray(verts).astype(dtype)
    ids, w = np.asarray(vertex_ids), np.asarray(weights).astype(dtype)
    p = np.zeros((V_.shape[0], ids.shape[0], 3), dtype)
    for k in range(ids.shape[1]):
        live = w[:, k] != 0
        p[:, live] = p[:, live] + w[live, k][None, :, None] * V_[:, ids[live, k]]
    return p


def project(p, cams, dtype=np.float64):
    """(q[B,V,L,3] camera-space points, u[B,V,L,2] pixels) of p[B,L,3]; cams (R, t, f, c) per view or per (problem, view)."""
    B = p.shape[0]
    R, t, f, c = (np.asarray(a).astype(dtype) for a in cams)
    f = f.reshape(R.shape[:-2])
    if R.ndim == 3:
        R, t, f, c = (np.broadcast_to(a[None], (B,) + a.shape) for a in (R, t, f, c))
    q = np.einsum('bvij,blj->bvli', R, p) + t[:, :, None, :]
    iz = dtype(1) / q[..., 2]
    u = f[:, :, None, None] * (q[..., :2] * iz[..., None]) + c[:, :, None, :]
    return R, f, q, iz, u


def landmark_loss(verts, vertex_ids, weights, cams, xy, conf, xyz=None, conf3=None, rho=100.0, w3d=0.0, rho3d=0.0,
                  dtype=np.float64, need_grad=True):
    """(loss[B], g_vertices[B,Nv,3] or None), both in ``dtype``."""
    dt = np.dtype(dtype).type
    V_ = np.asarray(verts).astype(dtype)
    B, Nv, _ = V_.shape
    ids, w = np.asarray(vertex_ids), np.asarray(weights).astype(dtype)
    L = ids.shape[0]
    p = landmark_points(V_, ids, w, dtype)
    R, f, q, iz, u = project(p, cams, dt)
    cf = np.asarray(conf).astype(dtype)
    live = cf > 0
    r = u - np.where(live[..., None], np.asarray(xy), 0).astype(dtype)
    val, der = gmof(r, rho)
    c2 = cf * cf
    loss = np.where(live, c2 * (val[..., 0] + val[..., 1]), dt(0)).reshape(B, -1).sum(axis=1, dtype=dtype)
    gu = np.where(live[..., None], c2[..., None] * der, dt(0))                  # [B,V,L,2]
    fz = f[:, :, None] * iz
    gq = np.stack([fz * gu[..., 0], fz * gu[..., 1], -fz * iz * (gu[..., 0] * q[..., 0] + gu[..., 1] * q[..., 1])], axis=-1)
    gp = np.zeros((B, L, 3), dtype)
    for v in range(gq.shape[1]):                                                # the views in ascending order
        gp = gp + np.einsum('bji,blj->bli', R[:, v], gq[:, v])
    if xyz is not None:
        c3 = np.asarray(conf3).astype(dtype)
        live3 = c3 > 0
        r3 = p - np.where(live3[..., None], np.asarray(xyz), 0).astype(dtype)
        val3, der3 = gmof(r3, rho3d)
        k3 = dt(w3d) * (c3 * c3)
        loss = loss + np.where(live3, k3 * ((val3[..., 0] + val3[..., 1]) + val3[..., 2]), dt(0)).sum(axis=1, dtype=dtype)
        gp = gp + np.where(live3[..., None], k3[..., None] * der3, dt(0))
    if not need_grad:
        return loss, None
    g = np.zeros((B, Nv, 3), dtype)
    for l in range(L):                                                          # (landmark, slot) in ascending order
        for k in range(ids.shape[1]):
            if w[l, k] != 0:
                g[:, ids[l, k]] += w[l, k] * gp[:, l]
    return loss, g
