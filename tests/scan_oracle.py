"""TESTS ONLY - the scan loss (include/mvfit.h:mvfit_scan_loss) restated in float64 NumPy: brute force, every point against
every face (vectorised over the faces) and every vertex against every point, loss and gradient.  The reference has no such
term; this restatement, checked against torch autograd in float64 (tests/test_scan_cpu.py), is what the GPU tests compare with.

torch_scan_loss is the same computation in torch (any dtype and device, chunked over points, differentiable by autograd): the
check of the oracle's gradient, and the baseline tools/scan_loss_timing.py times on the GPU."""
import numpy as np

REGIONS = ('a', 'b', 'ab', 'c', 'ac', 'bc', 'in')


def closest(p, a, ab, ac):
    """Closest point of triangle (a, a + ab, a + ac) to p by region (include/mvfit.h, term S), arrays broadcast over leading
    axes -> (v, w, d = q - p, m = |d|^2, region index into REGIONS)."""
    ap = p - a
    bp = ap - ab
    cp = ap - ac
    dot = lambda x, y: (x * y).sum(axis=-1)
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    e1, e2 = d4 - d3, d5 - d6
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e1 >= 0) & (e2 >= 0)]
    one, zero = np.ones_like(d1), np.zeros_like(d1)
    nv = np.select(conds, [zero, one, d1, zero, zero, e2], default=vb)
    nw = np.select(conds, [zero, zero, zero, one, d2, e1], default=vc)
    den = np.select(conds, [one, one, d1 - d3, one, d2 - d6, e1 + e2], default=va + vb + vc)
    region = np.select(conds, [0, 1, 2, 3, 4, 5], default=6)
    with np.errstate(divide='ignore', invalid='ignore'):
        v, w = nv / den, nw / den
    d = v[..., None] * ab + w[..., None] * ac - ap
    return v, w, d, (d * d).sum(axis=-1), region


def rho(m, sigma):
    """(rho(m), rho'(m))"""
    if sigma <= 0:
        return m, np.ones_like(m)
    s2 = float(sigma) ** 2
    return s2 * m / (s2 + m), (s2 / (s2 + m)) ** 2


def scan_to_mesh(points, verts, faces, rel=1e-5, absolute=1e-7, apart=1e-4, prune=True, chunk=256):
    """Per point: the winner (smallest m, ties to the lowest face), its m, (v, w), d, region - and ``ambiguous``: another
    face whose distance is within rel * best + absolute of the best and whose closest point lies more than ``apart`` from the
    best one.  A face whose m is NaN (a repeated vertex index can make it so) counts as +inf and never wins; a point whose
    every face is such has no winner: face -1, m, v, w and d zero, region -1, not ambiguous.
    prune=False evaluates every (point, face) pair.  prune=True first drops the pairs that cannot matter, in
    float64 and with room to spare: a face whose bounding sphere (centroid, largest corner distance) lies farther from the
    point than the nearest first corner of any face whose m cannot be NaN (three different indices, or three equal ones),
    widened by the ambiguity margin, is neither the winner nor near it; without such a face nothing is dropped."""
    P = len(points)
    out = dict(face=np.full(P, -1, np.int64), m=np.zeros(P), v=np.zeros(P), w=np.zeros(P), d=np.zeros((P, 3)),
               region=np.zeros(P, np.int64), ambiguous=np.zeros(P, bool))
    a = verts[faces[:, 0]]
    ab, ac = verts[faces[:, 1]] - a, verts[faces[:, 2]] - a
    cen = a + (ab + ac) / 3.0
    rad = np.sqrt(np.maximum(((a - cen) ** 2).sum(axis=1), np.maximum(((a + ab - cen) ** 2).sum(axis=1),
                                                                       ((a + ac - cen) ** 2).sum(axis=1))))
    f0, f1, f2 = faces[:, 0], faces[:, 1], faces[:, 2]
    sure = ((f0 != f1) & (f1 != f2) & (f0 != f2)) | ((f0 == f1) & (f1 == f2))
    for i0 in range(0, P, chunk):
        p = points[i0:i0 + chunk]
        if prune:
            lower = np.sqrt(((p[:, None, :] - cen[None]) ** 2).sum(axis=-1)) - rad[None]
            upper = np.sqrt(((p[:, None, :] - a[None, sure]) ** 2).sum(axis=-1)).min(axis=1, initial=np.inf)
            slack = 1e-9 * (np.abs(p).max() + np.abs(verts).max())
            pi, fi = np.nonzero(lower <= (upper * (1.0 + 2.0 * rel) + 2.0 * absolute + slack)[:, None])
        else:
            pi, fi = np.divmod(np.arange(len(p) * len(faces)), len(faces))
        v, w, d, m, region = closest(p[pi], a[fi], ab[fi], ac[fi])             # pairs sorted by (point, face)
        m = np.where(np.isnan(m), np.inf, m)
        start = np.searchsorted(pi, np.arange(len(p)))
        best_m = np.minimum.reduceat(m, start)
        hit = np.flatnonzero(m == best_m[pi])
        first = hit[np.unique(pi[hit], return_index=True)[1]]                    # the lowest face among equal m
        sl = slice(i0, i0 + len(p))
        out['face'][sl], out['m'][sl], out['v'][sl], out['w'][sl] = fi[first], m[first], v[first], w[first]
        out['d'][sl], out['region'][sl] = d[first], region[first]
        dist = np.sqrt(m)
        near = dist <= dist[first][pi] * (1.0 + rel) + absolute
        near[first] = False
        far = np.linalg.norm(d - d[first][pi], axis=-1) > apart                  # q_f - q_best = d_f - d_best
        out['ambiguous'][sl] = np.bincount(pi[near & far], minlength=len(p)) > 0
        none = i0 + np.flatnonzero(np.isinf(best_m))                             # every face's m was NaN
        out['face'][none], out['region'][none], out['ambiguous'][none] = -1, -1, False
        out['m'][none] = out['v'][none] = out['w'][none] = out['d'][none] = 0.0
    return out


def lowest_zero_face(points, verts, faces):
    """Per point the lowest face whose float64 m is exactly 0, -1 where no face has it (the winner of scan_to_mesh: the
    smallest m, ties to the lowest face - so where the smallest m is 0 the winner is that face)."""
    r = scan_to_mesh(points, verts, faces)
    return np.where((r['face'] >= 0) & (r['m'] == 0.0), r['face'], -1)


def repeated_faces(faces, copies):
    """faces repeated ``copies`` times: copy k with its corner order rotated by k mod 3, the odd copies in reverse face
    order.  Every copy is the same surface, so a point's closest point is shared by its winner's copies."""
    out = []
    for k in range(copies):
        f = np.roll(faces, -(k % 3), axis=1)
        out.append(f[::-1] if k % 2 else f)
    return np.ascontiguousarray(np.concatenate(out))


def far_points(verts, faces, k, lo=5.0, hi=50.0, tries=256, seed=0, rel=1e-5, absolute=1e-7):
    """k points between lo and hi from the mesh whose nearest feature is one vertex, by a margin the ambiguity test of
    scan_to_mesh cannot reach.  For a direction u let v be the vertex (of a face) with the largest u.x and s the gap to the
    second largest; every other point x of the surface has u.(v - x) >= s, so from p = v + t u it lies at
    sqrt(t^2 + 2 t u.(v - x) + |v - x|^2) >= t + s (as |v - x| >= u.(v - x)), while the faces at v tie at the closest
    point v itself.  Not ambiguous when s > rel t + absolute: the k directions of ``tries`` random ones with the largest s
    are taken, and t, spread geometrically over [lo, hi], is cut to s / (4 rel) where that is nearer.  -> ([k,3], s[k], t[k])"""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(tries, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    used = np.unique(faces)
    h = verts[used] @ u.T                                                        # [vertices, tries]
    top2 = np.sort(h, axis=0)[-2:]
    s = top2[1] - top2[0]
    pick = np.argsort(-s)[:k]
    t = np.minimum(lo * (hi / lo) ** (np.arange(k) / max(k - 1, 1)), s[pick] / (4.0 * rel))
    v = verts[used[h[:, pick].argmax(axis=0)]]
    return v + t[:, None] * u[pick], s[pick], t


def m_of_faces(points, verts, faces, face_idx):
    """float64 m of point i against face face_idx[i]"""
    f = faces[face_idx]
    a = verts[f[:, 0]]
    return closest(points, a, verts[f[:, 1]] - a, verts[f[:, 2]] - a)[3]


def evaluate(verts, faces, points, count, weights=None, w_s2m=1.0, w_m2s=0.0, sigma=0.0, face_override=None, found=None):
    """verts [N,Nv,3], faces [F,3], points [N,Pmax,3], count [N], weights [N,Pmax] or None, all float64 / int ->
    dict(loss [N], grad [N,Nv,3], S [N], M [N], nearest_face [N,Pmax], nearest_point [N,Nv], m_s [N,Pmax], m_m [N,Nv],
    ambiguous [N,Pmax], region [N,Pmax], part [N,Pmax] bool).  face_override [N,Pmax]: where >= 0, the gradient and loss
    of that point use this face instead of the winner (how the GPU's choice among tied faces is followed); found: the
    'found' entry of an earlier result for the same bodies and points, to skip the search."""
    verts = np.asarray(verts, np.float64)
    points = np.asarray(points, np.float64)
    N, Nv = verts.shape[:2]
    Pmax = points.shape[1]
    wt = np.ones((N, Pmax)) if weights is None else np.asarray(weights, np.float64)
    part = (np.arange(Pmax)[None, :] < np.asarray(count)[:, None]) & (wt > 0)
    out = dict(loss=np.zeros(N), grad=np.zeros((N, Nv, 3)), S=np.zeros(N), M=np.zeros(N),
               nearest_face=np.full((N, Pmax), -1, np.int64), nearest_point=np.full((N, Nv), -1, np.int64),
               m_s=np.zeros((N, Pmax)), m_m=np.zeros((N, Nv)), ambiguous=np.zeros((N, Pmax), bool),
               region=np.full((N, Pmax), -1, np.int64), part=part, found={})
    for n in range(N):
        idx = np.flatnonzero(part[n])
        if w_s2m > 0 and idx.size:
            r = found[n] if found is not None else scan_to_mesh(points[n, idx], verts[n], faces)
            out['found'][n] = r
            out['nearest_face'][n, idx], out['ambiguous'][n, idx], out['region'][n, idx] = r['face'], r['ambiguous'], r['region']
            face, v, w, d, m = r['face'], r['v'], r['w'], r['d'], r['m']
            if face_override is not None:
                ov = np.asarray(face_override)[n, idx]
                use = ov >= 0
                if use.any():
                    f = faces[ov[use]]
                    a = verts[n][f[:, 0]]
                    v2, w2, d2, m2, _ = closest(points[n, idx[use]], a, verts[n][f[:, 1]] - a, verts[n][f[:, 2]] - a)
                    face, v, w, d, m = face.copy(), v.copy(), w.copy(), d.copy(), m.copy()
                    face[use], v[use], w[use], d[use], m[use] = ov[use], v2, w2, d2, m2
            out['m_s'][n, idx] = m
            r_, dr = rho(m, sigma)
            out['S'][n] = (wt[n, idx] * r_).sum()
            k = (wt[n, idx] * dr * 2.0)[:, None] * d
            bary = np.stack([1.0 - v - w, v, w], axis=1)
            for c in range(3):
                np.add.at(out['grad'][n], faces[face, c], w_s2m * bary[:, c:c + 1] * k)
        if w_m2s > 0 and idx.size:
            best = np.concatenate([(((verts[n][j0:j0 + 512, None, :] - points[n, idx][None, :, :]) ** 2).sum(axis=-1)).argmin(axis=1)
                                   for j0 in range(0, Nv, 512)])
            diff = verts[n] - points[n, idx[best]]
            m = (diff * diff).sum(axis=-1)
            out['nearest_point'][n] = idx[best]
            out['m_m'][n] = m
            r_, dr = rho(m, sigma)
            out['M'][n] = r_.sum()
            out['grad'][n] += w_m2s * (dr * 2.0)[:, None] * diff
        out['loss'][n] = w_s2m * out['S'][n] + w_m2s * out['M'][n]
    return out


def m_bound(m, scale):
    """|m computed in fp32 - m| for coordinates up to ``scale``: each coordinate of q - p carries at most delta = 8 * 2^-24 *
    scale of rounding, so |dm| <= 2 sqrt(m) delta + delta^2 (the GPU tests' bound)."""
    delta = 8.0 * 2.0 ** -24 * scale
    return 2.0 * np.sqrt(m) * delta + delta * delta


# ------------------------------------------------------------------------------------------------------------ torch port
def torch_closest(p, a, ab, ac):
    """closest() in torch -> (d, m); differentiable in every argument"""
    import torch
    ap = p - a
    bp, cp = ap - ab, ap - ac
    dot = lambda x, y: (x * y).sum(dim=-1)
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    e1, e2 = d4 - d3, d5 - d6
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e1 >= 0) & (e2 >= 0)]
    one, zero = torch.ones_like(d1), torch.zeros_like(d1)
    nv, nw, den = vb, vc, va + vb + vc
    for cnd, a_, b_, c_ in reversed(list(zip(conds, [zero, one, d1, zero, zero, e2], [zero, zero, zero, one, d2, e1],
                                             [one, one, d1 - d3, one, d2 - d6, e1 + e2]))):
        nv, nw, den = torch.where(cnd, a_, nv), torch.where(cnd, b_, nw), torch.where(cnd, c_, den)
    den = torch.where(den == 0, torch.ones_like(den), den)
    v, w = nv / den, nw / den
    d = v[..., None] * ab + w[..., None] * ac - ap
    return d, (d * d).sum(dim=-1)


def torch_scan_loss(verts, faces, points, count, weights=None, w_s2m=1.0, w_m2s=0.0, sigma=0.0, chunk=256):
    """The loss [N] in torch on verts' device and dtype, chunked over points (term S) and vertices (term M).  The winners are
    searched without a graph, the winner's distance is recomputed with one: autograd then gives the gradient with the
    correspondences held fixed but the barycentrics free - the same thing wherever the closest point is unique."""
    import torch
    N, Nv = verts.shape[:2]
    faces = torch.as_tensor(faces, device=verts.device, dtype=torch.long)
    points = torch.as_tensor(points, device=verts.device, dtype=verts.dtype)
    s2 = float(sigma) ** 2

    def rho_t(m):
        return m if sigma <= 0 else s2 * m / (s2 + m)
    losses = []
    for n in range(N):
        cnt = int(count[n])
        wt = torch.ones(cnt, device=verts.device, dtype=verts.dtype) if weights is None else \
            torch.as_tensor(weights[n][:cnt], device=verts.device, dtype=verts.dtype)
        idx = torch.nonzero(wt > 0).reshape(-1)
        pts, wt = points[n, :cnt][idx], wt[idx]
        total = verts.new_zeros(())
        if w_s2m > 0 and len(pts):
            a = verts[n][faces[:, 0]]
            ab, ac = verts[n][faces[:, 1]] - a, verts[n][faces[:, 2]] - a
            with torch.no_grad():
                win = torch.cat([torch_closest(pts[i:i + chunk, None, :], a[None], ab[None], ac[None])[1].argmin(dim=1)
                                 for i in range(0, len(pts), chunk)])
            m = torch_closest(pts, a[win], ab[win], ac[win])[1]
            total = total + w_s2m * (wt * rho_t(m)).sum()
        if w_m2s > 0 and len(pts):
            with torch.no_grad():
                win = torch.cat([((verts[n][i:i + chunk, None, :] - pts[None]) ** 2).sum(dim=-1).argmin(dim=1)
                                 for i in range(0, Nv, chunk)])
            total = total + w_m2s * rho_t(((verts[n] - pts[win]) ** 2).sum(dim=-1)).sum()
        losses.append(total)
    return torch.stack(losses)
