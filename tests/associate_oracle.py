"""NumPy restatement of mvfit_associate_views (include/mvfit.h): the cost matrix with the header's operation order - every
product and sum its own float64 operation, nothing fused, so the device's bits are reproduced - and the complete-linkage
clustering with the Lance-Williams update L(A u B, X) = max(L(A, X), L(B, X)).  Shared by the CPU and the GPU tests, and
the decisive synthetic scene both use."""
import numpy as np

J = 17


def inv3(K):
    a, b, c, d, e, f, g, h, i = (np.float64(x) for x in np.asarray(K, np.float64).reshape(9))
    A, B, C = e * i - f * h, -(d * i - f * g), d * h - e * g
    det = a * A + b * B + c * C
    id_ = np.float64(1.0) / det
    return np.array([[A * id_, -(b * i - c * h) * id_, (b * f - c * e) * id_],
                     [B * id_, (a * i - c * g) * id_, -(a * f - c * d) * id_],
                     [C * id_, -(a * h - b * g) * id_, (a * e - b * d) * id_]], np.float64)


def rays(kp, intris, extris):
    """kp [V, N, 17, 3] float32 -> origins [V, 3], directions [V, N, 17, 3], confidences [V, N, 17] (float64)."""
    kp = np.asarray(kp, np.float32)
    V = kp.shape[0]
    org = np.zeros((V, 3))
    d = np.zeros(kp.shape[:3] + (3,))
    for v in range(V):
        E = np.asarray(extris[v], np.float64)
        R, t = E[:3, :3], E[:3, 3]
        for i in range(3):
            org[v, i] = -((R[0, i] * t[0] + R[1, i] * t[1]) + R[2, i] * t[2])
        Ki = inv3(intris[v])
        x, y = kp[v, :, :, 0].astype(np.float64), kp[v, :, :, 1].astype(np.float64)
        n = [Ki[r, 0] * x + Ki[r, 1] * y + Ki[r, 2] for r in range(3)]
        nn = np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
        n = [n_ / nn for n_ in n]
        for i in range(3):
            d[v, :, :, i] = (R[0, i] * n[0] + R[1, i] * n[1]) + R[2, i] * n[2]
    return org, d, kp[..., 2].astype(np.float64)


def _cross(p, q):
    return (p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0])


def cost_matrix(kp, count, intris, extris, min_joints=6):
    """One frame: kp [V, N, 17, 3], count [V] -> cost [D, D] float64, D = V * N."""
    kp = np.asarray(kp, np.float32)
    V, N = kp.shape[:2]
    D = V * N
    with np.errstate(all='ignore'):
        org, d, cf = rays(kp, intris, extris)
        cost = np.full((D, D), np.inf)
        for va in range(V):
            for vb in range(va + 1, V):
                na, nb = min(max(int(count[va]), 0), N), min(max(int(count[vb]), 0), N)
                if na == 0 or nb == 0:
                    continue
                b_ = [org[vb, i] - org[va, i] for i in range(3)]
                da = [d[va, :na, None, :, i] for i in range(3)]            # [na, 1, 17]
                db = [d[vb, None, :nb, :, i] for i in range(3)]            # [1, nb, 17]
                c = _cross(da, db)
                s2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
                skew = np.abs((b_[0] * c[0] + b_[1] * c[1]) + b_[2] * c[2]) / np.sqrt(s2)
                x = _cross(b_, da)
                par = np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) + np.zeros_like(s2)
                dist = np.where(s2 > 1e-18, skew, par)
                ca, cb = cf[va, :na, None, :], cf[vb, None, :nb, :]
                on = (ca > 0.0) & (cb > 0.0)
                w = np.sqrt(ca * cb)
                num, den = np.zeros((na, nb)), np.zeros((na, nb))
                for j in range(J):                                         # ascending j; a joint that takes no part adds nothing
                    num = np.where(on[:, :, j], num + w[:, :, j] * dist[:, :, j], num)
                    den = np.where(on[:, :, j], den + w[:, :, j], den)
                blk = np.where(on.sum(2) >= min_joints, num / den, np.inf)
                cost[va * N:va * N + na, vb * N:vb * N + nb] = blk
                cost[vb * N:vb * N + nb, va * N:va * N + na] = blk.T
    return cost


def cluster(cost, valid, max_cost, min_views):
    """cost [D, D], valid [D] bool -> (labels [D] int32, number of clusters).  A cluster lives in the slot of its smallest
    member; a dead slot's row and column are +inf."""
    L = np.array(cost, np.float64)
    D = L.shape[0]
    cl = np.where(valid, np.arange(D), -1)
    iu = np.triu_indices(D, 1)
    while True:
        vals = L[iu]
        vals = np.where(np.isnan(vals), np.inf, vals)  # a NaN never merges
        k = int(np.argmin(vals))                       # the first minimum in row-major order of the upper triangle: (A, B)
        if not vals[k] <= max_cost:
            break
        A, B = int(iu[0][k]), int(iu[1][k])
        m = np.maximum(L[A], L[B])
        L[A, :], L[:, A] = m, m
        L[B, :], L[:, B] = np.inf, np.inf
        L[A, A] = np.inf
        cl[cl == B] = A
    labels = np.full(D, -1, np.int32)
    n = 0
    for s in range(D):
        if cl[s] == s and (cl == s).sum() >= min_views:
            labels[cl == s] = n
            n += 1
    return labels, n


def associate(kp, count, intris, extris, max_cost=0.05, min_joints=6, min_views=2):
    """kp [F, V, N, 17, 3], count [F, V] -> (cost [F, D, D], labels [F, V, N] int32, num_clusters [F] int32)."""
    kp = np.asarray(kp, np.float32)
    F, V, N = kp.shape[:3]
    cost = np.stack([cost_matrix(kp[f], count[f], intris, extris, min_joints) for f in range(F)])
    labels, num = np.zeros((F, V, N), np.int32), np.zeros(F, np.int32)
    for f in range(F):
        valid = (np.arange(N)[None, :] < np.asarray(count[f])[:, None]).reshape(-1)
        lab, num[f] = cluster(cost[f], valid, max_cost, min_views)
        labels[f] = lab.reshape(V, N)
    return cost, labels, num


def camera_matrices(cams):
    """(R, t, f, c) of synthetic.make_camera_ring -> intris [V, 3, 3], extris [V, 4, 4] float64."""
    R, t, f, c = (np.asarray(a, np.float64) for a in cams)
    V = R.shape[0]
    K = np.zeros((V, 3, 3))
    K[:, 0, 0] = K[:, 1, 1] = f
    K[:, :2, 2] = c
    K[:, 2, 2] = 1.0
    E = np.tile(np.eye(4), (V, 1, 1))
    E[:, :3, :3], E[:, :3, 3] = R, t
    return K, E


def project(points, K, E):
    """points [..., 3] world -> pixels [V, ..., 2]."""
    p = np.einsum('vij,...j->v...i', E[:, :3, :3], points) + E[:, :3, 3].reshape((-1,) + (1,) * (points.ndim - 1) + (3,))
    uv = p[..., :2] / p[..., 2:3]
    return uv * K[:, 0, 0].reshape((-1,) + (1,) * (points.ndim - 1) + (1,)) + K[:, :2, 2].reshape((-1,) + (1,) * (points.ndim - 1) + (2,))


def decisive_scene(cams, seed=0, persons=3, noise_px=2.0, spacing=1.1, nmax=4):
    """The scene the default max_cost is sized on: ``persons`` skeletons of 17 points in a 0.7 x 1.7 x 0.4 m box, ``spacing``
    apart along x, seen by the camera ring with ``noise_px`` Gaussian pixel noise and confidences in [0.5, 1]; every view
    lists its detections in a shuffled order; person 1 is missing from view 2; view 1 carries one false positive of random
    pixels.  Returns dict(kp [1, V, nmax, 17, 3], count [1, V], truth [1, V, nmax]: person or -1, K, E)."""
    rng = np.random.default_rng(seed)
    K, E = camera_matrices(cams)
    V = K.shape[0]
    box = np.array([0.7, 1.7, 0.4])
    centres = np.stack([np.array([(p - (persons - 1) / 2.0) * spacing, 0.0, 0.1 * ((p % 3) - 1)]) for p in range(persons)])
    pts = centres[:, None, :] + (rng.random((persons, J, 3)) - 0.5) * box
    uv = project(pts, K, E)                                                # [V, P, 17, 2]
    kp = np.zeros((1, V, nmax, J, 3), np.float32)
    count = np.zeros((1, V), np.int32)
    truth = np.full((1, V, nmax), -1, np.int32)
    for v in range(V):
        who = [p for p in range(persons) if not (v == 2 and p == 1)]
        ent = [(p, np.concatenate([uv[v, p] + rng.normal(0, noise_px, (J, 2)), rng.uniform(0.5, 1.0, (J, 1))], 1)) for p in who]
        if v == 1:
            ent.append((-1, np.concatenate([rng.uniform([0, 0], [2048, 1536], (J, 2)), rng.uniform(0.5, 1.0, (J, 1))], 1)))
        for k, e in enumerate(rng.permutation(len(ent))):
            truth[0, v, k] = ent[e][0]
            kp[0, v, k] = ent[e][1]
        count[0, v] = len(ent)
    return dict(kp=kp, count=count, truth=truth, K=K, E=E)


def same_partition(labels, truth):
    """Do two label arrays (-1: nobody) describe the same grouping?"""
    labels, truth = np.asarray(labels).reshape(-1), np.asarray(truth).reshape(-1)
    if not np.array_equal(labels < 0, truth < 0):
        return False
    pairs = set(zip(labels[labels >= 0].tolist(), truth[truth >= 0].tolist()))
    return len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs})
