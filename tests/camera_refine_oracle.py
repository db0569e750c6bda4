"""NumPy float64 restatement of mvfit_camera_normal_eqs and mvfit_refine_cameras (include/mvfit.h): the keypoint data term of
one view as a function of its camera, with gradient and Gauss-Newton matrix, the step of the local parametrisation and the
Levenberg-Marquardt loop.  The residual rows are summed one after the other (cumsum), in ascending order of the points or, with
reverse=True, in descending order: the difference between the two is the oracle's own rounding, the measure the GPU tests take
their tolerance from.  Shared by the CPU and the GPU tests and by tools/camera_refine_timing.py."""
import numpy as np

J = 17
FREE = {'extrinsics': 3, 'extrinsics+focal': 7, 'all': 15}
GROUP = (0, 0, 0, 1, 1, 1, 2, 3, 3)                       # bit of free_mask per parameter


def free_list(free_mask):
    return [i for i in range(9) if (free_mask >> GROUP[i]) & 1]


def pack(R, t, f, c):
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3),
                           [np.float64(f)], np.asarray(c, np.float64).reshape(2)])


def jacobian(cam, X):
    """Rows of u and v over (omega, dt, f, cx, cy) for the points X [N,3] with pz > 1e-6: (p [N,3], Ju [N,9], Jv [N,9])."""
    R, t, f = cam[:9].reshape(3, 3), cam[9:12], cam[12]
    p = np.stack([((R[r, 0] * X[:, 0] + R[r, 1] * X[:, 1]) + R[r, 2] * X[:, 2]) + t[r] for r in range(3)], 1)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    a, b = px / pz, py / pz
    du = np.stack([f / pz, 0 * pz, -f * a / pz], 1)
    dv = np.stack([0 * pz, f / pz, -f * b / pz], 1)
    z = 0 * pz
    dpdw = np.stack([np.stack([z, pz, -py], 1), np.stack([-pz, z, px], 1), np.stack([py, -px, z], 1)], 1)   # [N,3(p),3(omega)]
    Ju = np.concatenate([np.einsum('np,npw->nw', du, dpdw), du, a[:, None], 1 + z[:, None], z[:, None]], 1)
    Jv = np.concatenate([np.einsum('np,npw->nw', dv, dpdw), dv, b[:, None], z[:, None], 1 + z[:, None]], 1)
    return p, Ju, Jv


def normal_eqs(joints, gt_xy, w_conf, cam, rho=100.0, data_weight=1.0, reverse=False, need_grad=True):
    """One view: joints [B,17,3], gt_xy [B,17,2], w_conf [B,17] (float32 values), cam [15].  Returns (E, g [9], H [9,9], count);
    a view with a counted point at pz <= 1e-6 has E = +inf and g, H of NaN."""
    cam = np.asarray(cam, np.float64)
    X = np.asarray(joints, np.float32).astype(np.float64).reshape(-1, 3)
    w = np.asarray(w_conf, np.float32).astype(np.float64).reshape(-1)
    g_ = np.asarray(gt_xy, np.float32).astype(np.float64).reshape(-1, 2)
    keep = w != 0.0
    count = int(keep.sum())
    X, w, g_ = X[keep], w[keep], g_[keep]
    nan9 = np.full(9, np.nan), np.full((9, 9), np.nan)
    if count == 0:
        return 0.0, np.zeros(9), np.zeros((9, 9)), 0
    p, Ju, Jv = jacobian(cam, X)
    if np.any(~(p[:, 2] > 1e-6)):
        return np.inf, nan9[0], nan9[1], count
    f, c = cam[12], cam[13:15]
    rho2 = np.float64(rho) ** 2
    k = (np.float64(data_weight) ** 2) * (w * w)
    uv = f * (p[:, :2] / p[:, 2:3]) + c
    r = (g_ - uv).reshape(-1)                                                   # rows: u, v of point 0, u, v of point 1, ...
    k2 = np.repeat(k, 2)
    Jr = np.stack([Ju, Jv], 1).reshape(-1, 9)
    r2 = r * r
    e = k2 * (rho2 * r2 / (r2 + rho2))
    s = 2.0 * k2 * (rho2 * rho2 / (r2 + rho2) ** 2)
    if reverse:
        e, s, r, Jr = e[::-1], s[::-1], r[::-1], Jr[::-1]
    E = float(np.cumsum(e)[-1])
    if not need_grad:
        return E, None, None, count
    g = -np.cumsum((s * r)[:, None] * Jr, 0)[-1]
    H = np.cumsum(s[:, None, None] * (Jr[:, :, None] * Jr[:, None, :]), 0)[-1]
    return E, g, H, count


def rodrigues(w):
    w = np.asarray(w, np.float64)
    t2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    A, B = 1.0, 0.5
    if t2 >= 1e-24:
        t = np.sqrt(t2)
        A, B = np.sin(t) / t, (1.0 - np.cos(t)) / t2
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + A * K + B * (np.outer(w, w) - t2 * np.eye(3))


def step(cam, d):
    """theta' = step(theta, d), d over all 9 parameters: R' = exp([omega]x) R, t' = exp([omega]x) t + dt, f' = f + df, c' = c + dc."""
    cam, d = np.asarray(cam, np.float64), np.asarray(d, np.float64)
    Ex = rodrigues(d[:3])
    out = cam.copy()
    out[:9] = (Ex @ cam[:9].reshape(3, 3)).reshape(9)
    out[9:12] = Ex @ cam[9:12] + d[3:6]
    out[12:] = cam[12:] + d[6:]
    return out


def cholesky_solve(A, b):
    """x with A x = b by the Cholesky factorisation, or None at a pivot that is not > 0."""
    n = A.shape[0]
    L = np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1):
            s = A[i, j]
            for k in range(j):
                s -= L[i, k] * L[j, k]
            if i == j:
                if not s > 0.0:
                    return None
                L[i, i] = np.sqrt(s)
            else:
                L[i, j] = s / L[j, j]
    y = np.zeros(n)
    for i in range(n):
        s = b[i]
        for k in range(i):
            s -= L[i, k] * y[k]
        y[i] = s / L[i, i]
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        s = y[i]
        for k in range(i + 1, n):
            s -= L[k, i] * x[k]
        x[i] = s / L[i, i]
    return x


def lm(joints, gt_xy, w_conf, cam, free_mask=3, fixed=False, max_iter=20, min_points=34, rho=100.0, data_weight=1.0,
       lambda0=1e-3, ftol=1e-12, reverse=False, decisions=None):
    """The loop of mvfit_refine_cameras for one view.  Returns (cam_out [15], report [8]); ``decisions`` (a list) receives
    (E, E') of every accept / reject comparison."""
    cam = np.asarray(cam, np.float64).copy()
    ev = lambda c_: normal_eqs(joints, gt_xy, w_conf, c_, rho, data_weight, reverse)
    E, g, H, count = ev(cam)
    E0, lam, it, acc, status = E, np.float64(lambda0), 0, 0, -1
    if fixed:
        status = 3
    elif count < min_points:
        status = 4
    elif E == np.inf:
        status = 5
    fr = free_list(free_mask)
    while status < 0:
        if it == max_iter:
            status = 1
            break
        it += 1
        A = H[np.ix_(fr, fr)].copy()
        A[np.diag_indices(len(fr))] *= (1.0 + lam)
        x = cholesky_solve(A, -g[fr])
        if x is None:
            lam *= 10.0
            continue
        d = np.zeros(9)
        d[fr] = x
        cand = step(cam, d)
        E2, g2, H2, _ = ev(cand)
        if decisions is not None:
            decisions.append((E, E2))
        if E2 < E:
            dec = E - E2
            cam, E, g, H = cand, E2, g2, H2
            lam = max(lam / 10.0, 1e-9)
            acc += 1
            if dec <= ftol * max(E, 1.0):
                status = 0
        else:
            lam *= 10.0
            if lam > 1e12:
                status = 2
    return cam, np.array([E0, E, it, acc, status, count, lam, 0.0])


def decision_margin(decisions):
    """The smallest relative distance |E' - E| / max(E, E', tiny) over the recorded comparisons (inf when none; a behind
    candidate, E' = inf, is as far as can be)."""
    m = np.inf
    for E, E2 in decisions:
        if np.isfinite(E2):
            m = min(m, abs(E2 - E) / max(abs(E), abs(E2), 1e-300))
    return m


def look_at(pos, target=(0.0, 0.0, 0.0)):
    """World-to-camera rotation of a camera at pos looking at target, y down."""
    pos, target = np.asarray(pos, np.float64), np.asarray(target, np.float64)
    z = target - pos
    z /= np.linalg.norm(z)
    x = np.cross(np.array([0.0, -1.0, 0.0]), z)
    if np.linalg.norm(x) < 1e-9:
        x = np.array([1.0, 0.0, 0.0])
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.stack([x, y, z])


def make_case(B, V, seed, noise=0.0, zero_frac=0.1, f=1500.0, dist=3.5, rot_deg=2.5, shift=0.07):
    """Random bodies' keypoints in front of a ring of V cameras dist metres away: (joints [B,17,3] f32, gt [B,V,17,2] f32,
    w [B,V,17] f32, true cams [V,15], perturbed start cams [V,15]).  gt are the exact float32 pixels of the true cameras plus
    ``noise`` px; zero_frac of the weights are 0."""
    rng = np.random.default_rng(seed)
    joints = ((rng.random((B, J, 3)) - 0.5) * [1.2, 1.7, 0.8]).astype(np.float32)
    true = np.zeros((V, 15))
    start = np.zeros((V, 15))
    for v in range(V):
        ang = 2 * np.pi * v / max(V, 1) + 0.3
        pos = np.array([dist * np.sin(ang), 0.2 * np.cos(3 * ang), dist * np.cos(ang)])
        R = look_at(pos)
        true[v] = pack(R, -R @ pos, f, (960.0, 540.0))
        ax = rng.normal(size=3)
        ax *= np.deg2rad(rot_deg) / np.linalg.norm(ax)
        sh = rng.normal(size=3)
        sh *= shift / np.linalg.norm(sh)
        start[v] = step(true[v], np.concatenate([ax, sh, np.zeros(3)]))
    X = joints.astype(np.float64).reshape(-1, 3)
    gt = np.zeros((B, V, J, 2), np.float32)
    for v in range(V):
        R, t = true[v, :9].reshape(3, 3), true[v, 9:12]
        p = X @ R.T + t
        uv = f * p[:, :2] / p[:, 2:3] + true[v, 13:15]
        gt[:, v] = (uv + noise * rng.normal(size=uv.shape)).reshape(B, J, 2).astype(np.float32)
    w = rng.uniform(0.2, 1.0, (B, V, J)).astype(np.float32)
    w[rng.random((B, V, J)) < zero_frac] = 0.0
    return joints, gt, w, true, start


def rot_angle(Ra, Rb):
    """Angle of Ra Rb^T in radians."""
    M = np.asarray(Ra).reshape(3, 3) @ np.asarray(Rb).reshape(3, 3).T
    s = np.linalg.norm([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]]) / 2
    return float(np.arctan2(s, (np.trace(M) - 1) / 2))
