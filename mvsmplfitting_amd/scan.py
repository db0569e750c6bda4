"""The scan loss - measured 3-D surface points against the posed body and back - as a differentiable PyTorch module, depth maps
turned into such points, and two drivers that refine a fit with it: refine_to_scan (a torch L-BFGS on shape, scale and
translation) and refine_fit (the term inside the engine's own fit rounds, moving pose, shape and translation together with the
keypoint term and the priors) (include/mvfit.h:mvfit_set_scans / mvfit_scan_loss / mvfit_set_scan_term; csrc/scan_loss.hip).

Keypoints leave limb girth and the body's depth along the viewing rays almost free; a depth camera, a multi-view-stereo point
cloud or a registered scan pins both down.  A scan has no correspondences with the model, so the loss searches them at every
evaluation: every scan point against the nearest point of the body's surface (exact point-triangle distance over all faces),
and - optionally - every vertex against its nearest scan point.  It composes with the differentiable body model:

    layer = BodyLayer(model_arrays)
    scan = ScanLoss(engine=layer.engine, points=points, count=count)      # points [N,Pmax,3] in world coordinates
    out = layer(betas, global_orient, body_pose, transl=transl, scale=scale)
    loss = scan(out.vertices)             # [N], one value per body
    loss.sum().backward()                 # -> betas.grad, ..., scale.grad

One autograd node maps the vertices to the loss; the forward call already computes the gradient and the node keeps it,
backward scales it by each body's incoming gradient.  Once differentiable: there is no double backward.

Distances are in the unit of the vertices (metres for SMPL), sigma is in that unit, the loss in its square.

Not built here: a share for the term in the term mix, a scans= option of the folder driver, normals (a point pulls the nearest
surface whichever way it faces).
"""
from __future__ import annotations

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from .layer import _WIDTHS


class ScanFunction(torch.autograd.Function):
    """v[N,Nv,3] float32 (translation included) -> loss[N] on module's engine; backward = grad_out[body] * g_vertices."""

    @staticmethod
    def forward(ctx, v, module):
        loss, g = module.engine.scan_loss(v.detach(), w_s2m=module.w_s2m, w_m2s=module.w_m2s, sigma=module.sigma, need_grad=True)
        ctx.save_for_backward(g)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        g, = ctx.saved_tensors
        return grad_out.to(g.dtype)[:, None, None] * g, None


class ScanLoss(torch.nn.Module):
    """points [N,Pmax,3] world points per body (tensor or array), count[N] = how many rows of a body are points (None: all),
    weights [N,Pmax] >= 0 (None: 1).  engine: an object with MvFit's set_scans / scan_loss and device (a BodyLayer's engine, or
    a stand-in in tests); without one the module builds an MvFit of its own on ``model``.  The scan set lives in the engine:
    one ScanLoss per engine at a time (``rebind()`` sets this module's scans again after another one used the engine).

    w_s2m weighs scan-to-mesh (every point to the nearest surface point), w_m2s mesh-to-scan (every vertex to the nearest
    point; use it only with scans that cover the whole body), sigma > 0 makes both robust against outliers."""

    def __init__(self, engine=None, points=None, count=None, weights=None, w_s2m=1.0, w_m2s=0.0, sigma=0.0,
                 model: dict | None = None, device: int = 0):
        super().__init__()
        if engine is None:
            if model is None:
                raise ValueError('ScanLoss needs engine= (an MvFit, e.g. BodyLayer(...).engine) or model=')
            from .engine import MvFit
            engine = MvFit(model, device=device)
        if points is None:
            raise ValueError('ScanLoss needs points=')
        shape = tuple(points.shape)
        if len(shape) != 3 or shape[2] != 3:
            raise ValueError('points must be [N, Pmax, 3], got %r' % (shape,))
        if count is not None:
            count = np.asarray(count).reshape(-1).astype(np.int64)
            if count.size != shape[0] or (count < 0).any() or (count > shape[1]).any():
                raise ValueError('count needs one entry in [0, %d] per body (%d), got %r' % (shape[1], shape[0], count.tolist()))
        if weights is not None and tuple(weights.shape) != shape[:2]:
            raise ValueError('weights must be [%d, %d], got %r' % (shape[0], shape[1], tuple(weights.shape)))
        for name, val in (('w_s2m', w_s2m), ('w_m2s', w_m2s), ('sigma', sigma)):
            if not np.isfinite(val) or val < 0:
                raise ValueError('%s = %r must be finite and >= 0' % (name, val))
        self.engine = engine
        self.w_s2m, self.w_m2s, self.sigma = float(w_s2m), float(w_m2s), float(sigma)
        self.num_bodies = int(shape[0])
        self._set = (points, count, weights)
        self.rebind()

    def rebind(self):
        points, count, weights = self._set
        self.engine.set_scans(points, count=count, weights=weights)

    def forward(self, vertices):
        """vertices[N,Nv,3] with the translation included (what BodyLayer returns with transl=) -> loss[N]."""
        vertices = torch.as_tensor(vertices)
        if vertices.dim() != 3 or vertices.shape[2] != 3:
            raise ValueError('vertices must be [N, Nv, 3], got %r' % (tuple(vertices.shape),))
        if int(vertices.shape[0]) != self.num_bodies:
            raise ValueError('vertices hold %d bodies, the scan set %d' % (int(vertices.shape[0]), self.num_bodies))
        v = vertices.to(device=self.engine.device, dtype=torch.float32)
        return ScanFunction.apply(v, self)


def points_from_depth(depth, cams, mask=None, stride=1, max_points=None):
    """Unproject depth maps into world points [P,3] float32 (NumPy).

    depth [V,H,W]: the camera-space z of what pixel (x, y) of view v sees at its centre (x + .5, y + .5) - the rasteriser's
    pixel convention; cams = (R[V,3,3], t[V,3], f[V], c[V,2]) with the project's pinhole model p = R X + t, u = f px / pz + cx.
    A pixel is kept iff its depth is finite and > 0, its mask[V,H,W] entry (when given) is non-zero and both its coordinates
    are multiples of ``stride``.  The points come view by view in raster order; with more than ``max_points`` of them, an
    evenly spaced subset of that size is returned."""
    d = depth.detach().cpu().numpy() if isinstance(depth, torch.Tensor) else np.asarray(depth)
    if d.ndim != 3:
        raise ValueError('depth must be [V, H, W], got %r' % (d.shape,))
    V, H, W = d.shape
    R, t, f, c = (np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, np.float64) for a in cams)
    f = f.reshape(-1)
    if R.shape != (V, 3, 3) or t.shape != (V, 3) or f.shape != (V,) or c.shape != (V, 2):
        raise ValueError('cams need one entry per view (%d)' % V)
    stride = int(stride)
    if stride < 1:
        raise ValueError('stride %d < 1' % stride)
    d = d.astype(np.float64)
    keep = np.isfinite(d) & (d > 0)
    if mask is not None:
        m = mask.detach().cpu().numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask)
        if m.shape != d.shape:
            raise ValueError('mask must be %r like depth, got %r' % (d.shape, m.shape))
        keep &= m != 0
    grid = np.zeros((H, W), bool)
    grid[::stride, ::stride] = True
    keep &= grid[None]
    out = []
    for v in range(V):
        ys, xs = np.nonzero(keep[v])
        z = d[v, ys, xs]
        p = np.stack([(xs + 0.5 - c[v, 0]) * z / f[v], (ys + 0.5 - c[v, 1]) * z / f[v], z], axis=1)
        out.append((p - t[v]) @ R[v])            # R^T (p - t), row-wise
    pts = np.concatenate(out, axis=0) if out else np.zeros((0, 3))
    if max_points is not None and len(pts) > int(max_points):
        pts = pts[np.floor(np.arange(int(max_points)) * (len(pts) / float(max_points))).astype(np.int64)]
    return np.ascontiguousarray(pts, dtype=np.float32)


def refine_to_scan(layer, params, points, count=None, weights=None, *, free=('betas', 'scale', 'transl'), weight, sigma,
                   shape_weight, max_iter=30, w_s2m=1.0, w_m2s=0.0):
    """Refine the result of a keypoint fit against scans.

    params[B,118] (flat parameter rows, include/mvfit.h); points / count / weights as ScanLoss takes them (body n of the scan
    set is row n of params).  free: the blocks that move ('betas', 'global_orient', 'body_pose', 'transl', 'scale').  Per body
    the objective is

        weight * scan_loss_b + shape_weight^2 |betas_b|^2

    (the shape prior in the reference's form).  All bodies are minimised together by one
    torch.optim.LBFGS(line_search_fn='strong_wolfe') on the sum; a body keeps its result only if its own objective dropped,
    otherwise its row comes back exactly as it was given.

    Returns (params_out[B,118], report) with report = dict(before, after, accepted, scan_before, scan_after: one entry per
    body; iterations: the optimiser's)."""
    names = [n for n, _ in _WIDTHS]
    free = tuple(free)
    for n in free:
        if n not in names or n == 'pose_embedding':
            raise ValueError('free block %r: one of betas, global_orient, body_pose, transl, scale' % (n,))
    dev = layer.engine.device
    x0 = torch.as_tensor(params).detach().to(device=dev, dtype=torch.float32).clone()
    if x0.dim() != 2 or x0.shape[1] != sum(w for _, w in _WIDTHS):
        raise ValueError('params must be [B, 118], got %r' % (tuple(x0.shape),))
    offs, o = {}, 0
    for n, w in _WIDTHS:
        offs[n] = (o, o + w)
        o += w
    var = {n: x0[:, offs[n][0]:offs[n][1]].clone().requires_grad_(True) for n in free}

    def rows(values):
        return [values[n] if n in values else x0[:, offs[n][0]:offs[n][1]] for n in names]

    scan = ScanLoss(engine=layer.engine, points=points, count=count, weights=weights, w_s2m=w_s2m, w_m2s=w_m2s, sigma=sigma)
    sw2 = float(shape_weight) ** 2

    def objective(parts):
        p = dict(zip(names, parts))
        out = layer(p['betas'], p['global_orient'], p['body_pose'], transl=p['transl'], scale=p['scale'])
        s = scan(out.vertices)
        return float(weight) * s + sw2 * (p['betas'] ** 2).sum(dim=1), s.detach()

    try:
        with torch.no_grad():
            before, scan_before = objective(rows({}))
        opt = torch.optim.LBFGS(list(var.values()), max_iter=int(max_iter), line_search_fn='strong_wolfe')

        def closure():
            opt.zero_grad()
            J, _ = objective(rows(var))
            total = J.sum()
            total.backward()
            return total
        if var:
            opt.step(closure)
        with torch.no_grad():
            x1 = torch.cat(rows({n: v.detach() for n, v in var.items()}), dim=1)
            after, scan_after = objective([x1[:, a:b] for a, b in (offs[n] for n in names)])
    finally:
        layer.engine.clear_scans()
    accepted = after < before
    out = torch.where(accepted[:, None], x1, x0)
    n_iter = int(opt.state[opt._params[0]].get('n_iter', 0)) if var else 0
    report = dict(before=before.tolist(), after=after.tolist(), accepted=accepted.tolist(), scan_before=scan_before.tolist(),
                  scan_after=scan_after.tolist(), iterations=n_iter)
    return out, report


def refine_fit(engine, params, stage, *, w_s2m=1.0, w_m2s=0.0, sigma=0.0, **fit_kwargs):
    """One fit of the engine's B problems with the scan term inside the fit's rounds.

    params [B,118] (set_problems and set_scans done: scan body j is problem j); ``stage``: one weight dict with
    coll_loss_weight w > 0.  The objective of problem j is its closure loss under ``stage`` with the term on: the stage's
    keypoint and prior terms + w^2 * scan_loss_j(w_s2m, w_m2s, sigma).

      1. the term is switched on; one closure gives J(x_0) and the scan losses L(x_0);
      2. x' = engine.fit(x_0, [stage], **fit_kwargs); one closure gives J(x'), L(x');
      3. problem j keeps its row of x' iff J_j(x') < J_j(x_0); otherwise the row reverts to x_0 exactly;
      4. the engine is left with the term cleared (also when something raises); the scan set stays.

    Returns (params, report).  report: dict(before [B], after [B] = J of the returned rows, accepted [B] bool,
    scan_before [B], scan_after [B] = L of the returned rows, n_closure [B] of the fit, loss [B] = after)."""
    if float(stage.get('coll_loss_weight', 0.0)) <= 0.0:
        raise ValueError('refine_fit: the stage needs coll_loss_weight > 0')
    x0 = params if isinstance(params, torch.Tensor) else torch.as_tensor(np.asarray(params, np.float32))
    x0 = x0.to(engine.device).clone()

    def host(t):
        return np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t)

    def objective(x):
        J = engine.closure(x, stage, want_grad=False)['loss']
        return host(J).astype(np.float64), host(engine.sdf_term_read()[1]).astype(np.float64)

    engine.set_scan_term(w_s2m=w_s2m, w_m2s=w_m2s, sigma=sigma)
    try:
        before, scan_before = objective(x0)
        x1, st = engine.fit(x0, [stage], **fit_kwargs)
        x1 = x1.to(x0.dtype)
        after, scan_after = objective(x1)
        accepted = after < before
        for j in np.flatnonzero(~accepted):
            x1[int(j)] = x0[int(j)]
        after = np.where(accepted, after, before)
        scan_after = np.where(accepted, scan_after, scan_before)
        report = dict(before=before, after=after, accepted=accepted, scan_before=scan_before, scan_after=scan_after,
                      n_closure=host(st['n_closure']), loss=after.copy())
        return x1, report
    finally:
        engine.clear_scan_term()
