"""The silhouette loss against per-view person masks as a differentiable PyTorch module, and a small driver that refines
shape and scale with it (include/mvfit.h:mvfit_set_silhouettes / mvfit_silhouette_loss; csrc/silhouette.hip).

Keypoints fix bone lengths and pose and say almost nothing about girth; masks do.  The loss has two terms per image: the
projected vertices must lie inside the mask (a bilinear sample of the mask's exact distance field) and the mask's contour
must be covered by the body (squared distance of every contour pixel to the nearest projected vertex).  It composes with the
differentiable body model:

    layer = BodyLayer(model_arrays)
    sil = SilhouetteLoss(engine=layer.engine, masks=masks, image_body=image_body, cams=(R, t, f, c))
    out = layer(betas, global_orient, body_pose, transl=transl, scale=scale)
    loss = sil(out.vertices)              # [N], one value per body
    loss.sum().backward()                 # -> betas.grad, ..., scale.grad

One autograd node maps the vertices to the loss; the forward call already computes the gradient and the node keeps it,
backward scales it by each body's incoming gradient.  Once differentiable: there is no double backward.

refine_fit runs the term inside the engine's own fit instead (include/mvfit.h:mvfit_set_silhouette_term): every parameter
the stage frees moves, the optimiser is the project's L-BFGS and no closure leaves the device.

refine_fit_occluded is refine_fit for persons that overlap in a view: the other bodies of a scene are frozen as occluder
depth maps (include/mvfit.h:mvfit_set_silhouette_occluders), and the term ignores the vertices and contour points they hide.

Not built here: label images shared between persons, a body's self-occlusion (its own mask already covers it), the joint=
folder plumbing and the service / single-launch form of the occluders, point-to-edge distances (the contour term measures the
distance to the nearest projected *vertex*; its floor is about half the projected vertex spacing).
"""
from __future__ import annotations

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from .layer import _WIDTHS


class SilhouetteFunction(torch.autograd.Function):
    """v[N,Nv,3] float32 (translation included) -> loss[N] on module's engine; backward = grad_out[body] * g_vertices."""

    @staticmethod
    def forward(ctx, v, module):
        loss, g = module.engine.silhouette_loss(v.detach(), w_in=module.w_in, w_out=module.w_out, sigma=module.sigma,
                                                need_grad=True)
        ctx.save_for_backward(g)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        g, = ctx.saved_tensors
        return grad_out.to(g.dtype)[:, None, None] * g, None


class SilhouetteLoss(torch.nn.Module):
    """masks uint8 [M,H,W] (non-zero = person), image_body[M] = which body of the batch every image shows, cams =
    (R[M,3,3], t[M,3], f[M], c[M,2]) per image.  engine: an object with MvFit's set_silhouettes / silhouette_loss and
    device (a BodyLayer's engine, or a stand-in in tests); without one the module builds an MvFit of its own on ``model``.
    The mask set lives in the engine: one SilhouetteLoss per engine at a time (``rebind()`` sets this module's masks again
    after another one used the engine).

    Pass cropped or downscaled masks, with f and c scaled to match, when full-resolution fields (5 bytes per pixel and
    image) do not fit."""

    def __init__(self, engine=None, masks=None, image_body=None, cams=None, contour_stride=1, w_in=1.0, w_out=1.0, sigma=0.0,
                 model: dict | None = None, device: int = 0):
        super().__init__()
        if engine is None:
            if model is None:
                raise ValueError('SilhouetteLoss needs engine= (an MvFit, e.g. BodyLayer(...).engine) or model=')
            from .engine import MvFit
            engine = MvFit(model, device=device)
        if masks is None or image_body is None or cams is None:
            raise ValueError('SilhouetteLoss needs masks=, image_body= and cams=')
        self.engine = engine
        self.w_in, self.w_out, self.sigma = float(w_in), float(w_out), float(sigma)
        self.contour_stride = int(contour_stride)
        self._set = (masks, np.asarray(image_body).reshape(-1).copy(), tuple(cams))
        self.rebind()

    def rebind(self):
        masks, body, cams = self._set
        self.engine.set_silhouettes(masks, body, cams, contour_stride=self.contour_stride)

    def forward(self, vertices):
        """vertices[N,Nv,3] with the translation included (what BodyLayer returns with transl=) -> loss[N]."""
        vertices = torch.as_tensor(vertices)
        if vertices.dim() != 3 or vertices.shape[2] != 3:
            raise ValueError('vertices must be [N, Nv, 3], got %r' % (tuple(vertices.shape),))
        v = vertices.to(device=self.engine.device, dtype=torch.float32)
        return SilhouetteFunction.apply(v, self)


def keypoint_term(joints, cams_fit, gt_xy, w_conf, data_weight, rho):
    """The closure's 2-D data term on joints[B,17,3], in torch: data_weight^2 * sum conf^2 * rho^2 r^2 / (r^2 + rho^2) per
    residual coordinate r over views, keypoints and (u, v) -> [B].  cams_fit = (R[V,3,3] | [B,V,3,3], t, f, c)."""
    dev, dt = joints.device, joints.dtype
    R, t, f, c = (torch.as_tensor(np.asarray(a, np.float32) if not isinstance(a, torch.Tensor) else a).to(device=dev, dtype=dt)
                  for a in cams_fit)
    if R.dim() == 3:
        R, t, f, c = R[None], t[None], f[None], c[None]
    gt = torch.as_tensor(gt_xy).to(device=dev, dtype=dt)
    w2 = torch.as_tensor(w_conf).to(device=dev, dtype=dt)[..., None] ** 2
    p = torch.einsum('bvac,bkc->bvka', R.expand(joints.shape[0], -1, -1, -1), joints) + t[:, :, None, :]
    uv = f[:, :, None, None] * p[..., :2] / p[..., 2:3] + c[:, :, None, :]
    r2 = (gt - uv) ** 2
    rho2 = float(rho) ** 2
    return (w2 * (rho2 * r2 / (r2 + rho2))).sum(dim=(1, 2, 3)) * float(data_weight) ** 2


def refine_shape(layer, params, masks, image_body, cams, *, free=('betas', 'scale'), share=None, weight, sigma, shape_weight,
                 keypoints=None, max_iter=30, contour_stride=1, w_in=1.0, w_out=1.0):
    """Refine the result of a keypoint fit against masks.

    params[B,118] (flat parameter rows, include/mvfit.h); masks / image_body / cams as SilhouetteLoss takes them (image_body
    indexes the rows of params).  free: the blocks that move ('betas', 'global_orient', 'body_pose', 'transl', 'scale').
    share: an integer group id per problem (None: every problem its own group); the problems of a group optimise ONE betas
    and ONE scale - one shape per person over all their frames - starting from the group's first row; the other free blocks
    stay per problem.  Per group the objective is

        weight * sum_b silhouette_b + shape_weight^2 |betas|^2 [+ sum_b keypoint_term_b]

    (the shape prior in the reference's form, once per group; keypoints = (cams_fit, gt_xy, w_conf, data_weight, rho) adds the
    closure's 2-D data term on the layer's joints).  All groups are minimised together by one
    torch.optim.LBFGS(line_search_fn='strong_wolfe') on the sum; a group keeps its result only if its own objective
    dropped, otherwise its rows come back exactly as they were given.

    Returns (params_out[B,118], report) with report = dict(groups, before, after, accepted, silhouette_before,
    silhouette_after: one entry per group in ascending group id; iterations: the optimiser's)."""
    names = [n for n, _ in _WIDTHS]
    free = tuple(free)
    for n in free:
        if n not in names or n == 'pose_embedding':
            raise ValueError('free block %r: one of betas, global_orient, body_pose, transl, scale' % (n,))
    dev = layer.engine.device
    x0 = torch.as_tensor(params).detach().to(device=dev, dtype=torch.float32).clone()
    B = int(x0.shape[0])
    if x0.dim() != 2 or x0.shape[1] != sum(w for _, w in _WIDTHS):
        raise ValueError('params must be [B, 118], got %r' % (tuple(x0.shape),))
    ids = np.arange(B) if share is None else np.asarray(share).reshape(-1)
    if ids.size != B:
        raise ValueError('share needs one group id per problem (%d)' % B)
    groups, inverse = np.unique(ids, return_inverse=True)
    G = len(groups)
    gi = torch.as_tensor(inverse.reshape(-1), device=dev, dtype=torch.long)
    first_row = torch.as_tensor(np.array([int(np.flatnonzero(inverse == g)[0]) for g in range(G)]), device=dev, dtype=torch.long)
    offs, o = {}, 0
    for n, w in _WIDTHS:
        offs[n] = (o, o + w)
        o += w
    shared = ('betas', 'scale')
    var = {}
    for n in free:
        a, b = offs[n]
        init = x0[first_row, a:b] if n in shared else x0[:, a:b]
        var[n] = init.clone().requires_grad_(True)

    def rows(values):
        """x[B,118] with the free blocks taken from values (shared ones expanded over their group)."""
        parts = []
        for n, _ in _WIDTHS:
            a, b = offs[n]
            if n in values:
                parts.append(values[n][gi] if n in shared else values[n])
            else:
                parts.append(x0[:, a:b])
        return parts

    sil = SilhouetteLoss(engine=layer.engine, masks=masks, image_body=image_body, cams=cams, contour_stride=contour_stride,
                         w_in=w_in, w_out=w_out, sigma=sigma)
    sw2 = float(shape_weight) ** 2

    def objective(parts):
        p = dict(zip(names, parts))
        out = layer(p['betas'], p['global_orient'], p['body_pose'], transl=p['transl'], scale=p['scale'])
        s = sil(out.vertices)
        per_body = float(weight) * s
        if keypoints is not None:
            cams_fit, gt_xy, w_conf, data_weight, rho = keypoints
            per_body = per_body + keypoint_term(out.joints, cams_fit, gt_xy, w_conf, data_weight, rho)
        zero = torch.zeros(G, device=dev, dtype=per_body.dtype)
        J = zero.index_add(0, gi, per_body) + sw2 * (p['betas'][first_row] ** 2).sum(dim=1)
        return J, zero.index_add(0, gi, s.detach())

    try:
        with torch.no_grad():
            before, sil_before = objective([x0[:, a:b] for a, b in (offs[n] for n in names)])
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
            after, sil_after = objective([x1[:, a:b] for a, b in (offs[n] for n in names)])
    finally:
        layer.engine.clear_silhouettes()
    accepted = after < before
    out = torch.where(accepted[gi][:, None], x1, x0)
    n_iter = int(opt.state[opt._params[0]].get('n_iter', 0)) if var else 0
    report = dict(groups=groups.tolist(), before=before.tolist(), after=after.tolist(), accepted=accepted.tolist(),
                  silhouette_before=sil_before.tolist(), silhouette_after=sil_after.tolist(), iterations=n_iter)
    return out, report


def refine_fit(engine, params, stage, *, w_in=1.0, w_out=1.0, sigma=0.0, **fit_kwargs):
    """One fit of the engine's B problems with the silhouette term inside the fit's rounds.

    params [B,118] (set_problems and set_silhouettes done: image_body indexes the problems); ``stage``: one weight dict with
    coll_loss_weight w > 0.  The objective of problem j is its closure loss under ``stage`` with the term on: the stage's
    keypoint and prior terms + w^2 * silhouette_loss_j.

      1. the term is switched on; one closure gives J(x_0) and the silhouette losses L(x_0);
      2. x' = engine.fit(x_0, [stage], **fit_kwargs); one closure gives J(x'), L(x');
      3. problem j keeps its row of x' iff J_j(x') < J_j(x_0); otherwise the row reverts to x_0 exactly;
      4. the engine is left with the term cleared (also when something raises); the mask set stays.

    Returns (params, report).  report: dict(before [B], after [B] = J of the returned rows, accepted [B] bool,
    silhouette_before [B], silhouette_after [B] = L of the returned rows, n_closure [B] of the fit, loss [B] = after)."""
    if float(stage.get('coll_loss_weight', 0.0)) <= 0.0:
        raise ValueError('refine_fit: the stage needs coll_loss_weight > 0')
    x0 = params if isinstance(params, torch.Tensor) else torch.as_tensor(np.asarray(params, np.float32))
    x0 = x0.to(engine.device).clone()

    def host(t):
        return np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t)

    def objective(x):
        J = engine.closure(x, stage, want_grad=False)['loss']
        return host(J).astype(np.float64), host(engine.sdf_term_read()[1]).astype(np.float64)

    engine.set_silhouette_term(w_in=w_in, w_out=w_out, sigma=sigma)
    try:
        before, sil_before = objective(x0)
        x1, st = engine.fit(x0, [stage], **fit_kwargs)
        x1 = x1.to(x0.dtype)
        after, sil_after = objective(x1)
        accepted = after < before
        for j in np.flatnonzero(~accepted):
            x1[int(j)] = x0[int(j)]
        after = np.where(accepted, after, before)
        sil_after = np.where(accepted, sil_after, sil_before)
        report = dict(before=before, after=after, accepted=accepted, silhouette_before=sil_before,
                      silhouette_after=sil_after, n_closure=host(st['n_closure']), loss=after.copy())
        return x1, report
    finally:
        engine.clear_silhouette_term()



def refine_fit_occluded(engine, params, stage, body_scene, *, margin=0.02, sweeps=2, **refine_fit_kwargs):
    """refine_fit for scenes whose persons overlap in a view: the masks are modal (a person's mask shows its visible part
    only), so the other bodies of each scene are frozen as occluder depth maps (include/mvfit.h:
    mvfit_set_silhouette_occluders) and the term ignores what they hide.

    params [B,118], ``body_scene`` [B] int: problems with the same value >= 0 occlude one another, < 0 none.  Per sweep:

      1. the occluders are frozen at the current rows' vertices (engine.vertices); after the first sweep the captured round
         graph is dropped, so that every sweep's fit runs on a graph of its own;
      2. refine_fit runs - it accepts per problem and judges before and after under the same frozen maps;
      3. a sweep that accepts nothing ends the loop.

    The engine is left without occluders (also when something raises); the mask set stays.  Returns (params, report):
    report holds the last sweep's refine_fit report (before, after, accepted, silhouette_before, silhouette_after,
    n_closure, loss - of the rows returned) and ``sweeps``: per sweep dict(accepted [B] bool, hidden [M] = hidden vertices
    per image at the frozen vertices, flagged [M] = flagged contour points per image)."""
    if int(sweeps) < 1:
        raise ValueError('refine_fit_occluded: sweeps must be >= 1')
    scene = np.asarray(body_scene).reshape(-1).astype(np.int32)
    x = params if isinstance(params, torch.Tensor) else torch.as_tensor(np.asarray(params, np.float32))
    x = x.to(engine.device).clone()
    if scene.size != int(x.shape[0]):
        raise ValueError('refine_fit_occluded: body_scene needs one entry per problem (%d), got %d' % (int(x.shape[0]), scene.size))

    def host(t):
        return np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t)

    report, done = None, []
    try:
        for sweep in range(int(sweeps)):
            verts = engine.vertices(x)[0]
            engine.set_silhouette_occluders(verts, scene, margin=margin)
            if sweep:
                # the freeze keeps the round graph valid, but a long fit that replays a graph captured before the maps changed
                # is not reproducible from engine to engine: every later sweep captures its own
                engine.round_graph_info(drop=True)
            first = host(engine.silhouettes()[1]).astype(np.int64)
            flag = host(engine.silhouette_occluders()[2]).astype(np.int64)
            csum = np.concatenate([[0], np.cumsum(flag)])
            hidden = host(engine.silhouette_hidden(verts)).astype(np.int64).sum(axis=1)
            x, report = refine_fit(engine, x, stage, **refine_fit_kwargs)
            done.append(dict(accepted=np.asarray(report['accepted']).copy(), hidden=hidden, flagged=csum[first[1:]] - csum[first[:-1]]))
            if not np.asarray(report['accepted']).any():
                break
        return x, dict(report, sweeps=done)
    finally:
        engine.clear_silhouette_occluders()
