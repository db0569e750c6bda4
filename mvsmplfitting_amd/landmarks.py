"""The surface landmark term - named points of the body's surface against the pixels they were seen at, or against measured
3-D positions - as a differentiable PyTorch module, the table file that names the points, and refine_fit, which runs the term
inside the engine's own fit rounds (include/mvfit.h:mvfit_set_landmarks / mvfit_set_landmark_targets / mvfit_landmark_loss /
mvfit_set_landmark_term; csrc/landmark.hip).

COCO-17 ends at the ankles: nothing in the keypoint term constrains the ankles' rotation or the direction of the feet.  A
whole-body detector (AlphaPose Halpe-26: both big toes, small toes and heels in rows 20-25 of ``pose_keypoints_2d``), optical
markers or manual correspondences say where a point of the SURFACE is; a landmark table maps each of them to an affine
combination of up to four vertices.  It composes with the differentiable body model:

    layer = BodyLayer(model_arrays)
    layer.engine.set_problems(cams, gt_xy, conf)                # the term projects with the problems' cameras
    lm = LandmarkLoss(engine=layer.engine, table=load_table(path), xy=xy, conf=conf)       # xy [B,V,L,2], conf [B,V,L]
    out = layer(betas, global_orient, body_pose, transl=transl, scale=scale)
    loss = lm(out.vertices)               # [B], one value per problem
    loss.sum().backward()

One autograd node maps the vertices to the loss; the forward call already computes the gradient and the node keeps it.  Once
differentiable.  rho is in pixels, rho3d in the unit of the vertices.

Not built here: a share for the term in the term mix (and so inside fit_folder's joint=), a pull-back that visits only the
touched vertices, landmarks offset along the surface normal, the term in the single-launch optimiser kernel, is_seq.
"""
from __future__ import annotations

import json

import numpy as np
import torch
from torch.autograd.function import once_differentiable

NNZ = 4                       # MVFIT_LANDMARK_NNZ
LANDMARKS_MAX = 256           # MVFIT_LANDMARKS_MAX


def load_table(path_or_dict):
    """A landmark table: dict(names [L] str, keypoint_index [L] int64 - the row of ``pose_keypoints_2d`` that feeds each
    landmark, or -1 -, vertex_ids [L,4] int32, weights [L,4] float32) from a JSON file or a dict with the same keys:

        {"names": [...], "keypoint_index": [...], "vertex_ids": [[...], ...], "weights": [[...], ...]}

    A landmark lists 1 to 4 vertices; shorter rows are filled with dead slots (weight 0).  ``weights`` may be left out when
    every landmark is one vertex (weight 1); ``keypoint_index`` and ``names`` may be left out too.  ValueError for anything else."""
    if isinstance(path_or_dict, dict):
        d, where = path_or_dict, 'landmark table'
    else:
        with open(path_or_dict) as f:
            d = json.load(f)
        where = str(path_or_dict)
    if not isinstance(d, dict) or 'vertex_ids' not in d:
        raise ValueError("%s: a dict with at least 'vertex_ids'" % where)
    unknown = set(d) - {'names', 'keypoint_index', 'vertex_ids', 'weights'}
    if unknown:
        raise ValueError('%s: unknown keys %s' % (where, sorted(unknown)))
    rows = [list(r) if isinstance(r, (list, tuple, np.ndarray)) else [r] for r in d['vertex_ids']]
    L = len(rows)
    if not 1 <= L <= LANDMARKS_MAX:
        raise ValueError('%s: %d landmarks, outside [1, %d]' % (where, L, LANDMARKS_MAX))
    if any(not 1 <= len(r) <= NNZ for r in rows):
        raise ValueError('%s: every landmark names 1 to %d vertices' % (where, NNZ))
    if d.get('weights') is None:
        if any(len(r) != 1 for r in rows):
            raise ValueError('%s: weights are needed when a landmark names more than one vertex' % where)
        wrows = [[1.0] for _ in rows]
    else:
        wrows = [list(r) if isinstance(r, (list, tuple, np.ndarray)) else [r] for r in d['weights']]
        if len(wrows) != L or any(len(a) != len(b) for a, b in zip(rows, wrows)):
            raise ValueError('%s: weights must have the shape of vertex_ids' % where)
    ids, w = np.zeros((L, NNZ), np.int32), np.zeros((L, NNZ), np.float32)
    for l, (a, b) in enumerate(zip(rows, wrows)):
        ids[l, :len(a)], w[l, :len(b)] = a, b
    if not np.isfinite(w).all():
        raise ValueError('%s: weights must be finite' % where)
    if (ids[w != 0] < 0).any():
        raise ValueError('%s: negative vertex id' % where)
    names = [str(n) for n in d.get('names', ['landmark_%d' % l for l in range(L)])]
    kpi = np.asarray(d.get('keypoint_index', [-1] * L), np.int64).reshape(-1)
    if len(names) != L or kpi.size != L:
        raise ValueError('%s: names and keypoint_index need one entry per landmark (%d)' % (where, L))
    return dict(names=names, keypoint_index=kpi, vertex_ids=ids, weights=w)


def targets_from_people(rows_per_problem, num_landmarks):
    """Stack per-view rows into the term's targets: rows_per_problem[n][v] is the [L,3] (x, y, confidence) array of problem n
    in view v, or None where the view does not list the problem -> (xy [N,V,L,2], conf [N,V,L]) float32.  Missing views and
    entries of confidence 0 get confidence 0 and NaN coordinates (they are never read)."""
    N = len(rows_per_problem)
    V = len(rows_per_problem[0]) if N else 0
    L = int(num_landmarks)
    xy = np.full((N, V, L, 2), np.nan, np.float32)
    conf = np.zeros((N, V, L), np.float32)
    for n, views in enumerate(rows_per_problem):
        if len(views) != V:
            raise ValueError('problem %d lists %d views, problem 0 lists %d' % (n, len(views), V))
        for v, a in enumerate(views):
            if a is None:
                continue
            a = np.asarray(a, np.float32)
            if a.shape != (L, 3):
                raise ValueError('problem %d, view %d: rows of shape %r, not (%d, 3)' % (n, v, a.shape, L))
            ok = np.isfinite(a).all(axis=1) & (a[:, 2] > 0)
            xy[n, v, ok] = a[ok, :2]
            conf[n, v, ok] = a[ok, 2]
    return xy, conf


class LandmarkFunction(torch.autograd.Function):
    """v[B,Nv,3] float32 (translation included) -> loss[B] on module's engine; backward = grad_out[problem] * g_vertices."""

    @staticmethod
    def forward(ctx, v, module):
        loss, g = module.engine.landmark_loss(v.detach(), rho=module.rho, w3d=module.w3d, rho3d=module.rho3d, need_grad=True)
        ctx.save_for_backward(g)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        g, = ctx.saved_tensors
        return grad_out.to(g.dtype)[:, None, None] * g, None


class LandmarkLoss(torch.nn.Module):
    """table: what load_table returns (or takes); xy [B,V,L,2], conf [B,V,L] and optionally xyz [B,L,3], conf3 [B,L] for the
    engine's current problems (set_problems done: B, V and the cameras are theirs).  engine: an object with MvFit's
    set_landmarks / set_landmark_targets / landmark_loss and device.  Table and targets live in the engine: one LandmarkLoss
    per engine at a time (``rebind()`` sets this module's again after another one used the engine)."""

    def __init__(self, engine, table, xy, conf, xyz=None, conf3=None, rho=100.0, w3d=0.0, rho3d=0.0):
        super().__init__()
        if engine is None:
            raise ValueError('LandmarkLoss needs engine= (an MvFit with its problems set, e.g. BodyLayer(...).engine)')
        for name, val in (('rho', rho), ('w3d', w3d), ('rho3d', rho3d)):
            if not np.isfinite(val) or val < 0:
                raise ValueError('%s = %r must be finite and >= 0' % (name, val))
        if (xyz is None) != (conf3 is None):
            raise ValueError('xyz and conf3 come together')
        self.engine = engine
        self.table = table if isinstance(table, dict) and 'keypoint_index' in table else load_table(table)
        self.rho, self.w3d, self.rho3d = float(rho), float(w3d), float(rho3d)
        self.num_problems = int(xy.shape[0])
        self._set = (xy, conf, xyz, conf3)
        self.rebind()

    def rebind(self):
        xy, conf, xyz, conf3 = self._set
        self.engine.set_landmarks(self.table['vertex_ids'], self.table['weights'])
        self.engine.set_landmark_targets(xy, conf, xyz, conf3)

    def forward(self, vertices):
        """vertices[B,Nv,3] with the translation included (what BodyLayer returns with transl=) -> loss[B]."""
        vertices = torch.as_tensor(vertices)
        if vertices.dim() != 3 or vertices.shape[2] != 3:
            raise ValueError('vertices must be [B, Nv, 3], got %r' % (tuple(vertices.shape),))
        if int(vertices.shape[0]) != self.num_problems:
            raise ValueError('vertices hold %d bodies, the targets %d' % (int(vertices.shape[0]), self.num_problems))
        v = vertices.to(device=self.engine.device, dtype=torch.float32)
        return LandmarkFunction.apply(v, self)


def refine_fit(engine, params, stage, *, rho=100.0, w3d=0.0, rho3d=0.0, **fit_kwargs):
    """One fit of the engine's B problems with the landmark term inside the fit's rounds.

    params [B,118] (set_problems, set_landmarks and set_landmark_targets done); ``stage``: one weight dict with
    coll_loss_weight w > 0.  The objective of problem j is its closure loss under ``stage`` with the term on: the stage's
    keypoint and prior terms + w^2 * landmark_loss_j(rho, w3d, rho3d).

      1. the term is switched on; one closure gives J(x_0) and the landmark losses L(x_0);
      2. x' = engine.fit(x_0, [stage], **fit_kwargs); one closure gives J(x'), L(x');
      3. problem j keeps its row of x' iff J_j(x') < J_j(x_0); otherwise the row reverts to x_0 exactly;
      4. the engine is left with the term cleared (also when something raises); table and targets stay.

    Returns (params, report).  report: dict(before [B], after [B] = J of the returned rows, accepted [B] bool,
    landmark_before [B], landmark_after [B] = L of the returned rows, n_closure [B] of the fit, loss [B] = after)."""
    if float(stage.get('coll_loss_weight', 0.0)) <= 0.0:
        raise ValueError('refine_fit: the stage needs coll_loss_weight > 0')
    x0 = params if isinstance(params, torch.Tensor) else torch.as_tensor(np.asarray(params, np.float32))
    x0 = x0.to(engine.device).clone()

    def host(t):
        return np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t)

    def objective(x):
        J = engine.closure(x, stage, want_grad=False)['loss']
        return host(J).astype(np.float64), host(engine.sdf_term_read()[1]).astype(np.float64)

    engine.set_landmark_term(rho=rho, w3d=w3d, rho3d=rho3d)
    try:
        before, lm_before = objective(x0)
        x1, st = engine.fit(x0, [stage], **fit_kwargs)
        x1 = x1.to(x0.dtype)
        after, lm_after = objective(x1)
        accepted = after < before
        for j in np.flatnonzero(~accepted):
            x1[int(j)] = x0[int(j)]
        after = np.where(accepted, after, before)
        lm_after = np.where(accepted, lm_after, lm_before)
        report = dict(before=before, after=after, accepted=accepted, landmark_before=lm_before, landmark_after=lm_after,
                      n_closure=host(st['n_closure']), loss=after.copy())
        return x1, report
    finally:
        engine.clear_landmark_term()


__all__ = ['NNZ', 'LANDMARKS_MAX', 'load_table', 'targets_from_people', 'LandmarkFunction', 'LandmarkLoss', 'refine_fit']
