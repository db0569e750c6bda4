"""Joint refinement of the persons of a scene: the fit with the collision term against the OTHER bodies of the scene, whose
fields are frozen at the start of every sweep (include/mvfit.h:mvfit_set_scene_obstacles).

The reference's SDFLoss gives the fields no gradient (sdf/sdf/sdf_loss.py:72-98), so freezing them loses nothing its gradient
ever contained and turns the coupled term into a per-problem one - the shape the batched fit is built around.  All bodies of
a scene move at once against fields frozen where the sweep started: a Jacobi sweep.  Nothing guarantees that such a step
lowers the joint objective with the fields re-frozen at the new bodies, so every sweep is judged on exactly that and a scene
whose objective did not fall keeps its previous parameters: the accept rule is what makes J non-increasing."""
import numpy as np
import torch


def _scene_sums(values, sizes):
    """Per-scene sums of a per-problem vector, in float64 on the host, problems in order."""
    v = np.asarray(values.detach().cpu().numpy() if isinstance(values, torch.Tensor) else values, np.float64)
    first = np.concatenate([[0], np.cumsum(sizes)])
    return np.array([v[first[s]:first[s + 1]].sum() for s in range(len(sizes))], np.float64)


def refine_scenes(engine, params, scene_sizes, stage, *, sweeps=3, grid_size=32, scale_factor=0.2, robustifier=0.05,
                  **fit_kwargs):
    """params [B,118] of the engine's B problems (set_problems done; the scenes are ``scene_sizes`` consecutive problems each);
    ``stage``: one weight dict with coll_loss_weight > 0.  The joint objective of scene s at x is
    J_s(x) = sum_{j in s} closure loss_j(x) with the obstacles frozen at x.

      1. freeze at x_0; one closure gives J(x_0);
      2. per sweep: x' = engine.fit(x_k, [stage]); freeze at vertices(x'); one closure gives J(x'); scene s is accepted iff
         J_s(x') < J_s(x_k), a rejected scene's rows revert to x_k exactly;
      3. stop when no scene was accepted, or after ``sweeps`` sweeps;
      4. the engine is left with the obstacles cleared (also when something raises).

    Returns (params, report).  report: dict(J0 [S], collision0 [S], params0 [B,118], sweeps = one dict per sweep run with
    J [S] (after the accept rule), accepted [S] bool, collision [S] = engine.scene_sdf_loss of the kept bodies, params
    [B,118] kept after the sweep, n_closure [B] of the sweep's fit; loss [B] = the per-problem closure loss of the returned
    params under obstacles frozen at them)."""
    sizes = [int(n) for n in scene_sizes]
    if float(stage.get('coll_loss_weight', 0.0)) <= 0.0:
        raise ValueError('refine_scenes: the stage needs coll_loss_weight > 0')
    if sum(sizes) != engine.B:
        raise ValueError('scene_sizes %r do not add up to the %d problems of the engine' % (sizes, engine.B))
    flags = int(stage.get('flags', 0))
    first = np.concatenate([[0], np.cumsum(sizes)])
    x = params if isinstance(params, torch.Tensor) else torch.as_tensor(np.asarray(params, np.float32))
    x = x.to(engine.device).clone()

    def freeze(xx):
        v, _ = engine.vertices(xx, flags=flags)
        engine.set_scene_obstacles(v, sizes, grid_size=grid_size, scale_factor=scale_factor, robustifier=robustifier)
        return v

    def collision(v):
        loss = engine.scene_sdf_loss(v, engine.faces, scene_sizes=sizes, grid_size=grid_size, scale_factor=scale_factor,
                                     robustifier=robustifier, need_grad=False)[0]
        return np.asarray(loss.detach().cpu().numpy(), np.float64)

    def objective(xx):
        return engine.closure(xx, stage, want_grad=False)['loss']

    try:
        v = freeze(x)
        loss = objective(x)
        J, coll = _scene_sums(loss, sizes), collision(v)
        report = dict(J0=J.copy(), collision0=coll.copy(), params0=x.detach().cpu().numpy().copy(), sweeps=[])
        for k in range(int(sweeps)):
            x_new, st = engine.fit(x, [stage], **fit_kwargs)
            x_new = x_new.to(x.dtype)
            v_new = freeze(x_new)
            loss_new = objective(x_new)
            J_new, coll_new = _scene_sums(loss_new, sizes), collision(v_new)
            accepted = J_new < J
            for s in np.flatnonzero(~accepted):
                a, b = int(first[s]), int(first[s + 1])
                x_new[a:b] = x[a:b]
                loss_new[a:b] = loss[a:b]
            x, loss = x_new, loss_new
            J, coll = np.where(accepted, J_new, J), np.where(accepted, coll_new, coll)
            n_closure = st['n_closure']
            report['sweeps'].append(dict(J=J.copy(), accepted=accepted.copy(), collision=coll.copy(),
                                         params=x.detach().cpu().numpy().copy(),
                                         n_closure=np.asarray(n_closure.detach().cpu().numpy() if isinstance(n_closure, torch.Tensor)
                                                              else n_closure)))
            if not accepted.any():
                break
            if k + 1 < int(sweeps) and not accepted.all():
                freeze(x)                    # the next sweep starts from the kept bodies of the rejected scenes
        report['loss'] = np.asarray(loss.detach().cpu().numpy(), np.float64)
        return x, report
    finally:
        engine.clear_scene_obstacles()


__all__ = ['refine_scenes']
