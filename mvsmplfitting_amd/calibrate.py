"""Refinement of the rig against the fitted bodies: hold the bodies and move the cameras, then hold the cameras and refit the
bodies.

Every term of a fit takes the rig of set_problems as exact, and a real rig drifts: a tripod that moved by a degree shifts a body
3.5 m away by about 25 px at f = 1500, a quarter of the robustifier's scale, and the fit takes that view's systematic error into
the pose, the scale and the shape.  The fitted bodies are the best calibration object a capture has - 17 points per person per
frame, seen by every view.  With the bodies held the views are independent, and MvFit.refine_cameras solves them on the device,
one workgroup per view (include/mvfit.h:mvfit_refine_cameras).

    E(x, C) = the float64 host sum of the closure losses of all problems under rig C with the stage's weights.

One sweep takes the keypoints of the bodies x under C, refines the cameras against them (C'), sets C' and warm-starts the fit
from x (x').  The sweep is kept only if E(x', C') < E(x, C) - the accept rule of temporal.py, scene_fit.py and joint_refine.py,
which makes E non-increasing; otherwise x and C stay as they were, bit for bit.  The anchor view is returned as given and fixes the
rigid gauge; with anchor=None every view moves and the gauge stays where the bodies are, because each half-step holds the other
half.

Not built: priors towards the start calibration, lens distortion, cameras per frame, the 3-D joint term (set_problems clears its
targets), vertices or masks as calibration points."""
import numpy as np
import torch

from . import _lib
from .engine import FREE_MASKS, pack_cameras, unpack_cameras

# keywords of refine_rig that go to MvFit.refine_cameras (max_iter and ftol of MvFit.fit keep their names: the cameras' loop
# takes them as cam_max_iter and cam_ftol); everything else goes to MvFit.fit
CAMERA_KEYS = {'min_points': 'min_points', 'lambda0': 'lambda0', 'cam_max_iter': 'max_iter', 'cam_ftol': 'ftol'}


def _np(t):
    return np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t)


def refine_rig(engine, params, stage, cams, gt_xy, w_conf, *, sweeps=3, anchor=0, free='extrinsics', **refine_and_fit_kwargs):
    """params [B,118] of the engine's problems; ``stage``: one weight dict (without F_USE_3D); ``cams``: the (R, t, f, c) tuple
    of set_problems - one rig, not per-problem cameras - or its [V,15] form (engine.pack_cameras); gt_xy [B,V,17,2] and w_conf
    [B,V,17] as set_problems takes them.  anchor: the view returned as given, or None; free: 'extrinsics' |
    'extrinsics+focal' | 'all'.  Keywords min_points, lambda0, cam_max_iter, cam_ftol go to MvFit.refine_cameras, the others to
    MvFit.fit.

    Stops after a rejected sweep, or after ``sweeps`` sweeps.  The engine is left with the returned rig set (its float32
    rounding, as set_problems stores every rig), also when something raises.

    Returns (params [B,118] tensor, cams [V,15] float64 array, report).  report: dict(E0, cams0 [V,15], sweeps = one dict per
    sweep run with E (after the accept rule), accepted, report [V,8] (the op's: E0, E1, it, acc, status, count, lam, 0 per
    view), cams [V,15] and params [B,118] kept after the sweep, n_closure [B] of the sweep's fit; loss [B] = the closure loss
    of the returned params under the returned rig)."""
    if int(stage.get('flags', 0)) & _lib.F_USE_3D:
        raise ValueError('refine_rig: a stage with F_USE_3D is not available (set_problems clears the 3-D targets)')
    if isinstance(cams, (tuple, list)) and len(cams) == 4:
        if np.ndim(_np(cams[0])) != 3:
            raise ValueError('refine_rig: one rig [V,3,3] is refined, not per-problem cameras')
        C_ = pack_cameras(cams)
    else:
        C_ = np.array(_np(cams), np.float64)
        if C_.ndim != 2 or C_.shape[1] != 15:
            raise ValueError('refine_rig: cams must be the (R, t, f, c) tuple of one rig or a [V,15] array')
    if free not in FREE_MASKS:
        raise ValueError('refine_rig: free must be one of %s, got %r' % (sorted(FREE_MASKS), free))
    V = C_.shape[0]
    if anchor is not None and not 0 <= int(anchor) < V:
        raise ValueError('refine_rig: anchor %r outside [0, %d)' % (anchor, V))
    cam_kw = {CAMERA_KEYS[k]: refine_and_fit_kwargs.pop(k) for k in list(refine_and_fit_kwargs) if k in CAMERA_KEYS}
    fit_kw = refine_and_fit_kwargs
    fixed = () if anchor is None else (int(anchor),)
    x = params if isinstance(params, torch.Tensor) else torch.as_tensor(np.asarray(params, np.float32))
    x = x.to(engine.device).clone()

    def set_rig(c15):
        engine.set_problems(unpack_cameras(c15, np.float32), gt_xy, w_conf)

    def evaluate(xx):
        out = engine.closure(xx, stage, want_grad=False, want_joints=True)
        return out['loss'], out['joints'], float(_np(out['loss']).astype(np.float64).sum())

    try:
        set_rig(C_)
        loss, joints, E = evaluate(x)
        report = dict(E0=E, cams0=C_.copy(), sweeps=[])
        for _ in range(int(sweeps)):
            C_new, rep = engine.refine_cameras(joints, C_, free=free, fixed_views=fixed, rho=float(stage.get('rho', 100.0)),
                                               data_weight=float(stage['data_weight']), **cam_kw)
            C_new = _np(C_new).astype(np.float64)
            set_rig(C_new)
            x_new, st = engine.fit(x, [stage], **fit_kw)
            x_new = x_new.to(x.dtype)
            loss_new, joints_new, E_new = evaluate(x_new)
            accepted = bool(E_new < E)
            if accepted:
                x, C_, loss, joints, E = x_new, C_new, loss_new, joints_new, E_new
            else:
                set_rig(C_)
            report['sweeps'].append(dict(E=E, accepted=accepted, report=_np(rep).copy(), cams=C_.copy(), params=_np(x).copy(),
                                         n_closure=_np(st['n_closure']).copy()))
            if not accepted:
                break
        report['loss'] = _np(loss).astype(np.float64)
        return x, C_, report
    except BaseException:
        set_rig(C_)
        raise


def camera_matrices(cams15, intris0=None):
    """The rig [V,15] as the matrices of a camera file: (extris [V,4,4], intris [V,3,3]) float64.  The intrinsics are those of
    ``intris0`` (identity-like when None) with f in [0,0] and [1,1] and c in [:2,2]."""
    R, t, f, c = unpack_cameras(cams15)
    V = R.shape[0]
    ex = np.tile(np.eye(4), (V, 1, 1))
    ex[:, :3, :3], ex[:, :3, 3] = R, t
    K = np.tile(np.eye(3), (V, 1, 1)) if intris0 is None else np.array(intris0, np.float64)[:V].copy()
    K[:, 0, 0] = K[:, 1, 1] = f
    K[:, :2, 2] = c
    return ex, K


__all__ = ['refine_rig', 'camera_matrices', 'CAMERA_KEYS']
