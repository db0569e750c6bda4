"""Inputs and runs shared by tools/record_closure_bits.py (writes tests/golden/closure_bits.npz) and
tests/test_gpu_closure_bits.py (compares against it word for word): closure loss + gradient at four points in the three
prior modes, and one complete 4-stage L2 fit.  Everything is small: B = 3 problems x 2 views for the closures, B = 2 for the fit."""
import os

import numpy as np

from mvsmplfitting_amd import _lib
from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import MvFit, stage_weights

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'closure_bits.npz')
MODES = ('l2', 'gmm', 'vposer')
B_CLOSURE, B_FIT, VIEWS, SKIN_TOPK = 3, 2, 2, 4
ANGLE_IDX = (9, 12, 52, 55)            # body_pose indices of the elbow / knee bending prior
POINT_STAGE = (0, 1, 0, 3)             # the stage whose weights each point is evaluated with (0: the largest prior weights)
IMAGE_HEIGHT = 1536.0


def model():
    return syn.make_body_model(0, skin_topk=SKIN_TOPK)


def mode_flags(mode):
    return dict(l2=0, gmm=_lib.F_PRIOR_GMM, vposer=_lib.F_VPOSER)[mode]


def mode_stages(mode):
    return stage_weights(IMAGE_HEIGHT, flags=mode_flags(mode))


def make_inputs():
    """Observations (from the float64 oracle's keypoints of seeded ground-truth frames: no GPU involved) and the four points.
    Returns dict(cam_R, cam_t, cam_f, cam_c, gt, conf, x[4, B, 118])."""
    from oracle import closure_np as cn
    m = model()
    cams = syn.make_camera_ring(VIEWS)
    orc = cn.ClosureOracle(m, np.float64)
    fr = syn.make_frames(B_CLOSURE, seed0=3100)
    kp = np.stack([orc.body(dict({k: fr[k][b] for k in fr}, use_vposer=False), want_cache=False)['joints']
                   for b in range(B_CLOSURE)])
    gt, conf = syn.make_observations(kp, cams, seed=3107)
    rng = np.random.RandomState(31)
    B = B_CLOSURE
    x0 = np.zeros((B, 118), np.float32)
    x0[:, 85] = 1.0
    x1 = x0 + (0.05 * rng.randn(B, 118)).astype(np.float32)
    x2 = x1.copy()                                                        # body pose N(0, 1.5): both prior drops fire
    x2[:, 13:82] = (1.5 * rng.randn(B, 69)).astype(np.float32)
    x2[:, 86:118] = (1.5 * rng.randn(B, 32)).astype(np.float32)
    x2[:, 13 + 52] = np.abs(x2[:, 13 + 52]) + 1.2                         # (exp(2 * 1.2) * bending weight of stage 0 > 1e4 on its own)
    x3 = x1.copy()                                                        # joints at exactly zero, elbows and knees bent
    x3[:, 10:82] = 0.0
    for i in ANGLE_IDX:
        x3[:, 13 + i] = (0.6 * rng.randn(B) + (0.8 if i == 52 else -0.8)).astype(np.float32)
    x = np.stack([x0, x1, x2, x3]).astype(np.float32)
    return dict(cam_R=cams[0], cam_t=cams[1], cam_f=cams[2], cam_c=cams[3], gt=gt, conf=conf, x=x)


def prior_drops(inp, mode, point):
    """(pose prior dropped, angle prior dropped) per problem at a point, by the float64 oracle's loss terms."""
    from oracle import closure_np as cn
    gmm = syn.gmm_constants(syn.make_gmm(), np.float64) if mode == 'gmm' else None
    orc = cn.ClosureOracle(model(), np.float64, gmm=gmm)
    cams = tuple(inp[k] for k in ('cam_R', 'cam_t', 'cam_f', 'cam_c'))
    w = mode_stages(mode)[POINT_STAGE[point]]
    out = []
    for b in range(B_CLOSURE):
        xb = inp['x'][point, b, :86].astype(np.float64)
        p = dict(cn.unpack(xb, False), use_vposer=False)
        o = orc.body(p, want_cache=False)
        _, aux = orc.loss_terms(o, cams, inp['gt'][b], inp['conf'][b], w, False, None,
                                cn.PRIOR_GMM if mode == 'gmm' else cn.PRIOR_L2, False, p['betas'])
        out.append((aux['pose_dropped'], aux['angle_dropped']))
    return out


def run_closures(inp, mode):
    """loss[4, B], grad[4, B, 118] of the four points in one prior mode."""
    eng = MvFit(model(), vposer=syn.make_vposer_decoder() if mode == 'vposer' else None,
                gmm=syn.gmm_constants(syn.make_gmm()) if mode == 'gmm' else None)
    try:
        eng.set_problems(tuple(inp[k] for k in ('cam_R', 'cam_t', 'cam_f', 'cam_c')), inp['gt'], inp['conf'])
        stages = mode_stages(mode)
        loss, grad = [], []
        for k in range(inp['x'].shape[0]):
            c = eng.closure(inp['x'][k], stages[POINT_STAGE[k]])
            loss.append(c['loss'].cpu().numpy())
            grad.append(c['grad'].cpu().numpy())
    finally:
        eng.close()
    return np.stack(loss), np.stack(grad)


def run_fit(inp):
    """A complete 4-stage L2 fit of the first B_FIT problems from x0, default options."""
    eng = MvFit(model())
    try:
        eng.set_problems(tuple(inp[k] for k in ('cam_R', 'cam_t', 'cam_f', 'cam_c')), inp['gt'][:B_FIT], inp['conf'][:B_FIT])
        xf, st = eng.fit(inp['x'][0, :B_FIT], mode_stages('l2'))
        return dict(fit_x=xf.cpu().numpy(), fit_n_closure=st['n_closure'].cpu().numpy(), fit_n_iter=st['n_iter'].cpu().numpy(),
                    fit_final_loss=st['final_loss'].cpu().numpy())
    finally:
        eng.close()
