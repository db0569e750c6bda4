"""Timing of the scan term inside the fit (include/mvfit.h:mvfit_set_scan_term) and of the op alone.

  python tools/scan_fit_timing.py [--reps 30] [--bodies 32] [--views 8] [--points 8192] [--rounds 96] [--only-rounds] [--mix]

Workload: ``bodies`` synthetic bodies x ``views`` cameras (the bodies of tools/vertex_target_fit_timing.py), every problem with
``points`` scan points of weight 1 on a noisy copy of its own surface (5 mm) and every problem live; w_s2m = 1, w_m2s = 0,
sigma = 0.  Medians of ``reps`` after a warm-up, from device events:
  chained round   a fit whose tolerances are 0 and whose round cap is ``rounds`` (a multiple of 24, the rounds of one graph
                  replay): no problem finishes, the fit stops at the cap (reported as an error, which is expected here) and
                  the time of the call / ``rounds`` is one round.  With the term (weight w) and, under round_mode = 1, the same
                  rounds with weight 0 (vertex pass and step kernel alone).  The call's fixed part (initialisation, results,
                  one host wait per replay) is inside both.
  op              scan_loss with the gradient (culled search), 20 calls inside one pair of events.
--mix adds the same rounds with the scan as a share of the term mix (mvfit_set_term_mix) beside the scene term - the bodies
paired into scenes of two, obstacles frozen at the start: with scan share 1 (the scan buffers go to the pull-back as they are)
and with scan share 2 at weight w / sqrt(2) (the same penalty through the cotangent kernel).
--only-rounds runs the two round fits alone: the run to put under rocprofv3 --kernel-trace --stats for the per-kernel split
(no counters in that run).  Run every invocation under a time limit of its own."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mvsmplfitting_amd import synthetic as syn  # noqa: E402
from mvsmplfitting_amd.engine import MvFit, MvFitError, pack_params, stage_weights  # noqa: E402
from tests.helpers import body_model  # noqa: E402


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def stats(per):
    per = np.asarray(per)
    return float(np.median(per)), float(per.min()), float(per.max())


def surface_points(verts, faces, P, noise, rng):
    """P barycentric samples of the faces of verts [Nv,3] plus Gaussian noise"""
    f = faces[rng.integers(0, len(faces), P)]
    u = rng.random((P, 2))
    flip = u.sum(axis=1) > 1
    u[flip] = 1.0 - u[flip]
    a, b, c = verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]]
    return a + u[:, :1] * (b - a) + u[:, 1:] * (c - a) + rng.normal(0, noise, (P, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--bodies', type=int, default=32)
    ap.add_argument('--views', type=int, default=8)
    ap.add_argument('--points', type=int, default=8192)
    ap.add_argument('--rounds', type=int, default=96)
    ap.add_argument('--only-rounds', action='store_true')
    ap.add_argument('--mix', action='store_true')
    a = ap.parse_args()
    N, V, P = a.bodies, a.views, a.points
    rounds = max(24, a.rounds // 24 * 24)
    model = body_model()
    faces = np.asarray(model['faces'], np.int64)
    eng = MvFit(model)
    rig = syn.make_camera_ring(V)
    x = pack_params(B=N, **syn.make_frames(N))
    eng.set_problems(rig, np.zeros((N, V, 17, 2), np.float32), np.zeros((N, V, 17), np.float32))
    _, jd = eng.vertices(x)
    gt, conf = syn.make_observations(jd.cpu().numpy(), rig, seed=3, noise_px=0.5)
    eng.set_problems(rig, gt, conf)
    rng = np.random.default_rng(8)
    v0 = eng.vertices(x)[0]
    v64 = v0.cpu().numpy().astype(np.float64)
    eng.set_scans(np.stack([surface_points(v64[n], faces, P, 0.005, rng) for n in range(N)]).astype(np.float32))
    L = eng.scan_loss(v0, need_grad=False)[0]
    base = stage_weights(1536.0)[3]
    data = eng.closure(x, base, want_grad=False)['loss']
    w = float(torch.sqrt(data.mean() / L.mean()))
    print('%d bodies x %d views, %d points per body against %d faces: mean loss %.5g, w %.4g'
          % (N, V, P, len(faces), float(L.mean()), w))
    fmt = '%-52s median %9.3f ms  min %9.3f  max %9.3f  (%d reps)'
    never = dict(tolerance_grad=0.0, tolerance_change=0.0, ftol=0.0, gtol=0.0, max_iter=100000, maxiters=100000, max_rounds=rounds)

    def capped_fit(weight):
        try:
            eng.fit(x, [dict(base, coll_loss_weight=weight)], **never)
        except MvFitError as e:
            if 'round cap' not in str(e):
                raise
        else:
            raise RuntimeError('the fit finished before the round cap: the rounds were not all live')

    eng.set_options(round_mode=1)                      # weight 0: the same chained rounds without the term's kernels
    eng.set_scan_term()
    per = {0.0: [], w: []}
    for weight in (0.0, w):
        capped_fit(weight)
        capped_fit(weight)
    for _ in range(a.reps):
        for weight in (0.0, w):
            per[weight].append(timed(lambda: capped_fit(weight)) / rounds)
    print(fmt % (('chained round, weight 0 (pass + step)',) + stats(per[0.0]) + (a.reps,)))
    print(fmt % (('chained round with the term',) + stats(per[w]) + (a.reps,)))
    print('the term adds %.3f ms per round (medians)' % (stats(per[w])[0] - stats(per[0.0])[0]))
    eng.clear_scan_term()
    if a.mix:
        if N % 2:
            raise SystemExit('--mix pairs the bodies into scenes of two: --bodies must be even')
        eng.set_scene_obstacles(v0, [2] * (N // 2), grid_size=32, scale_factor=0.2, robustifier=0.05)
        for share, weight, what in ((1.0, w, 'scan share 1: pass-through'), (2.0, w / np.sqrt(2.0), 'scan share 2: cotangent kernel')):
            eng.set_term_mix(scene=1.0, scan=share)
            capped_fit(weight)
            capped_fit(weight)
            pm = [timed(lambda: capped_fit(weight)) / rounds for _ in range(a.reps)]
            print(fmt % (('chained round, mix scene + scan (%s)' % what,) + stats(pm) + (a.reps,)))
        eng.clear_term_mix()
        eng.clear_scene_obstacles()
    if not a.only_rounds:
        calls = 20
        loss, g = torch.empty(N, device=eng.device), torch.empty_like(v0)

        def op():
            for _ in range(calls):
                eng._check(eng._lib.mvfit_scan_loss(eng._ctx, v0.data_ptr(), N, 1.0, 0.0, 0.0, 0, loss.data_ptr(), g.data_ptr(), None, None))

        op()
        torch.cuda.synchronize()
        po = [timed(op) / calls for _ in range(a.reps)]
        print(fmt % (('scan_loss with gradient (op alone)',) + stats(po) + (a.reps,)))
    eng.close()


if __name__ == '__main__':
    main()
