"""Timing of the collision term against frozen obstacles (include/mvfit.h:mvfit_set_scene_obstacles, csrc/scene_sdf.hip:
scene_entries_kernel) on the workload of tools/scene_sdf_timing.py.

  python tools/scene_refine_timing.py [--reps 30] [--scenes 32] [--bodies 4] [--grid 32] [--rounds 240] [--only-rounds]

Workload: ``scenes`` scenes of ``bodies`` synthetic bodies (6890 vertices / 13776 faces, random shape and pose, standing
0.25 m apart so that neighbours interpenetrate), 4 views, robustifier 0.05.  Prints medians of ``reps`` after a warm-up, from
hipEvents around the call:
  1. ms per freeze (MvFit.set_scene_obstacles);
  2. us per chained round (vertex pass -> term -> step kernel, replayed as a graph) with the term and with weight 0 - the same
     rounds without the term's two kernels; the difference is the term's cost.  A fit is stopped by its round cap after
     ``rounds`` rounds with tolerances that let no problem finish earlier, so every round carries every problem;
  3. (--only-rounds: the fit with the term alone - the run to put under rocprofv3 --kernel-trace --stats for the split);
  4. ms per MvFit.scene_sdf_loss call on the same bodies: what re-voxelising in every round would cost."""
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


def median(fn, reps):
    fn()
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per = []
    for _ in range(reps):
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        per.append(t0.elapsed_time(t1))
    per = np.asarray(per)
    return float(np.median(per)), float(per.min()), float(per.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--scenes', type=int, default=32)
    ap.add_argument('--bodies', type=int, default=4)
    ap.add_argument('--grid', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=240)
    ap.add_argument('--weight', type=float, default=1e-3)
    ap.add_argument('--only-rounds', action='store_true')
    a = ap.parse_args()
    model = body_model()
    eng = MvFit(model, options=dict(round_mode=1))         # chained rounds also for the fit without the term
    N, G, r, V = a.scenes * a.bodies, a.grid, 0.05, 4
    cams = syn.make_camera_ring(V)
    eng.set_problems(cams, np.zeros((N, V, 17, 2), np.float32), np.zeros((N, V, 17), np.float32))
    x = pack_params(B=N, **syn.make_frames(N))
    x[:, 82:85] = 0.0
    x[:, 82] = 0.25 * (np.arange(N) % a.bodies)
    v, joints = eng.vertices(x)
    gt, conf = syn.make_observations(joints.cpu().numpy(), cams, seed=1)
    eng.set_problems(cams, gt, conf)
    sizes = [a.bodies] * a.scenes
    kw = dict(grid_size=G, scale_factor=0.2, robustifier=r)
    eng.set_scene_obstacles(v, sizes, **kw)
    eng.closure(x, dict(stage_weights(1536.0)[-1], coll_loss_weight=a.weight), want_grad=False)
    S = eng.sdf_term_read()[1]
    print('%d scenes x %d bodies, G = %d, %d views: mean S_j %.2f, %d of %d problems pay the term'
          % (a.scenes, a.bodies, G, V, float(S.mean()), int((S > 0).sum()), N))

    def rounds(weight):
        # no tolerance lets a problem finish: the round cap ends the fit (reported as an error: expected here)
        try:
            eng.fit(x, [dict(stage_weights(1536.0)[-1], coll_loss_weight=weight)], max_rounds=a.rounds, maxiters=10 ** 6,
                    tolerance_grad=0.0, tolerance_change=0.0, ftol=-1.0, gtol=-1.0)
        except MvFitError as e:
            if 'round cap' not in str(e):
                raise
            return
        raise SystemExit('the fit finished before its round cap: the rounds of this run are not all full')

    fmt = '%-46s median %9.3f %s  min %9.3f  max %9.3f  (%d reps)'
    if not a.only_rounds:
        m = median(lambda: eng.set_scene_obstacles(v, sizes, **kw), a.reps)
        print(fmt % (('freeze (set_scene_obstacles)', m[0], 'ms') + m[1:] + (a.reps,)))
    with_term = median(lambda: rounds(a.weight), a.reps)
    per = lambda m: tuple(1e3 * t / a.rounds for t in m)
    print(fmt % (('chained round with the term', per(with_term)[0], 'us') + per(with_term)[1:] + (a.reps,)))
    if not a.only_rounds:
        without = median(lambda: rounds(0.0), a.reps)
        print(fmt % (('chained round, weight 0', per(without)[0], 'us') + per(without)[1:] + (a.reps,)))
        print('the term costs %.2f us per round (%d problems; %d rounds per fit)' % (per(with_term)[0] - per(without)[0], N, a.rounds))
        m = median(lambda: eng.scene_sdf_loss(v, model['faces'], scene_sizes=sizes, **kw), a.reps)
        print(fmt % (('scene_sdf_loss (boxes, fields, pairs)', m[0], 'ms') + m[1:] + (a.reps,)))
    eng.close()


if __name__ == '__main__':
    main()
