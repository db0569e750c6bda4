"""Timing of the occlusion between bodies in the silhouette term (include/mvfit.h:mvfit_set_silhouette_occluders).

  python tools/silhouette_occlusion_timing.py [--reps 30] [--bodies 32] [--views 8] [--width 512] [--height 384] [--rounds 96]

Workload: that of tools/silhouette_fit_timing.py (``bodies`` synthetic bodies x ``views`` cameras, every problem with images
and every problem live), the bodies paired into scenes: body_scene[n] = n // 2, so every image has one occluder.  Medians of
``reps`` after a warm-up, with min and max, from device events:
  freeze          one mvfit_set_silhouette_occluders at the start vertices (instance list on the host, two map fills, the
                  raster over 2 x bodies x views instances, the flag kernel, one wait for the stream);
  chained round   a fit whose tolerances are 0 and whose round cap is ``rounds`` (a multiple of 24), as in
                  tools/silhouette_fit_timing.py: the time of the call / ``rounds``.  With occluders set, and with them
                  cleared - the second is the round tools/silhouette_fit_timing.py --only-rounds reports as "chained round
                  with the term"; run that tool from a checkout of another commit for the same round of that build.
  own graph       the same fit with occluders after mvfit_round_graph_info(drop = 1), against the fit that replays the kept
                  graph: what every sweep after the first of silhouette.refine_fit_occluded pays for capturing its own.
Each state is timed in a loop of its own (it is part of the round graph's key).  Run every invocation under a time limit of its own."""
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
from tools.silhouette_fit_timing import stats, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--bodies', type=int, default=32)
    ap.add_argument('--views', type=int, default=8)
    ap.add_argument('--width', type=int, default=512)
    ap.add_argument('--height', type=int, default=384)
    ap.add_argument('--rounds', type=int, default=96)
    ap.add_argument('--margin', type=float, default=0.02)
    a = ap.parse_args()
    N, V, H, W = a.bodies, a.views, a.height, a.width
    rounds = max(24, a.rounds // 24 * 24)
    model = body_model()
    eng = MvFit(model)
    R, t, f, c = syn.make_camera_ring(V)
    f = (f * np.float32(W / 2048.0)).astype(np.float32)
    c = np.tile(np.array([W / 2.0, H / 2.0], np.float32), (V, 1))
    rig = (R, t, f, c)
    x = pack_params(B=N, **syn.make_frames(N))
    xd = x.copy()
    xd[:, 0:10] += np.random.default_rng(8).normal(0, 0.8, (N, 10)).astype(np.float32)
    xd[:, 82:85] += np.float32([0.03, -0.02, 0.01])
    xd[:, 85] = 1.05
    eng.set_problems(rig, np.zeros((N, V, 17, 2), np.float32), np.zeros((N, V, 17), np.float32))
    vd, jd = eng.vertices(xd)
    gt, conf = syn.make_observations(jd.cpu().numpy(), rig, seed=3, noise_px=0.5)
    eng.set_problems(rig, gt, conf)
    image_body = np.repeat(np.arange(N), V).astype(np.int32)
    view = np.tile(np.arange(V), N)
    masks = torch.empty(N * V, H, W, dtype=torch.uint8, device=eng.device)
    for b in range(N):
        _, fid = eng.render_overlay(vd, None, np.zeros((V, H, W, 3), np.uint8), image_body[b * V:(b + 1) * V], view[:V],
                                    face_id=True)
        masks[b * V:(b + 1) * V] = (fid >= 0).to(torch.uint8)
    cams = tuple(np.ascontiguousarray(q[view]) for q in rig)
    eng.set_silhouettes(masks, image_body, cams)
    n_pts = int(eng.silhouettes()[1][-1])
    scene = (np.arange(N) // 2).astype(np.int32)
    v0 = eng.vertices(x)[0]
    L = eng.silhouette_loss(v0, need_grad=False)[0]
    base = stage_weights(float(H))[3]
    data = eng.closure(x, base, want_grad=False)['loss']
    w = float(torch.sqrt(data.mean() / L.mean()))
    fmt = '%-52s median %9.3f ms  min %9.3f  max %9.3f  (%d reps)'

    def freeze():
        eng.set_silhouette_occluders(v0, scene, margin=a.margin)

    freeze()
    freeze()
    hidden = int(eng.silhouette_hidden(v0).sum())
    flagged = int(eng.silhouette_occluders()[2].sum())
    print('%d bodies in %d scenes x %d views at %d x %d: %d contour points (%d flagged), %d of %d (image, vertex) pairs hidden, w %.4g'
          % (N, len(set(scene.tolist())), V, W, H, n_pts, flagged, hidden, N * V * eng.nv, w))
    print(fmt % (('freeze (mvfit_set_silhouette_occluders)',) + stats([timed(freeze) for _ in range(a.reps)]) + (a.reps,)))
    never = dict(tolerance_grad=0.0, tolerance_change=0.0, ftol=0.0, gtol=0.0, max_iter=100000, maxiters=100000, max_rounds=rounds)

    def capped_fit():
        try:
            eng.fit(x, [dict(base, coll_loss_weight=w)], **never)
        except MvFitError as e:
            if 'round cap' not in str(e):
                raise
        else:
            raise RuntimeError('the fit finished before the round cap: the rounds were not all live')

    # whether occluders are set is part of the captured round graph's key: each state is timed in a loop of its own (the warm-up
    # builds its graph), the state without occluders before and after the one with them
    eng.set_silhouette_term()

    def loop(occluders):
        if occluders:
            freeze()
        else:
            eng.clear_silhouette_occluders()
        capped_fit()
        capped_fit()
        return stats([timed(capped_fit) / rounds for _ in range(a.reps)])

    plain0, with_occ, plain1 = loop(False), loop(True), loop(False)
    print(fmt % (('chained round with the term, no occluders',) + plain0 + (a.reps,)))
    print(fmt % (('chained round with the term, occluders set',) + with_occ + (a.reps,)))
    print(fmt % (('chained round with the term, no occluders (again)',) + plain1 + (a.reps,)))
    print('the occluders add %.4f ms per round (medians, against the mean of the two runs without)'
          % (with_occ[0] - 0.5 * (plain0[0] + plain1[0])))
    # what a sweep of silhouette.refine_fit_occluded pays for a round graph of its own: the same call after the graph was dropped
    freeze()
    capped_fit()
    kept = [timed(capped_fit) for _ in range(a.reps)]

    def fresh():
        eng.round_graph_info(drop=True)
        capped_fit()

    own = [timed(fresh) for _ in range(a.reps)]
    print(fmt % (('fit of %d rounds, graph kept' % rounds,) + stats(kept) + (a.reps,)))
    print(fmt % (('fit of %d rounds, graph dropped before' % rounds,) + stats(own) + (a.reps,)))
    print('a round graph of its own costs %.3f ms per fit (medians)' % (stats(own)[0] - stats(kept)[0]))
    eng.clear_silhouette_term()
    eng.close()


if __name__ == '__main__':
    main()
