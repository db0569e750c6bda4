"""Timing of the silhouette term inside the fit (include/mvfit.h:mvfit_set_silhouette_term) next to the two ways a caller
could evaluate the same closure from outside the fit.

  python tools/silhouette_fit_timing.py [--reps 30] [--bodies 32] [--views 8] [--width 512] [--height 384] [--rounds 96]
                                        [--only-rounds]

Workload: ``bodies`` synthetic bodies x ``views`` cameras (the workload of tools/silhouette_timing.py), every problem with
images and every problem live.  Medians of ``reps`` after a warm-up, from device events:
  chained round   a fit whose tolerances are 0 and whose round cap is ``rounds`` (a multiple of 24, the rounds of one graph
                  replay): no problem finishes, the fit stops at the cap (reported as an error, which is expected here) and
                  the time of the call / ``rounds`` is one round.  With the term (weight w) and, under round_mode = 1, the same
                  rounds with weight 0 (vertex pass and step kernel alone).  The call's fixed part (initialisation, results,
                  one host wait per replay) is inside both.
  engine-composed closure(want_verts) + silhouette_loss + vertices_backward: one closure of the same objective through the
                  engine's entries;
  BodyLayer       BodyLayer -> SilhouetteLoss -> .backward(): what silhouette.refine_shape pays per closure (no keypoint term).
The two compositions alternate inside one loop.  --only-rounds runs the two round fits alone: the run to put under
rocprofv3 --kernel-trace --stats for the per-kernel split (no counters in that run).  Run every invocation under a time limit
of its own."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mvsmplfitting_amd import synthetic as syn  # noqa: E402
from mvsmplfitting_amd.engine import MvFit, MvFitError, pack_params, stage_weights  # noqa: E402
from mvsmplfitting_amd.layer import BodyLayer  # noqa: E402
from mvsmplfitting_amd.silhouette import SilhouetteLoss  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--bodies', type=int, default=32)
    ap.add_argument('--views', type=int, default=8)
    ap.add_argument('--width', type=int, default=512)
    ap.add_argument('--height', type=int, default=384)
    ap.add_argument('--rounds', type=int, default=96)
    ap.add_argument('--only-rounds', action='store_true')
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
    v0 = eng.vertices(x)[0]
    L = eng.silhouette_loss(v0, need_grad=False)[0]
    base = stage_weights(float(H))[3]
    data = eng.closure(x, base, want_grad=False)['loss']
    w = float(torch.sqrt(data.mean() / L.mean()))
    print('%d bodies x %d views at %d x %d: %d contour points (%.0f per image), mean silhouette loss %.5g, w %.4g'
          % (N, V, W, H, n_pts, n_pts / (N * V), float(L.mean()), w))
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
    eng.set_silhouette_term()
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
    eng.clear_silhouette_term()
    if a.only_rounds:
        eng.close()
        return

    def composed():
        out = eng.closure(x, base, want_grad=True, want_verts=True)
        loss, g = eng.silhouette_loss(out['verts'])
        return out['loss'] + w * w * loss, out['grad'] + w * w * eng.vertices_backward(x, grad_verts=g)

    layer = BodyLayer(model)
    sil = SilhouetteLoss(engine=layer.engine, masks=masks, image_body=image_body, cams=cams)
    xt = torch.from_numpy(x).to(layer.engine.device)
    parts = [xt[:, 0:10].clone().requires_grad_(True), xt[:, 10:13].clone().requires_grad_(True),
             xt[:, 13:82].clone().requires_grad_(True), xt[:, 82:85].clone().requires_grad_(True),
             xt[:, 85:86].clone().requires_grad_(True)]

    def through_layer():
        for p in parts:
            p.grad = None
        out = layer(parts[0], parts[1], parts[2], transl=parts[3], scale=parts[4])
        (w * w * sil(out.vertices)).sum().backward()

    for fn in (composed, through_layer, composed, through_layer):
        fn()
    torch.cuda.synchronize()
    pc, pl = [], []
    for _ in range(a.reps):
        pc.append(timed(composed))
        pl.append(timed(through_layer))
    print(fmt % (('engine-composed closure (3 entries)',) + stats(pc) + (a.reps,)))
    print(fmt % (('BodyLayer + SilhouetteLoss + backward',) + stats(pl) + (a.reps,)))
    eng.close()
    layer.engine.close()


if __name__ == '__main__':
    main()
