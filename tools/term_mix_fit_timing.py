"""Timing of the term mix inside the fit (include/mvfit.h:mvfit_set_term_mix) next to the single terms' rounds.

  python tools/term_mix_fit_timing.py [--reps 30] [--bodies 32] [--views 8] [--width 512] [--height 384] [--rounds 96]
                                      [--only-rounds NAME]

Workload: ``bodies`` synthetic bodies x ``views`` cameras (the bodies, masks and targets of tools/silhouette_fit_timing.py and
tools/vertex_target_fit_timing.py): every problem with one image per view, two target sets of weight 1, scenes of two bodies
each (the bodies stand within a few centimetres of one another: every scene's fields are sampled), every problem live.
Medians of ``reps`` after a warm-up, from device events, of a chained round: a fit whose tolerances are 0 and whose round cap
is ``rounds`` (a multiple of 24, the rounds of one graph replay) - no problem finishes, the fit stops at the cap (reported as
an error, which is expected here) and the time of the call / ``rounds`` is one round; the call's fixed part (initialisation,
results, one host wait per replay) is inside every figure.  Configurations, each measured in two blocks of reps / 2 (a change
of configuration rebuilds the captured round graph: that happens in the block's warm-up):
  none            weight 0 under round_mode = 1: vertex pass and step kernel alone
  scene, silhouette, vertex-target     each single term through its own setter (the code of the commit before the mix)
  mix sil+vt      the mix with the two vertex terms (one cotangent kernel, one pull-back)
  mix all         the mix with all three (plus the scene term and the record merge)
and the sums of the single terms' additions over `none` next to the mixes' additions.  --only-rounds NAME runs one
configuration's fits alone: the run to put under rocprofv3 --kernel-trace --stats for the per-kernel split (no counters in
that run).  Run every invocation under a time limit of its own."""
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

CONFIGS = ('none', 'scene', 'silhouette', 'vertex-target', 'mix sil+vt', 'mix all')


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
    ap.add_argument('--only-rounds', choices=CONFIGS, default=None)
    a = ap.parse_args()
    N, V, H, W = a.bodies // 2 * 2, a.views, a.height, a.width
    rounds = max(24, a.rounds // 24 * 24)
    eng = MvFit(body_model())
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
    eng.set_silhouettes(masks, image_body, tuple(np.ascontiguousarray(q[view]) for q in rig))
    rng = np.random.default_rng(8)
    rows = []
    for _ in range(2):
        y = x.copy()
        y[:, 10:82] += rng.normal(0, 0.05, (N, 72)).astype(np.float32)
        y[:, 82:85] += rng.normal(0, 0.02, (N, 3)).astype(np.float32)
        rows.append(eng.vertices(y)[0])
    eng.set_vertex_targets(torch.stack(rows, dim=1), np.ones((N, 2), np.float32))
    v0 = eng.vertices(x)[0]
    sizes = [2] * (N // 2)
    scene_kw = dict(grid_size=32, scale_factor=0.2, robustifier=0.05)
    base = stage_weights(float(H))[3]
    data = eng.closure(x, base, want_grad=False)['loss']
    eng.set_scene_obstacles(v0, sizes, **scene_kw)
    eng.set_term_mix(scene=1.0, silhouette=1.0, vertex_targets=1.0)
    eng.closure(x, dict(base, coll_loss_weight=1.0), want_grad=False)
    parts = eng.term_mix_read().cpu().numpy().astype(np.float64)
    w = float(np.sqrt(float(data.mean()) / parts.sum(axis=1).mean()))
    eng.clear_term_mix()
    eng.clear_scene_obstacles()
    print('%d bodies x %d views at %d x %d, scenes of two: mean parts S_sc^2 %.5g (%d of %d > 0), L_sil %.5g, L_vt %.5g, w %.4g'
          % (N, V, W, H, parts[:, 0].mean(), int((parts[:, 0] > 0).sum()), N, parts[:, 1].mean(), parts[:, 2].mean(), w))
    never = dict(tolerance_grad=0.0, tolerance_change=0.0, ftol=0.0, gtol=0.0, max_iter=100000, maxiters=100000, max_rounds=rounds)

    def capped_fit(weight):
        try:
            eng.fit(x, [dict(base, coll_loss_weight=weight)], **never)
        except MvFitError as e:
            if 'round cap' not in str(e):
                raise
        else:
            raise RuntimeError('the fit finished before the round cap: the rounds were not all live')

    def configure(name):
        """Everything off, then the one configuration; returns the stage's weight."""
        eng.clear_term_mix()
        eng.clear_silhouette_term()
        eng.clear_vertex_target_term()
        eng.clear_scene_obstacles()
        if name in ('scene', 'mix all'):
            eng.set_scene_obstacles(v0, sizes, **scene_kw)
        if name == 'silhouette':
            eng.set_silhouette_term()
        elif name == 'vertex-target':
            eng.set_vertex_target_term()
        elif name == 'mix sil+vt':
            eng.set_term_mix(silhouette=1.0, vertex_targets=1.0)
        elif name == 'mix all':
            eng.set_term_mix(scene=1.0, silhouette=1.0, vertex_targets=1.0)
        elif name == 'none':
            eng.set_silhouette_term()              # (a term has to be configured for the chained rounds; its weight is 0)
            return 0.0
        return w

    eng.set_options(round_mode=1)                  # weight 0: the same chained rounds without the term's kernels
    names = CONFIGS if a.only_rounds is None else (a.only_rounds,)
    per = {n: [] for n in names}
    blocks = 2 if a.only_rounds is None else 1
    for _ in range(blocks):
        for name in names:
            weight = configure(name)
            capped_fit(weight)
            capped_fit(weight)
            for _ in range(max(1, a.reps // blocks)):
                per[name].append(timed(lambda: capped_fit(weight)) / rounds)
    fmt = '%-52s median %9.3f ms  min %9.3f  max %9.3f  (%d reps)'
    med = {}
    for name in names:
        med[name] = stats(per[name])[0]
        print(fmt % (('chained round: %s' % name,) + stats(per[name]) + (len(per[name]),)))
    if a.only_rounds is None:
        add = {n: med[n] - med['none'] for n in names}
        print('additions over `none` (medians): ' + ', '.join('%s %.3f ms' % (n, add[n]) for n in names if n != 'none'))
        print('mix sil+vt adds %.3f ms, silhouette + vertex-target add %.3f ms: %.3f ms saved'
              % (add['mix sil+vt'], add['silhouette'] + add['vertex-target'],
                 add['silhouette'] + add['vertex-target'] - add['mix sil+vt']))
        print('mix all adds %.3f ms, the three single terms add %.3f ms: %.3f ms saved'
              % (add['mix all'], add['scene'] + add['silhouette'] + add['vertex-target'],
                 add['scene'] + add['silhouette'] + add['vertex-target'] - add['mix all']))
        print('a mix round against the SUM of the single-term rounds: sil+vt %.3f vs %.3f ms, all %.3f vs %.3f ms'
              % (med['mix sil+vt'], med['silhouette'] + med['vertex-target'], med['mix all'],
                 med['scene'] + med['silhouette'] + med['vertex-target']))
    configure('none')
    eng.clear_silhouette_term()
    eng.close()


if __name__ == '__main__':
    main()
