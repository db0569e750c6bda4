"""Timing of the surface landmark term: the op alone (include/mvfit.h:mvfit_landmark_loss) and a chained round with the term
(mvfit_set_landmark_term) against a chained round with the vertex-target term on the same problems.

  python tools/landmark_fit_timing.py [--reps 30] [--bodies 32] [--rounds 96]

Workload: ``bodies`` synthetic bodies (the bodies of tools/vertex_target_fit_timing.py), every problem and every target live.
Medians of ``reps`` after a warm-up, from device events:
  op              landmark_loss with the gradient, 20 calls inside one pair of events, at 8 views x 6 landmarks (one vertex
                  each: the feet) and at 16 views x 256 landmarks (1, 2 and 4 vertices in turn: both maxima).
  chained round   8 views; a fit whose tolerances are 0 and whose round cap is ``rounds`` (a multiple of 24, the rounds of one
                  graph replay): no problem finishes, the fit stops at the cap (reported as an error, which is expected here)
                  and the time of the call / ``rounds`` is one round.  With the landmark term (6 landmarks) and with the
                  vertex-target term (K = 2, tools/vertex_target_fit_timing.py's) on a second engine with the same
                  problems, the repetitions of the two interleaved in this one run; each term at the weight that makes it as
                  large as the keypoint objective.
Run every invocation under a time limit of its own."""
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


def table(L, nv, rng):
    """ids [L,4], weights [L,4]: landmark l names (1, 2, 4)[l % 3] distinct vertices (L = 6: one each)"""
    ids, w = np.zeros((L, 4), np.int32), np.zeros((L, 4), np.float32)
    for l in range(L):
        n = 1 if L == 6 else (1, 2, 4)[l % 3]
        ids[l, :n] = rng.choice(nv, n, replace=False)
        w[l, :n] = 1.0 / n
    return ids, w


def problems(eng, N, V, x):
    rig = syn.make_camera_ring(V)
    eng.set_problems(rig, np.zeros((N, V, 17, 2), np.float32), np.zeros((N, V, 17), np.float32))
    _, jd = eng.vertices(x)
    gt, conf = syn.make_observations(jd.cpu().numpy(), rig, seed=3, noise_px=0.5)
    eng.set_problems(rig, gt, conf)
    return rig


def landmarks(eng, rig, L, y, rng):
    """table and targets: the landmarks of the perturbed bodies ``y`` seen in every view, confidence 1"""
    ids, w = table(L, eng.nv, rng)
    vy = eng.vertices(y)[0].cpu().numpy().astype(np.float64)
    p = np.einsum('lk,blkc->blc', w.astype(np.float64), vy[:, ids])
    xy = syn.project_points(p, *rig).astype(np.float32)
    eng.set_landmarks(ids, w)
    eng.set_landmark_targets(xy, np.ones(xy.shape[:-1], np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--bodies', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=96)
    a = ap.parse_args()
    N = a.bodies
    rounds = max(24, a.rounds // 24 * 24)
    eng = MvFit(body_model())
    x = pack_params(B=N, **syn.make_frames(N))
    rng = np.random.default_rng(8)
    ys = []
    for _ in range(2):
        y = x.copy()
        y[:, 10:82] += rng.normal(0, 0.05, (N, 72)).astype(np.float32)
        y[:, 82:85] += rng.normal(0, 0.02, (N, 3)).astype(np.float32)
        ys.append(y)
    fmt = '%-58s median %9.4f ms  min %9.4f  max %9.4f  (%d reps)'
    calls = 20
    for V, L in ((16, 256), (8, 6)):                    # (the round's shape last: its problems stay set)
        rig = problems(eng, N, V, x)
        landmarks(eng, rig, L, ys[0], rng)
        v0 = eng.vertices(x)[0]
        loss, g = torch.empty(N, device=eng.device), torch.empty_like(v0)

        def op():
            for _ in range(calls):
                eng._check(eng._lib.mvfit_landmark_loss(eng._ctx, v0.data_ptr(), 100.0, 0.0, 0.0, loss.data_ptr(), g.data_ptr()))

        op()
        torch.cuda.synchronize()
        po = [timed(op) / calls for _ in range(a.reps)]
        print(fmt % (('landmark_loss with gradient, %d bodies x %d views x %d landmarks' % (N, V, L),) + stats(po) + (a.reps,)))
    base = stage_weights(1536.0)[3]
    data = eng.closure(x, base, want_grad=False)['loss']
    L_lm = eng.landmark_loss(v0, need_grad=False)[0]
    # the vertex-target term on an engine of its own with the same problems: each engine keeps its captured round graph, and
    # the repetitions of the two alternate
    eng_vt = MvFit(body_model())
    problems(eng_vt, N, 8, x)
    eng_vt.set_vertex_targets(torch.stack([eng_vt.vertices(y)[0] for y in ys], dim=1), np.ones((N, 2), np.float32))
    L_vt = eng_vt.vertex_target_loss(eng_vt.vertices(x)[0], need_grad=False)[0]
    w = dict(landmark=float(torch.sqrt(data.mean() / L_lm.mean())), vertex_target=float(torch.sqrt(data.mean() / L_vt.mean())))
    print('%d bodies x 8 views: mean landmark loss %.5g (w %.4g), mean vertex-target loss %.5g (w %.4g)'
          % (N, float(L_lm.mean()), w['landmark'], float(L_vt.mean()), w['vertex_target']))
    never = dict(tolerance_grad=0.0, tolerance_change=0.0, ftol=0.0, gtol=0.0, max_iter=100000, maxiters=100000, max_rounds=rounds)
    eng.set_landmark_term()
    eng_vt.set_vertex_target_term()
    engines = dict(landmark=eng, vertex_target=eng_vt)

    def capped_fit(term):
        try:
            engines[term].fit(x, [dict(base, coll_loss_weight=w[term])], **never)
        except MvFitError as e:
            if 'round cap' not in str(e):
                raise
        else:
            raise RuntimeError('the fit finished before the round cap: the rounds were not all live')

    per = dict(landmark=[], vertex_target=[])
    for term in per:
        capped_fit(term)
        capped_fit(term)
    for _ in range(a.reps):
        for term in per:
            per[term].append(timed(lambda: capped_fit(term)) / rounds)
    print(fmt % (('chained round with the vertex-target term (K = 2)',) + stats(per['vertex_target']) + (a.reps,)))
    print(fmt % (('chained round with the landmark term (6 landmarks)',) + stats(per['landmark']) + (a.reps,)))
    eng.close()
    eng_vt.close()


if __name__ == '__main__':
    main()
