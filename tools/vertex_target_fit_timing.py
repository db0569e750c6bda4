"""Timing of the vertex-target term inside the fit (include/mvfit.h:mvfit_set_vertex_target_term) and of the op alone.

  python tools/vertex_target_fit_timing.py [--reps 30] [--bodies 32] [--views 8] [--targets 2] [--rounds 96] [--only-rounds]

Workload: ``bodies`` synthetic bodies x ``views`` cameras (the bodies of tools/silhouette_fit_timing.py), every problem with
``targets`` target sets of weight 1 (the vertices of perturbed parameters) and every problem live.  Medians of ``reps`` after
a warm-up, from device events:
  chained round   a fit whose tolerances are 0 and whose round cap is ``rounds`` (a multiple of 24, the rounds of one graph
                  replay): no problem finishes, the fit stops at the cap (reported as an error, which is expected here) and
                  the time of the call / ``rounds`` is one round.  With the term (weight w) and, under round_mode = 1, the same
                  rounds with weight 0 (vertex pass and step kernel alone).  The call's fixed part (initialisation, results,
                  one host wait per replay) is inside both.
  op              vertex_target_loss with the gradient, 20 calls inside one pair of events.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--bodies', type=int, default=32)
    ap.add_argument('--views', type=int, default=8)
    ap.add_argument('--targets', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=96)
    ap.add_argument('--only-rounds', action='store_true')
    a = ap.parse_args()
    N, V, K = a.bodies, a.views, a.targets
    rounds = max(24, a.rounds // 24 * 24)
    eng = MvFit(body_model())
    rig = syn.make_camera_ring(V)
    x = pack_params(B=N, **syn.make_frames(N))
    eng.set_problems(rig, np.zeros((N, V, 17, 2), np.float32), np.zeros((N, V, 17), np.float32))
    _, jd = eng.vertices(x)
    gt, conf = syn.make_observations(jd.cpu().numpy(), rig, seed=3, noise_px=0.5)
    eng.set_problems(rig, gt, conf)
    rng = np.random.default_rng(8)
    rows = []
    for _ in range(K):
        y = x.copy()
        y[:, 10:82] += rng.normal(0, 0.05, (N, 72)).astype(np.float32)
        y[:, 82:85] += rng.normal(0, 0.02, (N, 3)).astype(np.float32)
        rows.append(eng.vertices(y)[0])
    eng.set_vertex_targets(torch.stack(rows, dim=1), np.ones((N, K), np.float32))
    v0 = eng.vertices(x)[0]
    L = eng.vertex_target_loss(v0, need_grad=False)[0]
    base = stage_weights(1536.0)[3]
    data = eng.closure(x, base, want_grad=False)['loss']
    w = float(torch.sqrt(data.mean() / L.mean()))
    print('%d bodies x %d views, %d target sets: %.1f MB read per evaluation, mean loss %.5g, w %.4g'
          % (N, V, K, N * (1 + K) * eng.nv * 12 / 1e6, float(L.mean()), w))
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
    eng.set_vertex_target_term()
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
    eng.clear_vertex_target_term()
    if not a.only_rounds:
        calls = 20
        loss, g = torch.empty(N, device=eng.device), torch.empty_like(v0)

        def op():
            for _ in range(calls):
                eng._check(eng._lib.mvfit_vertex_target_loss(eng._ctx, v0.data_ptr(), loss.data_ptr(), g.data_ptr()))

        op()
        torch.cuda.synchronize()
        po = [timed(op) / calls for _ in range(a.reps)]
        print(fmt % (('vertex_target_loss with gradient (op alone)',) + stats(po) + (a.reps,)))
    eng.close()


if __name__ == '__main__':
    main()
