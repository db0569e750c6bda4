"""Developer tool: the cost of one closure round of the staged fit for the two body-model kinds side by side - 'smpllsp'
(keypoints from the LSP regressor, 69 objective vertices) and 'smpl' (posed skeleton joints + 5 face vertices) - on bench.py's
synthetic inputs (configs[1] shape: 32 frames x 8 views, top-4 skinning, L2 prior).  bench.py cannot select the model kind.
    python tools/smpl_round_timing.py [--frames 32] [--views 8] [--reps 5]
Prints one JSON line: per kind the median fit time over the repetitions and us_per_round = fit time / closure rounds."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from mvsmplfitting_amd import synthetic as syn  # noqa: E402
from mvsmplfitting_amd.engine import MvFit, stage_weights  # noqa: E402
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--views', type=int, default=8)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    out = {}
    for kind in ('smpllsp', 'smpl'):
        model = syn.make_body_model(0, skin_topk=4, model_type=kind)
        eng = MvFit(model)
        cams, gt, conf, x0 = bench.build_inputs(eng, syn, 0, a.frames, 1, a.views)
        if kind == 'smpl':
            eng.set_problems(cams, gt, conf * syn.COCO17_JOINT_WEIGHTS)
        stages = stage_weights(1536.0)
        eng.fit(x0, stages)                                  # warm-up
        ms, rounds = [], 0
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            xf, st = eng.fit(x0, stages)
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
            rounds = int(st['n_closure'].max().item())
            assert st['passes']['run'] > 0 and st['passes']['missed'] == 0 and st['passes']['timed_out'] == 0, st['passes']
        t = float(np.median(ms))
        out[kind] = dict(fit_ms=round(t, 3), closure_rounds=rounds, us_per_round=round(1e3 * t / max(rounds, 1), 2),
                         final_loss_median=float(st['final_loss'].median().item()))
        eng.close()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
