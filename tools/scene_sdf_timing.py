"""Timing of the scene collision loss (include/mvfit.h:mvfit_scene_sdf_loss, csrc/scene_sdf.hip) next to the same loss
composed from what the library offered before it: MvFit.sdf for the fields plus boxes, grid_sample and autograd in PyTorch
on the GPU.

  python tools/scene_sdf_timing.py [--reps 30] [--scenes 32] [--bodies 4] [--grid 32] [--only-op]

Workload: ``scenes`` scenes of ``bodies`` synthetic bodies (6890 vertices / 13776 faces, random shape and pose, standing
0.25 m apart so that neighbours interpenetrate), robustifier 0.05.  Prints medians of ``reps`` calls after a warm-up, from
hipEvents around the call: the op with and without g_vertices, and the composition with and without backward.
--only-op runs the op alone (the run to put under rocprofv3 --kernel-trace --stats for the per-kernel split)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mvsmplfitting_amd import synthetic as syn  # noqa: E402
from mvsmplfitting_amd.engine import MvFit, pack_params  # noqa: E402
from tests.helpers import body_model  # noqa: E402


def composed(eng, v, faces, sizes, G, scale_factor, r, backward):
    """The loss of every scene from MvFit.sdf + torch: what a caller could write on the parent commit."""
    v = v.detach().requires_grad_(backward)
    losses, b0 = [], 0
    with torch.no_grad():
        lo, hi = v.min(dim=1)[0], v.max(dim=1)[0]
        c = torch.stack([lo, hi], dim=1).mean(dim=1)
        s = (1 + scale_factor) * 0.5 * (hi - lo).max(dim=-1)[0]
        phi = eng.sdf(faces, (v - c[:, None]) / s[:, None, None], grid_size=G)
    for P in sizes:
        loss = v.new_zeros(())
        if P > 1:
            vs = v[b0:b0 + P]
            for i in range(P):
                x = (vs - c[b0 + i]) / s[b0 + i]
                p = torch.nn.functional.grid_sample(phi[b0 + i][None, None], x.view(1, -1, 1, 1, 3), align_corners=False).view(P, -1)
                w = torch.ones(P, 1, device=v.device)
                w[i, 0] = 0.0
                p = w * p
                if r:
                    f = (p / r) ** 2
                    p = f / (f + 1)
                loss = loss + p.sum() / P ** 2
        losses.append(loss)
        b0 += P
    losses = torch.stack(losses)
    if backward:
        losses.sum().backward()
    return losses, v.grad


def median_ms(fn, reps):
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
    ap.add_argument('--only-op', action='store_true')
    a = ap.parse_args()
    model = body_model()
    eng = MvFit(model)
    N, G, r = a.scenes * a.bodies, a.grid, 0.05
    cams = syn.make_camera_ring(1)
    eng.set_problems(cams, np.zeros((N, 1, 17, 2), np.float32), np.zeros((N, 1, 17), np.float32))
    x = pack_params(B=N, **syn.make_frames(N))
    x[:, 82:85] = 0.0
    x[:, 82] = 0.25 * (np.arange(N) % a.bodies)
    v = eng.vertices(x)[0].contiguous()
    faces = torch.tensor(np.asarray(model['faces'], np.int32), device=eng.device)
    sizes = [a.bodies] * a.scenes
    loss, g, _ = eng.scene_sdf_loss(v, faces, scene_sizes=sizes, grid_size=G, robustifier=r)
    print('%d scenes x %d bodies, G = %d: mean loss %.4f, %.1f%% of the vertices carry gradient, fields by %s'
          % (a.scenes, a.bodies, G, float(loss.mean()), 100 * float((g.abs().sum(dim=-1) > 0).float().mean()), eng.sdf_info()['op']))
    for name, fn in (('op, loss and g_vertices', lambda: eng.scene_sdf_loss(v, faces, scene_sizes=sizes, grid_size=G, robustifier=r)),
                     ('op, loss only', lambda: eng.scene_sdf_loss(v, faces, scene_sizes=sizes, grid_size=G, robustifier=r, need_grad=False))):
        print('%-42s median %8.3f ms  min %8.3f  max %8.3f  (%d reps)' % ((name,) + median_ms(fn, a.reps) + (a.reps,)))
    if a.only_op:
        return
    lc, gc = composed(eng, v, faces, sizes, G, 0.2, r, True)
    lc = lc.detach()
    print('composition vs op: loss max rel diff %.2e, gradient max diff / max %.2e'
          % (float(((lc - loss).abs() / loss.abs().clamp_min(1e-30)).max()), float((gc - g).abs().max() / g.abs().max())))
    for name, bw in (('MvFit.sdf + torch, forward and backward', True), ('MvFit.sdf + torch, forward only', False)):
        print('%-42s median %8.3f ms  min %8.3f  max %8.3f  (%d reps)'
              % ((name,) + median_ms(lambda: composed(eng, v, faces, sizes, G, 0.2, r, bw), a.reps) + (a.reps,)))
    eng.close()


if __name__ == '__main__':
    main()
