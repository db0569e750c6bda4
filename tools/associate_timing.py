"""Timing of the cross-view association (include/mvfit.h:mvfit_associate_views, csrc/associate.hip) next to the same cost
matrix composed in vectorised PyTorch on the GPU and to the NumPy oracle on the host.

  python tools/associate_timing.py [--reps 30] [--frames 1024] [--views 16] [--det 8] [--only-op]

Workload: ``frames`` frames of ``det`` persons (17 points in a 0.7 x 1.7 x 0.4 m box, a metre apart on a grid) seen by a
ring of ``views`` cameras with 3 px noise, every view listing them in its own shuffled order: D = views * det detections
per frame, frames * D * (D - 1) / 2 * 17 ray pairs less the same-view ones.  Prints medians of ``reps`` calls after a
warm-up, from hipEvents around the call.  --only-op runs the op alone (the run to put under rocprofv3 --kernel-trace
--stats for the per-kernel split)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mvsmplfitting_amd import synthetic as syn  # noqa: E402
from mvsmplfitting_amd.engine import MvFit  # noqa: E402
from tests import associate_oracle as ao  # noqa: E402
from tests.helpers import body_model  # noqa: E402


def workload(F, V, N, seed=0):
    rng = np.random.default_rng(seed)
    K, E = ao.camera_matrices(syn.make_camera_ring(V))
    side = int(np.ceil(np.sqrt(N)))
    centres = np.array([[(p % side) - (side - 1) / 2.0, 0.0, (p // side) - (side - 1) / 2.0] for p in range(N)])
    pts = centres[None, :, None, :] + (rng.random((F, N, 17, 3)) - 0.5) * [0.7, 1.7, 0.4]
    uv = ao.project(pts, K, E)                                             # [V, F, N, 17, 2]
    uv = uv + rng.normal(0, 3.0, uv.shape)
    kp = np.concatenate([uv, rng.uniform(0.5, 1.0, uv.shape[:-1] + (1,))], -1).transpose(1, 0, 2, 3, 4)
    order = np.argsort(rng.random((F, V, N)), axis=2)
    kp = np.take_along_axis(kp, order[..., None, None], axis=2).astype(np.float32)
    return np.ascontiguousarray(kp), np.full((F, V), N, np.int32), order.astype(np.int32), K, E


def torch_cost(kp, K, E, min_joints, chunk=64):
    """The cost matrix [F, D, D] in vectorised float64 PyTorch: what a caller could write without the op."""
    F, V, N = kp.shape[:3]
    D = V * N
    Ki = torch.linalg.inv(K)
    R, t = E[:, :3, :3], E[:, :3, 3]
    org = -(R.transpose(1, 2) @ t[:, :, None])[:, :, 0]                     # [V, 3]
    out = torch.empty(F, D, D, dtype=torch.float64, device=kp.device)
    view = torch.arange(V, device=kp.device).repeat_interleave(N)
    b_ = (org[view][None, :] - org[view][:, None])                          # [D, D, 3]: o_b - o_a
    for f0 in range(0, F, chunk):
        k = kp[f0:f0 + chunk].double()
        pix = torch.cat([k[..., :2], torch.ones_like(k[..., :1])], -1)
        n = torch.einsum('vij,fvnkj->fvnki', Ki, pix)
        n = n / n.norm(dim=-1, keepdim=True)
        d = torch.einsum('vji,fvnkj->fvnki', R, n).reshape(-1, D, 17, 3)
        cf = k[..., 2].reshape(-1, D, 17)
        c = torch.cross(d[:, :, None].expand(-1, -1, D, -1, -1), d[:, None].expand(-1, D, -1, -1, -1), dim=-1)
        dist = (b_[None, :, :, None, :] * c).sum(-1).abs() / c.norm(dim=-1)
        w = (cf[:, :, None] * cf[:, None]).sqrt()
        on = w > 0
        cost = (w * torch.where(on, dist, torch.zeros_like(dist))).sum(-1) / w.sum(-1)
        bad = (on.sum(-1) < min_joints) | (view[:, None] == view[None, :])[None]
        out[f0:f0 + chunk] = torch.where(bad, torch.full_like(cost, float('inf')), cost)
    return out


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
    ap.add_argument('--frames', type=int, default=1024)
    ap.add_argument('--views', type=int, default=16)
    ap.add_argument('--det', type=int, default=8)
    ap.add_argument('--only-op', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('associate_timing: no GPU - this tool measures on the device only')
    F, V, N = a.frames, a.views, a.det
    D = V * N
    kp_h, count_h, order, K_h, E_h = workload(F, V, N)
    eng = MvFit(body_model())
    dev = eng.device
    kp, count = torch.as_tensor(kp_h, device=dev), torch.as_tensor(count_h, device=dev)
    K, E = torch.as_tensor(K_h, device=dev), torch.as_tensor(E_h, device=dev)
    labels, num, cost = eng.associate_views(kp, count, K, E, return_cost=True)
    lab = labels.cpu().numpy()
    person = np.take_along_axis(np.broadcast_to(np.arange(N)[None, None], order.shape), order, axis=2)    # slot -> person
    ok = sum(ao.same_partition(lab[f], person[f]) for f in range(F))
    pairs = F * (D * (D - 1) // 2 - V * (N * (N - 1) // 2)) * 17
    print('%d frames x %d views x %d detections (D = %d): %.3g ray pairs; %d of %d frames recover the persons exactly, '
          'clusters per frame %d..%d' % (F, V, N, D, pairs, ok, F, int(num.min()), int(num.max())))
    for name, fn in (('op, labels only', lambda: eng.associate_views(kp, count, K, E)),
                     ('op, labels and cost matrix', lambda: eng.associate_views(kp, count, K, E, return_cost=True))):
        print('%-42s median %8.3f ms  min %8.3f  max %8.3f  (%d reps)' % ((name,) + median_ms(fn, a.reps) + (a.reps,)))
    if a.only_op:
        eng.close()
        return
    ct = torch_cost(kp, K, E, 6)
    fin = torch.isfinite(cost)
    assert torch.equal(fin, torch.isfinite(ct))
    print('torch composition vs op: cost max abs diff %.2e m' % float((ct[fin] - cost[fin]).abs().max()))
    del ct
    print('%-42s median %8.3f ms  min %8.3f  max %8.3f  (%d reps)'
          % (('torch composition, cost matrix only',) + median_ms(lambda: torch_cost(kp, K, E, 6), max(3, a.reps // 6))
             + (max(3, a.reps // 6),)))
    t0 = time.perf_counter()
    c0, l0, n0 = ao.associate(kp_h[:1], count_h[:1], K_h, E_h)
    t_np = time.perf_counter() - t0
    same = np.array_equal(c0.view(np.uint64), cost[:1].cpu().numpy().view(np.uint64)) and np.array_equal(l0, lab[:1])
    print('NumPy oracle on the host, one frame: %.1f ms (x %d frames = %.1f s); bits equal to the op: %s'
          % (1e3 * t_np, F, t_np * F, same))
    eng.close()


if __name__ == '__main__':
    main()
