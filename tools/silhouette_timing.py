"""Timing of the silhouette term (include/mvfit.h:mvfit_set_silhouettes / mvfit_silhouette_loss, csrc/silhouette.hip) next to
the same loss composed in PyTorch on the same GPU: grid_sample with border padding on the op's own distance fields plus
cdist / argmin for the contour term, gradient by autograd.

  python tools/silhouette_timing.py [--reps 30] [--bodies 32] [--views 8] [--width 512] [--height 384] [--only-op]

Workload: ``bodies`` synthetic bodies (6890 vertices, random shape and pose) seen by a ring of ``views`` cameras; the masks
are rendered from displaced copies (other betas, 3 cm off, scale 1.05), so both terms are active.  Prints medians of ``reps``
calls after a warm-up, from hipEvents around the call: the set, the loss with and without g_vertices, the composition.
--only-op runs the op alone (the run to put under rocprofv3 --kernel-trace --stats for the per-kernel split).  Run every
invocation under a time limit of its own."""
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


def composed(v, field, first, xy, image_body, cams, backward):
    """loss[N] from torch ops (sigma = 0, w_in = w_out = 1, contour_stride = 1, every vertex in front of its camera)."""
    v = v.detach().requires_grad_(backward)
    R, t, f, c = cams
    M, H, W = field.shape
    loss = v.new_zeros(v.shape[0], dtype=torch.float64)
    for i in range(M):
        n = int(image_body[i])
        p = v[n] @ R[i].T + t[i]
        uv = f[i] * p[:, :2] / p[:, 2:3] + c[i]
        g = (uv - 0.5) / uv.new_tensor([W - 1.0, H - 1.0]) * 2.0 - 1.0
        d = torch.nn.functional.grid_sample(field[i][None, None], g[None, None], mode='bilinear', padding_mode='border',
                                            align_corners=True).view(-1)
        a = (d.double() ** 2).sum()
        pts = xy[first[i]:first[i + 1]].to(v.dtype) + 0.5
        if len(pts):
            m = torch.cdist(pts, uv.detach()).argmin(dim=1)
            a = a + ((uv[m] - pts).double() ** 2).sum()
        loss = loss.index_add(0, torch.tensor([n], device=v.device), a[None])
    if backward:
        loss.sum().backward()
    return loss, v.grad


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
    ap.add_argument('--bodies', type=int, default=32)
    ap.add_argument('--views', type=int, default=8)
    ap.add_argument('--width', type=int, default=512)
    ap.add_argument('--height', type=int, default=384)
    ap.add_argument('--only-op', action='store_true')
    a = ap.parse_args()
    N, V, H, W = a.bodies, a.views, a.height, a.width
    eng = MvFit(body_model())
    R, t, f, c = syn.make_camera_ring(V)
    f = (f * np.float32(W / 2048.0)).astype(np.float32)
    c = np.tile(np.array([W / 2.0, H / 2.0], np.float32), (V, 1))
    eng.set_problems((R, t, f, c), np.zeros((N, V, 17, 2), np.float32), np.zeros((N, V, 17), np.float32))
    x = pack_params(B=N, **syn.make_frames(N))
    xd = x.copy()
    xd[:, 0:10] += np.random.default_rng(8).normal(0, 0.8, (N, 10)).astype(np.float32)
    xd[:, 82:85] += np.float32([0.03, -0.02, 0.01])
    xd[:, 85] = 1.05
    v = eng.vertices(x)[0].contiguous()
    image_body = np.repeat(np.arange(N), V).astype(np.int32)
    view = np.tile(np.arange(V), N)
    masks = torch.empty(N * V, H, W, dtype=torch.uint8, device=eng.device)
    vd = eng.vertices(xd)[0]
    for b in range(N):                                   # one body's views per call: the background stays small
        _, fid = eng.render_overlay(vd, None, np.zeros((V, H, W, 3), np.uint8), image_body[b * V:(b + 1) * V], view[:V],
                                    face_id=True)
        masks[b * V:(b + 1) * V] = (fid >= 0).to(torch.uint8)
    cams = tuple(np.ascontiguousarray(q[view]) for q in (R, t, f, c))
    eng.set_silhouettes(masks, image_body, cams)
    field, first, xy = eng.silhouettes()
    loss, g = eng.silhouette_loss(v)
    print('%d bodies x %d views at %d x %d: %d contour points (%.0f per image), mean loss %.5g'
          % (N, V, W, H, len(xy), len(xy) / (N * V), float(loss.mean())))
    fmt = '%-44s median %9.3f ms  min %9.3f  max %9.3f  (%d reps)'
    for name, fn in (('set (fields and contours)', lambda: eng.set_silhouettes(masks, image_body, cams)),
                     ('op, loss and g_vertices', lambda: eng.silhouette_loss(v)),
                     ('op, loss only', lambda: eng.silhouette_loss(v, need_grad=False))):
        print(fmt % ((name,) + median_ms(fn, a.reps) + (a.reps,)))
    if a.only_op:
        eng.close()
        return
    tc = tuple(torch.from_numpy(q).to(eng.device) for q in cams)
    first_h = first.cpu().numpy()
    lc, gc = composed(v, field, first_h, xy, image_body, tc, True)
    print('composition vs op: loss max rel diff %.2e, gradient max diff / max %.2e'
          % (float(((lc.float() - loss).abs() / loss.abs().clamp_min(1e-30)).max()), float((gc - g).abs().max() / g.abs().max())))
    reps = max(3, a.reps // 10)
    for name, bw in (('torch composition, forward and backward', True), ('torch composition, forward only', False)):
        print(fmt % ((name,) + median_ms(lambda: composed(v, field, first_h, xy, image_body, tc, bw), reps) + (reps,)))
    eng.close()


if __name__ == '__main__':
    main()
