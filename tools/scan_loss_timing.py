"""Timing of the scan loss (include/mvfit.h:mvfit_scan_loss; csrc/scan_loss.hip) next to the test oracle's chunked torch port
(tests/scan_oracle.py:torch_scan_loss, fp32, winners searched without a graph, gradient by autograd) on the same GPU.

  python tools/scan_loss_timing.py [--bodies 32] [--points 8192] [--reps 30] [--baseline-bodies 4] [--baseline-reps 3] [--out FILE]

Workload: the full 6890-vertex model at ``bodies`` make_frames poses, per body ``points`` barycentric samples of its own posed
surface plus 5 mm of Gaussian noise.  One evaluation = loss and vertex gradient.  Milliseconds are medians of ``reps``
evaluations after two warm-up calls, from hipEvents around the call; search 'auto' and 'exhaustive', w_m2s 0 and 1.  The torch port
works body by body at the same cost each, so it is timed on the first ``baseline-bodies`` bodies only and the table gives
that time and, marked as scaled, that time times bodies / baseline-bodies.  The report is Markdown on stdout and, with --out, in that file."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, reps, warm=2):
    import torch
    for _ in range(warm):
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
    ap.add_argument('--bodies', type=int, default=32)
    ap.add_argument('--points', type=int, default=8192)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--baseline-bodies', type=int, default=4)
    ap.add_argument('--baseline-reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from mvsmplfitting_amd import synthetic as syn
    from mvsmplfitting_amd.layer import BodyLayer
    from tests import scan_oracle as so
    if not torch.cuda.is_available():
        raise SystemExit('scan_loss_timing: no GPU - this tool measures on the device only')
    N, P = a.bodies, a.points
    nb = max(1, min(N, a.baseline_bodies))
    model = syn.make_body_model(skin_topk=4)
    faces = np.asarray(model['faces'], np.int64)
    layer = BodyLayer(model)
    eng = layer.engine
    fr = {k: torch.from_numpy(v) for k, v in syn.make_frames(N, seed0=7000).items()}
    with torch.no_grad():
        verts = layer(fr['betas'], fr['global_orient'], fr['body_pose'], transl=fr['transl'], scale=fr['scale']).vertices.contiguous()
    rng = np.random.default_rng(1)
    v = verts.cpu().numpy().astype(np.float64)
    points = np.zeros((N, P, 3), np.float32)
    for n in range(N):
        f = faces[rng.integers(0, len(faces), P)]
        u = rng.random((P, 2))
        flip = u.sum(axis=1) > 1
        u[flip] = 1.0 - u[flip]
        points[n] = (v[n][f[:, 0]] + u[:, :1] * (v[n][f[:, 1]] - v[n][f[:, 0]]) + u[:, 1:] * (v[n][f[:, 2]] - v[n][f[:, 0]])
                     + rng.normal(0, 0.005, (P, 3)))
    count = np.full(N, P, np.int32)
    eng.set_scans(points, count)
    pts_dev = torch.from_numpy(points).to(eng.device)
    rows = []
    for w_m2s in (0.0, 1.0):
        got = {}
        for search in ('auto', 'exhaustive'):
            fn = lambda: eng.scan_loss(verts, w_s2m=1.0, w_m2s=w_m2s, search=search)
            got[search] = fn()
            rows.append(('libmvfit, search=%s, w_m2s=%g' % (search, w_m2s),) + median_ms(fn, a.reps))
        same = all(torch.equal(x, y) for x, y in zip(got['auto'], got['exhaustive']))

        def baseline():
            vv = verts[:nb].clone().requires_grad_(True)
            loss = so.torch_scan_loss(vv, faces, pts_dev[:nb], count[:nb], None, w_s2m=1.0, w_m2s=w_m2s, chunk=256)
            loss.sum().backward()
            return loss.detach(), vv.grad
        ref = baseline()
        rel = float((got['auto'][0][:nb] - ref[0]).abs().max() / ref[0].abs().max())
        base = median_ms(baseline, a.baseline_reps, warm=0)
        rows.append(('torch port (fp32, chunks of 256), %d of the %d bodies, w_m2s=%g' % (nb, N, w_m2s),) + base)
        rows.append(('torch port, scaled to %d bodies (x %g), w_m2s=%g' % (N, N / nb, w_m2s),) + tuple(x * N / nb for x in base))
        rows.append(('  auto == exhaustive bit for bit: %s; loss vs torch port: %.2e relative' % (same, rel), None, None, None))
    eng.clear_scans()
    lines = ['scan loss with gradient: %d bodies x %d points, %d vertices, %d faces, %s' %
             (N, P, verts.shape[1], len(faces), torch.cuda.get_device_name(0)), '',
             '| evaluation | median ms | min | max |', '|---|---|---|---|']
    for name, med, lo, hi in rows:
        lines.append('| %s | %s |' % (name, ' | '.join('' if x is None else '%.3f' % x for x in (med, lo, hi))))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
