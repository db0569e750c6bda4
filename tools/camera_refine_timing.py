"""Timing of the camera refinement ops (include/mvfit.h:mvfit_camera_normal_eqs, mvfit_refine_cameras;
csrc/camera_refine.hip) next to their NumPy oracle on the host.

  python tools/camera_refine_timing.py [--reps 30] [--shapes 32x8,4096x16] [--limit 240] [--out FILE]

Workload per shape B x V: B bodies of 17 random points seen by a ring of V cameras 3.5 m away with 30 px noise and 10 % zero
weights, every camera started 2.5 degrees and 7 cm off (tests/camera_refine_oracle.py:make_case).  Medians of ``reps`` (at least
20) launches after a warm-up, from hipEvents around the call; the oracle's time is that of ONE view, times V.  Each shape runs in
a child process of its own under a time limit of ``limit`` seconds; a child that fails or runs out of time ends the tool, nothing
further is started on the device.  The report is Markdown on stdout and, with --out, in that file (profiles/camera_refine.md
holds one)."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, reps):
    import torch
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


def child(B, V, reps):
    import torch
    from mvsmplfitting_amd.engine import MvFit, unpack_cameras
    from tests import camera_refine_oracle as co
    from tests.helpers import body_model
    if not torch.cuda.is_available():
        raise SystemExit('camera_refine_timing: no GPU - this tool measures on the device only')
    joints, gt, w, true, start = co.make_case(B, V, seed=3, noise=30.0)
    eng = MvFit(body_model())
    eng.set_problems(unpack_cameras(start, np.float32), gt, w)
    j = torch.as_tensor(joints, device=eng.device)
    cm = torch.as_tensor(start, device=eng.device)
    cams, rep = eng.refine_cameras(j, cm, free='all')
    rep = rep.cpu().numpy()
    rows = []
    for name, fn in (('camera_normal_eqs, E only', lambda: eng.camera_normal_eqs(j, cm, need_grad=False)),
                     ('camera_normal_eqs, E, g, H', lambda: eng.camera_normal_eqs(j, cm)),
                     ("refine_cameras, free='extrinsics'", lambda: eng.refine_cameras(j, cm)),
                     ("refine_cameras, free='all'", lambda: eng.refine_cameras(j, cm, free='all'))):
        rows.append((name,) + median_ms(fn, reps))
    t0 = time.perf_counter()
    E, g, H, count = co.normal_eqs(joints, gt[:, 0], w[:, 0], start[0])
    t_ne = time.perf_counter() - t0
    t0 = time.perf_counter()
    a, ra = co.lm(joints, gt[:, 0], w[:, 0], start[0], free_mask=15)
    t_lm = time.perf_counter() - t0
    dev = eng.camera_normal_eqs(j, cm)
    err = abs(float(dev['E'][0]) - E) / E
    print('### B = %d, V = %d (%d points per view)\n' % (B, V, B * 17))
    print('| call | median ms | min | max | reps |\n|---|---|---|---|---|')
    for name, med, lo, hi in rows:
        print('| %s | %.3f | %.3f | %.3f | %d |' % (name, med, lo, hi, reps))
    print('| NumPy oracle on the host, normal_eqs of one view (x %d views) | %.3f (%.1f) | | | 1 |' % (V, 1e3 * t_ne, 1e3 * t_ne * V))
    print('| NumPy oracle on the host, lm of one view, all free (x %d views) | %.1f (%.1f) | | | 1 |' % (V, 1e3 * t_lm, 1e3 * t_lm * V))
    print("\nfree='all': iterations per view %s, statuses %s; view 0: device %d iterations, oracle %d; E of view 0 device vs "
          'oracle %.1e relative.\n' % (rep[:, 2].astype(int).tolist(), rep[:, 4].astype(int).tolist(), rep[0, 2], ra[2], err))
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--shapes', default='32x8,4096x16')
    ap.add_argument('--limit', type=int, default=240)
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', nargs=2, type=int, default=None)
    a = ap.parse_args()
    reps = max(20, a.reps)
    if a.child:
        child(a.child[0], a.child[1], reps)
        return
    text = ['## Measured times\n']
    for shape in a.shapes.split(','):
        B, V = (int(x) for x in shape.split('x'))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', str(B), str(V), '--reps', str(reps)],
                           capture_output=True, text=True, timeout=a.limit)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit('camera_refine_timing: shape %s ended with status %d; nothing further is started' % (shape, r.returncode))
        text.append(r.stdout)
    out = '\n'.join(text)
    print(out)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(out)


if __name__ == '__main__':
    main()
