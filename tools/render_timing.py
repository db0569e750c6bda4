"""Timing of the overlay renderer (include/mvfit.h:mvfit_render_overlay / mvfit_render_scene, csrc/render.hip) and of
fit_folder's stages with and without save_images.

  python tools/render_timing.py [--reps 20] [--bodies 4] [--no-folder]

Prints (1) the render kernels' time per 2048 x 1536 image from hipEvents around render_overlay, for one image per call,
64 images per call (the batch driver's largest call) and a close-up whose faces cover thousands of pixels each, and
(2) fit_folder's stage times on the reference's demo inputs (tests/golden/demo_data) plus synthetic 2048 x 1536 JPEGs,
once without and once with save_images.  With --bodies N > 0 also (3) render_scene with one body per image (the work of
render_overlay through the other entry point) and with N bodies per image, 1 and 64 images per call."""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mvsmplfitting_amd import batch, io_formats as iof, synthetic as syn  # noqa: E402
from mvsmplfitting_amd.engine import MvFit, pack_params  # noqa: E402
from tests.helpers import GOLD, body_model  # noqa: E402


def kernel_time(eng, n, reps):
    H, W, V = 1536, 2048, 8
    cams = syn.make_camera_ring(V)
    B = (n + V - 1) // V
    eng.set_problems(cams, np.zeros((B, V, 17, 2), np.float32), np.zeros((B, V, 17), np.float32))
    verts, joints = eng.vertices(pack_params(B=B, **syn.make_frames(B)))
    imgs = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device=eng.device)
    out = torch.empty_like(imgs)
    prob = [i // V for i in range(n)]
    view = [i % V for i in range(n)]
    eng.render_overlay(verts, joints, imgs, prob, view, out=out)           # warm-up (workspace allocation)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per = []
    for _ in range(reps):
        t0.record()
        eng.render_overlay(verts, joints, imgs, prob, view, out=out)
        t1.record()
        t1.synchronize()
        per.append(t0.elapsed_time(t1) / n)
    per = np.asarray(per)
    print('render_overlay 2048x1536, n=%-3d  per image: median %.3f ms  min %.3f ms  max %.3f ms  (%d reps)'
          % (n, np.median(per), per.min(), per.max(), reps))


def scene_time(eng, n, bodies, reps):
    """render_scene, ``bodies`` bodies per 2048 x 1536 image standing 0.7 m apart on a line through the ring's centre; with
    one body the problems, views and vertices of kernel_time, i.e. the work of render_overlay."""
    H, W, V = 1536, 2048, 8
    cams = syn.make_camera_ring(V)
    B = max(bodies, (n + V - 1) // V)
    eng.set_problems(cams, np.zeros((B, V, 17, 2), np.float32), np.zeros((B, V, 17), np.float32))
    x = pack_params(B=B, **syn.make_frames(B))
    x[:, 82] += 0.7 * (np.arange(B) % bodies - 0.5 * (bodies - 1))
    verts, joints = eng.vertices(x)
    imgs = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device=eng.device)
    out = torch.empty_like(imgs)
    lists = [[(i // V + k) % B for k in range(bodies)] for i in range(n)]
    view = [i % V for i in range(n)]
    _, bid = eng.render_scene(verts, joints, imgs, lists, view, out=out, body_id=True)          # warm-up
    covered = float((bid >= 0).float().mean())
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per = []
    for _ in range(reps):
        t0.record()
        eng.render_scene(verts, joints, imgs, lists, view, out=out)
        t1.record()
        t1.synchronize()
        per.append(t0.elapsed_time(t1) / n)
    per = np.asarray(per)
    print('render_scene   2048x1536, n=%-3d bodies=%d  per image: median %.3f ms  min %.3f ms  max %.3f ms  (%d reps, '
          '%.1f%% of the pixels covered)' % (n, bodies, np.median(per), per.min(), per.max(), reps, 100 * covered))


def close_up_time(eng, model, reps):
    """Worst case of the raster: the body 1 m in front of a 2048 x 1536 camera with f = 12000, so that its faces cover
    thousands of pixels each and go through the workgroup-per-face path."""
    cams = (np.eye(3, dtype=np.float32)[None], np.array([[0.0, 0.0, 1.0]], np.float32), np.array([12000.0], np.float32),
            np.array([[1024.0, 768.0]], np.float32))
    eng.set_problems(cams, np.zeros((1, 1, 17, 2), np.float32), np.zeros((1, 1, 17), np.float32))
    verts = torch.from_numpy(np.asarray(model['v_template'], np.float32))[None].to(eng.device)
    imgs = torch.randint(0, 256, (1, 1536, 2048, 3), dtype=torch.uint8, device=eng.device)
    out, fid = eng.render_overlay(verts, None, imgs, [0], [0], face_id=True)
    cnt = torch.bincount(fid[fid >= 0].flatten().long())
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per = []
    for _ in range(reps):
        t0.record()
        eng.render_overlay(verts, None, imgs, [0], [0], out=out)
        t1.record()
        t1.synchronize()
        per.append(t0.elapsed_time(t1))
    print('render_overlay close-up 2048x1536 (%d faces visible, largest %d px, %d over 1024 px): median %.3f ms'
          % (int((cnt > 0).sum()), int(cnt.max()), int((cnt > 1024).sum()), float(np.median(per))))


def folder_stages(model):
    tmp = tempfile.mkdtemp(prefix='render_timing_')
    try:
        keyp = os.path.join(tmp, 'data', 'keypoints')
        shutil.copytree(os.path.join(GOLD, 'demo_data', 'keypoints'), keyp)
        yy, xx = np.mgrid[0:1536, 0:2048]
        for serial, cams, frames in batch.list_frames(keyp):
            for v, cam in enumerate(cams):
                d = os.path.join(tmp, 'data', 'images', serial, cam)
                os.makedirs(d, exist_ok=True)
                img = np.stack([xx * 255 // 2047, yy * 255 // 1535, np.full_like(xx, 40 * v)], -1).astype(np.uint8)
                for fn, _ in frames:
                    iof.save_image(os.path.join(d, fn + '.jpg'), img)
        cam_file = os.path.join(GOLD, 'demo_data', '3DOH50K_Parameters.txt')
        with MvFit(model) as eng:
            batch.fit_folder(model, keyp, cam_file, os.path.join(tmp, 'warm'), engine=eng, save_images=True)
            for save in (False, True):
                timing = {}
                t = time.time()
                batch.fit_folder(model, keyp, cam_file, os.path.join(tmp, 'res%d' % save), engine=eng, save_images=save,
                                 timing=timing)
                total = time.time() - t
                print('fit_folder save_images=%-5s total %.3f s  ' % (save, total)
                      + '  '.join('%s %.3f s' % kv for kv in timing.items()))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--bodies', type=int, default=0, help='also time render_scene with 1 and with this many bodies per image')
    ap.add_argument('--no-folder', action='store_true', help='skip the fit_folder stage times')
    a = ap.parse_args()
    model = body_model()
    with MvFit(model) as eng:
        for n in (1, 64):
            kernel_time(eng, n, a.reps)
        for nb in sorted({1, a.bodies} if a.bodies > 0 else ()):
            for n in (1, 64):
                scene_time(eng, n, nb, a.reps)
        close_up_time(eng, model, a.reps)
    if not a.no_folder:
        folder_stages(model)


if __name__ == '__main__':
    main()
