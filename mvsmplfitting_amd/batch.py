"""File-to-file batch driver: what the reference's `main.py` does for a data folder (code/main.py:21-130) with every
frame of a serial fitted in ONE batched device fit (the reference walks the frames one by one):

    keypoint files  <keyp_root>/<serial>/<camera>/<frame>_keypoints.json   (data_parser.py:375-411: cameras and frames
                    in sorted order, view v = the v-th camera of the camera file; a view without a file does not take
                    part in that frame (main.py:44-66) - here: zero confidence in the fit, and left out of that frame's
                    initial guess: triangulation over the frame's own views, the single-view depth guess when it has one)
    camera file     io_formats.load_camera_para  (utils.py:352-394)
      -> joint weights: hips 11, 12 ignored unless pose_format == 'lsp14' and use_hip (data_parser.py:340-357;
         model_type 'smpllsp' -> 'lsp14', init.py:63-69, and fit_smpl.yaml has use_hip: true: the default here).
         The format follows the model kind (smpl_to_annotation, utils.py:441-457): 'lsp14' for a model with a keypoint
         regressor ('smpllsp'), 'coco17' for one without ('smpl': posed skeleton joints); anything else is a ValueError
      -> initial guess on the device (init_guess.py:18-106 + fix_params :190-212): init_guess.init_guess_batch
      -> staged fit of all frames at once (non_linear_solver.py:156-211), or the warm-start chain with is_seq
         (main.py:76-79, init_guess.py:137-166): sequence.fit_sequences
      -> per frame `<result_folder>/<serial>/<frame>/000.pkl` (utils.py:744-766, 859-864: pickle protocol 2, body pose
         decoded and feet / hands zeroed) and, with save_meshes, `<mesh_folder>/<serial>/<frame>/000.obj` of the model at the
         SAVED (zeroed) pose (utils.py:866-890).

With save_images, the fitted body is drawn over each view's image with the 17 model keypoints as red dots
(utils.py:866-883 -> project_to_img / visualize_results / Renderer.__call__) by the renderer of csrc/render.hip
(MvFit.render_overlay): input `<image_root>/<serial>/<camera>/<frame>.jpg|.png` (data_parser.py's layout), output
`<image_folder>/<serial>/<frame>/<camera>.jpg` for the views that had a keypoint file in that frame (main.py:44-66).
The interactive viewer of main.py is out of scope; the fit itself reads no image, so the image height
the data weight 500 / H refers to (non_linear_solver.py:150,177) is an argument.
"""
from __future__ import annotations

import dataclasses
import os
import time
import warnings
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib
from . import associate as assoc
from . import io_formats as iof
from .engine import MvFit, SCENE_PALETTE, stage_weights
from .init_guess import init_guess_batch, initial_params
from .scene_fit import refine_scenes
from .sequence import fit_sequences
from .silhouette import refine_fit, refine_fit_occluded
from .calibrate import camera_matrices, refine_rig
from .joint_refine import refine_joint
from .temporal import smooth_sequences
from .scan import points_from_depth
from .scan import refine_fit as scan_refine_fit
from . import landmarks as lmk


# pose format -> the model kind whose joint tensor it maps (reference code/utils/utils.py:441-457 smpl_to_annotation)
POSE_FORMATS = {'lsp14': 'smpllsp', 'coco17': 'smpl'}


def list_frames(keyp_root):
    """[(serial, [camera names], [(frame name, [json path or None per camera])])] in the reference's order."""
    out = []
    for serial in sorted(os.listdir(keyp_root)):
        sdir = os.path.join(keyp_root, serial)
        if not os.path.isdir(sdir):
            continue
        cams = sorted(c for c in os.listdir(sdir) if os.path.isdir(os.path.join(sdir, c)))
        names = set()
        for c in cams:
            names.update(f[:-len('_keypoints.json')] for f in os.listdir(os.path.join(sdir, c)) if f.endswith('_keypoints.json'))
        frames = []
        for fn in sorted(names):
            paths = [os.path.join(sdir, c, fn + '_keypoints.json') for c in cams]
            frames.append((fn, [p if os.path.exists(p) else None for p in paths]))
        out.append((serial, cams, frames))
    return out


def load_serial(frames, num_views, person=0, return_mask=False):
    """Keypoints [F, V, 17, 3] float32 of one serial (missing view / person: zeros, i.e. zero confidence) and, with
    return_mask, which (frame, view) pairs exist - the reference drops the others from the frame (main.py:44-66)."""
    kp = np.zeros((len(frames), num_views, 17, 3), np.float32)
    mask = np.zeros((len(frames), num_views), bool)
    for f, (_, paths) in enumerate(frames):
        for v, p in enumerate(paths[:num_views]):
            if p is None:
                continue
            people = iof.read_keypoints(p)
            if len(people) > person:
                kp[f, v] = people[person]
                mask[f, v] = True
    return (kp, mask) if return_mask else kp


def load_serial_joints3d(frames, person=0):
    """use_3d annotation (data_parser.py:396-400): per frame the 'pose_keypoints_3d' of the FIRST camera that has a file,
    [F, 17, 4] = (x, y, z, confidence) float32, and a mask of the frames that carry one."""
    j3 = np.zeros((len(frames), 17, 4), np.float32)
    has = np.zeros(len(frames), bool)
    for f, (_, paths) in enumerate(frames):
        for p in paths:
            if p is None:
                continue
            try:
                people = iof.read_joints3d(p)
            except KeyError:                                   # no 3-D annotation in this file (the reference: None)
                break
            if len(people) > person:
                j3[f] = people[person][:17]
                has[f] = True
            break
    return j3, has


def load_serial_people(frames, num_views):
    """Every person of one serial: (ids, kp [F, P, V, 17, 3] float32, mask [F, P, V] bool) with ``ids`` the sorted person
    ids that occur anywhere in the serial (io_formats.read_people: the ``person_id`` field when every entry of a file has
    one, else the index in ``people``; an all-zero entry is absent) and mask[f, p, v]: view v lists person ids[p] in frame
    f.  Missing entries are zeros, i.e. zero confidence."""
    seen = {}
    for f, (_, paths) in enumerate(frames):
        for v, p in enumerate(paths[:num_views]):
            if p is not None:
                for pid, a in iof.read_people(p).items():
                    seen[(f, pid, v)] = a
    ids = sorted({k[1] for k in seen})
    col = {pid: i for i, pid in enumerate(ids)}
    kp = np.zeros((len(frames), len(ids), num_views, 17, 3), np.float32)
    mask = np.zeros((len(frames), len(ids), num_views), bool)
    for (f, pid, v), a in seen.items():
        kp[f, col[pid], v, :a.shape[0]] = a
        mask[f, col[pid], v] = True
    return ids, kp, mask


def load_serial_people3d(frames, ids):
    """use_3d annotation per person: [F, P, 17, 4] float32 (x, y, z, confidence) and has [F, P] - for person ids[p] in
    frame f the ``pose_keypoints_3d`` entry of the first camera whose file carries one for that id (same id rule)."""
    col = {pid: i for i, pid in enumerate(ids)}
    j3 = np.zeros((len(frames), len(ids), 17, 4), np.float32)
    has = np.zeros((len(frames), len(ids)), bool)
    for f, (_, paths) in enumerate(frames):
        for p in paths:
            if p is None:
                continue
            for pid, a in iof.read_people3d(p).items():
                if pid in col and not has[f, col[pid]]:
                    j3[f, col[pid], :a.shape[0]] = a
                    has[f, col[pid]] = True
    return j3, has


IMAGE_EXTS = ('.jpg', '.png')
RENDER_BATCH = 64          # images per render_overlay call
IO_WORKERS = 16            # decode / encode threads


def image_path(image_root, serial, camera, frame):
    """The input image of one view of one frame, or ValueError naming the paths tried."""
    base = os.path.join(image_root, serial, camera, frame)
    for ext in IMAGE_EXTS:
        if os.path.isfile(base + ext):
            return base + ext
    raise ValueError('save_images: no image for serial %s camera %s frame %s (looked for %s)'
                     % (serial, camera, frame, ' / '.join(base + e for e in IMAGE_EXTS)))


def render_serial_images(eng: MvFit, verts, joints, jobs, out_folder, pool, scene=None):
    """jobs: [(frame index f, view v, input path, (serial, frame name, camera))]; draws problem f seen by view v over the
    input image and writes `<out_folder>/<serial>/<frame>/<camera>.jpg`.  Returns the written paths in job order.
    ``scene`` = {f: (problems, colours [n, 3])}: frame f shows these problems, each in its colour, in one depth-tested
    image (MvFit.render_scene) instead of problem f alone in grey.
    Streamed: the jobs are grouped by image size (read from the file headers) and go through in chunks of at most
    RENDER_BATCH images - decode on the thread pool, one GPU call, encode on the thread pool.  Before the next chunk is
    decoded, the encodes of the chunk before the current one have finished, so at most two chunks of images are held on
    the host whatever the length of the serial."""
    paths = [None] * len(jobs)
    by_size = {}
    for i, j in enumerate(jobs):
        by_size.setdefault(iof.image_size(j[2]), []).append(i)

    def wait(futures):
        for fu in futures:
            fu.result()
    prev = []
    try:
        for (H, W), idx in sorted(by_size.items()):
            for s0 in range(0, len(idx), RENDER_BATCH):
                part = idx[s0:s0 + RENDER_BATCH]
                imgs = np.empty((len(part), H, W, 3), np.uint8)

                def decode(k, path):
                    im = iof.read_image(path)
                    if im.shape != imgs.shape[1:]:
                        raise ValueError('save_images: %s decoded to %s, its header says %s' % (path, im.shape, (H, W)))
                    imgs[k] = im
                wait([pool.submit(decode, k, jobs[i][2]) for k, i in enumerate(part)])
                if scene is None:
                    out = eng.render_overlay(verts, joints, imgs, [jobs[i][0] for i in part], [jobs[i][1] for i in part])
                else:
                    out = eng.render_scene(verts, joints, imgs, [scene[jobs[i][0]][0] for i in part],
                                           [jobs[i][1] for i in part],
                                           colors=np.concatenate([scene[jobs[i][0]][1] for i in part]))
                out = out.cpu().numpy()
                del imgs
                cur = []
                for k, i in enumerate(part):
                    serial, frame, camera = jobs[i][3]
                    d = os.path.join(out_folder, serial, frame)
                    os.makedirs(d, exist_ok=True)
                    paths[i] = os.path.join(d, camera + '.jpg')
                    cur.append(pool.submit(iof.save_image, paths[i], out[k]))
                del out
                wait(prev)
                prev = cur
        wait(prev)
    finally:
        for fu in prev:
            fu.cancel()
    return paths


SILHOUETTE_DEFAULTS = dict(w_in=1.0, w_out=1.0, sigma=0.0, contour_stride=1, downscale=1, max_mask_bytes=2 ** 31, occlusion=None)
OCCLUSION_DEFAULTS = dict(margin=0.02, sweeps=2)
SCAN_DEFAULTS = dict(root=None, depth_root=None, w_s2m=1.0, w_m2s=0.0, sigma=0.05, max_points=8192, stride=1, mask_root=None)


def check_scene_collision(cfg, is_seq=False, multi=True):
    """fit_folder's ``scene_collision`` option, or ValueError (its defaults are scene_fit.refine_scenes' own)."""
    if not multi:
        raise ValueError('scene_collision refines the persons of a frame together: it needs persons= a list of ids or \'all\'')
    if is_seq:
        raise ValueError('scene_collision is not available with is_seq=True')
    if not isinstance(cfg, dict) or 'weight' not in cfg:
        raise ValueError("scene_collision: a dict with at least 'weight' (the collision term's coll_loss_weight)")
    unknown = set(cfg) - {'weight', 'sweeps', 'grid_size', 'robustifier', 'scale_factor'}
    if unknown:
        raise ValueError('scene_collision: unknown keys %s' % sorted(unknown))
    return cfg


def check_silhouettes(silhouettes, is_seq=False, scene_collision=None, multi=True):
    """fit_folder's ``silhouettes`` option with the defaults filled in, or ValueError.  ``occlusion`` (None, or a dict with
    margin and sweeps; the multi-person path only) comes back with its own defaults filled in."""
    if not isinstance(silhouettes, dict) or 'mask_root' not in silhouettes or 'weight' not in silhouettes:
        raise ValueError("silhouettes: a dict with at least 'mask_root' and 'weight' (the term's coll_loss_weight)")
    unknown = set(silhouettes) - set(SILHOUETTE_DEFAULTS) - {'mask_root', 'weight'}
    if unknown:
        raise ValueError('silhouettes: unknown keys %s' % sorted(unknown))
    if is_seq:
        raise ValueError('silhouettes is not available with is_seq=True')
    if scene_collision is not None:
        raise ValueError('silhouettes and scene_collision both use the fit\'s one term slot: choose one')
    cfg = dict(SILHOUETTE_DEFAULTS, **silhouettes)
    if int(cfg['downscale']) < 1 or int(cfg['contour_stride']) < 1:
        raise ValueError('silhouettes: downscale and contour_stride must be >= 1')
    if not float(cfg['weight']) > 0.0:
        raise ValueError('silhouettes: weight must be > 0')
    if cfg['occlusion'] is not None:
        occ = cfg['occlusion']
        if not isinstance(occ, dict) or set(occ) - set(OCCLUSION_DEFAULTS):
            raise ValueError('silhouettes: occlusion: a dict with the keys %s, got %r' % (sorted(OCCLUSION_DEFAULTS), occ))
        if not multi:
            raise ValueError('silhouettes: occlusion is between the persons of a frame: it needs persons= a list of ids or \'all\'')
        occ = dict(OCCLUSION_DEFAULTS, **occ)
        if not (np.isfinite(float(occ['margin'])) and float(occ['margin']) >= 0.0) or int(occ['sweeps']) < 1:
            raise ValueError('silhouettes: occlusion: margin must be finite and >= 0, sweeps >= 1')
        cfg['occlusion'] = occ
    return cfg


def check_temporal(temporal, scene_collision=None, silhouettes=None):
    """fit_folder's ``temporal`` option with the defaults filled in, or ValueError."""
    if not isinstance(temporal, dict) or 'weight' not in temporal:
        raise ValueError("temporal: a dict with at least 'weight' (the smoothing term's coll_loss_weight)")
    unknown = set(temporal) - {'weight', 'sweeps'}
    if unknown:
        raise ValueError('temporal: unknown keys %s' % sorted(unknown))
    if scene_collision is not None or silhouettes is not None:
        raise ValueError('temporal and %s both use the fit\'s one term slot: choose one'
                         % ('scene_collision' if scene_collision is not None else 'silhouettes'))
    cfg = dict(dict(sweeps=3), **temporal)
    if not float(cfg['weight']) > 0.0:
        raise ValueError('temporal: weight must be > 0')
    if int(cfg['sweeps']) < 1:
        raise ValueError('temporal: sweeps must be >= 1')
    return cfg


JOINT_PARTS = dict(scene_collision=dict(grid_size=32, robustifier=0.05, scale_factor=0.2),
                   silhouettes={k: v for k, v in SILHOUETTE_DEFAULTS.items() if k != 'occlusion'},      # (not built under joint)
                   temporal=dict(),
                   scans=dict(SCAN_DEFAULTS))


def check_joint(joint, is_seq=False, multi=False, scene_collision=None, silhouettes=None, temporal=None, scans=None):
    """fit_folder's ``joint`` option with the defaults filled in, or ValueError."""
    if not isinstance(joint, dict) or 'weight' not in joint:
        raise ValueError("joint: a dict with at least 'weight' (the mixed term's coll_loss_weight) and two parts")
    unknown = set(joint) - {'weight', 'sweeps'} - set(JOINT_PARTS)
    if unknown:
        raise ValueError('joint: unknown keys %s' % sorted(unknown))
    for name, single in (('scene_collision', scene_collision), ('silhouettes', silhouettes), ('temporal', temporal), ('scans', scans)):
        if single is not None:
            raise ValueError('joint and %s: the joint refinement takes the place of the single ones - name its parts inside joint' % name)
    if is_seq:
        raise ValueError('joint is not available with is_seq=True')
    cfg = dict(weight=float(joint['weight']), sweeps=int(joint.get('sweeps', 3)))
    if not cfg['weight'] > 0.0:
        raise ValueError('joint: weight must be > 0')
    if cfg['sweeps'] < 1:
        raise ValueError('joint: sweeps must be >= 1')
    parts = [k for k in JOINT_PARTS if joint.get(k) is not None]
    if len(parts) < 2:
        raise ValueError('joint: at least two of scene_collision, silhouettes and temporal must be given (a single part has an option of its own); '
                         'scans counts as a fourth')
    for k in parts:
        part = joint[k]
        if not isinstance(part, dict) or 'share' not in part:
            raise ValueError("joint: %s: a dict with at least 'share'" % k)
        if k == 'silhouettes' and 'mask_root' not in part:
            raise ValueError("joint: silhouettes: a dict with at least 'share' and 'mask_root'")
        unknown = set(part) - {'share', 'mask_root' if k == 'silhouettes' else 'share'} - set(JOINT_PARTS[k])
        if unknown:
            raise ValueError('joint: %s: unknown keys %s' % (k, sorted(unknown)))
        c = dict(JOINT_PARTS[k], **part)
        if not float(c['share']) > 0.0 or not np.isfinite(float(c['share'])):
            raise ValueError('joint: %s: share must be > 0' % k)
        if k == 'scene_collision' and (int(c['grid_size']) < 2 or not float(c['robustifier']) > 0.0 or not float(c['scale_factor']) > 0.0):
            raise ValueError('joint: scene_collision: grid_size must be >= 2, robustifier and scale_factor > 0')
        if k == 'silhouettes' and (int(c['downscale']) < 1 or int(c['contour_stride']) < 1):
            raise ValueError('joint: silhouettes: downscale and contour_stride must be >= 1')
        if k == 'scans':
            _check_scan_values('joint: scans', c, multi)
        cfg[k] = c
    if 'scene_collision' in cfg and not multi:
        raise ValueError('joint: scene_collision refines the persons of a frame together: it needs persons= a list of ids or \'all\'')
    return cfg


def mask_path(mask_root, serial, camera, frame, person=None):
    """The mask file of one view of one frame: `<mask_root>/<serial>/<camera>/<frame>.png`, or `<frame>_<id:03d>.png` for
    person ``id`` of the multi-person path."""
    name = frame + '.png' if person is None else '%s_%03d.png' % (frame, int(person))
    return os.path.join(mask_root, serial, camera, name)


def _check_scan_values(who, cfg, multi):
    """what the ``scans`` option and the ``scans`` part of ``joint`` share: one source, the scalars, the sizes"""
    if (cfg['root'] is None) == (cfg['depth_root'] is None):
        raise ValueError('%s: exactly one of root (point files) and depth_root (depth maps) must be given' % who)
    vals = [float(cfg[k]) for k in ('w_s2m', 'w_m2s', 'sigma')]
    if any(not np.isfinite(v) or v < 0.0 for v in vals):
        raise ValueError('%s: w_s2m, w_m2s and sigma must be finite and >= 0' % who)
    if not (vals[0] > 0.0 or vals[1] > 0.0):
        raise ValueError('%s: w_s2m and w_m2s are both 0' % who)
    if int(cfg['max_points']) < 1 or int(cfg['stride']) < 1:
        raise ValueError('%s: max_points and stride must be >= 1' % who)
    if cfg['depth_root'] is not None and multi and cfg['mask_root'] is None:
        raise ValueError('%s: depth maps of more than one person need mask_root: without masks every person would get everyone\'s points'
                         % who)
    if cfg['root'] is not None and cfg['mask_root'] is not None:
        raise ValueError('%s: mask_root selects the pixels of depth maps: it goes with depth_root' % who)


def check_scans(scans, is_seq=False, multi=False, scene_collision=None, silhouettes=None, temporal=None, refine_cameras=None):
    """fit_folder's ``scans`` option with the defaults filled in, or ValueError."""
    if not isinstance(scans, dict) or 'weight' not in scans:
        raise ValueError("scans: a dict with at least 'weight' (the term's coll_loss_weight, against metres squared) and one of "
                         "'root' and 'depth_root'")
    unknown = set(scans) - set(SCAN_DEFAULTS) - {'weight'}
    if unknown:
        raise ValueError('scans: unknown keys %s' % sorted(unknown))
    if is_seq:
        raise ValueError('scans is not available with is_seq=True')
    if refine_cameras is not None:
        raise ValueError('refine_cameras with scans is not built')
    for name, single in (('scene_collision', scene_collision), ('silhouettes', silhouettes), ('temporal', temporal)):
        if single is not None:
            raise ValueError('scans and %s both use the fit\'s one term slot: choose one (they combine inside joint)' % name)
    cfg = dict(SCAN_DEFAULTS, **scans)
    if not float(cfg['weight']) > 0.0 or not np.isfinite(float(cfg['weight'])):
        raise ValueError('scans: weight must be > 0')
    _check_scan_values('scans', cfg, multi)
    return cfg


def scan_path(root, serial, frame, person=None, camera=None):
    """The scan file of one frame.  Point files (camera None): `<root>/<serial>/<frame>.npy`, or `<frame>_<id:03d>.npy` for
    person ``id`` of the multi-person path.  Depth maps: `<depth_root>/<serial>/<camera>/<frame>.npy`, one per view, shared by the
    persons of the frame (their masks tell them apart)."""
    if camera is not None:
        return os.path.join(root, serial, camera, frame + '.npy')
    name = frame + '.npy' if person is None else '%s_%03d.npy' % (frame, int(person))
    return os.path.join(root, serial, name)


def subsample_rows(P, max_points):
    """The rows kept of P > max_points: floor(i * P / max_points), scan.points_from_depth's rule."""
    return np.floor(np.arange(int(max_points)) * (P / float(max_points))).astype(np.int64)


def load_serial_scans(cfg, serial, cams, frames, problems, rig):
    """The scan set of one serial's problems for MvFit.set_scans: (points float32 [N,Pmax,3], count int32 [N], weights float32
    [N,Pmax] or None, found = [(problem, path)]).

    problems, cams, rig as for load_serial_masks.  ``root``: every problem's own file of world points [P,3], or [P,4] with a
    weight >= 0 in the last column (io_formats.read_points).  ``depth_root``: the problem's points are scan.points_from_depth
    over its views in rig order (a view without a depth file contributes nothing), with ``stride``, masked by the person's
    mask file where ``mask_root`` is given and the file exists.  A problem without a file gets count 0 and pays nothing; more
    than max_points points keep the rows subsample_rows names; Pmax is the serial's largest count (at least 1).  ValueError: no
    file at all in the serial, a file of another shape or dtype, a negative or non-finite weight, a depth map or mask whose
    size differs from the others of its problem."""
    cap = int(cfg['max_points'])
    per, wts, found = [], [], []
    if cfg['root'] is not None:
        for n, (f, person) in enumerate(problems):
            path = scan_path(cfg['root'], serial, frames[f][0], person)
            if not os.path.isfile(path):
                per.append(np.zeros((0, 3), np.float32))
                wts.append(None)
                continue
            pts, w = iof.read_points(path)
            if len(pts) > cap:
                keep = subsample_rows(len(pts), cap)
                pts, w = pts[keep], (None if w is None else w[keep])
            per.append(pts)
            wts.append(w)
            found.append((n, path))
        example = scan_path(cfg['root'], serial, frames[problems[0][0]][0], problems[0][1])
        where = cfg['root']
    else:
        R, t, f_, c = (np.asarray(a, np.float32) for a in rig)
        for n, (f, person) in enumerate(problems):
            views, depth, masks = [], [], []
            for v, cam in enumerate(cams):
                path = scan_path(cfg['depth_root'], serial, frames[f][0], camera=cam)
                if not os.path.isfile(path):
                    continue
                d = iof.read_depth(path)
                if depth and d.shape != depth[0].shape:
                    raise ValueError('scans: the depth maps of serial %s frame %s differ in size: %s is %s, another %s'
                                     % (serial, frames[f][0], path, d.shape, depth[0].shape))
                m = np.ones(d.shape, np.uint8)
                if cfg['mask_root'] is not None:
                    mp = mask_path(cfg['mask_root'], serial, cam, frames[f][0], person)
                    if os.path.isfile(mp):
                        m = iof.read_mask(mp)
                        if m.shape != d.shape:
                            raise ValueError('scans: mask %s is %s, its depth map %s is %s' % (mp, m.shape, path, d.shape))
                views.append(v)
                depth.append(d)
                masks.append(m)
                found.append((n, path))
            if not views:
                per.append(np.zeros((0, 3), np.float32))
            else:
                vv = np.array(views)
                per.append(points_from_depth(np.stack(depth), (R[vv], t[vv], f_[vv], c[vv]), mask=np.stack(masks),
                                             stride=int(cfg['stride']), max_points=cap))
            wts.append(None)
        example = scan_path(cfg['depth_root'], serial, frames[problems[0][0]][0], camera=cams[0])
        where = cfg['depth_root']
    if not found:
        raise ValueError('scans: serial %s has no scan file under %s (looked for e.g. %s)' % (serial, where, example))
    count = np.array([len(p) for p in per], np.int32)
    Pmax = max(int(count.max()), 1)
    points = np.zeros((len(per), Pmax, 3), np.float32)
    weights = np.ones((len(per), Pmax), np.float32) if any(w is not None for w in wts) else None
    for n, p in enumerate(per):
        points[n, :len(p)] = p
        if wts[n] is not None:
            weights[n, :len(p)] = wts[n]
    return points, count, weights, found


def refine_serial_scans(eng, xf, stage, cfg, serial, cams, frames, problems, rig):
    """The scan refinement of one serial's fitted problems (scan.refine_fit: the scan term inside the engine's fit) against the
    scan set of load_serial_scans, with coll_loss_weight = cfg['weight'].  Returns (params, report): refine_fit's report plus
    points = the count per problem; the engine is left without scan set and term."""
    points, count, weights, _ = load_serial_scans(cfg, serial, cams, frames, problems, rig)
    eng.set_scans(points, count=count, weights=weights)
    try:
        out, report = scan_refine_fit(eng, xf, dict(stage, coll_loss_weight=float(cfg['weight'])), w_s2m=float(cfg['w_s2m']),
                                      w_m2s=float(cfg['w_m2s']), sigma=float(cfg['sigma']))
    finally:
        eng.clear_scans()
    return out, dict(report, points=count.copy())


LANDMARK_DEFAULTS = dict(table=None, rho=100.0)


def check_landmarks(landmarks, num_verts, is_seq=False, scene_collision=None, silhouettes=None, temporal=None, scans=None, joint=None,
                    refine_cameras=None):
    """fit_folder's ``landmarks`` option with the defaults filled in and the table loaded (landmarks.load_table), or
    ValueError."""
    if not isinstance(landmarks, dict) or 'weight' not in landmarks or landmarks.get('table') is None:
        raise ValueError("landmarks: a dict with at least 'weight' (the term's coll_loss_weight, against pixels squared) and "
                         "'table' (a landmark table file or dict)")
    unknown = set(landmarks) - set(LANDMARK_DEFAULTS) - {'weight'}
    if unknown:
        raise ValueError('landmarks: unknown keys %s' % sorted(unknown))
    if is_seq:
        raise ValueError('landmarks is not available with is_seq=True')
    if refine_cameras is not None:
        raise ValueError('refine_cameras with landmarks is not built')
    for name, single in (('scene_collision', scene_collision), ('silhouettes', silhouettes), ('temporal', temporal), ('scans', scans),
                         ('joint', joint)):
        if single is not None:
            raise ValueError('landmarks and %s both use the fit\'s one term slot: choose one (the landmark term takes no share of the '
                             'term mix)' % name)
    cfg = dict(LANDMARK_DEFAULTS, **landmarks)
    if not float(cfg['weight']) > 0.0 or not np.isfinite(float(cfg['weight'])):
        raise ValueError('landmarks: weight must be > 0')
    if not np.isfinite(float(cfg['rho'])) or float(cfg['rho']) < 0.0:
        raise ValueError('landmarks: rho must be finite and >= 0')
    table = lmk.load_table(cfg['table'])
    if (table['keypoint_index'] < 0).any():
        raise ValueError('landmarks: every landmark of the table needs a keypoint_index (its row of pose_keypoints_2d)')
    ids = table['vertex_ids'][table['weights'] != 0]
    if (ids >= int(num_verts)).any():
        raise ValueError('landmarks: the table names vertex %d, the model has %d vertices' % (int(ids.max()), int(num_verts)))
    cfg['table'] = table
    return cfg


def load_serial_landmarks(table, frames, problems, num_views, association=None):
    """The landmark targets of one serial's problems from the keypoint files the 17 keypoints came from: (xy [N,V,L,2], conf
    [N,V,L]) float32 with the rows table['keypoint_index'] of ``pose_keypoints_2d`` (io_formats.read_people_extra).  A problem
    (frame, person) follows the entry the keypoints follow: persons=0 (person None) the first entry of every file, persons=
    the entry with that id by read_people's rule, associate= (``association``: associate_serial's report) the detection the
    track holds in that view."""
    rows = table['keypoint_index']
    L = len(rows)
    by_index = association is not None or any(p is None for _, p in problems)
    files = {}

    def people(f, v):
        if (f, v) not in files:
            path = frames[f][1][v] if v < len(frames[f][1]) else None
            files[(f, v)] = iof.read_people_extra(path, rows, by_index=by_index) if path is not None else {}
        return files[(f, v)]

    per_problem_rows = []
    for f, person in problems:
        views = []
        for v in range(num_views):
            entry = 0 if person is None else person
            if association is not None:
                k = np.flatnonzero(association['track_ids'][f, v] == person)
                entry = int(association['slot'][f, v, k[0]]) if k.size else None
            views.append(people(f, v).get(entry) if entry is not None else None)
        per_problem_rows.append(views)
    return lmk.targets_from_people(per_problem_rows, L)


def refine_serial_landmarks(eng, xf, stage, cfg, frames, problems, num_views, association=None):
    """The landmark refinement of one serial's fitted problems (landmarks.refine_fit: the landmark term inside the engine's
    fit) against the targets of load_serial_landmarks, with coll_loss_weight = cfg['weight'].  A problem without a live
    target keeps its row exactly; a serial without one is not refitted at all (report['loss'] is None: the fit's own losses
    stand).  Returns (params, report): refine_fit's report plus targets = the live entries per problem; the engine is left
    without table, targets and term."""
    table = cfg['table']
    xy, conf = load_serial_landmarks(table, frames, problems, num_views, association)
    live = (conf > 0).reshape(len(problems), -1).sum(axis=1)
    if not live.any():
        return xf, dict(accepted=np.zeros(len(problems), bool), targets=live, loss=None)
    eng.set_landmarks(table['vertex_ids'], table['weights'])
    try:
        eng.set_landmark_targets(xy, conf)
        out, report = lmk.refine_fit(eng, xf, dict(stage, coll_loss_weight=float(cfg['weight'])), rho=float(cfg['rho']))
    finally:
        eng.clear_landmarks()
    for j in np.flatnonzero(live == 0):
        out[int(j)] = xf[int(j)]
        report['accepted'][j] = False
        report['after'][j] = report['loss'][j] = report['before'][j]
        report['landmark_after'][j] = report['landmark_before'][j]
    return out, dict(report, targets=live)


def silhouette_workspace_bytes(M, H, W, Nv):
    """The mask set's workspace of include/mvfit.h (mvfit_set_silhouettes), without the contour lists."""
    return M * H * W * 5 + M * H * 4 + M * (16 * Nv + 8 * -(-Nv // 256) + 92) + 8


def load_serial_masks(cfg, serial, cams, frames, problems, rig, num_verts):
    """The mask set of one serial's problems for MvFit.set_silhouettes: (masks uint8 [M,H,W], image_body [M], cams per image,
    found = [(problem, view, path)]).

    problems: [(frame index, person id or None)] per problem; cams: the serial's camera folder names, view v = rig row v;
    rig = (R, t, f, c) of set_problems.  Every existing mask file of a (problem, view) is one image of that problem; masks
    are brought to 1 / downscale of their resolution (io_formats.downscale_mask) and the cameras follow with f and c divided
    by it.  ValueError: no mask file at all, masks of different sizes, a workspace above max_mask_bytes."""
    k = int(cfg['downscale'])
    found = []
    for n, (f, person) in enumerate(problems):
        for v, cam in enumerate(cams):
            path = mask_path(cfg['mask_root'], serial, cam, frames[f][0], person)
            if os.path.isfile(path):
                found.append((n, v, path))
    if not found:
        raise ValueError('silhouettes: serial %s has no mask file under %s (looked for e.g. %s)'
                         % (serial, cfg['mask_root'], mask_path(cfg['mask_root'], serial, cams[0], frames[problems[0][0]][0],
                                                                problems[0][1])))
    H0, W0 = iof.image_size(found[0][2])
    M = len(found)

    def need(kk):
        return silhouette_workspace_bytes(M, -(-H0 // kk), -(-W0 // kk), int(num_verts))
    if need(k) > int(cfg['max_mask_bytes']):
        fit = k + 1
        while need(fit) > int(cfg['max_mask_bytes']) and (-(-H0 // fit) > 2 or -(-W0 // fit) > 2):
            fit += 1
        raise ValueError('silhouettes: %d masks of %d x %d at downscale=%d need a workspace of %d bytes, more than '
                         'max_mask_bytes=%d; the smallest downscale that fits is %d'
                         % (M, H0, W0, k, need(k), int(cfg['max_mask_bytes']), fit))
    masks = np.empty((M, -(-H0 // k), -(-W0 // k)), np.uint8)
    for i, (_, _, path) in enumerate(found):
        m = iof.read_mask(path)
        if m.shape != (H0, W0):
            raise ValueError('silhouettes: the masks of serial %s differ in size: %s is %s, %s is %s'
                             % (serial, found[0][2], (H0, W0), path, m.shape))
        masks[i] = iof.downscale_mask(m, k)
    body = np.array([n for n, _, _ in found], np.int32)
    view = np.array([v for _, v, _ in found])
    R, t, f, c = (np.asarray(a, np.float32) for a in rig)
    per_image = (R[view], t[view], (f[view] / np.float32(k)).astype(np.float32), (c[view] / np.float32(k)).astype(np.float32))
    return masks, body, per_image, found


def refine_serial_silhouettes(eng, xf, stage, cfg, serial, cams, frames, problems, rig, num_verts):
    """The silhouette refinement of one serial's fitted problems (silhouette.refine_fit, the term inside the engine's fit)
    against the mask set of load_serial_masks.  With cfg['occlusion'] the persons of a frame are a scene and occlude one
    another (silhouette.refine_fit_occluded; the report gains its per-sweep counts).  Returns (params, report); the engine is
    left without mask set, occluders and term."""
    masks, body, per_image, found = load_serial_masks(cfg, serial, cams, frames, problems, rig, num_verts)
    eng.set_silhouettes(masks, body, per_image, contour_stride=int(cfg['contour_stride']))
    try:
        st, kw = dict(stage, coll_loss_weight=float(cfg['weight'])), dict(w_in=float(cfg['w_in']), w_out=float(cfg['w_out']),
                                                                          sigma=float(cfg['sigma']))
        if cfg.get('occlusion') is not None:
            out, report = refine_fit_occluded(eng, xf, st, [int(f) for f, _ in problems], margin=float(cfg['occlusion']['margin']),
                                              sweeps=int(cfg['occlusion']['sweeps']), **kw)
        else:
            out, report = refine_fit(eng, xf, st, **kw)
    finally:
        eng.clear_silhouettes()
    report = dict(report, images=[(int(n), int(v)) for n, v, _ in found], mask_size=tuple(masks.shape[1:]))
    return out, report


def refine_serial_joint(eng, xf, stage, cfg, serial, cams, frames, problems, rig, num_verts, scene_sizes, seq_id, frame_idx):
    """The joint refinement of one serial's fitted problems (joint_refine.refine_joint: the term mix inside the engine's fit)
    with the parts of ``cfg`` (check_joint).  problems, cams, rig as for load_serial_masks; scene_sizes: problems per frame
    (frame-major rows); seq_id / frame_idx: every problem's track and its position in the serial's frame list.  Returns
    (params, report); the engine is left without mask set, scan set, mix, targets and obstacles."""
    shares, kw = {}, {}
    sil = cfg.get('silhouettes')
    if 'scene_collision' in cfg:
        sc = cfg['scene_collision']
        shares['scene'] = float(sc['share'])
        kw.update(scene_sizes=scene_sizes, grid_size=int(sc['grid_size']), scale_factor=float(sc['scale_factor']),
                  robustifier=float(sc['robustifier']))
    if 'temporal' in cfg:
        shares['temporal'] = float(cfg['temporal']['share'])
        kw.update(seq_id=seq_id, frame_idx=frame_idx)
    found = masks = None
    if sil is not None:
        shares['silhouette'] = float(sil['share'])
        kw.update(w_in=float(sil['w_in']), w_out=float(sil['w_out']), sigma=float(sil['sigma']))
        masks, body, per_image, found = load_serial_masks(sil, serial, cams, frames, problems, rig, num_verts)
        eng.set_silhouettes(masks, body, per_image, contour_stride=int(sil['contour_stride']))
    scn, count = cfg.get('scans'), None
    try:
        if scn is not None:
            shares['scan'] = float(scn['share'])
            kw.update(scan_w_s2m=float(scn['w_s2m']), scan_w_m2s=float(scn['w_m2s']), scan_sigma=float(scn['sigma']))
            points, count, weights, _ = load_serial_scans(scn, serial, cams, frames, problems, rig)
            eng.set_scans(points, count=count, weights=weights)
        out, report = refine_joint(eng, xf, dict(stage, coll_loss_weight=float(cfg['weight'])), shares=shares,
                                   sweeps=int(cfg['sweeps']), **kw)
    finally:
        if scn is not None:
            eng.clear_scans()
        if sil is not None:
            eng.clear_silhouettes()
    if found is not None:
        report = dict(report, images=[(int(n), int(v)) for n, v, _ in found], mask_size=tuple(masks.shape[1:]))
    if count is not None:
        report = dict(report, points=count.copy())
    return out, report


CAMERA_REFINE_DEFAULTS = dict(sweeps=2, anchor=0, free='extrinsics', min_points=34)


def check_refine_cameras(cfg, is_seq=False, use_3d=False, scene_collision=None, silhouettes=None, temporal=None, joint=None, scans=None):
    """The refine_cameras option of fit_folder -> its dict with the defaults filled in; ValueError for what is not built."""
    if not isinstance(cfg, dict):
        raise ValueError('refine_cameras: a dict with any of the keys %s' % sorted(CAMERA_REFINE_DEFAULTS))
    unknown = set(cfg) - set(CAMERA_REFINE_DEFAULTS)
    if unknown:
        raise ValueError('refine_cameras: unknown keys %s' % sorted(unknown))
    for name, on in (('is_seq', is_seq), ('use_3d', use_3d), ('scene_collision', scene_collision is not None),
                     ('silhouettes', silhouettes is not None), ('temporal', temporal is not None), ('joint', joint is not None),
                     ('scans', scans is not None)):
        if on:
            raise ValueError('refine_cameras with %s is not built' % name)
    out = dict(CAMERA_REFINE_DEFAULTS, **cfg)
    if int(out['sweeps']) < 1 or int(out['min_points']) < 1:
        raise ValueError('refine_cameras: sweeps and min_points must be >= 1')
    if out['free'] not in ('extrinsics', 'extrinsics+focal', 'all'):
        raise ValueError("refine_cameras: free must be 'extrinsics', 'extrinsics+focal' or 'all'")
    return out


def refine_serial_cameras(eng, xf, stage, cfg, serial, rig, gt_xy, conf, intris, result_folder):
    """refine_rig on a serial's whole batch after its fit (the engine holds the serial's problems under ``rig``) -> (params,
    report, (extris [V,4,4], intris [V,3,3])); writes <result_folder>/<serial>/cameras_refined.txt.  The engine is left with
    the refined rig, so the vertices and overlays that follow are those of the refined fit."""
    xr, cams15, report = refine_rig(eng, xf, stage, rig, gt_xy, conf, sweeps=int(cfg['sweeps']), anchor=cfg['anchor'],
                                    free=cfg['free'], min_points=int(cfg['min_points']))
    ex, K = camera_matrices(cams15, intris)
    d = os.path.join(result_folder, serial)
    os.makedirs(d, exist_ok=True)
    iof.save_camera_para(os.path.join(d, 'cameras_refined.txt'), ex, K)
    return xr, report, (ex, K)


@dataclasses.dataclass
class SerialProblems:
    """One serial's problems as fit_serial takes them, from either path; row n of every array is problem n."""
    serial: str
    cams: list                   # camera folder names, view v = rig row v
    frames: list                 # list_frames' [(frame name, [json path or None per camera])]
    V: int
    prob: list                   # [(frame index, person id or None)]
    pf: np.ndarray               # [N] frame index
    pp: np.ndarray | None        # [N] person id; None: the single-person path
    kp: np.ndarray               # [N, V, 17, 3] (u, v, confidence)
    vmask: np.ndarray            # [N, V] the views that list the problem
    ann: np.ndarray | None       # [N, 17, 4] 3-D annotation (x, y, z, confidence)
    has: np.ndarray              # [N] the problems that carry one
    scales: np.ndarray | None    # [N, 1] fixed scale
    shapes: np.ndarray | None    # [N, 10] fixed shape
    jobs: list | None            # render_serial_images' jobs (save_images)
    association: dict | None = None


@dataclasses.dataclass
class FitContext:
    """What one fit_folder call hands to every serial: the engine, the checked settings, where the files go, the clock."""
    eng: MvFit
    model: dict
    extris: np.ndarray
    intris: np.ndarray
    jw: np.ndarray               # [17] joint weights
    flags: int
    use_vposer: bool
    use_hip: bool
    use_3d: bool
    is_seq: bool
    stages_for: object           # with_3d -> stage list
    want: list | None            # the person ids asked for; None: all
    associate: dict | None
    fix_scale: object
    fix_shape: object
    options: dict                # the checked refinement options by name; None: not asked for
    result_folder: str
    mesh_folder: str | None      # None: no meshes
    image_root: str | None
    image_folder: str | None     # None: no overlays
    timing: dict | None
    pool: ThreadPoolExecutor | None
    t: float                     # start of the step being timed


def _tick(ctx, key):
    if ctx.timing is not None:
        torch.cuda.synchronize(ctx.eng.device)
        ctx.timing[key] = ctx.timing.get(key, 0.0) + (time.time() - ctx.t)
    ctx.t = time.time()


def per_problem(val, pp, width, name, dtype=np.float32):
    """fix_scale / fix_shape as one row per problem (None: not fixed)."""
    if val is None:
        return None
    if isinstance(val, dict):
        missing = sorted(set(pp.tolist()) - set(val))
        if missing:
            raise ValueError('%s holds no value for persons %s' % (name, missing))
        return np.stack([np.asarray(val[int(p)], dtype).reshape(width) for p in pp])
    return np.tile(np.asarray(val, dtype).reshape(1, width), (len(pp), 1))


def overlay_jobs(image_root, serial, cams, frames, which):
    """render_serial_images' jobs of the frames ``which``: the views that had a keypoint file in the frame (main.py:44-66);
    a missing image is a ValueError, before the fit."""
    return [(f, v, image_path(image_root, serial, cams[v], frames[f][0]), (serial, frames[f][0], cams[v]))
            for f in which for v in range(len(cams)) if frames[f][1][v] is not None]


def single_person_problems(ctx, serial, cams, frames):
    """persons=0: person 0 of every frame of the serial."""
    V, F = len(cams), len(frames)
    kp, vmask = load_serial(frames, V, return_mask=True)
    jobs = overlay_jobs(ctx.image_root, serial, cams, frames, range(F)) if ctx.image_folder is not None else None
    if not vmask.any(1).all():
        raise ValueError('serial %s: frames %s have no keypoint file in any camera folder'
                         % (serial, [frames[f][0] for f in np.flatnonzero(~vmask.any(1))]))
    ann, has = load_serial_joints3d(frames) if ctx.use_3d else (None, np.zeros(F, bool))
    one = np.zeros(F, np.int64)
    # (the one fixed scale reaches the initial guess as the caller's double; per person it is a float32 row)
    return SerialProblems(serial, cams, frames, V, [(f, None) for f in range(F)], np.arange(F), None, kp, vmask, ann, has,
                          per_problem(ctx.fix_scale, one, 1, 'fix_scale', np.float64),
                          per_problem(ctx.fix_shape, one, 10, 'fix_shape'), jobs)


def persons_problems(ctx, serial, cams, frames):
    """persons= a list or 'all': every (frame, person) pair that a view lists, frame-major in ascending id order; None when no
    requested person occurs in the serial."""
    V, F = len(cams), len(frames)
    association = None
    if ctx.associate is not None:
        _tick(ctx, 'read')
        ids_all, kpp, pmask, association = assoc.associate_serial(ctx.eng, frames, ctx.extris, ctx.intris, **ctx.associate)
        _tick(ctx, 'associate')
    else:
        ids_all, kpp, pmask = load_serial_people(frames, V)
    col = {p: i for i, p in enumerate(ids_all)}
    ids = [p for p in (ids_all if ctx.want is None else ctx.want) if p in col]
    prob = [(f, p) for f in range(F) for p in ids if pmask[f, col[p]].any()]
    empty = sorted(set(range(F)) - {f for f, _ in prob})
    if empty:
        warnings.warn('serial %s: frames %s list none of the persons %s in any view; skipped'
                      % (serial, [frames[f][0] for f in empty], 'all' if ctx.want is None else ctx.want), RuntimeWarning)
    if not prob:
        return None
    pf, pp = np.array([f for f, _ in prob]), np.array([p for _, p in prob])
    jobs = overlay_jobs(ctx.image_root, serial, cams, frames, sorted(set(pf.tolist()))) if ctx.image_folder is not None else None
    ann, has = None, np.zeros(len(prob), bool)
    if ctx.use_3d:
        j3p, hasp = load_serial_people3d(frames, ids_all)
        ann = np.stack([j3p[f, col[p]] for f, p in prob])
        has = np.array([hasp[f, col[p]] for f, p in prob])
    return SerialProblems(serial, cams, frames, V, prob, pf, pp, np.stack([kpp[f, col[p]] for f, p in prob]),
                          np.stack([pmask[f, col[p]] for f, p in prob]), ann, has, per_problem(ctx.fix_scale, pp, 1, 'fix_scale'),
                          per_problem(ctx.fix_shape, pp, 10, 'fix_shape'), jobs, association)


def serial_refinements(ctx, sp, rig, gt_xy, conf, intris, has):
    """The refinements the call asks for, in the order they run on a serial's fitted problems: [(name, timing key, result key,
    targets, run)].  run(eng, xf, sp) -> (params, report[, what the result holds under 'cameras']); ``targets``: the 3-D
    targets are set before it when every problem carries them (after a fit in one group they are still in place).  Every one
    runs with the last stage's weights.  A frame is a scene (the problems are frame-major); a person id is a track whose
    frame_idx is the position in the serial's frame list, so an absence breaks the chain; persons=0 is one track."""
    N, o = len(sp.prob), ctx.options
    problems = [(int(f), None if p is None else int(p)) for f, p in sp.prob]
    if sp.pp is None:
        seq_id, frame_idx, sizes = np.zeros(N, np.int64), np.arange(N), None
    else:
        seq_id, frame_idx, sizes = sp.pp, sp.pf, [int((sp.pf == f).sum()) for f in sorted(set(sp.pf.tolist()))]

    def last(with_3d=True):
        return ctx.stages_for(with_3d and bool(has.all()))[-1]
    table = []
    if o['scene_collision'] is not None:
        sc = dict(o['scene_collision'])
        weight = float(sc.pop('weight'))
        table.append(('scene collision', 'refine', 'scene_report', False,
                      lambda eng, xf, sp: refine_scenes(eng, xf, sizes, dict(last(), coll_loss_weight=weight), **sc)))
    if o['silhouettes'] is not None:
        table.append(('silhouettes', 'silhouette', 'silhouette_report', False,
                      lambda eng, xf, sp: refine_serial_silhouettes(eng, xf, last(), o['silhouettes'], sp.serial, sp.cams, sp.frames,
                                                                    problems, rig, eng.nv)))
    if o['scans'] is not None:
        table.append(('scans', 'scan', 'scan_report', False,
                      lambda eng, xf, sp: refine_serial_scans(eng, xf, last(), o['scans'], sp.serial, sp.cams, sp.frames, problems, rig)))
    if o['landmarks'] is not None:
        table.append(('landmarks', 'landmark', 'landmark_report', False,
                      lambda eng, xf, sp: refine_serial_landmarks(eng, xf, last(), o['landmarks'], sp.frames, problems, sp.V,
                                                                  sp.association)))
    if o['temporal'] is not None:
        table.append(('temporal', 'temporal', 'temporal_report', True,
                      lambda eng, xf, sp: smooth_sequences(eng, xf, dict(last(), coll_loss_weight=float(o['temporal']['weight'])),
                                                           seq_id, frame_idx, sweeps=int(o['temporal']['sweeps']))))
    if o['joint'] is not None:
        table.append(('joint', 'joint', 'joint_report', True,
                      lambda eng, xf, sp: refine_serial_joint(eng, xf, last(), o['joint'], sp.serial, sp.cams, sp.frames, problems, rig,
                                                              eng.nv, sizes, seq_id, frame_idx)))
    if o['refine_cameras'] is not None:
        table.append(('cameras', 'cameras', 'camera_report', False,
                      lambda eng, xf, sp: refine_serial_cameras(eng, xf, last(False), o['refine_cameras'], sp.serial, rig, gt_xy, conf,
                                                                intris, ctx.result_folder)))
    return table


def fit_serial(ctx, sp):
    """One serial's problems from the engine's set_problems to the overlays -> the serial's result dict of fit_folder."""
    eng, N, single = ctx.eng, len(sp.prob), sp.pp is None
    F, kp, pf, ann = len(sp.frames), sp.kp, sp.pf, sp.ann
    ex, it = np.asarray(ctx.extris[:sp.V], np.float64), np.asarray(ctx.intris[:sp.V], np.float64)
    rig = (ex[:, :3, :3].astype(np.float32), ex[:, :3, 3].astype(np.float32),
           it[:, 0, 0].astype(np.float32), it[:, :2, 2].astype(np.float32))
    gt_xy = kp[..., :2].copy()
    conf = kp[..., 2] * ctx.jw[None, None, :]
    eng.set_problems(rig, gt_xy, conf)
    _tick(ctx, 'read')
    # 3-D joint targets (non_linear_solver.py:86-99) and the initial alignment to them instead of the triangulation
    # (init_guess.py:84-85) - decided PER PROBLEM like the reference (:68-69): problems with an annotation are fitted with
    # the 3-D term, the others without it (two batched fits when a serial mixes both)
    has = sp.has
    if ctx.is_seq and has.any() and not has.all():
        warnings.warn('serial %s: %d of %d %s carry no 3-D annotation; the is_seq chain runs on one objective - '
                      'fitting the whole serial from the 2-D keypoints only'
                      % (sp.serial, int((~has).sum()), N, 'frames' if single else 'problems'))
        has = np.zeros(N, bool)
    mixed = bool(has.any() and not has.all())
    c3 = None
    if has.any():
        c3 = ann[:, :, 3].copy()
        if not ctx.use_hip:
            c3[:, 11] = c3[:, 12] = 0.0
    # one init_guess_batch per distinct fixed scale (one call when everybody shares it); in a mixed serial the annotated
    # problems are then aligned to their 3-D joints and the rest keep the triangulation / depth guess
    guess = None
    for rows, with_3d in [(np.arange(N), bool(has.all()))] + ([(np.flatnonzero(has), True)] if mixed else []):
        groups = [rows] if sp.scales is None else [rows[sp.scales[rows, 0] == v_] for v_ in np.unique(sp.scales[rows, 0])]
        for g in groups:
            if g.size < N:
                eng.set_problems(rig, gt_xy[g], conf[g])
            r = init_guess_batch(eng, ex, it, kp[g], est_scale=sp.scales is None,
                                 fixed_scale=None if sp.scales is None else float(sp.scales[g[0], 0]),
                                 joints3d=ann[g][:, :, :3].astype(np.float64) if with_3d else None, view_mask=sp.vmask[g])
            if g.size == N:
                guess = r
            else:
                if guess is None:
                    guess = {k: torch.zeros((N,) + tuple(r[k].shape[1:]), dtype=r[k].dtype, device=r[k].device) for k in r}
                idx = torch.as_tensor(g, device=eng.device)
                for k in r:
                    guess[k][idx] = r[k]
                eng.set_problems(rig, gt_xy, conf)
    x0 = initial_params(guess, ctx.use_vposer)
    if sp.shapes is not None:
        x0[:, 0:10] = torch.as_tensor(sp.shapes, device=x0.device)
    _tick(ctx, 'init_guess')

    if ctx.is_seq and single:
        t3 = (ann[None, :, :, :3], c3[None]) if has.all() else None
        xs, st = fit_sequences(eng, rig, gt_xy[None], conf[None], x0[None], ctx.stages_for(has.all()), joints3d=t3)
        xf, final, ncl = xs[0], st['final_loss'][0], st['n_closure'][0]
        restarted = st['restarted'][0]
        eng.set_problems(rig, gt_xy, conf)                  # back to the whole serial for the outputs below
    elif ctx.is_seq:
        # the persons are the sequences; a person's chain runs over the frames they are in
        seq = sorted(set(sp.pp.tolist()))
        row = {p: s_ for s_, p in enumerate(seq)}
        S = len(seq)
        ps = np.array([row[p] for p in sp.pp.tolist()])
        present = np.zeros((S, F), bool)
        present[ps, pf] = True
        gt_s = np.zeros((S, F) + gt_xy.shape[1:], np.float32)
        conf_s = np.zeros((S, F) + conf.shape[1:], np.float32)
        gt_s[ps, pf], conf_s[ps, pf] = gt_xy, conf
        x0_s = torch.zeros(S, F, x0.shape[1], dtype=x0.dtype, device=x0.device)
        x0_s[torch.as_tensor(ps), torch.as_tensor(pf)] = x0
        t3 = None
        if has.all():
            a3, c3_s = np.zeros((S, F, 17, 3), np.float32), np.zeros((S, F, 17), np.float32)
            a3[ps, pf], c3_s[ps, pf] = ann[:, :, :3], c3
            t3 = (a3, c3_s)
        xs, st = fit_sequences(eng, rig, gt_s, conf_s, x0_s, ctx.stages_for(has.all()), joints3d=t3, present=present)
        si, fi = torch.as_tensor(ps, device=xs.device), torch.as_tensor(pf, device=xs.device)
        xf = xs[si, fi].to(x0.dtype)
        final, ncl = st['final_loss'][si, fi], st['n_closure'][si, fi]
        restarted = st['restarted'][ps, pf]
        eng.set_problems(rig, gt_xy, conf)
    else:
        xf = torch.empty_like(x0)
        final = torch.empty(N, device=eng.device)
        ncl = torch.zeros(N, dtype=torch.int32, device=eng.device)
        for sel, with_3d in ((np.flatnonzero(has), True), (np.flatnonzero(~has), False)):
            if sel.size == 0:
                continue
            if sel.size < N:
                eng.set_problems(rig, gt_xy[sel], conf[sel])
            if with_3d:
                eng.set_joints3d(ann[sel][:, :, :3], c3[sel])
            idx = torch.as_tensor(sel, device=eng.device)
            xs_, st = eng.fit(x0[idx], ctx.stages_for(with_3d))
            xf[idx], final[idx], ncl[idx] = xs_.to(xf.dtype), st['final_loss'].to(final.dtype), st['n_closure'].to(ncl.dtype)
        if mixed:
            eng.set_problems(rig, gt_xy, conf)
        restarted = np.ones(N, bool)
    _tick(ctx, 'fit')

    reports = {}
    for _, timing_key, result_key, targets, run in serial_refinements(ctx, sp, rig, gt_xy, conf, it, has):
        if targets and has.all():
            eng.set_joints3d(ann[:, :, :3], c3)
        xr, report, *extra = run(eng, xf, sp)
        xf = xr.to(xf.dtype)
        if report['loss'] is not None:                      # (None: the refinement had nothing to do - the fit's own losses stand)
            final = torch.as_tensor(report['loss'], dtype=final.dtype, device=final.device)
        reports[result_key] = report
        if extra:
            reports['cameras'] = extra[0]
        _tick(ctx, timing_key)

    pid = np.zeros(N, np.int64) if single else sp.pp
    full = eng.full_pose(xf, flags=ctx.flags & ~_lib.F_USE_3D).cpu().numpy()
    xf_h, final_h = xf.cpu().numpy(), final.cpu().numpy()
    res = [iof.result_dict(xf_h[n], loss=final_h[n], body_pose_decoded=full[n, 3:] if ctx.use_vposer else None) for n in range(N)]
    files = [iof.save_result_pkl(ctx.result_folder, sp.serial, sp.frames[pf[n]][0], res[n], person_id=int(pid[n])) for n in range(N)]
    if ctx.mesh_folder is not None or ctx.image_folder is not None:
        # the body of the SAVED parameters: zeroed feet / hands, model(global_orient, transl, body_pose, betas)
        # (utils.py:866-874); its joints are the keypoints save_images draws
        xm = xf_h.copy()
        xm[:, 13:82] = np.stack([r['body_pose'][0] for r in res])
        verts_d, joints_d = eng.vertices(xm, flags=ctx.flags & ~_lib.F_VPOSER)
    if ctx.mesh_folder is not None:
        verts = verts_d.cpu().numpy()
        for n in range(N):
            d = os.path.join(ctx.mesh_folder, sp.serial, sp.frames[pf[n]][0])
            os.makedirs(d, exist_ok=True)
            iof.save_obj(os.path.join(d, '%03d.obj' % int(pid[n])), verts[n], ctx.model['faces'])
    out = dict(frames=[fr[0] for fr in sp.frames], params=xf_h, final_loss=final_h, n_closure=ncl.cpu().numpy(), files=files,
               init=x0.cpu().numpy(), restarted=restarted, used_3d=has.copy(), views_per_frame=sp.vmask.sum(1))
    if not single:
        out.update(problem_frame=pf, problem_person=sp.pp, persons=sorted(set(sp.pp.tolist())))
    out.update(reports)
    if sp.association is not None:
        out['association'] = sp.association
    _tick(ctx, 'write')
    if ctx.image_folder is not None:
        scene = None
        if not single:
            palette = np.asarray(SCENE_PALETTE, np.float32)
            scene = {f: (np.flatnonzero(pf == f).tolist(), palette[sp.pp[pf == f] % 7]) for f in set(pf.tolist())}
        out['images'] = render_serial_images(eng, verts_d, joints_d, sp.jobs, ctx.image_folder, ctx.pool, scene=scene)
        _tick(ctx, 'render')
    return out




def fit_folder(model: dict, keyp_root, cam_file, result_folder, *, vposer=None, image_height=1536.0, is_seq=False,
               pose_format='lsp14', use_hip=True, use_3d=False, fix_scale=None, fix_shape=None, save_meshes=False,
               mesh_folder=None, device=0, stages=None, engine: MvFit | None = None, timing: dict | None = None,
               save_images=False, image_root=None, image_folder=None, persons=0, scene_collision=None, associate=None,
               silhouettes=None, temporal=None, joint=None, refine_cameras=None, scans=None, landmarks=None):
    """Fits every frame under keyp_root and writes the reference's result files.  Returns
    {serial: dict(frames, params [F,118], final_loss [F], n_closure [F], files [F], init [F,118], restarted [F]:
    frames fitted from their own initial guess - all of them unless is_seq, used_3d [F]: frames fitted with the 3-D joint
    term, views_per_frame [F])}.  ``timing``: a dict that receives the wall-clock seconds of the four steps of the pipeline
    (read = directory walk + keypoint / camera files, init_guess, fit, write = decoded pose + result files [+ meshes]),
    summed over the serials - the end-to-end figure next to the reference's only timer (code/main.py:27,91-94).
    save_images: draw the fitted body (the saved parameters, as save_meshes) and its keypoints over each view's image;
    inputs under ``image_root`` (default: the ``images`` folder next to ``keyp_root``, the reference's data layout),
    outputs under ``image_folder`` (default ``<result_folder>/images``); a missing input image is a ValueError.  The
    serial's result gains ``images`` [written paths] and ``timing`` a 'render' entry (decode + GPU + encode).
    persons: which entries of the files' ``people`` lists are fitted.  0 (the default): person 0 only, everything above.
    A list of ids, 'all' (every id that occurs anywhere in the serial; ids as io_formats.read_people defines them) or
    another int p (= [p]): every (frame, person) pair that at least one view lists is one problem, all problems of a serial
    go through one batched fit in frame-major, ascending-id order, and the files are `<frame>/<id:03d>.pkl` / `.obj` with
    the single-person content.  A frame without any of the requested persons is skipped with a RuntimeWarning.  The
    result rows are then per problem, with ``problem_frame`` (index into ``frames``), ``problem_person`` (id) and
    ``persons`` (the sorted ids fitted).  With is_seq the persons are the sequences of fit_sequences: a person's chain
    skips the frames they are absent from and starts cold at their first one.  save_images draws all fitted persons of a
    frame into every view that had a keypoint file, depth-tested, person p in palette colour p mod 7.  fix_scale /
    fix_shape: one value for everybody or a dict {id: value} holding every requested id.
    scene_collision: None, or dict(weight=..., sweeps=3, grid_size=32, robustifier=0.05, scale_factor=0.2) - after the
    batched fit the persons of every frame are refined together (scene_fit.refine_scenes: a frame is a scene) with the last
    stage's weights plus coll_loss_weight = weight, and the refined parameters are what is written; ``final_loss`` is then
    the refined objective, collision term included, the serial's result gains ``scene_report`` and ``timing`` a 'refine'
    entry.  It needs the multi-person path without is_seq (ValueError for persons=0, is_seq=True or a dict without
    ``weight``).  Problems fitted in two groups (with and without 3-D targets) are refined with the 2-D objective only.
    associate: None, True or a dict of max_cost=0.05, min_joints=6, min_views=2, max_move=0.5, max_gap=5 (distances in
    metres; associate.DEFAULTS) - the files' ``people`` lists are in detector order, view by view: the persons are found by
    associate.associate_serial (cross-view association on the device, tracks over the frames) instead of being read off
    the list index or ``person_id``, and ``persons`` ('all' or a list) then names track ids, which count from 0 in order
    of first appearance.  Everything after the keypoints is the multi-person path unchanged.  The serial's result gains
    ``association`` (the report of associate_serial) and ``timing`` an 'associate' entry (reading the detections
    included).  ValueError with persons=0 (one
    identity needs no association), for an unknown key, and with use_3d: the files' 3-D annotations are keyed by
    ``person_id`` and matching them to tracks is not built.
    silhouettes: None, or dict(mask_root=..., weight=..., w_in=1.0, w_out=1.0, sigma=0.0, contour_stride=1, downscale=1,
    max_mask_bytes=2**31) - after the batched keypoint fit the serial's problems are refined against person masks by
    silhouette.refine_fit (the silhouette term inside the engine's fit) with the last stage's weights plus
    coll_loss_weight = weight; a problem keeps the refined row only if its objective fell.  Mask files:
    `<mask_root>/<serial>/<camera>/<frame>.png` for persons=0, `<frame>_<id:03d>.png` on the multi-person path (any Pillow
    image, non-zero = person; io_formats.read_mask).  A missing file means that (problem, view) has no image; a serial with
    no mask at all is a ValueError, and so are masks of different sizes within a serial.  downscale=k fits against masks of
    1/k the resolution (io_formats.downscale_mask) with the rig's f and c divided by k.  ValueError for unknown keys, a
    missing mask_root / weight, is_seq=True, together with scene_collision (one term slot), or when the mask workspace of
    include/mvfit.h exceeds max_mask_bytes (the message names the smallest downscale that fits).  The serial's result gains
    ``silhouette_report`` (refine_fit's, plus images = [(problem, view)] and mask_size), ``timing`` a 'silhouette' entry, and
    ``final_loss`` is the refined objective.  ``occlusion=dict(margin=0.02, sweeps=2)`` (the multi-person path only;
    ValueError with persons=0 or an unknown key) makes the persons of a frame a scene whose bodies occlude one another:
    the masks are modal, so silhouette.refine_fit_occluded freezes the other persons as occluder depth maps per sweep and the
    term ignores what they hide; ``silhouette_report`` then carries ``sweeps`` (per sweep the accepted rows and the
    hidden-vertex and flagged-point counts per image).  Not built: occlusion under ``joint=``.
    temporal: None, or dict(weight=..., sweeps=3) - after the serial's batched fit (or its is_seq chain) every person's track
    over the serial's sorted frame list is smoothed by temporal.smooth_sequences (the vertex-target term inside the engine's
    fit: first-order smoothness of the vertices over consecutive frames) with the last stage's weights plus
    coll_loss_weight = weight; a sequence keeps a sweep's rows only if its joint energy fell.  One sequence per serial for
    persons=0, one per person id on the multi-person path, where a frame the person is absent from breaks the chain.  The
    serial's result gains ``temporal_report`` (smooth_sequences'), ``timing`` a 'temporal' entry, and ``final_loss`` is the
    report's loss (smoothing term included, neighbours frozen at the result).  ValueError for unknown keys, a missing or
    non-positive weight, sweeps < 1, or together with scene_collision or silhouettes (one term slot).
    joint: None, or dict(weight=..., sweeps=3, scene_collision=dict(share=..., grid_size=32, robustifier=0.05,
    scale_factor=0.2), silhouettes=dict(share=..., mask_root=..., w_in=1.0, w_out=1.0, sigma=0.0, contour_stride=1,
    downscale=1, max_mask_bytes=2**31), temporal=dict(share=...)) with at least two of the three parts - after the serial's
    batched fit the problems are refined by joint_refine.refine_joint: ONE fit per sweep carries weight^2 * (the parts'
    shares times the scene collision, silhouette and temporal terms) behind the last stage's weights (the term mix inside the
    engine's fit), obstacles and neighbours frozen where the sweep starts; the problems linked by a frame (scene part) or a
    track (temporal part) keep a sweep only if their joint energy fell.  Masks, scenes and tracks are those of the three
    single options.  The serial's result gains ``joint_report`` (refine_joint's, plus images and mask_size with a silhouette
    part), ``timing`` a 'joint' entry, and ``final_loss`` is the report's loss.  ValueError together with any of the three
    single options, with is_seq=True, for a scene part without persons=, fewer than two parts, unknown keys and non-positive
    numbers.
    scans: None, or dict(weight=..., root=... | depth_root=..., w_s2m=1.0, w_m2s=0.0, sigma=0.05, max_points=8192, stride=1,
    mask_root=None) - after the serial's batched keypoint fit its problems are refined against depth data by scan.refine_fit
    (the scan term inside the engine's fit) with the last stage's weights plus coll_loss_weight = weight (against metres
    squared); a problem keeps the refined row only if its objective fell.  Exactly one source: ``root`` holds world points,
    `<root>/<serial>/<frame>.npy` for persons=0 and `<frame>_<id:03d>.npy` on the multi-person path, float [P,3] in metres, or
    [P,4] with a weight >= 0 in the last column; ``depth_root`` holds camera-space z in metres at the camera file's
    resolution, `<depth_root>/<serial>/<camera>/<frame>.npy` float [H,W], unprojected by scan.points_from_depth over the
    problem's views in rig order with ``stride`` and masked by `mask_path(mask_root, ...)` where mask_root is given and the
    file exists (required with more than one person).  A problem without a file has no points and pays nothing; a serial with no
    file at all is a ValueError that names an example path, and so are files of another shape or dtype and negative or
    non-finite weights.  More than max_points points per problem keep rows floor(i * P / max_points).  `.npy` only: depth PNGs
    and `.ply` files are not built.  ValueError before any engine is created with is_seq, with refine_cameras and next to a
    single scene_collision, silhouettes or temporal (they combine inside ``joint``).  The serial's result gains ``scan_report``
    (refine_fit's, plus points = the count per problem), ``timing`` a 'scan' entry, and ``final_loss`` is the refined
    objective.  Inside ``joint``, ``scans=dict(share=..., root= | depth_root=, ...)`` with the same keys is a fourth part: at
    least two of the four.
    landmarks: None, or dict(weight=..., table=..., rho=100.0) - after the serial's batched keypoint fit its problems are
    refined against the points of the SAME keypoint files that the 17-row readers drop, by landmarks.refine_fit (the surface
    landmark term inside the engine's fit) with the last stage's weights plus coll_loss_weight = weight (against pixels
    squared); a problem keeps the refined row only if its objective fell.  ``table``: a landmark table file or dict
    (landmarks.load_table) whose keypoint_index names each landmark's row of ``pose_keypoints_2d`` - for AlphaPose Halpe-26
    the six foot points are rows 20-25.  A problem follows the entry its 17 keypoints follow (persons=0 the first entry,
    persons= the id, associate= the track's detection); files with fewer rows give no targets, and a serial without any is
    not refitted: its results are those of the call without the option, bit for bit.  ValueError before any engine is
    created for unknown keys, weight <= 0, is_seq, a vertex id outside the model, and next to scene_collision, silhouettes,
    temporal, scans, joint or refine_cameras.  The serial's result gains ``landmark_report`` (refine_fit's, plus targets =
    the live entries per problem) and ``timing`` a 'landmark' entry.
    refine_cameras: None, or dict(sweeps=2, anchor=0, free='extrinsics', min_points=34) - after the serial's batched fit the
    rig is refined against the fitted bodies of the serial's whole batch and the bodies are refitted under it, with the last
    stage (calibrate.refine_rig; anchor: the view kept as the camera file gives it, or None).  Single-person and persons=
    path alike.  The result files, meshes and overlays come from the refined fit and rig; <result_folder>/<serial>/
    cameras_refined.txt is written in the camera file's layout (its intrinsics are the file's with f in [0,0] and [1,1] and c
    in [:2,2]); the serial's result gains ``camera_report`` (refine_rig's) and ``cameras`` = (extris, intris), ``timing`` a
    'cameras' entry, and ``final_loss`` is the report's loss.  The next serial starts from the camera file again.  Not built,
    ValueError before any engine work: together with is_seq, use_3d, scene_collision, silhouettes, temporal or joint; also
    for unknown keys."""
    t0 = time.time()
    model_type = 'smpllsp' if model.get('kp_regressor') is not None else 'smpl'
    if pose_format not in POSE_FORMATS:
        raise ValueError('Unknown pose format: {}'.format(pose_format))
    if POSE_FORMATS[pose_format] != model_type:                   # utils.py:444-457
        raise ValueError("pose_format '%s' needs a model of type '%s'; this model is of type '%s'"
                         % (pose_format, POSE_FORMATS[pose_format], model_type))
    multi = not (isinstance(persons, (int, np.integer)) and not isinstance(persons, bool) and int(persons) == 0)
    want = None                                                    # 'all'
    if multi and not (isinstance(persons, str) and persons == 'all'):
        if isinstance(persons, (str, bool)):
            raise ValueError("persons: an id, a list of ids or 'all', not %r" % (persons,))
        want = sorted({int(p) for p in (persons if isinstance(persons, (list, tuple, set, np.ndarray)) else [persons])})
    options = dict(
        scene_collision=check_scene_collision(scene_collision, is_seq, multi) if scene_collision is not None else None,
        silhouettes=check_silhouettes(silhouettes, is_seq, scene_collision, multi) if silhouettes is not None else None,
        temporal=check_temporal(temporal, scene_collision, silhouettes) if temporal is not None else None,
        scans=(check_scans(scans, is_seq, multi, scene_collision, silhouettes, temporal, refine_cameras)
               if scans is not None else None),
        joint=check_joint(joint, is_seq, multi, scene_collision, silhouettes, temporal, scans) if joint is not None else None,
        refine_cameras=(check_refine_cameras(refine_cameras, is_seq, use_3d, scene_collision, silhouettes, temporal, joint, scans)
                        if refine_cameras is not None else None),
        landmarks=(check_landmarks(landmarks, model['v_template'].shape[0], is_seq, scene_collision, silhouettes, temporal, scans, joint,
                                   refine_cameras) if landmarks is not None else None))
    if associate is not None and associate is not False:
        if not multi:
            raise ValueError('associate finds the persons of a serial: it needs persons= a list of track ids or \'all\'')
        if use_3d:
            raise ValueError('associate with use_3d is not available: 3-D annotations are keyed by person_id, not by track')
        associate = assoc.check_params(associate)
    else:
        associate = None
    for name, val in (('fix_scale', fix_scale), ('fix_shape', fix_shape)):
        if isinstance(val, dict) and want is not None and not set(want) <= set(val):
            raise ValueError('%s holds no value for persons %s' % (name, sorted(set(want) - set(val))))
    if not multi:
        fix_scale = fix_scale[0] if isinstance(fix_scale, dict) else fix_scale
        fix_shape = fix_shape[0] if isinstance(fix_shape, dict) else fix_shape
    extris, intris = iof.load_camera_para(cam_file)
    flags = _lib.F_VPOSER if vposer is not None else 0
    if fix_scale is not None:
        flags |= _lib.F_FIX_SCALE
    if fix_shape is not None:
        flags |= _lib.F_FIX_SHAPE
    eng = engine if engine is not None else MvFit(model, vposer=vposer, device=device)
    jw = np.ones(17, np.float32)
    if pose_format != 'lsp14' or not use_hip:                      # data_parser.py:353-356
        jw[11] = jw[12] = 0.0

    def stages_for(with_3d):
        if stages is None:
            return stage_weights(float(image_height), flags=flags | (_lib.F_USE_3D if with_3d else 0))
        # caller's stage list: the 3-D term follows the group being fitted (annotated frames carry it, the others
        # must not run it against absent targets), whatever the caller's flag words say
        out = []
        for st_ in stages:
            st_ = dict(st_)
            f_ = int(st_.get('flags', 0))
            st_['flags'] = (f_ | _lib.F_USE_3D) if with_3d else (f_ & ~_lib.F_USE_3D)
            out.append(st_)
        return out
    if save_images and image_root is None:
        image_root = os.path.join(os.path.dirname(os.path.normpath(keyp_root)), 'images')
    pool = ThreadPoolExecutor(max_workers=IO_WORKERS) if save_images else None
    ctx = FitContext(eng=eng, model=model, extris=extris, intris=intris, jw=jw, flags=flags, use_vposer=vposer is not None,
                     use_hip=use_hip, use_3d=use_3d, is_seq=is_seq, stages_for=stages_for, want=want, associate=associate,
                     fix_scale=fix_scale, fix_shape=fix_shape, options=options, result_folder=result_folder,
                     mesh_folder=(mesh_folder or os.path.join(result_folder, 'meshes')) if save_meshes else None,
                     image_root=image_root,
                     image_folder=(image_folder or os.path.join(result_folder, 'images')) if save_images else None,
                     timing=timing, pool=pool, t=t0)
    results = {}
    try:
        _tick(ctx, 'read')
        for serial, cams, frames in list_frames(keyp_root):
            V, F = len(cams), len(frames)
            if F == 0 or V < 1:
                continue
            if V > len(extris):
                raise ValueError('serial %s has %d camera folders, the camera file %s holds %d cameras' % (serial, V, cam_file, len(extris)))
            sp = (persons_problems if multi else single_person_problems)(ctx, serial, cams, frames)
            if sp is not None:
                results[serial] = fit_serial(ctx, sp)
    finally:
        if pool is not None:
            pool.shutdown()
        if engine is None:
            eng.close()
    return results


__all__ = ['list_frames', 'load_serial', 'load_serial_people', 'load_serial_people3d', 'fit_folder', 'fit_serial', 'SerialProblems',
           'FitContext', 'single_person_problems', 'persons_problems', 'check_scene_collision', 'image_path', 'render_serial_images', 'POSE_FORMATS',
           'check_silhouettes', 'check_temporal', 'mask_path', 'silhouette_workspace_bytes', 'refine_serial_silhouettes',
           'check_joint', 'load_serial_masks', 'refine_serial_joint', 'check_refine_cameras', 'refine_serial_cameras',
           'check_scans', 'scan_path', 'subsample_rows', 'load_serial_scans', 'refine_serial_scans',
           'check_landmarks', 'load_serial_landmarks', 'refine_serial_landmarks']
