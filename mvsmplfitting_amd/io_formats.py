"""Data formats either side of the fitting path, host side only - so that keypoint files and
camera files of a reference data folder can be turned into the tensors `MvFit.set_problems` / `triangulate` take,
and fitted parameters written the way the reference's tools read them.

  load_camera_para   camera text file: 3-number lines are rows of K, 4-number lines rows of [R|t]; every three rows one
                     matrix, [0,0,0,1] appended to the extrinsics  (reference code/utils/utils.py:352-394)
  read_keypoints     OpenPose-style json {"people":[{"pose_keypoints_2d":[51 floats]}]} -> per person [17,3] float32
                     (reference code/utils/data_parser.py:42-90 with use_hands=False, use_face=False, the
                     'smpllsp' / halpe-17 configuration of fit_smpl.yaml)
  read_people_extra  the rows of ``pose_keypoints_2d`` those readers drop (a Halpe-26 file's foot points, rows 20-25), per person
  read_joints3d      {"people":[{"pose_keypoints_3d":[...]}]} -> per person [-1,4] float32 (data_parser.py:93-109)
  problem_tensors    one rig + per-view keypoints -> (cams, gt_xy, conf) of MvFit.set_problems, fx for both axes
                     like the reference camera (code/init.py:113-119)
  result_dict        what the reference pickles per person (code/utils/utils.py:744-764, 826-857): the decoded
                     VPoser body_pose has the foot / hand joints zeroed ([18:24], [27:33], [57:]) before it is stored
  save_result_pkl    pickle protocol 2, `<folder>/<serial>/<fn>/000.pkl` (utils.py:859-864)
  save_obj           Wavefront obj, 1-based faces (code/utils/FileLoaders.py:154-160)
  read_image         image file -> RGB uint8 [H,W,3], EXIF orientation applied like cv2.imread's default (the
                     reference: cv2.imread, BGR; data_parser.py)
  image_size         (H, W) read_image will return, from the file header (no pixel decode)
  save_image         RGB uint8 [H,W,3] -> file, JPEG quality 95 like cv2.imwrite's default (utils.py:700-712)
                     (both through PIL, imported when first used)
  read_mask          person mask file -> uint8 [H,W], non-zero = on: any Pillow mode converted to 8-bit grey, EXIF
                     orientation applied as for the overlay inputs
  downscale_mask     [H,W] -> [ceil(H/k), ceil(W/k)]: a low-res pixel is on when at least half of the pixels its k x k block
                     has are on
"""
from __future__ import annotations

import json
import os
import pickle

import numpy as np


def load_camera_para(path):
    intr_rows, extr_rows = [], []
    with open(path, 'r') as f:
        for line in f:
            words = line.strip('\n').rstrip().split()
            if len(words) == 3:
                intr_rows.append([float(w) for w in words])
            elif len(words) == 4:
                extr_rows.append([float(w) for w in words])
    intris = [intr_rows[i:i + 3] for i in range(0, len(intr_rows) - len(intr_rows) % 3, 3)]
    extris = [extr_rows[i:i + 3] + [[0., 0., 0., 1.]] for i in range(0, len(extr_rows) - len(extr_rows) % 3, 3)]
    return np.array(extris), np.array(intris)


def save_camera_para(path, extris, intris):
    """The inverse of load_camera_para, in the layout of the 3DOH50K parameter file: per camera an index line, three
    intrinsic rows, ``0 0``, the three upper extrinsic rows and a blank line.  Numbers are written with repr, so that
    load after save returns the same bits."""
    extris, intris = np.asarray(extris, np.float64), np.asarray(intris, np.float64)
    if extris.ndim != 3 or extris.shape[1] < 3 or extris.shape[2] != 4 or intris.shape != (extris.shape[0], 3, 3):
        raise ValueError('extris must be [V,4,4] (or [V,3,4]) and intris [V,3,3]')
    with open(path, 'w') as f:
        for v in range(extris.shape[0]):
            f.write('%d\n' % v)
            for row in intris[v]:
                f.write(' '.join(repr(float(x)) for x in row) + ' \n')
            f.write('0 0\n')
            for row in extris[v, :3]:
                f.write(' '.join(repr(float(x)) for x in row) + ' \n')
            f.write('\n')


def read_keypoints(path):
    with open(path) as f:
        data = json.load(f)
    return [np.array(p['pose_keypoints_2d'], dtype=np.float32).reshape([-1, 3])[:17] for p in data['people']]


def read_joints3d(path):
    with open(path) as f:
        data = json.load(f)
    return [np.array(p['pose_keypoints_3d'], dtype=np.float32).reshape([-1, 4]) for p in data['people']]


def _read_people(path, key, width):
    with open(path) as f:
        people = json.load(f)['people']
    by_id = all(isinstance(p.get('person_id'), int) and not isinstance(p.get('person_id'), bool) for p in people)
    out = {}
    for k, p in enumerate(people):
        if key not in p:
            if key == 'pose_keypoints_2d':
                raise KeyError(key)
            continue
        a = np.array(p[key], dtype=np.float32).reshape([-1, width])[:17]
        if not a[:, width - 1].any():                      # every confidence zero: the person is not in this file
            continue
        pid = int(p['person_id']) if by_id else k
        if pid in out:
            raise ValueError('%s lists person %d twice' % (path, pid))
        out[pid] = a
    return out


def read_people(path):
    """{person id: [17, 3] float32 (x, y, confidence)} of one keypoint file.  The id of a ``people`` entry is its integer
    ``person_id`` field when EVERY entry of the file carries one, else its index in the list.  An entry whose confidences
    are all zero counts as absent - how an index-identified file says "person 1 is not in this view but person 2 is".
    Files whose lists are in detector order carry no identity this rule could read: those go through
    associate.associate_serial (batch.fit_folder(associate=...)), which finds the persons across views and frames.
    Two entries with one id: ValueError naming the file."""
    return _read_people(path, 'pose_keypoints_2d', 3)


def read_people_extra(path, rows, by_index=False):
    """{person id: [len(rows), 3] float32 (x, y, confidence)}: the rows ``rows`` of every person's ``pose_keypoints_2d``,
    those that read_keypoints and read_people drop included (a whole-body detector's foot, hand and face points; Halpe-26
    keeps both big toes, small toes and heels in rows 20-25).  Ids by read_people's rule, or - by_index - the entry's index
    in the list whatever ``person_id`` says (the single-person and the associate= paths count that way).  A file with fewer
    rows gives zeros, i.e. confidence 0, for the missing ones.  Like read_people, an entry whose first 17 confidences are all zero counts as absent (by_index:
    every entry is listed)."""
    rows = np.asarray(rows, np.int64).reshape(-1)
    if (rows < 0).any():
        raise ValueError('read_people_extra: negative row')
    with open(path) as f:
        people = json.load(f)['people']
    by_id = not by_index and all(isinstance(p.get('person_id'), int) and not isinstance(p.get('person_id'), bool) for p in people)
    out = {}
    for k, p in enumerate(people):
        a = np.array(p['pose_keypoints_2d'], dtype=np.float32).reshape([-1, 3])
        if not by_index and not a[:17, 2].any():           # read_people's rule: the person is not in this file
            continue
        got = np.zeros((rows.size, 3), np.float32)
        ok = rows < a.shape[0]
        got[ok] = a[rows[ok]]
        pid = int(p['person_id']) if by_id else k
        if pid in out:
            raise ValueError('%s lists person %d twice' % (path, pid))
        out[pid] = got
    return out


def read_people3d(path):
    """The 3-D twin of read_people: {person id: [17, 4] float32 (x, y, z, confidence)} from ``pose_keypoints_3d``, by the
    same id rule; entries without the field are left out."""
    return _read_people(path, 'pose_keypoints_3d', 4)


def problem_tensors(extris, intris, keypoints_per_view):
    """extris [V,4,4], intris [V,3,3]; keypoints_per_view: list over views of [17,3] (one person, one frame).
    Returns cams = (R[V,3,3], t[V,3], f[V], c[V,2]) float32, gt_xy [1,V,17,2], conf [1,V,17]."""
    extris = np.asarray(extris, np.float64)
    intris = np.asarray(intris, np.float64)
    kp = np.stack([np.asarray(k, np.float32).reshape(-1, 3)[:17] for k in keypoints_per_view])
    cams = (extris[:, :3, :3].astype(np.float32), extris[:, :3, 3].astype(np.float32),
            intris[:, 0, 0].astype(np.float32), intris[:, :2, 2].astype(np.float32))
    return cams, kp[None, :, :, :2].copy(), kp[None, :, :, 2].copy()


def result_dict(x118, loss=None, body_pose_decoded=None):
    """x118: one row of the engine's flat parameter layout (include/mvfit.h); body_pose_decoded [69]: the VPoser
    decode of the fitted embedding when VPoser was used.  Like save_results (utils/utils.py:744-766) the saved body_pose /
    pose have the feet and hand joints zeroed, with or without VPoser."""
    x = np.asarray(x118, np.float32).reshape(-1)
    res = dict(betas=x[0:10][None].copy(), global_orient=x[10:13][None].copy(), transl=x[82:85][None].copy(),
               scale=x[85:86][None].copy())
    if loss is not None:
        res['loss'] = float(loss)
    if body_pose_decoded is not None:
        bp = np.asarray(body_pose_decoded, np.float32).reshape(1, 69).copy()
        res['pose_embedding'] = x[86:118][None].copy()
    else:
        bp = x[13:82][None].copy()
        res['pose_embedding'] = None      # the reference stores the key in both branches (non_linear_solver.py:286: None without VPoser)
    bp[:, 18:24] = 0.          # feet and hands are zeroed in both branches (utils/utils.py:750-753 and :761-764)
    bp[:, 27:33] = 0.
    bp[:, 57:] = 0.
    res['body_pose'] = bp
    res['pose'] = np.hstack((res['global_orient'], bp))
    return res


def save_result_pkl(result_folder, serial, fn, result, person_id=0):
    d = os.path.join(result_folder, serial, fn)
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, '{:03d}.pkl'.format(person_id))
    with open(path, 'wb') as f:
        pickle.dump(result, f, protocol=2)
    return path


def save_obj(path, vertices, faces):
    v = np.asarray(vertices).reshape(-1, 3)
    fc = np.asarray(faces).reshape(-1, 3) + 1
    with open(path, 'w') as fp:
        for p in v:
            fp.write('v %f %f %f\n' % (p[0], p[1], p[2]))
        for f in fc:
            fp.write('f %d %d %d\n' % (f[0], f[1], f[2]))


def _pil():
    try:
        from PIL import Image
    except ImportError as e:                     # pragma: no cover - depends on the installation
        raise ImportError('reading and writing images needs the Pillow package (PIL), which is not installed') from e
    return Image


_EXIF_ORIENTATION = 0x0112


def read_image(path):
    from PIL import ImageOps
    with _pil().open(path) as im:
        return np.asarray(ImageOps.exif_transpose(im).convert('RGB'), dtype=np.uint8)


def read_mask(path):
    """A person mask -> uint8 [H, W], non-zero = on (what MvFit.set_silhouettes takes per image)."""
    from PIL import ImageOps
    with _pil().open(path) as im:
        return np.asarray(ImageOps.exif_transpose(im).convert('L'), dtype=np.uint8)


def read_points(path):
    """A scan's point file (.npy) -> (points float32 [P,3] in world coordinates, weights float32 [P] or None): a float array
    [P,3], or [P,4] with a weight >= 0 in the last column.  ValueError for another shape or dtype and for a negative or
    non-finite weight."""
    a = np.load(path, allow_pickle=False)
    if a.ndim != 2 or a.shape[1] not in (3, 4) or not np.issubdtype(a.dtype, np.floating):
        raise ValueError('%s: a point file holds a float array [P,3] or [P,4], not %s %r' % (path, a.dtype, a.shape))
    if a.shape[1] == 3:
        return np.ascontiguousarray(a, np.float32), None
    w = a[:, 3].astype(np.float32)
    if not np.isfinite(w).all() or (w < 0).any():
        raise ValueError('%s: the weights (last column) must be finite and >= 0' % path)
    return np.ascontiguousarray(a[:, :3], np.float32), w


def read_depth(path):
    """A depth map (.npy) -> float32 [H,W], camera-space z; a pixel without a measurement holds 0, a negative value, inf or NaN.
    ValueError for another shape or dtype."""
    a = np.load(path, allow_pickle=False)
    if a.ndim != 2 or not np.issubdtype(a.dtype, np.floating):
        raise ValueError('%s: a depth map holds a float array [H,W], not %s %r' % (path, a.dtype, a.shape))
    return np.ascontiguousarray(a, np.float32)


def downscale_mask(mask, k):
    """mask [H, W] (non-zero = on) at 1/k of the resolution: low-res pixel (y, x) covers the block rows k y .. k y + k - 1,
    columns likewise, cut at the image's edge, and is on (1) when at least half of the pixels the block HAS are on.  k = 1
    gives the mask back unchanged.  Cameras follow with f / k and c / k."""
    m = np.asarray(mask)
    if m.ndim != 2:
        raise ValueError('downscale_mask: expected [H, W], got %s' % (m.shape,))
    k = int(k)
    if k < 1:
        raise ValueError('downscale_mask: k = %d < 1' % k)
    if k == 1:
        return np.ascontiguousarray(m, dtype=np.uint8)
    H, W = m.shape
    h, w = -(-H // k), -(-W // k)
    on = np.zeros((h * k, w * k), np.int64)
    on[:H, :W] = m != 0
    have = np.zeros((h * k, w * k), np.int64)
    have[:H, :W] = 1
    on = on.reshape(h, k, w, k).sum(axis=(1, 3))
    have = have.reshape(h, k, w, k).sum(axis=(1, 3))
    return (2 * on >= have).astype(np.uint8)


def image_size(path):
    with _pil().open(path) as im:                # opening reads the header only
        w, h = im.size
        if im.getexif().get(_EXIF_ORIENTATION, 1) in (5, 6, 7, 8):     # a quarter turn: exif_transpose swaps the axes
            w, h = h, w
    return h, w


def save_image(path, rgb, quality=95):
    a = np.ascontiguousarray(rgb, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError('save_image: expected RGB uint8 [H, W, 3], got %s' % (a.shape,))
    _pil().fromarray(a, 'RGB').save(path, quality=int(quality))
    return path


__all__ = ['read_image', 'image_size', 'save_image', 'read_mask', 'read_points', 'read_depth', 'downscale_mask', 'load_camera_para', 'read_keypoints', 'read_joints3d', 'read_people', 'read_people3d', 'problem_tensors', 'result_dict',
           'save_result_pkl', 'save_obj']
