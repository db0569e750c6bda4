"""TESTS ONLY - the world of tests/test_gpu_silhouette_occlusion.py: five bodies in two scenes seen by five cameras.

  scene 0: body 0 stands in front of body 1 in view 0; in view 1 the two stand side by side
  scene 1: body 2 (no image of its own: it only occludes) in front of body 3 in view 2, in a close-up of body 2's largest
           faces (they take the rasteriser's whole-workgroup path, and most of body 2 lies outside the image) and in a camera
           that stands inside body 2's extent (part of body 2 lies behind the near plane)
  body 4 : scene -1, far to the side

Cameras 0..2 are views 0, 1, 2 of a four-camera ring at radius 4; cameras 3 and 4 look along view 2's axis."""
import numpy as np

from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import pack_params

N = 5
BODY_SCENE = np.array([0, 0, 1, 1, -1], np.int32)
TRANSL = np.array([[0.3, 0.0, 0.5], [0.0, 0.0, -0.4], [-0.15, 0.0, -0.5], [-0.3, 0.0, 0.3], [0.9, 0.0, 0.0]], np.float32)
IMAGES = [(1, 0), (1, 1), (0, 0), (3, 2), (3, 3), (3, 4), (4, 0)]          # (body, camera)
BACK = 1                                                                   # the back body of scene 0
H, W = 96, 128
CLOSE_EYE = np.array([-0.40, 0.05, -1.5], np.float32)                     # camera 3
CLOSE_F = 1100.0
NEAR_EYE = np.array([-0.50, -0.30, -0.62], np.float32)                     # camera 4
NEAR_F = 60.0


def params():
    """x [N,118] float32: poses of seeded frames, betas 0, scale 1, the translations above."""
    fr = syn.make_frames(N, seed0=7100)
    x = pack_params(B=N, **fr)
    x[:, 0:10] = 0.0
    x[:, 85] = 1.0
    x[:, 82:85] = TRANSL
    return x.astype(np.float32)


def cameras(height=H, width=W):
    """(R[5,3,3], t[5,3], f[5], c[5,2]) float32 for images of height x width: the same fields of view at every size."""
    R4, t4, _, _ = syn.make_camera_ring(4, radius=4.0)
    k = np.float32(width / float(W))
    R = np.concatenate([R4[:3], R4[2:3], R4[2:3]]).astype(np.float32)
    t = np.concatenate([t4[:3], (-R4[2] @ CLOSE_EYE)[None], (-R4[2] @ NEAR_EYE)[None]]).astype(np.float32)
    f = (np.array([200.0, 200.0, 200.0, CLOSE_F, NEAR_F], np.float32) * k).astype(np.float32)
    c = np.tile(np.array([width / 2.0, height / 2.0], np.float32), (5, 1))
    return R, t, f, c


def per_image(cams, images=IMAGES):
    view = np.array([i[1] for i in images])
    return tuple(a[view] for a in cams)


def scene_members(body):
    s = BODY_SCENE[body]
    return [body] if s < 0 else [int(m) for m in np.flatnonzero(BODY_SCENE == s)]
