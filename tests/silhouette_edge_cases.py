"""TESTS ONLY - builders for the silhouette term at its tile, chunk and instance-group edges (pure NumPy, no GPU):
tests/test_silhouette_edge_cases_cpu.py proves on the oracles that every case reaches the edge it is named for,
tests/test_gpu_silhouette_edges.py runs the kernels on the same cases.

  masks     400 x 400, K isolated on pixels at even (y, x) in raster order: each is a contour point, so an image keeps exactly
            ceil(K / stride) points - full last chunks, last chunks of one point, an empty image between non-empty ones, 65
            chunks in one image - and an all-on image
  bodies    sub_model(body_model(), nv), posed (oracle/closure_np.py on the CPU, MvFit.vertices on the GPU), three of them,
            the middle one without an image, under cameras on an arc in front of them
  edits     of the vertex rows: ties inside one 16-byte read, across two reads and across the LDS tile boundary, a body with
            one valid vertex; of a camera: an image whose body lies behind it
  occluders twelve bodies of one scene in 48 images at 96 x 128: 576 (image, body) instances, the close-up camera from image
            43 on"""
import functools

import numpy as np

from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import pack_params
from oracle import closure_np as cn
from tests import render_oracle as ro
from tests import silhouette_occlusion_world as wd
from tests import silhouette_oracle as so
from tests.helpers import body_model
from tests.small_models import sub_model

SIZE = 400
COUNTS = (1, 511, 512, 513, 1024, 1025, 0, 1536, 1537, 32769)           # on pixels of images 0 .. 9; image 10 is all on
KEPT = {1: (1, 511, 512, 513, 1024, 1025, 0, 1536, 1537, 32769, 0),      # kept contour points per image and stride
        3: (1, 171, 171, 171, 342, 342, 0, 512, 513, 10923, 0)}
IMAGE_BODY = np.array([0, 2, 0, 2, 0, 2, 0, 2, 0, 2, 0], np.int32)       # interleaved; body 1 has no image
BIG_IMAGE, BIG_BODY = 9, 2                                               # the 32769-point image and its body
N = 3
NVS = (701, 3456, 3457, 6890)
TRANSL = np.array([[0.0, 0.0, 0.0], [0.3, 0.0, 0.2], [-0.1, 0.05, 0.1]], np.float32)
BEHIND = np.array([0.0, 0.0, -10.0], np.float32)                         # behind every camera of arc_cameras
SETTINGS = dict(both=dict(w_in=1.0, w_out=1.0, sigma=0.0), sigma20=dict(w_in=1.0, w_out=1.0, sigma=20.0),
                termB=dict(w_in=0.0, w_out=1.0, sigma=0.0), termA=dict(w_in=1.0, w_out=0.0, sigma=0.0))


@functools.lru_cache(maxsize=None)
def model(nv):
    full = body_model()
    return full if nv == full['v_template'].shape[0] else sub_model(full, nv)


# ---------------------------------------------------------------------------------------------------------------- masks
@functools.lru_cache(maxsize=None)
def exact_count_masks():
    """uint8 [11,400,400] (shared: treat it as read-only)."""
    masks = np.zeros((len(COUNTS) + 1, SIZE, SIZE), np.uint8)
    ys, xs = (a.ravel() for a in np.mgrid[0:SIZE:2, 0:SIZE:2])
    for i, K in enumerate(COUNTS):
        masks[i, ys[:K], xs[:K]] = 200
    masks[-1] = 200
    return masks


@functools.lru_cache(maxsize=None)
def prepared(stride):
    return so.prepare(exact_count_masks(), stride)


# -------------------------------------------------------------------------------------------------------------- cameras
def arc_cameras(M=len(IMAGE_BODY), size=SIZE):
    """(R[M,3,3], t[M,3], f[M], c[M,2]) float32, one camera per image: eyes at distance 4 on an arc of +-0.6 rad around
    (0, 0, -4) at three heights, looking at the origin; a standing body fills half of the image's height."""
    R, t = [], []
    for i in range(M):
        a, h = 0.3 * (i % 5 - 2), 0.5 * (i % 3 - 1)
        eye = np.array([4.0 * np.sin(a), h, -4.0 * np.cos(a)])
        R.append(syn.look_at_rotation(eye))
        t.append(-R[-1] @ eye)
    f = np.full(M, 2400.0 * size / 2048.0, np.float32)
    c = np.full((M, 2), size / 2.0, np.float32)
    return np.asarray(R, np.float32), np.asarray(t, np.float32), f, c


def all_behind(cams, image):
    """The cameras with the one of ``image`` moved 20 units forward along its axis: every vertex of its body has pz < 0."""
    R, t, f, c = (a.copy() for a in cams)
    t[image, 2] -= 20.0
    return R, t, f, c


# --------------------------------------------------------------------------------------------------------------- bodies
def params(n=N, seed0=4100, transl=TRANSL):
    """x [n,118] float32: seeded poses, betas 0, scale 1."""
    fr = syn.make_frames(n, seed0=seed0)
    x = pack_params(B=n, **fr)
    x[:, 0:10] = 0.0
    x[:, 85] = 1.0
    x[:, 82:85] = transl
    return x.astype(np.float32)


def posed(nv, x):
    """float32 [n,nv,3]: the float64 body model of oracle/closure_np.py at the rows of x, rounded (the CPU's stand-in for
    MvFit.vertices)."""
    orc = cn.ClosureOracle(model(nv), np.float64)
    out = [orc.body(dict(betas=r[0:10], global_orient=r[10:13], body_pose=r[13:82], transl=r[82:85], scale=r[85],
                         use_vposer=False), want_cache=False)['vertices'] for r in np.asarray(x, np.float64)]
    return np.asarray(out).astype(np.float32)


# ------------------------------------------------------------------------------------------------- winners, restated once more
def winners(prep, vertices, image_body, cams):
    """(first, last) int32 [C]: tests/silhouette_oracle.py's distance matrix (fp32 projection, fp32 products and sum, valid
    vertices only) with its first minimum per point - the contract - and the last minimum on the same matrix: what a
    search with ``<=`` in place of ``<`` would report."""
    V = np.asarray(vertices, np.float32)
    first, xy = prep['first'], prep['xy']
    lo, hi = np.full(len(xy), -1, np.int32), np.full(len(xy), -1, np.int32)
    for i in range(len(first) - 1):
        pts = xy[first[i]:first[i + 1]]
        p, u, w = ro.transform(V[int(image_body[i])], cams[0][i], cams[1][i], cams[2][i], cams[3][i])
        idx = np.flatnonzero(p[:, 2] > np.float32(so.ZNEAR))
        if not len(pts) or not len(idx):
            continue
        uu, ww = u[idx], w[idx]
        for k0 in range(0, len(pts), 256):
            q = pts[k0:k0 + 256]
            cx, cy = q[:, 0].astype(np.float32) + np.float32(0.5), q[:, 1].astype(np.float32) + np.float32(0.5)
            dx, dy = uu[None, :] - cx[:, None], ww[None, :] - cy[:, None]
            m = dx * dx + dy * dy
            lo[first[i] + k0:first[i] + k0 + len(q)] = idx[np.argmin(m, axis=1)]
            hi[first[i] + k0:first[i] + k0 + len(q)] = idx[m.shape[1] - 1 - np.argmin(m[:, ::-1], axis=1)]
    return lo, hi


def wins(winner, first, image_body, body, nv):
    """int64 [nv]: how many kept contour points of the body's images each vertex wins."""
    w = np.concatenate([winner[first[i]:first[i + 1]] for i in np.flatnonzero(np.asarray(image_body) == body)])
    return np.bincount(w[w >= 0], minlength=nv)


def most_winning(winner, first, image_body, nv):
    """{body: the vertex that wins most points} for the bodies with images."""
    return {int(b): int(np.argmax(wins(winner, first, image_body, b, nv))) for b in np.unique(image_body)}


# ------------------------------------------------------------------------------------------------------------------ ties
# kind -> (the rows that take a copy of row jw, given jw; whether jw itself goes behind the cameras).  With the LDS tile of
# 3456 vertices and two vertices per 16-byte read: vertices 2k and 2k + 1 share a read, 3455 ends tile 0, 3456 opens tile 1.
TIES = {
    'pair': (lambda jw: [jw ^ 1], False),                                # one read; the lower index is even
    'next_read': (lambda jw: [jw + 2 - (jw & 1)], False),                # the first vertex of the next read
    'second_tile': (lambda jw: [3456], False),
    'all_three': (lambda jw: [jw ^ 1, jw + 2 - (jw & 1), 3456], False),
    'tile_boundary': (lambda jw: [3455, 3456], True),                    # the lower index is odd, the last of tile 0
    'tile_boundary_even': (lambda jw: [3454, 3456], True),
    'next_read_odd': (lambda jw: [501, 502], True),                    # the lower index is odd, the higher opens the next read
    'next_read_even': (lambda jw: [500, 502], True),
    'second_tile_odd': (lambda jw: [501, 3456], True),
}
TIES_701 = ('pair', 'next_read', 'next_read_odd')                        # one tile: the kinds that need no second one


def tie_world(vertices, jw_of, kind):
    """(vertices with the edit, {body: (lower, [higher, ...])}): in every body of ``jw_of`` = {body: jw} the rows of the kind
    take row jw's position, so they tie at every contour point; jw stays (and belongs to the tie) or goes behind the cameras."""
    rows_of, hide = TIES[kind]
    V = np.array(vertices, np.float32, copy=True)
    tied = {}
    for body, jw in jw_of.items():
        rows = rows_of(int(jw))
        assert jw not in rows and max(rows) < V.shape[1] and len(set(rows)) == len(rows), (kind, jw, rows)
        V[body, rows] = V[body, jw]
        if hide:
            V[body, jw] = BEHIND
        group = sorted(rows + ([] if hide else [int(jw)]))
        tied[body] = (group[0], group[1:])
    return V, tied


def single_valid(vertices, keep):
    """Every vertex but ``keep`` behind the cameras."""
    V = np.array(vertices, np.float32, copy=True)
    row = V[:, keep].copy()
    V[:] = BEHIND
    V[:, keep] = row
    return V


# ------------------------------------------------------------------------------------------------------------- occluders
OCC_NV, OCC_N, OCC_M = 701, 12, 48
OCC_H, OCC_W = wd.H, wd.W
OCC_BODY = (np.arange(OCC_M) % OCC_N).astype(np.int32)
OCC_SCENE = np.zeros(OCC_N, np.int32)
OCC_CLOSE_FROM = 43                                                      # images 43 .. 47: the close-up camera (view 3)
OCC_VIEW = np.array([(0, 1, 2, 4)[(i + i // OCC_N) % 4] if i < OCC_CLOSE_FROM else 3 for i in range(OCC_M)])
# three rows of four, 0.3 apart, so that they overlap in every view; body 2 stands 0.55 in front of the close-up camera
OCC_TRANSL = np.array([[0.3 * (k % 4) - 0.45, 0.0, 0.5 * (k // 4) - 0.5] for k in range(OCC_N)], np.float32)
OCC_TRANSL[2] = [-0.35, 0.0, -0.95]
OCC_MARGIN = 0.02
OCC_SHIFT = np.array([0.02, -0.015, 0.03], np.float32)


def occ_params():
    return params(OCC_N, seed0=7100, transl=OCC_TRANSL)


def occ_cameras():
    """(the five cameras of tests/silhouette_occlusion_world.py, the same per image)."""
    cams = wd.cameras(OCC_H, OCC_W)
    return cams, tuple(a[OCC_VIEW] for a in cams)


def instances(image_body, body_scene):
    """[(image, body, map)] in the order csrc/silhouette_occlusion.hip:sil_occ_set lists them: per image its own body
    (map 0), then its scene mates in ascending body index (map 1)."""
    scene = np.asarray(body_scene).reshape(-1)
    out = []
    for i, n in enumerate(np.asarray(image_body).reshape(-1)):
        out.append((i, int(n), 0))
        if scene[n] >= 0:
            out += [(i, int(m), 1) for m in np.flatnonzero(scene == scene[n]) if m != n]
    return out


def modal_masks(z_occ, z_own):
    """uint8 [M,H,W]: the pixels where the image's own body is drawn and no scene mate lies in front of it."""
    return (np.isfinite(z_own) & (z_own <= z_occ)).astype(np.uint8)
