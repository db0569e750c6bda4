"""GPU: mvfit_render_overlay (csrc/render.hip) against the NumPy restatement of its contract (tests/render_oracle.py):
the face-ID image identical on every pixel, covered pixels within 1 per channel, background and dot pixels bit-identical;
determinism, grouping and in-place invariance; the documented error codes."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from mvsmplfitting_amd import io_formats as iof
from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import MvFit, MvFitError, pack_params
from tests import render_oracle as ro
from tests.helpers import GOLD, body_model

pytestmark = pytest.mark.gpu


def _model(kind):
    return body_model() if kind == 'smpllsp' else syn.make_body_model(0, model_type='smpl')


def _ring(W=320, H=240, V=8, radius=4.0):
    R, t, f, c = syn.make_camera_ring(V, radius=radius)
    return R, t, f * np.float32(W / 2048.0), np.tile(np.array([W / 2.0, H / 2.0], np.float32), (V, 1))


def _params(B, seed0=1000):
    fr = syn.make_frames(B, seed0=seed0)
    return pack_params(B=B, **fr)


def _set(eng, cams, B):
    V = cams[0].shape[-3]
    eng.set_problems(cams, np.zeros((B, V, 17, 2), np.float32), np.zeros((B, V, 17), np.float32))


def _cam(cams, b, v):
    R, t, f, c = cams
    if R.ndim == 4:
        return R[b, v], t[b, v], f[b, v], c[b, v]
    return R[v], t[v], f[v], c[v]


def _background(n, H, W, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def _compare(model, verts, joints, cams, prob, view, imgs, out, fid):
    """Every image of a call against the oracle."""
    normals = {}
    for i, (b, v) in enumerate(zip(prob, view)):
        if b not in normals:
            normals[b] = ro.vertex_normals(verts[b], model['faces'])
        cam = _cam(cams, b, v)
        H, W = imgs.shape[1:3]
        want, want_fid = ro.render(verts[b], model['faces'], cam, H, W, image=imgs[i], points=joints[b], normals=normals[b])
        assert np.array_equal(fid[i], want_fid), (i, int((fid[i] != want_fid).sum()))
        assert (want_fid >= 0).sum() > 100, 'the body should be in view'
        dots = np.zeros((H, W), bool)
        for cx, cy in ro.dot_centres(joints[b], cam, H, W):
            ys, xs = np.ogrid[0:H, 0:W]
            dots |= (xs - cx) ** 2 + (ys - cy) ** 2 <= 64
        exact = (want_fid < 0) | dots
        assert np.array_equal(out[i][exact], want[exact]), i
        d = np.abs(out[i].astype(np.int16) - want.astype(np.int16))
        assert d.max() <= 1, (i, int(d.max()), int((d > 1).sum()))
        cov = (want_fid >= 0) & ~dots
        assert np.all(out[i][cov] == out[i][cov][:, :1])          # grey: one value on all channels


@pytest.mark.parametrize('kind', ['smpllsp', 'smpl'])
def test_ring_matches_oracle(kind):
    model = _model(kind)
    B, H, W = 3, 240, 320
    cams = _ring(W, H)
    with MvFit(model) as eng:
        _set(eng, cams, B)
        verts, joints = eng.vertices(_params(B))
        prob = [b for b in range(B) for v in range(8)]
        view = [v for b in range(B) for v in range(8)]
        imgs = _background(len(prob), H, W)
        out, fid = eng.render_overlay(verts, joints, imgs, prob, view, face_id=True)
        torch.cuda.synchronize()
        _compare(model, verts.cpu().numpy(), joints.cpu().numpy(), cams, prob, view, imgs, out.cpu().numpy(),
                 fid.cpu().numpy())


def test_per_problem_cameras_and_a_view_that_leaves_the_image():
    model = _model('smpllsp')
    B, H, W = 2, 240, 320
    R, t, f, c = _ring(W, H, V=4, radius=3.0)
    rng = np.random.default_rng(9)
    Rb = np.stack([R, R]).astype(np.float32)
    tb = np.stack([t, t + rng.normal(0, 0.05, t.shape)]).astype(np.float32)
    fb = np.stack([f, f * 1.3]).astype(np.float32)
    cb = np.stack([c, c]).astype(np.float32)
    cb[1, 2] = (15.0, 200.0)                      # problem 1, view 2: the body crosses the left and bottom borders
    cams = (Rb, tb, fb, cb)
    with MvFit(model) as eng:
        _set(eng, cams, B)
        verts, joints = eng.vertices(_params(B, seed0=77))
        prob, view = [0, 1, 1, 0, 1], [0, 2, 3, 3, 0]
        imgs = _background(len(prob), H, W, seed=5)
        out, fid = eng.render_overlay(verts, joints, imgs, prob, view, face_id=True)
        torch.cuda.synchronize()
        fid_h = fid.cpu().numpy()
        # the clipped view touches the left border, and the body continues past it
        assert (fid_h[1][:, 0] >= 0).any()
        _compare(model, verts.cpu().numpy(), joints.cpu().numpy(), cams, prob, view, imgs, out.cpu().numpy(), fid_h)


def test_full_size_image_with_the_demo_camera():
    model = _model('smpllsp')
    ex, it = iof.load_camera_para(os.path.join(GOLD, 'demo_data', '3DOH50K_Parameters.txt'))
    R = ex[0, :3, :3].astype(np.float32)[None]
    t = ex[0, :3, 3].astype(np.float32)[None]
    cams = (R, t, it[0, 0, 0].astype(np.float32)[None], it[0, :2, 2].astype(np.float32)[None])
    # the body 4 m in front of the camera, on its optical axis
    R64, t64 = ex[0, :3, :3], ex[0, :3, 3]
    centre = -R64.T @ t64 + 4.0 * R64.T @ np.array([0.0, 0.0, 1.0])
    x = _params(1, seed0=5)
    x[0, 82:85] = centre
    with MvFit(model) as eng:
        _set(eng, cams, 1)
        verts, joints = eng.vertices(x)
        imgs = _background(1, 1536, 2048, seed=11)
        out, fid = eng.render_overlay(verts, joints, imgs, [0], [0], face_id=True)
        torch.cuda.synchronize()
        _compare(model, verts.cpu().numpy(), joints.cpu().numpy(), cams, [0], [0], imgs, out.cpu().numpy(), fid.cpu().numpy())


def test_close_up_faces_larger_than_a_thread_walks():
    """A close-up in which dozens of faces cover more than 1024 pixels each: those go through the workgroup-per-face
    raster path and must give the same keys as the oracle."""
    model = _model('smpllsp')
    cams = (np.eye(3, dtype=np.float32)[None], np.array([[0.0, 0.0, 1.0]], np.float32), np.array([2000.0], np.float32),
            np.array([[160.0, 120.0]], np.float32))
    with MvFit(model) as eng:
        _set(eng, cams, 1)
        verts = torch.from_numpy(model['v_template'].astype(np.float32))[None].cuda()
        joints = torch.zeros(1, 17, 3, device='cuda')
        joints[0, :, 2] = -1.0                           # behind the camera: no dots
        imgs = _background(1, 240, 320, seed=17)
        out, fid = eng.render_overlay(verts, joints, imgs, [0], [0], face_id=True)
        fid_h = fid.cpu().numpy()
        assert (np.bincount(fid_h[fid_h >= 0].ravel()) > 1024).sum() >= 10
        _compare(model, verts.cpu().numpy(), joints.cpu().numpy(), cams, [0], [0], imgs, out.cpu().numpy(), fid_h)


def test_deterministic_grouping_and_in_place():
    model = _model('smpl')
    B, H, W = 2, 240, 320
    cams = _ring(W, H)
    with MvFit(model) as eng:
        _set(eng, cams, B)
        verts, joints = eng.vertices(_params(B, seed0=31))
        prob = [0, 1, 0, 1, 1, 0]
        view = [0, 1, 2, 5, 7, 7]
        imgs = torch.from_numpy(_background(len(prob), H, W, seed=13)).cuda()
        a, fa = eng.render_overlay(verts, joints, imgs, prob, view, face_id=True)
        b, fb = eng.render_overlay(verts, joints, imgs, prob, view, face_id=True)
        assert torch.equal(a, b) and torch.equal(fa, fb)
        for i in range(len(prob)):
            s, fs = eng.render_overlay(verts, joints, imgs[i:i + 1], [prob[i]], [view[i]], face_id=True)
            assert torch.equal(s[0], a[i]) and torch.equal(fs[0], fa[i]), i
        no_dots = eng.render_overlay(verts, None, imgs, prob, view)
        assert not torch.equal(no_dots, a)
        assert torch.equal(no_dots[fa < 0], imgs[fa < 0])
        inplace = imgs.clone()
        r = eng.render_overlay(verts, joints, inplace, prob, view, out=inplace)
        assert r.data_ptr() == inplace.data_ptr() and torch.equal(inplace, a)
        assert not torch.equal(inplace, imgs)
        host = imgs.cpu().numpy()                        # in place needs a device tensor: a host array is refused
        with pytest.raises(MvFitError):
            eng.render_overlay(verts, joints, host, prob, view, out=host)


def test_error_codes():
    model = _model('smpllsp')
    H, W = 24, 32
    verts = torch.zeros(1, 6890, 3, device='cuda')
    img = torch.zeros(1, H, W, 3, dtype=torch.uint8, device='cuda')
    ip = C.POINTER(C.c_int32)

    def call(eng, n=1, prob=(0,), view=(0,), h=H, w=W, num_points=0, points=None):
        pr, vw = np.asarray(prob, np.int32), np.asarray(view, np.int32)
        return eng._lib.mvfit_render_overlay(eng._ctx, verts.data_ptr(), points, num_points, n, pr.ctypes.data_as(ip),
                                             vw.ctypes.data_as(ip), h, w, img.data_ptr(), img.data_ptr(), None)
    nofaces = dict(model)
    nofaces['faces'] = None
    with MvFit(nofaces) as eng:
        cams = _ring(W, H, V=2)
        _set(eng, cams, 1)
        assert call(eng) == -3                          # MVFIT_E_STATE: no faces
    with MvFit(model) as eng:
        assert call(eng) == -3                          # MVFIT_E_STATE: no set_problems
        cams = _ring(W, H, V=2)
        _set(eng, cams, 1)
        assert call(eng) == 0
        eng.sync()
        for kw in (dict(prob=(1,)), dict(prob=(-1,)), dict(view=(2,)), dict(view=(-1,)), dict(h=0), dict(w=0),
                   dict(h=8193), dict(w=8193), dict(num_points=-1), dict(num_points=65), dict(n=0)):
            assert call(eng, **kw) == -1, kw            # MVFIT_E_ARG
        with pytest.raises(MvFitError):
            eng.render_overlay(verts, None, img, [0], [5])
