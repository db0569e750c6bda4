"""GPU: mvfit_render_scene (csrc/render.hip) - identity with mvfit_render_overlay for one grey body per image, the scene
contract against its NumPy restatement (tests/render_scene_oracle.py: ids identical on every pixel, covered pixels within
1 per channel - the rule and bound of tests/test_gpu_render.py::_compare, background and dots bit-identical), the palette,
independence of the grouping, in-place, empty lists, error codes."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from mvsmplfitting_amd import io_formats as iof
from mvsmplfitting_amd.engine import MvFit, MvFitError
from tests import render_oracle as ro
from tests import render_scene_oracle as rso
from tests.helpers import GOLD
from tests.test_gpu_render import _background, _cam, _model, _params, _ring, _set

pytestmark = pytest.mark.gpu

GREY = (0.5, 0.5, 0.5)
# three bodies on the ring of _ring (view 0 looks from +z): body 0 stands between the camera of view 0 and body 1
TRANSL = np.array([[0.0, 0.0, 1.0], [0.15, 0.0, -0.8], [-1.1, 0.0, 0.0]], np.float32)


def three_body_params():
    x = _params(3, seed0=2100)
    x[:, 82:85] = TRANSL
    return x


def _identity(eng, verts, joints, imgs, prob, view):
    want, want_fid = eng.render_overlay(verts, joints, imgs, prob, view, face_id=True)
    out, fid, bid = eng.render_scene(verts, joints, imgs, [[b] for b in prob], view, colors=[[GREY]] * len(prob),
                                     face_id=True, body_id=True)
    assert (want_fid >= 0).sum() > 100
    assert torch.equal(out, want) and torch.equal(fid, want_fid)
    assert torch.equal(bid, torch.where(want_fid >= 0, 0, -1).to(torch.int32))


@pytest.mark.parametrize('kind', ['smpllsp', 'smpl'])
def test_identity_ring(kind):
    model = _model(kind)
    B, H, W = 3, 240, 320
    cams = _ring(W, H)
    with MvFit(model) as eng:
        _set(eng, cams, B)
        verts, joints = eng.vertices(_params(B))
        prob = [b for b in range(B) for v in range(8)]
        view = [v for b in range(B) for v in range(8)]
        _identity(eng, verts, joints, _background(len(prob), H, W), prob, view)


def test_identity_per_problem_cameras():
    model = _model('smpllsp')
    B, H, W = 2, 240, 320
    R, t, f, c = _ring(W, H, V=4, radius=3.0)
    rng = np.random.default_rng(9)
    Rb = np.stack([R, R]).astype(np.float32)
    tb = np.stack([t, t + rng.normal(0, 0.05, t.shape)]).astype(np.float32)
    fb = np.stack([f, f * 1.3]).astype(np.float32)
    cb = np.stack([c, c]).astype(np.float32)
    cb[1, 2] = (15.0, 200.0)
    with MvFit(model) as eng:
        _set(eng, (Rb, tb, fb, cb), B)
        verts, joints = eng.vertices(_params(B, seed0=77))
        prob, view = [0, 1, 1, 0, 1], [0, 2, 3, 3, 0]
        _identity(eng, verts, joints, _background(len(prob), H, W, seed=5), prob, view)


def test_identity_full_size_image():
    model = _model('smpllsp')
    ex, it = iof.load_camera_para(os.path.join(GOLD, 'demo_data', '3DOH50K_Parameters.txt'))
    cams = (ex[0, :3, :3].astype(np.float32)[None], ex[0, :3, 3].astype(np.float32)[None],
            it[0, 0, 0].astype(np.float32)[None], it[0, :2, 2].astype(np.float32)[None])
    R64, t64 = ex[0, :3, :3], ex[0, :3, 3]
    x = _params(1, seed0=5)
    x[0, 82:85] = -R64.T @ t64 + 4.0 * R64.T @ np.array([0.0, 0.0, 1.0])
    with MvFit(model) as eng:
        _set(eng, cams, 1)
        verts, joints = eng.vertices(x)
        _identity(eng, verts, joints, _background(1, 1536, 2048, seed=11), [0], [0])


def test_identity_close_up():
    model = _model('smpllsp')
    cams = (np.eye(3, dtype=np.float32)[None], np.array([[0.0, 0.0, 1.0]], np.float32), np.array([2000.0], np.float32),
            np.array([[160.0, 120.0]], np.float32))
    with MvFit(model) as eng:
        _set(eng, cams, 1)
        verts = torch.from_numpy(model['v_template'].astype(np.float32))[None].cuda()
        joints = torch.zeros(1, 17, 3, device='cuda')
        joints[0, :, 2] = -1.0
        imgs = _background(1, 240, 320, seed=17)
        _identity(eng, verts, joints, imgs, [0], [0])
        fid = eng.render_scene(verts, joints, imgs, [[0]], [0], face_id=True)[1].cpu().numpy()
        assert (np.bincount(fid[fid >= 0].ravel()) > 1024).sum() >= 10       # the workgroup-per-face path ran


def _compare_scene(model, verts, joints, cams, bodies, view, colors, imgs, out, fid, bid):
    """Every image of a call against the scene oracle; returns the oracle's (face_id, body_id) per image."""
    normals = {b: ro.vertex_normals(verts[b], model['faces']) for b in sorted({b for lst in bodies for b in lst})}
    ids = []
    k0 = 0
    for i, (lst, v) in enumerate(zip(bodies, view)):
        cam = _cam(cams, lst[0] if lst else 0, v)
        H, W = imgs.shape[1:3]
        col = None if colors is None else colors[k0:k0 + len(lst)]
        k0 += len(lst)
        want, want_fid, want_bid = rso.render_scene([verts[b] for b in lst], model['faces'], cam, H, W, image=imgs[i],
                                                    points=[joints[b] for b in lst], colors=col,
                                                    normals=[normals[b] for b in lst])
        ids.append((want_fid, want_bid))
        print('image %d: face_id differs on %d px, body_id on %d px' % (i, int((fid[i] != want_fid).sum()),
                                                                        int((bid[i] != want_bid).sum())))
        assert np.array_equal(fid[i], want_fid), (i, int((fid[i] != want_fid).sum()))
        assert np.array_equal(bid[i], want_bid), (i, int((bid[i] != want_bid).sum()))
        dots = np.zeros((H, W), bool)
        for b in lst:
            for cx, cy in ro.dot_centres(joints[b], cam, H, W):
                ys, xs = np.ogrid[0:H, 0:W]
                dots |= (xs - cx) ** 2 + (ys - cy) ** 2 <= 64
        exact = (want_fid < 0) | dots
        assert np.array_equal(out[i][exact], want[exact]), i
        d = np.abs(out[i].astype(np.int16) - want.astype(np.int16))
        print('image %d: max |byte difference| %d on %d covered px' % (i, int(d.max()), int((want_fid >= 0).sum())))
        assert d.max() <= 1, (i, int(d.max()), int((d > 1).sum()))
    return ids


def occlusion_guard(ids, verts, cams, view, H, W, front=0, hidden=1, occlusion_image=0):
    """On the oracle's own output: every body owns >= 1000 px in some view, and in the occlusion view the box of the hidden
    body's projected vertices holds >= 200 px owned by the front body."""
    for k in range(3):
        assert max(int((bid == k).sum()) for _, bid in ids) >= 1000, k
    cam = _cam(cams, 0, view[occlusion_image])
    p, u, w = ro.transform(verts[hidden], *cam)
    x0, x1 = max(0, int(np.floor(u.min()))), min(W - 1, int(np.ceil(u.max())))
    y0, y1 = max(0, int(np.floor(w.min()))), min(H - 1, int(np.ceil(w.max())))
    bid = ids[occlusion_image][1]
    assert int((bid[y0:y1 + 1, x0:x1 + 1] == front).sum()) >= 200


def test_three_bodies_match_the_oracle():
    model = _model('smpllsp')
    B, H, W = 3, 240, 320
    cams = _ring(W, H)
    with MvFit(model) as eng:
        _set(eng, cams, B)
        verts, joints = eng.vertices(three_body_params())
        view = [0, 1, 2, 3, 4, 6]
        bodies = [[0, 1, 2]] * len(view)
        rng = np.random.default_rng(4)
        colors = rng.uniform(0, 1, (3 * len(view), 3)).astype(np.float32)
        imgs = _background(len(view), H, W, seed=21)
        out, fid, bid = eng.render_scene(verts, joints, imgs, bodies, view, colors=colors, face_id=True, body_id=True)
        torch.cuda.synchronize()
        vh, jh = verts.cpu().numpy(), joints.cpu().numpy()
        ids = _compare_scene(model, vh, jh, cams, bodies, view, colors, imgs, out.cpu().numpy(), fid.cpu().numpy(),
                             bid.cpu().numpy())
        occlusion_guard(ids, vh, cams, view, H, W)


def test_palette_and_wrap():
    model = _model('smpl')
    B, H, W = 3, 240, 320
    cams = _ring(W, H)
    with MvFit(model) as eng:
        _set(eng, cams, B)
        verts, joints = eng.vertices(three_body_params())
        vh, jh = verts.cpu().numpy(), joints.cpu().numpy()
        # the palette against the oracle's seven triples: seven bodies in one image (problems repeat), then nine
        for lst in ([0, 1, 2, 0, 1, 2, 0], [2, 2, 2, 2, 2, 2, 2, 0, 1]):
            imgs = _background(1, H, W, seed=len(lst))
            out, fid, bid = eng.render_scene(verts, joints, imgs, [lst], [2], face_id=True, body_id=True)
            _compare_scene(model, vh, jh, cams, [lst], [2], None, imgs, out.cpu().numpy(), fid.cpu().numpy(),
                           bid.cpu().numpy())
            explicit = eng.render_scene(verts, joints, imgs, [lst], [2],
                                        colors=rso.PALETTE[np.arange(len(lst)) % 7])
            assert torch.equal(explicit, out)
        # nine bodies: slots 7 and 8 (palette entries 0 and 1 again) own pixels, so the wrap was compared above
        bid_h = bid.cpu().numpy()[0]
        assert (bid_h == 7).sum() > 100 and (bid_h == 8).sum() > 100
        # nested colours equal the flat array
        nested = eng.render_scene(verts, joints, imgs, [[0, 1]], [1], colors=[[(0.2, 0.4, 0.6), (1.0, 0.0, 0.3)]])
        flat = eng.render_scene(verts, joints, imgs, [[0, 1]], [1], colors=np.array([(0.2, 0.4, 0.6), (1.0, 0.0, 0.3)]))
        assert torch.equal(nested, flat)
        pal = eng.render_scene(verts, joints, imgs, [[0, 1]], [1])
        assert not torch.equal(pal, flat)


def test_grouping_in_place_dots_and_empty_lists():
    model = _model('smpl')
    B, H, W = 3, 120, 160
    cams = _ring(W, H)
    rng = np.random.default_rng(8)
    with MvFit(model) as eng:
        _set(eng, cams, B)
        verts, joints = eng.vertices(three_body_params())
        n = 70
        bodies = [list(rng.permutation(3)[:1 + i % 3]) for i in range(n)]
        view = [int(v) for v in rng.integers(0, 8, n)]
        imgs = torch.from_numpy(_background(n, H, W, seed=13)).cuda()
        a, fa, ba = eng.render_scene(verts, joints, imgs, bodies, view, face_id=True, body_id=True)
        for i in range(n):
            s, fs, bs = eng.render_scene(verts, joints, imgs[i:i + 1], [bodies[i]], [view[i]], face_id=True, body_id=True)
            assert torch.equal(s[0], a[i]) and torch.equal(fs[0], fa[i]) and torch.equal(bs[0], ba[i]), i
        # in place
        inplace = imgs.clone()
        r = eng.render_scene(verts, joints, inplace, bodies, view, out=inplace)
        assert r.data_ptr() == inplace.data_ptr() and torch.equal(inplace, a)
        host = imgs.cpu().numpy()
        with pytest.raises(MvFitError):
            eng.render_scene(verts, joints, host, bodies, view, out=host)
        # the dots of every body: each body's dot pixels that lie in the image are red
        jh = joints.cpu().numpy()
        ah = a.cpu().numpy()
        seen = 0
        for i in (1, 2, 5):
            for b in bodies[i]:
                for cx, cy in ro.dot_centres(jh[b], _cam(cams, 0, view[i]), H, W):
                    if 0 <= cx < W and 0 <= cy < H:
                        assert tuple(ah[i, cy, cx]) == (255, 0, 0), (i, b)
                        seen += 1
        assert seen >= 17
        no_dots = eng.render_scene(verts, None, imgs, bodies, view)
        assert not torch.equal(no_dots, a) and torch.equal(no_dots[fa < 0], imgs[fa < 0])
        # empty lists: the image comes back, ids -1; between two drawn images too
        e, fe, be = eng.render_scene(verts, joints, imgs[:3], [[0], [], [1, 2]], [0, 1, 2], face_id=True, body_id=True)
        assert torch.equal(e[1], imgs[1]) and bool((fe[1] == -1).all()) and bool((be[1] == -1).all())
        assert (be[2] == 1).any() and (be[0] == 0).any()
        e = eng.render_scene(verts, joints, imgs[:2], [[], []], [0, 1])
        assert torch.equal(e, imgs[:2])


def test_error_codes():
    model = _model('smpllsp')
    H, W = 24, 32
    verts = torch.zeros(1, 6890, 3, device='cuda')
    img = torch.zeros(2, H, W, 3, dtype=torch.uint8, device='cuda')
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)

    def call(eng, n=1, first=(0, 1), prob=(0,), view=(0,), color=None, h=H, w=W, num_points=0, null=None):
        fi, pr, vw = np.asarray(first, np.int32), np.asarray(prob, np.int32), np.asarray(view, np.int32)
        col = None if color is None else np.ascontiguousarray(color, np.float32)
        return eng._lib.mvfit_render_scene(
            eng._ctx, verts.data_ptr(), None, num_points, n, None if null == 'first' else fi.ctypes.data_as(ip),
            None if null == 'prob' else pr.ctypes.data_as(ip), None if null == 'view' else vw.ctypes.data_as(ip),
            None if col is None else col.ctypes.data_as(fp), h, w, img.data_ptr(), img.data_ptr(), None, None)
    nofaces = dict(model)
    nofaces['faces'] = None
    with MvFit(nofaces) as eng:
        _set(eng, _ring(W, H, V=2), 1)
        assert call(eng) == -3                          # MVFIT_E_STATE: no faces
    with MvFit(model) as eng:
        assert call(eng) == -3                          # MVFIT_E_STATE: no set_problems
        _set(eng, _ring(W, H, V=2), 1)
        assert call(eng) == 0
        assert call(eng, color=[(0.0, 1.0, 0.5)]) == 0
        assert call(eng, n=2, first=(0, 0, 1), view=(0, 1)) == 0       # an empty list is no error
        eng.sync()
        many = 257
        for kw in (dict(null='first'), dict(null='prob'), dict(null='view'),
                   dict(n=2, first=(0, 1, 0), view=(0, 0)), dict(first=(1, 1)), dict(first=(0, -1)),
                   dict(prob=(1,)), dict(prob=(-1,)), dict(view=(2,)), dict(view=(-1,)),
                   dict(color=[(0.0, 1.5, 0.0)]), dict(color=[(-0.1, 0.0, 0.0)]), dict(color=[(np.nan, 0.0, 0.0)]),
                   dict(color=[(np.inf, 0.0, 0.0)]),
                   dict(first=(0, many), prob=(0,) * many),
                   dict(h=0), dict(w=0), dict(h=8193), dict(w=8193), dict(num_points=-1), dict(num_points=65), dict(n=0)):
            assert call(eng, **kw) == -1, kw            # MVFIT_E_ARG
        assert call(eng, first=(0, 256), prob=(0,) * 256) == 0
        eng.sync()
        with pytest.raises(MvFitError):
            eng.render_scene(verts, None, img[:1], [[0]], [5])
        with pytest.raises(MvFitError):
            eng.render_scene(verts, None, img[:1], [[0]], [0], colors=[[(0.1, 0.2, 0.3)] * 2])
