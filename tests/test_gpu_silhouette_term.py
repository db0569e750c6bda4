"""GPU: the silhouette loss as a term of the fit (mvfit_set_silhouette_term; silhouette.hip: the gated evaluation ->
vertex_backward.hip: vjp_tile_gated_kernel -> vjp_record_kernel) in closure() and in fit()'s chained rounds.

Full body model, a 4-view ring at radius 4 with the cameras scaled as in tests/test_gpu_silhouette_refine.py, to 384 x 512:
at 192 x 256 no image keeps more than 512 contour points, and a search-chunk boundary has to lie inside an image (here
494 .. 600 points per image).
B = 34 problems, so the pull-back has a second, ragged 32-problem chunk; images exist for body 0 (2 views), 31 (1), 32 (4) and
33 (1), masks rendered at "truth" parameters, evaluation points = the truth with betas zeroed, scale 1 and the translation a
few cm off.  References: MvFit.silhouette_loss (checked against the NumPy oracle in tests/test_gpu_silhouette.py) and
MvFit.vertices_backward (tests/test_gpu_vertices_backward.py).  Bounds: the project's own (tests/scene_sdf_cases.py) -
LOSS_RTOL = 1e-5, GRAD_TOL = 2e-4 of max; chained rounds against the closure 1e-6 (tests/test_gpu_trajectory.py);
independence, the no-image rows and the graph's mask set bit for bit."""
import numpy as np
import pytest
import torch

from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import MvFitError, pack_params, stage_weights
from mvsmplfitting_amd.silhouette import refine_fit
from tests.gpu_helpers import make_engine
from tests.helpers import body_model
from tests.scene_sdf_cases import GRAD_TOL, LOSS_RTOL

pytestmark = pytest.mark.gpu

V, B = 4, 34
BETAS = np.array([3.0, -2.0, 1.5, -1.0, 2.5, 0.5, -3.0, 1.0, -0.5, 2.0], np.float32)
SCALE = 1.08
IMAGES = [(0, 0), (0, 1), (31, 2), (32, 0), (32, 1), (32, 2), (32, 3), (33, 3)]      # (body, view)
WITH_IMAGES = (0, 31, 32, 33)
SHIFT = np.array([0.03, -0.02, 0.04], np.float32)


def _np(t):
    return t.detach().cpu().numpy()


def _stage(w):
    return dict(stage_weights(1536.0)[3], coll_loss_weight=float(w))


def _cams(k):
    R, t, f, c = syn.make_camera_ring(V, radius=4.0)
    Wd, Hd = 256 * k, 192 * k
    f = (f * np.float32(Wd / 2048.0)).astype(np.float32)
    c = np.tile(np.array([Wd / 2.0, Hd / 2.0], np.float32), (V, 1))
    return (R, t, f, c), Hd, Wd


def _render(eng, x, images, H, W):
    """Masks [M,H,W] bool of the (problem, view) pairs at x, with the cameras of set_problems."""
    v, _ = eng.vertices(x)
    prob, view = np.array([i[0] for i in images], np.int32), np.array([i[1] for i in images], np.int32)
    _, fid = eng.render_overlay(v, None, np.zeros((len(images), H, W, 3), np.uint8), prob, view, face_id=True)
    return fid >= 0


def _per_image(cams, images):
    view = np.array([i[1] for i in images])
    return tuple(a[view] for a in cams)


def _truth(n, seed0):
    fr = syn.make_frames(n, seed0=seed0, betas=BETAS)
    fr['scale'][:] = SCALE
    return pack_params(B=n, **fr)


def _start(x_true):
    x = x_true.copy()
    x[:, 0:10] = 0.0
    x[:, 85] = 1.0
    x[:, 82:85] += SHIFT
    return x


def _observe(eng, cams, x_true):
    """Keypoint observations of the truth; leaves the problems set."""
    n = x_true.shape[0]
    eng.set_problems(cams, np.zeros((n, V, 17, 2), np.float32), np.zeros((n, V, 17), np.float32))
    _, joints = eng.vertices(x_true)
    gt, conf = syn.make_observations(_np(joints), cams, seed=3)
    eng.set_problems(cams, gt, conf)
    return gt, conf


def _evaluate(eng, x, w):
    """closure with the term at weight w (and its sums), closure without it."""
    o1 = eng.closure(x, _stage(w), want_grad=True)
    smp, S = eng.sdf_term_read()
    assert smp is None
    o0 = eng.closure(x, _stage(0.0), want_grad=True)
    return dict(loss=_np(o1['loss']), grad=_np(o1['grad']), S=_np(S), loss0=_np(o0['loss']), grad0=_np(o0['grad']))


@pytest.fixture(scope='module')
def world():
    model = body_model()
    eng = make_engine(model)
    cams, H, W = _cams(2)
    x_true = _truth(B, 5300)
    gt, conf = _observe(eng, cams, x_true)
    masks = _render(eng, x_true, IMAGES, H, W).to(torch.uint8)
    body = np.array([i[0] for i in IMAGES], np.int32)
    eng.set_silhouettes(masks, body, _per_image(cams, IMAGES))
    first = _np(eng.silhouettes()[1])
    print('images %d x %d, kept contour points per image %s' % (H, W, np.diff(first)))
    assert np.diff(first).max() > 512, 'no search-chunk boundary inside an image'
    x = _start(x_true)
    verts, _ = eng.vertices(x)
    yield dict(eng=eng, model=model, cams=cams, H=H, W=W, x_true=x_true, x=x, gt=gt, conf=conf, masks=masks, body=body,
               verts=verts)
    eng.close()


def _reference(eng, x, verts, sigma):
    """(L_ref [B], the pulled-back gradient of L [B,118]) from the op and vertices_backward, float64."""
    L, g = eng.silhouette_loss(verts, sigma=sigma)
    return _np(L).astype(np.float64), _np(eng.vertices_backward(x, grad_verts=g)).astype(np.float64)


def _weight(eng, x, L_ref, row):
    """w with w^2 = data term / L_ref of the row: neither term drowns the other."""
    data = float(eng.closure(x, _stage(0.0), want_grad=False)['loss'][row])
    return float(np.sqrt(data / L_ref[row]))


def test_the_fixture_exercises_both_partial_terms(world):
    eng = world['eng']
    A = _np(eng.silhouette_loss(world['verts'], w_out=0.0, need_grad=False)[0])
    Bt = _np(eng.silhouette_loss(world['verts'], w_in=0.0, need_grad=False)[0])
    print('term A %s, term B %s' % (A[list(WITH_IMAGES)], Bt[list(WITH_IMAGES)]))
    for j in WITH_IMAGES:
        assert A[j] > 0 and Bt[j] > 0, j
    rest = [j for j in range(B) if j not in WITH_IMAGES]
    assert not A[rest].any() and not Bt[rest].any()


@pytest.mark.parametrize('sigma', [0.0, 20.0])
def test_closure_adds_w2_L_and_its_pulled_back_gradient(world, sigma):
    eng, x = world['eng'], world['x']
    L_ref, g_ref = _reference(eng, x, world['verts'], sigma)
    w = _weight(eng, x, L_ref, 32)
    eng.set_silhouette_term(sigma=sigma)
    try:
        r = _evaluate(eng, x, w)
    finally:
        eng.clear_silhouette_term()
    for j in WITH_IMAGES:
        pen, pen_ref = float(r['loss'][j]) - float(r['loss0'][j]), w * w * L_ref[j]
        gp = r['grad'][j].astype(np.float64) - r['grad0'][j].astype(np.float64)
        gp_ref = w * w * g_ref[j]
        e_s = abs(float(r['S'][j]) - L_ref[j]) / L_ref[j]
        e_g = np.abs(gp - gp_ref).max() / np.abs(gp_ref).max()
        print('sigma %g problem %d: L %.7g ref %.7g rel %.2e | pen %.7g ref %.7g (loss %.7g) | grad err/max %.2e (max %.4g)'
              % (sigma, j, r['S'][j], L_ref[j], e_s, pen, pen_ref, r['loss'][j], e_g, np.abs(gp_ref).max()))
        assert L_ref[j] > 0
        assert e_s <= 1e-5
        assert abs(pen - pen_ref) <= LOSS_RTOL * float(r['loss'][j])
        assert e_g <= GRAD_TOL


def test_a_problem_without_images_pays_exactly_nothing(world):
    eng, x = world['eng'], world['x']
    L_ref, _ = _reference(eng, x, world['verts'], 0.0)
    eng.set_silhouette_term()
    try:
        r = _evaluate(eng, x, _weight(eng, x, L_ref, 32))
    finally:
        eng.clear_silhouette_term()
    rest = [j for j in range(B) if j not in WITH_IMAGES]
    assert len(rest) == 30
    assert not r['S'][rest].any()
    assert np.array_equal(r['loss'][rest], r['loss0'][rest]) and np.array_equal(r['grad'][rest], r['grad0'][rest])
    assert not np.array_equal(r['loss'][32], r['loss0'][32])


def test_a_problems_numbers_do_not_depend_on_the_batch(world):
    eng, x, cams = world['eng'], world['x'], world['cams']
    L_ref, _ = _reference(eng, x, world['verts'], 0.0)
    w = _weight(eng, x, L_ref, 32)
    eng.set_silhouette_term()
    try:
        r = _evaluate(eng, x, w)
    finally:
        eng.clear_silhouette_term()
    own = [i for i, (b, _) in enumerate(IMAGES) if b == 32]
    one = make_engine(world['model'])
    try:
        one.set_problems(cams, world['gt'][32:33], world['conf'][32:33])
        one.set_silhouettes(world['masks'][own], np.zeros(len(own), np.int32), _per_image(cams, [IMAGES[i] for i in own]))
        one.set_silhouette_term()
        a = _evaluate(one, x[32:33], w)
    finally:
        one.close()
    for k in ('loss', 'grad', 'S'):
        assert np.array_equal(a[k][0], r[k][32]), k


# ---- the fit: B = 3, bodies with 4 / 1 / 0 images
ROWS3 = (32, 31, 5)
IMAGES3 = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 2)]
FIT_KW = dict(max_iter=6, maxiters=2)


def _three(world, images=IMAGES3):
    """A fresh engine with the three problems, their masks (rendered at the truth) set, and the start point."""
    cams = world['cams']
    eng = make_engine(world['model'])
    rows = list(ROWS3)
    eng.set_problems(cams, world['gt'][rows], world['conf'][rows])
    masks = _render(eng, world['x_true'][rows], images, world['H'], world['W']).to(torch.uint8)
    eng.set_silhouettes(masks, np.array([i[0] for i in images], np.int32), _per_image(cams, images))
    return eng, world['x'][rows].copy()


def _w3(eng, x):
    v, _ = eng.vertices(x)
    L = _np(eng.silhouette_loss(v, need_grad=False)[0]).astype(np.float64)
    return _weight(eng, x, L, 0)


def test_chained_rounds_evaluate_the_closures_function(world):
    eng, x = _three(world)
    try:
        w = _w3(eng, x)
        eng.set_silhouette_term()
        tr = eng.fit_trace(12)
        xf, st = eng.fit(x, [_stage(w)], **FIT_KW)
        tr = _np(tr).astype(np.float64)
        eng.fit_trace(0)
        ncl = _np(st['n_closure'])
        checked = 0
        for k in range(12):
            rows = [b for b in range(3) if k < ncl[b] and np.isfinite(tr[b, k]).all()]
            if not rows:
                continue
            xk = x.copy()
            xk[rows] = tr[rows, k, :118].astype(np.float32)
            L = _np(eng.closure(xk, _stage(w), want_grad=False)['loss']).astype(np.float64)
            for b in rows:
                print('closure %d problem %d: round %.9g closure %.9g' % (k, b, tr[b, k, 118], L[b]))
                assert abs(L[b] - tr[b, k, 118]) <= 1e-6 * abs(L[b]), (k, b)
                checked += 1
        assert checked >= 9
        # two stages, the first without the term: a single-launch lead phase, then chained rounds
        xf2, st2 = eng.fit(x, [_stage(0.0), _stage(w)], **FIT_KW)
        print('two-stage fit: passes %s, closures %s' % (st2['passes'], _np(st2['n_closure'])))
        assert st2['passes']['missed'] == 0 and st2['passes']['timed_out'] == 0
        assert torch.isfinite(xf2).all() and torch.isfinite(st2['final_loss']).all()
        # the problem without images against the same two stages with the term cleared.  A cleared term refuses a weight > 0
        # (MVFIT_E_STATE), so the second stage's is 0 there; and only round_mode = 1 runs both fits through the same kernels
        # (a fit without a term otherwise never enters the chained rounds, whose direction differs in form from the
        # single-launch kernel's)
        eng.set_options(round_mode=1)
        xa, sta = eng.fit(x, [_stage(0.0), _stage(w)], **FIT_KW)
        eng.clear_silhouette_term()
        xb, stb = eng.fit(x, [_stage(0.0), _stage(0.0)], **FIT_KW)
        assert torch.equal(xa[2], xb[2]) and torch.equal(sta['final_loss'][2], stb['final_loss'][2])
        assert torch.equal(sta['n_closure'][2], stb['n_closure'][2])
        assert not torch.equal(xa[0], xb[0])
    finally:
        eng.close()


def test_the_round_graph_follows_the_mask_set(world):
    other = [(0, 3), (0, 2), (0, 1), (1, 0), (1, 1)]          # same sizes, another contour
    eng, x = _three(world)
    try:
        w = _w3(eng, x)
        eng.set_silhouette_term()
        first, _ = eng.fit(x, [_stage(w)], **FIT_KW)
        cams, rows = world['cams'], list(ROWS3)
        masks = _render(eng, world['x_true'][rows], other, world['H'], world['W']).to(torch.uint8)
        eng.set_silhouettes(masks, np.array([i[0] for i in other], np.int32), _per_image(cams, other))
        second, st = eng.fit(x, [_stage(w)], **FIT_KW)
    finally:
        eng.close()
    fresh, xs = _three(world, other)
    try:
        fresh.set_silhouette_term()
        ref, st_ref = fresh.fit(xs, [_stage(w)], **FIT_KW)
    finally:
        fresh.close()
    assert torch.equal(second.cpu(), ref.cpu()) and torch.equal(st['final_loss'].cpu(), st_ref['final_loss'].cpu())
    assert not torch.equal(second[:2].cpu(), first[:2].cpu())


def test_refine_fit_moves_towards_the_masks(world):
    """The refine test's scene: one person, 3 frames x 4 views, keypoints from the truth, start betas 0 / scale 1."""
    F = 3
    cams, H, W = world['cams'], world['H'], world['W']
    images = [(b, v) for b in range(F) for v in range(V)]
    x_true = _truth(F, 5200)
    eng = make_engine(world['model'])
    try:
        _observe(eng, cams, x_true)
        masks = _render(eng, x_true, images, H, W)
        x0 = x_true.copy()
        x0[:, 0:10] = 0.0
        x0[:, 85] = 1.0
        eng.set_silhouettes(masks.to(torch.uint8), np.array([i[0] for i in images], np.int32), _per_image(cams, images))

        def iou(x):
            m = _render(eng, x, images, H, W)
            return _np((m & masks).sum(dim=(1, 2)).double() / (m | masks).sum(dim=(1, 2)).double())

        def sil(x):
            return _np(eng.silhouette_loss(eng.vertices(x)[0], need_grad=False)[0]).astype(np.float64)

        L0 = sil(x0)
        w = _weight(eng, x0, L0, 0)
        iou0 = iou(x0)
        out, rep = refine_fit(eng, x0, _stage(w))
        iou1, L1 = iou(out), sil(out)
        plain, _ = eng.fit(x0, [_stage(0.0)])
        print('w %.5g; objective %s -> %s; silhouette loss %s -> %s (the same fit with w = 0 ends at %s)'
              % (w, rep['before'], rep['after'], L0, L1, sil(plain)))
        print('IoU per image before %s' % np.round(iou0, 4))
        print('IoU per image after  %s' % np.round(iou1, 4))
        print('closures %s, scale %s (truth %.2f)' % (rep['n_closure'], _np(out[:, 85]), SCALE))
        assert rep['accepted'].all()
        assert (rep['after'] < rep['before']).all()
        assert (L1 < L0).all() and (rep['silhouette_after'] < rep['silhouette_before']).all()
        assert iou1.mean() > iou0.mean()
        with pytest.raises(MvFitError, match='error -3'):           # the term is left cleared
            eng.closure(x0, _stage(w))
    finally:
        eng.close()


def test_contract(world):
    eng, x, cams = world['eng'], world['x'], world['cams']
    faces = world['model']['faces']
    per_image = _per_image(cams, IMAGES)
    try:
        with pytest.raises(MvFitError, match='error -3'):                  # no term: a weight > 0 is refused
            eng.closure(x, _stage(1.0))
        for bad in (dict(w_in=-1.0), dict(w_out=-1.0), dict(w_in=float('nan')), dict(w_out=float('inf')), dict(sigma=float('nan')),
                    dict(sigma=float('inf'))):
            with pytest.raises(MvFitError, match='error -1: mvfit_set_silhouette_term'):
                eng.set_silhouette_term(**bad)
        eng.set_silhouette_term(sigma=-1.0)                                 # (sigma <= 0: the plain squares)
        eng.closure(x, _stage(1.0))
        with pytest.raises(MvFitError, match='error -4'):                   # samples: not kept by this term
            eng._check(eng._lib.mvfit_sdf_term_read(eng._ctx, torch.empty(B, eng.nv, 4, device=eng.device).data_ptr(), None))
        # one term slot
        with pytest.raises(MvFitError, match='error -3: mvfit_set_sdf'):
            eng.set_sdf(faces, num_faces=1, grid_size=32)
        with pytest.raises(MvFitError, match='error -3: mvfit_set_scene_obstacles'):
            eng.set_scene_obstacles(world['verts'], [B], grid_size=8)
        eng.clear_silhouette_term()
        eng.set_sdf(faces, num_faces=1, grid_size=32)
        with pytest.raises(MvFitError, match='error -3: mvfit_set_silhouette_term'):
            eng.set_silhouette_term()
        eng.set_sdf(None)
        eng.set_scene_obstacles(world['verts'], [B], grid_size=8)
        with pytest.raises(MvFitError, match='error -3: mvfit_set_silhouette_term'):
            eng.set_silhouette_term()
        eng.clear_scene_obstacles()
        # clearing the masks switches the term off; no masks, no term
        eng.set_silhouette_term()
        eng.clear_silhouettes()
        with pytest.raises(MvFitError, match='error -3'):
            eng.closure(x, _stage(1.0))
        with pytest.raises(MvFitError, match='error -3: mvfit_set_silhouette_term'):
            eng.set_silhouette_term()
        # image_body must stay below B: at the enable, and for a set that replaces the one of an enabled term
        beyond = world['body'].copy()
        beyond[-1] = B
        eng.set_silhouettes(world['masks'], beyond, per_image)
        with pytest.raises(MvFitError, match='error -1: mvfit_set_silhouette_term'):
            eng.set_silhouette_term()
        eng.set_silhouettes(world['masks'], world['body'], per_image)
        eng.set_silhouette_term()
        with pytest.raises(MvFitError, match='error -1: mvfit_set_silhouettes'):
            eng.set_silhouettes(world['masks'], beyond, per_image)
        with pytest.raises(MvFitError, match='error -3'):                  # ... which switched the term off
            eng.closure(x, _stage(1.0))
        # another B switches the term off
        eng.set_silhouettes(world['masks'][:2], world['body'][:2], _per_image(cams, IMAGES[:2]))
        eng.set_silhouette_term()
        eng.closure(x, _stage(1.0))
        eng.set_problems(cams, world['gt'][:2], world['conf'][:2])
        with pytest.raises(MvFitError, match='error -3'):
            eng.closure(x[:2], _stage(1.0))
        with pytest.raises(MvFitError, match='error -3'):
            eng.fit(x[:2], [_stage(1.0)])
        # without problems
        bare = make_engine(world['model'])
        try:
            with pytest.raises(MvFitError, match='error -3'):
                bare.set_silhouette_term()
        finally:
            bare.close()
    finally:
        eng.set_sdf(None)
        eng.clear_scene_obstacles()
        eng.set_problems(cams, world['gt'], world['conf'])
        eng.set_silhouettes(world['masks'], world['body'], per_image)
        eng.clear_silhouette_term()
