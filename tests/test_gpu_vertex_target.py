"""GPU: the vertex-target term (mvfit_set_vertex_targets / mvfit_vertex_target_loss / mvfit_set_vertex_target_term;
vertex_target.hip -> vertex_backward.hip's gated pull-back and record kernel) as an op, in closure() and in fit()'s chained
rounds.

Full body model, 4-view ring, B = 34 problems: the pull-back has a second, ragged 32-problem chunk, and a problem's 3 Nv =
20,670 floats are 11 workgroups of the target kernel, the last one ragged, no multiple of any vector width but 2.  Targets
are the vertices of perturbed parameters; K = 2, and K = 4 with the same two sets in rows 0 and 2 and NaN-filled rows of
weight 0 in 1 and 3.  Problems 1 and 33 have all weights zero, 0 and 32 one zero weight (a sequence's ends).
References: the NumPy oracle (tests/vertex_target_oracle.py) and MvFit.vertices_backward.  Bounds: the gradient bit for bit;
the loss within one float32 ulp of the oracle's float64 value (the float64 accumulation error is orders below it, only the
final rounding can differ); the closure within the project's own LOSS_RTOL / GRAD_TOL (tests/scene_sdf_cases.py); chained
rounds against the closure 1e-6 (tests/test_gpu_silhouette_term.py); independence, zero-weight rows and the graph bit for
bit."""
import numpy as np
import pytest
import torch

from mvsmplfitting_amd import _lib
from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import MvFitError, pack_params, stage_weights
from tests.gpu_helpers import make_engine
from tests.helpers import body_model
from tests.scene_sdf_cases import GRAD_TOL, LOSS_RTOL
from tests.vertex_target_oracle import vertex_target_loss

pytestmark = pytest.mark.gpu

V, B = 4, 34
ZERO = (1, 33)
ROWS3 = (32, 31, 1)                     # the fit's three problems: two weights, two weights, none
FIT_KW = dict(max_iter=6, maxiters=2)


def _np(t):
    return t.detach().cpu().numpy()


def _stage(w, flags=0):
    return dict(stage_weights(1536.0, flags=flags)[3], coll_loss_weight=float(w))


def _perturbed(x, seed):
    rng = np.random.default_rng(seed)
    y = x.copy()
    y[:, 10:82] += rng.normal(0, 0.05, (x.shape[0], 72)).astype(np.float32)
    y[:, 82:85] += rng.normal(0, 0.02, (x.shape[0], 3)).astype(np.float32)
    return y


def _k4(T2, a2):
    """The K = 2 set as a K = 4 one: rows 1 and 3 NaN-filled with weight 0."""
    n = T2.shape[0]
    T4 = torch.full((n, 4) + tuple(T2.shape[2:]), float('nan'), device=T2.device)
    T4[:, 0], T4[:, 2] = T2[:, 0], T2[:, 1]
    a4 = np.zeros((n, 4), np.float32)
    a4[:, 0], a4[:, 2] = a2[:, 0], a2[:, 1]
    return T4, a4


@pytest.fixture(scope='module')
def world():
    model = body_model()
    vpw = syn.make_vposer_decoder()
    eng = make_engine(model, vpw=vpw)
    cams = syn.make_camera_ring(V)
    x_true = pack_params(B=B, **syn.make_frames(B, seed0=6100))
    eng.set_problems(cams, np.zeros((B, V, 17, 2), np.float32), np.zeros((B, V, 17), np.float32))
    _, joints = eng.vertices(x_true)
    gt, conf = syn.make_observations(_np(joints), cams, seed=3)
    eng.set_problems(cams, gt, conf)
    x = _perturbed(x_true, 1)
    x[:, 86:118] = np.random.default_rng(2).normal(0, 0.3, (B, 32)).astype(np.float32)      # (the embedding, read with F_VPOSER only)
    verts, _ = eng.vertices(x)
    T2 = torch.stack([eng.vertices(_perturbed(x, 10))[0], eng.vertices(_perturbed(x, 11))[0]], dim=1)
    a2 = np.random.default_rng(4).uniform(0.5, 1.5, (B, 2)).astype(np.float32)
    a2[list(ZERO)] = 0.0
    a2[0, 0] = 0.0
    a2[32, 1] = 0.0
    T4, a4 = _k4(T2, a2)
    ref2 = vertex_target_loss(_np(verts), _np(T2), a2)
    ref4 = vertex_target_loss(_np(verts), _np(T4), a4)
    yield dict(eng=eng, model=model, vpw=vpw, cams=cams, x=x, gt=gt, conf=conf, verts=verts,
               sets={2: (T2, a2, ref2), 4: (T4, a4, ref4)})
    eng.close()


# ------------------------------------------------------------------------------------------------ 1. the op
@pytest.mark.parametrize('K', [2, 4])
def test_the_op_against_the_oracle(world, K):
    eng, verts = world['eng'], world['verts']
    T, a, (L_ref, g_ref) = world['sets'][K]
    eng.set_vertex_targets(T, a)
    try:
        L, g = eng.vertex_target_loss(verts)
        L_only, none = eng.vertex_target_loss(verts, need_grad=False)
    finally:
        eng.clear_vertex_targets()
    L, g = _np(L), _np(g)
    assert none is None and np.array_equal(_np(L_only), L)
    assert np.isfinite(L).all() and np.isfinite(g).all()
    assert np.array_equal(g.view(np.uint32), g_ref.view(np.uint32))                  # bit for bit
    ulp = np.spacing(np.abs(L_ref).astype(np.float32)).astype(np.float64)
    err = np.abs(L.astype(np.float64) - L_ref)
    print('K %d: L %.7g .. %.7g, worst error %.3g ulp' % (K, L_ref[L_ref > 0].min(), L_ref.max(), (err / ulp).max()))
    assert (L_ref[[j for j in range(B) if j not in ZERO]] > 0).all()
    assert (err <= ulp).all()
    for j in ZERO:
        assert L[j] == 0.0 and not g[j].any()
    # the two sets state the same term: the rows of weight 0 change no bit
    T2, a2, (L2, g2) = world['sets'][2]
    assert np.array_equal(g_ref, g2) and np.array_equal(L_ref, L2)


# ------------------------------------------------------------------------------------------------ 2. independence
def test_a_problems_numbers_do_not_depend_on_the_batch_the_run_or_the_alignment(world):
    eng, verts, cams = world['eng'], world['verts'], world['cams']
    T, a, _ = world['sets'][2]
    eng.set_vertex_targets(T, a)
    try:
        L, g = eng.vertex_target_loss(verts)
        L_again, g_again = eng.vertex_target_loss(verts)
        # vertices and gradient at addresses that are no multiple of 8: the kernel's two-loads-per-pair form
        n = verts.numel()
        flat = torch.empty(n + 1, device=verts.device)
        flat[1:] = verts.reshape(-1)
        off = flat[1:].view(B, eng.nv, 3)
        assert off.data_ptr() % 8 == 4 and off.is_contiguous()
        L_off = torch.empty(B, device=verts.device)
        g_flat = torch.empty(n + 1, device=verts.device)
        g_off = g_flat[1:].view(B, eng.nv, 3)
        eng._check(eng._lib.mvfit_vertex_target_loss(eng._ctx, off.data_ptr(), L_off.data_ptr(), g_off.data_ptr()))
    finally:
        eng.clear_vertex_targets()
    assert torch.equal(L, L_again) and torch.equal(g, g_again)
    assert torch.equal(L, L_off) and torch.equal(g, g_off)
    one = make_engine(world['model'])
    try:
        one.set_problems(cams, world['gt'][32:33], world['conf'][32:33])
        one.set_vertex_targets(T[32:33], a[32:33])
        L1, g1 = one.vertex_target_loss(verts[32:33])
    finally:
        one.close()
    assert torch.equal(L1[0].cpu(), L[32].cpu()) and torch.equal(g1[0].cpu(), g[32].cpu())


# ------------------------------------------------------------------------------------------------ 3. the closure
def _weight(eng, x, L_ref, row, flags=0):
    """w with w^2 = data term / L_ref of the row: neither term drowns the other."""
    data = float(eng.closure(x, _stage(0.0, flags), want_grad=False)['loss'][row])
    return float(np.sqrt(data / L_ref[row]))


def _evaluate(eng, x, w, flags=0):
    """closure with the term at weight w (its sums, its vertices), closure without it."""
    o1 = eng.closure(x, _stage(w, flags), want_grad=True, want_verts=True)
    smp, S = eng.sdf_term_read()
    assert smp is None
    o0 = eng.closure(x, _stage(0.0, flags), want_grad=True)
    return dict(loss=_np(o1['loss']), grad=_np(o1['grad']), S=_np(S), verts=o1['verts'], loss0=_np(o0['loss']),
                grad0=_np(o0['grad']))


@pytest.mark.parametrize('flags', [0, _lib.F_VPOSER])
def test_closure_adds_w2_L_and_its_pulled_back_gradient(world, flags):
    eng, x = world['eng'], world['x']
    T, a, _ = world['sets'][2]
    eng.set_vertex_targets(T, a)
    try:
        verts, _ = eng.vertices(x, flags=flags)
        L_op, g_op = eng.vertex_target_loss(verts)
        L_ref = _np(L_op).astype(np.float64)
        g_ref = _np(eng.vertices_backward(x, grad_verts=g_op, flags=flags)).astype(np.float64)
        w = _weight(eng, x, L_ref, 32, flags)
        eng.set_vertex_target_term()
        r = _evaluate(eng, x, w, flags)
        L_at = _np(eng.vertex_target_loss(r['verts'], need_grad=False)[0])
    finally:
        eng.clear_vertex_targets()
    # L_j is exactly the op at the trial point's vertices
    assert np.array_equal(r['S'], L_at)
    live = [j for j in range(B) if j not in ZERO]
    for j in live:
        pen, pen_ref = float(r['loss'][j]) - float(r['loss0'][j]), w * w * L_ref[j]
        gp = r['grad'][j].astype(np.float64) - r['grad0'][j].astype(np.float64)
        gp_ref = w * w * g_ref[j]
        e_g = np.abs(gp - gp_ref).max() / np.abs(gp_ref).max()
        if j in (0, 31, 32):
            print('flags %d problem %d: L %.7g | pen %.7g ref %.7g (loss %.7g) | grad err/max %.2e (max %.4g)'
                  % (flags, j, r['S'][j], pen, pen_ref, r['loss'][j], e_g, np.abs(gp_ref).max()))
        assert L_ref[j] > 0
        assert abs(pen - pen_ref) <= LOSS_RTOL * float(r['loss'][j]), j
        assert e_g <= GRAD_TOL, j
    # all weights zero: the bits of the closure without the term
    z = list(ZERO)
    assert not r['S'][z].any()
    assert np.array_equal(r['loss'][z], r['loss0'][z]) and np.array_equal(r['grad'][z], r['grad0'][z])
    assert not np.array_equal(r['loss'][32], r['loss0'][32])


def test_sparse_verts_is_ignored_while_the_term_is_on(world):
    eng, x = world['eng'], world['x']
    T, a, _ = world['sets'][2]
    eng.set_vertex_targets(T, a)
    try:
        eng.set_vertex_target_term()
        o = eng.closure(x, _stage(0.5))
        o_sparse = eng.closure(x, _stage(0.5, _lib.F_SPARSE_VERTS))
    finally:
        eng.clear_vertex_targets()
    assert torch.equal(o['loss'], o_sparse['loss']) and torch.equal(o['grad'], o_sparse['grad'])


# ------------------------------------------------------------------------------------------------ 4. and 5. the fit
def _three(world, K=2, seeds=(10, 11), **options):
    """A fresh engine with the three problems and a target set of its own (vertices of perturbed parameters)."""
    rows = list(ROWS3)
    eng = make_engine(world['model'], **options)
    eng.set_problems(world['cams'], world['gt'][rows], world['conf'][rows])
    x = world['x'][rows].copy()
    T, a = _targets3(eng, x, seeds)
    if K == 4:
        T, a = _k4(T, a)
    eng.set_vertex_targets(T, a)
    return eng, x


def _targets3(eng, x, seeds):
    T = torch.stack([eng.vertices(_perturbed(x, s))[0] for s in seeds], dim=1)
    a = np.array([[1.0, 0.75], [0.5, 1.25], [0.0, 0.0]], np.float32)
    return T, a


def _w3(eng, x):
    L = _np(eng.vertex_target_loss(eng.vertices(x)[0], need_grad=False)[0]).astype(np.float64)
    return _weight(eng, x, L, 0)


def test_chained_rounds_evaluate_the_closures_function(world):
    eng, x = _three(world)
    try:
        w = _w3(eng, x)
        eng.set_vertex_target_term()
        tr = eng.fit_trace(12)
        xf, st = eng.fit(x, [_stage(w)], **FIT_KW)
        tr = _np(tr).astype(np.float64)
        eng.fit_trace(0)
        assert st['passes']['run'] == 0                       # chained rounds from the first stage on: no single-launch phase
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
        # two stages, the first without the term: a single-launch lead phase, then chained rounds.  A problem's traced
        # closures are the first stage's, then the second's: each equals the closure of its stage at the traced point
        NT = 32
        tr = eng.fit_trace(NT)
        xf2, st2 = eng.fit(x, [_stage(0.0), _stage(w)], **FIT_KW)
        tr = _np(tr).astype(np.float64)
        eng.fit_trace(0)
        print('two-stage fit: passes %s, closures %s' % (st2['passes'], _np(st2['n_closure'])))
        assert st2['passes']['run'] > 0                       # the lead phase's passes: it ran as the single launch
        assert st2['passes']['missed'] == 0 and st2['passes']['timed_out'] == 0
        assert torch.isfinite(xf2).all() and torch.isfinite(st2['final_loss']).all()
        ncl2 = _np(st2['n_closure'])
        second = [0, 0, 0]                                    # traced closures of the second stage, per problem
        for k in range(NT):
            rows = [b for b in range(3) if k < ncl2[b] and np.isfinite(tr[b, k]).all()]
            if not rows:
                continue
            xk = x.copy()
            xk[rows] = tr[rows, k, :118].astype(np.float32)
            La = _np(eng.closure(xk, _stage(0.0), want_grad=False)['loss']).astype(np.float64)
            Lb = _np(eng.closure(xk, _stage(w), want_grad=False)['loss']).astype(np.float64)
            for b in rows:
                ok_a = abs(La[b] - tr[b, k, 118]) <= 1e-6 * abs(La[b])
                ok_b = abs(Lb[b] - tr[b, k, 118]) <= 1e-6 * abs(Lb[b])
                if second[b] or not ok_a:
                    assert ok_b, (k, b, tr[b, k, 118], La[b], Lb[b])
                    second[b] += 1
                if b == 2:
                    assert La[b] == Lb[b]
        print('two-stage fit: traced closures of the second stage per problem %s' % second)
        assert second[0] >= 2 and second[1] >= 2
        # the problem whose weights are all zero against the same stages with the term off.  A cleared term refuses a
        # weight > 0 (MVFIT_E_STATE), so the second stage's is 0 there; and only round_mode = 1 runs both fits through the
        # same kernels
        eng.set_options(round_mode=1)
        xa, sta = eng.fit(x, [_stage(0.0), _stage(w)], **FIT_KW)
        eng.clear_vertex_target_term()
        xb, stb = eng.fit(x, [_stage(0.0), _stage(0.0)], **FIT_KW)
        assert torch.equal(xa[2], xb[2]) and torch.equal(sta['final_loss'][2], stb['final_loss'][2])
        assert torch.equal(sta['n_closure'][2], stb['n_closure'][2])
        assert not torch.equal(xa[0], xb[0])
    finally:
        eng.close()


def test_the_round_graph_follows_the_target_set(world):
    eng, x = _three(world)
    try:
        w = _w3(eng, x)
        eng.set_vertex_target_term()
        first, _ = eng.fit(x, [_stage(w)], **FIT_KW)
        # a re-freeze with the same (B, K): other targets and other weights in the same buffers
        T, a = _targets3(eng, x, (20, 21))
        a = (a * np.float32(1.5)).astype(np.float32)
        eng.set_vertex_targets(T, a)
        second, st = eng.fit(x, [_stage(w)], **FIT_KW)
        # another K
        eng.set_vertex_targets(*_k4(T, a))
        third, st3 = eng.fit(x, [_stage(w)], **FIT_KW)
    finally:
        eng.close()
    for K, got, st_got in ((2, second, st), (4, third, st3)):
        fresh, xs = _three(world, seeds=(20, 21))
        try:
            Tf, af = _targets3(fresh, xs, (20, 21))
            af = (af * np.float32(1.5)).astype(np.float32)
            fresh.set_vertex_targets(*((Tf, af) if K == 2 else _k4(Tf, af)))
            fresh.set_vertex_target_term()
            ref, st_ref = fresh.fit(xs, [_stage(w)], **FIT_KW)
        finally:
            fresh.close()
        assert torch.equal(got.cpu(), ref.cpu()) and torch.equal(st_got['final_loss'].cpu(), st_ref['final_loss'].cpu()), K
        assert torch.equal(st_got['n_closure'].cpu(), st_ref['n_closure'].cpu()), K
    assert not torch.equal(second[:2].cpu(), first[:2].cpu())
    assert torch.equal(second[2].cpu(), first[2].cpu())              # (all weights zero: the targets do not reach it)


# ------------------------------------------------------------------------------------------------ 6. the contract
def test_contract(world):
    eng, x, cams, verts = world['eng'], world['x'], world['cams'], world['verts']
    faces = world['model']['faces']
    T, a, _ = world['sets'][2]
    try:
        # no set: the op and the term refuse
        with pytest.raises(MvFitError, match='error -3: mvfit_vertex_target_loss'):
            eng.vertex_target_loss(verts)
        with pytest.raises(MvFitError, match='error -3: mvfit_set_vertex_target_term'):
            eng.set_vertex_target_term()
        with pytest.raises(MvFitError, match='error -3'):                  # no term: a weight > 0 is refused
            eng.closure(x, _stage(1.0))
        # K and the weights
        with pytest.raises(MvFitError, match='error -1: mvfit_set_vertex_targets: K = 5'):
            eng.set_vertex_targets(torch.zeros(B, 5, eng.nv, 3), np.ones((B, 5), np.float32))
        for bad in (-1.0, float('nan'), float('inf')):
            w_bad = a.copy()
            w_bad[7, 1] = bad
            with pytest.raises(MvFitError, match='error -1: mvfit_set_vertex_targets: weight'):
                eng.set_vertex_targets(T, w_bad)
        assert eng._lib.mvfit_set_vertex_targets(eng._ctx, 2, T.data_ptr(), None) == -1          # null weights
        eng.set_vertex_targets(T, a)
        assert eng._lib.mvfit_vertex_target_loss(eng._ctx, None, torch.empty(B, device=eng.device).data_ptr(), None) == -1
        assert eng._lib.mvfit_vertex_target_loss(eng._ctx, verts.data_ptr(), None, None) == -1
        # a refused set leaves the one in place
        L0 = eng.vertex_target_loss(verts, need_grad=False)[0]
        with pytest.raises(MvFitError, match='error -1'):
            eng.set_vertex_targets(T, -a - 1.0)
        assert torch.equal(eng.vertex_target_loss(verts, need_grad=False)[0], L0)
        eng.set_vertex_target_term()
        eng.closure(x, _stage(1.0))
        with pytest.raises(MvFitError, match='error -4'):                   # samples: not kept by this term
            eng._check(eng._lib.mvfit_sdf_term_read(eng._ctx, torch.empty(B, eng.nv, 4, device=eng.device).data_ptr(), None))
        # one term slot: the three other setters refuse while this term is on ...
        with pytest.raises(MvFitError, match='error -3: mvfit_set_sdf'):
            eng.set_sdf(faces, num_faces=1, grid_size=32)
        with pytest.raises(MvFitError, match='error -3: mvfit_set_scene_obstacles'):
            eng.set_scene_obstacles(verts, [B], grid_size=8)
        masks = torch.zeros(1, 8, 8, dtype=torch.uint8, device=eng.device)
        masks[0, 2:6, 2:6] = 1
        eng.set_silhouettes(masks, np.zeros(1, np.int32), tuple(c[:1] for c in cams))
        with pytest.raises(MvFitError, match='error -3: mvfit_set_silhouette_term'):
            eng.set_silhouette_term()
        # ... and this one while one of them is configured
        eng.clear_vertex_target_term()
        eng.set_silhouette_term()
        with pytest.raises(MvFitError, match='error -3: mvfit_set_vertex_target_term'):
            eng.set_vertex_target_term()
        eng.clear_silhouettes()
        eng.set_sdf(faces, num_faces=1, grid_size=32)
        with pytest.raises(MvFitError, match='error -3: mvfit_set_vertex_target_term'):
            eng.set_vertex_target_term()
        eng.set_sdf(None)
        eng.set_scene_obstacles(verts, [B], grid_size=8)
        with pytest.raises(MvFitError, match='error -3: mvfit_set_vertex_target_term'):
            eng.set_vertex_target_term()
        eng.clear_scene_obstacles()
        # clearing the targets switches the term off; no targets, no term
        eng.set_vertex_target_term()
        eng.clear_vertex_targets()
        with pytest.raises(MvFitError, match='error -3'):
            eng.closure(x, _stage(1.0))
        with pytest.raises(MvFitError, match='error -3: mvfit_set_vertex_target_term'):
            eng.set_vertex_target_term()
        # another B clears the set and the term
        eng.set_vertex_targets(T, a)
        eng.set_vertex_target_term()
        eng.closure(x, _stage(1.0))
        eng.set_problems(cams, world['gt'][:2], world['conf'][:2])
        with pytest.raises(MvFitError, match='error -3'):
            eng.closure(x[:2], _stage(1.0))
        with pytest.raises(MvFitError, match='error -3'):
            eng.fit(x[:2], [_stage(1.0)])
        with pytest.raises(MvFitError, match='error -3: mvfit_vertex_target_loss'):
            eng.vertex_target_loss(verts[:2])
        # without problems
        bare = make_engine(world['model'])
        try:
            with pytest.raises(MvFitError, match='error -3'):
                bare._check(bare._lib.mvfit_set_vertex_targets(bare._ctx, 2, T.data_ptr(), a.ctypes.data))
            with pytest.raises(MvFitError, match='error -3'):
                bare.set_vertex_target_term()
        finally:
            bare.close()
    finally:
        eng.set_sdf(None)
        eng.clear_scene_obstacles()
        eng.clear_silhouettes()
        eng.set_problems(cams, world['gt'], world['conf'])
        eng.clear_vertex_targets()
