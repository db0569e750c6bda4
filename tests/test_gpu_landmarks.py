"""GPU: the surface landmark term (mvfit_set_landmarks / mvfit_set_landmark_targets / mvfit_landmark_loss /
mvfit_set_landmark_term; landmark.hip -> vertex_backward.hip's gated pull-back and record kernel) as an op, in closure() and in
fit()'s chained rounds.

Full body model, B = 34 problems: the pull-back has a second, ragged 32-problem chunk.  (V, L) are the smallest shapes at which
each phase of the kernel can go wrong: (1, 1) a single item; (3, 65) 195 items - one ragged pass - and landmarks past one wave;
(4, 65) 260 items - a second pass of 4; (8, 6) the feet; (16, 256) both maxima, 4096 items.  One case runs on
small_models.sub_model at an odd Nv.  The tables hold vertex 0 and vertex Nv - 1, two landmarks sharing a vertex, a landmark
naming one vertex in two slots, landmarks with 1, 2 and 4 live slots, and dead slots with id -1.  Targets are the projections of
perturbed parameters' landmarks plus 2 px of noise, confidences in [0.5, 1]; problems 1 and 33 have all confidences zero,
problem 2 a single live item, and every dead target holds NaN.

Bounds.  (a) the op against the float64 oracle (tests/landmark_oracle.py): at most 4 times the case's yardstick - the float32
evaluation of the oracle against its float64 evaluation on the same inputs, worst relative deviation of the loss over the live
problems and worst deviation of the gradient over max|g_ref|; the kernel's fused multiply-adds and reduction order differ from
NumPy's, errors of the same kind and size, and 4 is the factor of tests/scene_sdf_cases.check_gap.  A case counts only with
yardsticks <= 1e-3.  (b) independence, dead entries, (e) the graph: bit for bit.  (c) the closure: the project's LOSS_RTOL /
GRAD_TOL (tests/scene_sdf_cases.py).  (d) chained rounds against the closure: 1e-6 relative.  (f) direction only."""
import numpy as np
import pytest
import torch

from mvsmplfitting_amd import _lib
from mvsmplfitting_amd import landmarks as lmk
from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import MvFitError, pack_params, stage_weights
from tests.gpu_helpers import make_engine
from tests.helpers import body_model
from tests.landmark_oracle import landmark_loss, landmark_points
from tests.scene_sdf_cases import GRAD_TOL, LOSS_RTOL
from tests.small_models import sub_model

pytestmark = pytest.mark.gpu

B = 34
ZERO = (1, 33)
ONE = 2                                 # the problem with a single live item
SHAPES = [(1, 1), (3, 65), (4, 65), (8, 6), (16, 256)]
ROWS3 = (32, 31, 1)                     # the fit's three problems: live, live, all confidences zero
FIT_KW = dict(max_iter=6, maxiters=2)
SCALARS = dict(rho=100.0, w3d=2.0e5, rho3d=0.05)


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


def make_table(L, nv, seed=0, shared=True):
    """ids [L,4] int32, weights [L,4] float32: landmark l has (1, 2, 4)[l % 3] live slots with weights that sum to 1; dead slots
    carry id -1.  shared: vertex 0, vertex nv - 1, a vertex in two landmarks and a vertex twice in one landmark are in."""
    rng = np.random.default_rng(1000 + seed)
    pool = rng.permutation(np.arange(1, nv - 1))[:4 * L].reshape(L, 4)             # (distinct vertices everywhere)
    ids, w = np.full((L, 4), -1, np.int32), np.zeros((L, 4), np.float32)
    for l in range(L):
        n = (1, 2, 4)[l % 3] if L > 1 else 2
        ids[l, :n] = pool[l, :n]
        a = rng.uniform(0.2, 1.0, n)
        w[l, :n] = (a / a.sum()).astype(np.float32)
    if shared:
        ids[0, 0] = 0
        ids[min(1, L - 1), 1] = nv - 1                                             # (L = 1: slots (0, nv - 1))
        if L > 3:
            ids[2, 1] = ids[2, 0]                                                  # one vertex in two slots
            ids[3, 0] = ids[1, 0]                                                  # one vertex in two landmarks
    return ids, w


def make_targets(verts_t, ids, w, cams, seed, zero=ZERO, one=ONE):
    """xy [B,V,L,2], conf [B,V,L], xyz [B,L,3], conf3 [B,L] float32 from the target bodies' vertices."""
    rng = np.random.default_rng(seed)
    p = landmark_points(verts_t, np.where(w != 0, ids, 0), w)
    n, L = p.shape[:2]
    xy = syn.project_points(p, *cams) + rng.normal(0.0, 2.0, (n, len(cams[2]), L, 2))
    conf = rng.uniform(0.5, 1.0, xy.shape[:-1])
    xyz = p + rng.normal(0.0, 0.01, p.shape)
    conf3 = rng.uniform(0.5, 1.0, (n, L))
    conf[rng.uniform(size=conf.shape) < 0.1] = 0.0                                 # (dead items everywhere)
    for j in zero:
        if j < n:
            conf[j], conf3[j] = 0.0, 0.0
    if one is not None and one < n:
        keep = conf[one, -1, L // 2] or 0.75
        conf[one], conf3[one] = 0.0, 0.0
        conf[one, -1, L // 2] = keep
    xy[conf == 0] = np.nan
    xyz[conf3 == 0] = np.nan
    return tuple(a.astype(np.float32) for a in (xy, conf, xyz, conf3))


@pytest.fixture(scope='module')
def world():
    model = body_model()
    vpw = syn.make_vposer_decoder()
    eng = make_engine(model, vpw=vpw)
    cams = syn.make_camera_ring(4)
    x_true = pack_params(B=B, **syn.make_frames(B, seed0=6100))
    eng.set_problems(cams, np.zeros((B, 4, 17, 2), np.float32), np.zeros((B, 4, 17), np.float32))
    _, joints = eng.vertices(x_true)
    gt, conf = syn.make_observations(_np(joints), cams, seed=3)
    eng.set_problems(cams, gt, conf)
    x = _perturbed(x_true, 1)
    x[:, 86:118] = np.random.default_rng(2).normal(0, 0.3, (B, 32)).astype(np.float32)      # (the embedding, read with F_VPOSER only)
    verts = eng.vertices(x)[0]
    verts_t = _np(eng.vertices(_perturbed(x, 10))[0])
    yield dict(eng=eng, model=model, vpw=vpw, cams=cams, x=x, gt=gt, conf=conf, verts=verts, verts_t=verts_t, cases={})
    eng.close()


def case(world, V, L, nv=None):
    """The inputs of one shape and both oracle evaluations, computed once: cameras, table, targets, yardsticks."""
    key = (V, L, nv)
    if key not in world['cases']:
        verts, verts_t = _np(world['verts']), world['verts_t']
        if nv is not None:
            verts, verts_t = world['sub'][1], world['sub'][2]
        cams = syn.make_camera_ring(V)
        ids, w = make_table(L, verts.shape[1], seed=L)
        tg = make_targets(verts_t, ids, w, cams, seed=7 * V + L)
        ref = landmark_loss(verts, ids, w, cams, *tg, **SCALARS)
        f32 = landmark_loss(verts, ids, w, cams, *tg, dtype=np.float32, **SCALARS)
        live = [j for j in range(B) if j not in ZERO]
        assert (ref[0][live] > 0).all()
        y_loss = float((np.abs(f32[0][live] - ref[0][live]) / ref[0][live]).max())
        y_grad = float(np.abs(f32[1] - ref[1]).max() / np.abs(ref[1]).max())
        world['cases'][key] = dict(cams=cams, ids=ids, w=w, tg=tg, ref=ref, y=(y_loss, y_grad), live=live, verts=verts)
    return world['cases'][key]


def use(eng, c, gt=None, conf=None, rows=None, with3d=True):
    """The case's cameras, table and targets on ``eng`` (rows: a subset of the problems)."""
    V = len(c['cams'][2])
    n = B if rows is None else len(rows)
    eng.set_problems(c['cams'], np.zeros((n, V, 17, 2), np.float32) if gt is None else gt,
                     np.zeros((n, V, 17), np.float32) if conf is None else conf)
    eng.set_landmarks(c['ids'], c['w'])
    tg = c['tg'] if rows is None else tuple(a[list(rows)] for a in c['tg'])
    eng.set_landmark_targets(*(tg if with3d else tg[:2]))


# ------------------------------------------------------------------------------------------------ (a) the op
def _check_op(eng, c, verts, tag):
    L_ref, g_ref = c['ref']
    y_loss, y_grad = c['y']
    pre = torch.full_like(verts, float('nan'))                                      # the output buffer holds NaN beforehand
    loss = torch.empty(verts.shape[0], device=verts.device)
    eng._check(eng._lib.mvfit_landmark_loss(eng._ctx, verts.data_ptr(), SCALARS['rho'], SCALARS['w3d'], SCALARS['rho3d'],
                                            loss.data_ptr(), pre.data_ptr()))
    L_only, none = eng.landmark_loss(verts, need_grad=False, **SCALARS)
    L, g = _np(loss), _np(pre)
    assert none is None and np.array_equal(_np(L_only), L)
    assert np.isfinite(L).all() and np.isfinite(g).all()
    live = c['live']
    e_loss = float((np.abs(L[live].astype(np.float64) - L_ref[live]) / L_ref[live]).max())
    e_grad = float(np.abs(g.astype(np.float64) - g_ref).max() / np.abs(g_ref).max())
    print('%s: loss %.7g .. %.7g | yardstick loss %.3g grad %.3g | kernel loss %.3g grad %.3g'
          % (tag, L_ref[live].min(), L_ref[live].max(), y_loss, y_grad, e_loss, e_grad))
    assert y_loss <= 1e-3 and y_grad <= 1e-3                                        # the case counts
    assert e_loss <= 4 * y_loss and e_grad <= 4 * y_grad
    for j in ZERO:
        assert L[j] == 0.0 and not g[j].view(np.uint32).any()
    used = np.unique(c['ids'][c['w'] != 0])
    rest = np.setdiff1d(np.arange(g.shape[1]), used)
    assert not g[:, rest].view(np.uint32).any()                                     # untouched rows: exactly zero (no -0, no NaN)
    assert g[0][used].any(axis=1).all()
    return L, g


@pytest.mark.parametrize('V,L', SHAPES)
def test_the_op_against_the_oracle(world, V, L):
    eng, c = world['eng'], case(world, V, L)
    try:
        use(eng, c)
        _check_op(eng, c, world['verts'], '(%d, %d)' % (V, L))
    finally:
        eng.clear_landmarks()
        eng.set_problems(world['cams'], world['gt'], world['conf'])


def test_the_op_at_an_odd_vertex_count(world):
    nv = 2001
    sub = sub_model(world['model'], nv)
    eng = make_engine(sub)
    try:
        eng.set_problems(world['cams'], np.zeros((B, 4, 17, 2), np.float32), np.zeros((B, 4, 17), np.float32))
        verts = eng.vertices(world['x'])[0]
        world['sub'] = (sub, _np(verts), _np(eng.vertices(_perturbed(world['x'], 10))[0]))
        c = case(world, 3, 65, nv)
        use(eng, c)
        _check_op(eng, c, verts, 'Nv %d (3, 65)' % nv)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ (b) independence
def test_a_problems_numbers_do_not_depend_on_the_batch_the_run_or_the_alignment(world):
    eng, verts, c = world['eng'], world['verts'], case(world, 4, 65)
    try:
        use(eng, c)
        L, g = eng.landmark_loss(verts, **SCALARS)
        L_again, g_again = eng.landmark_loss(verts, **SCALARS)
        n = verts.numel()
        flat = torch.empty(n + 1, device=verts.device)
        flat[1:] = verts.reshape(-1)
        off = flat[1:].view(B, eng.nv, 3)
        assert off.data_ptr() % 8 == 4 and off.is_contiguous()
        L_flat = torch.empty(B + 1, device=verts.device)
        g_flat = torch.full((n + 1,), float('nan'), device=verts.device)
        eng._check(eng._lib.mvfit_landmark_loss(eng._ctx, off.data_ptr(), SCALARS['rho'], SCALARS['w3d'], SCALARS['rho3d'],
                                                L_flat[1:].data_ptr(), g_flat[1:].data_ptr()))
        assert torch.equal(L, L_again) and torch.equal(g, g_again)
        assert torch.equal(L, L_flat[1:]) and torch.equal(g.reshape(-1), g_flat[1:]) and torch.isnan(g_flat[0])
        # a dead slot's id and a dead target's content change no bit
        ids2 = c['ids'].copy()
        ids2[c['w'] == 0] = 2 ** 31 - 1
        xy, conf, xyz, conf3 = (a.copy() for a in c['tg'])
        xy[conf == 0] = 123.0
        xyz[conf3 == 0] = float('inf')
        eng.set_landmarks(ids2, c['w'])
        eng.set_landmark_targets(xy, conf, xyz, conf3)
        L_dead, g_dead = eng.landmark_loss(verts, **SCALARS)
        assert torch.equal(L, L_dead) and torch.equal(g, g_dead)
        # the same landmarks in another table order, no vertex shared: the gradient's bits
        ids_u, w_u = make_table(65, eng.nv, seed=99, shared=False)
        tg = make_targets(world['verts_t'], ids_u, w_u, c['cams'], seed=5)
        perm = np.random.default_rng(8).permutation(65)
        eng.set_landmarks(ids_u, w_u)
        eng.set_landmark_targets(*tg)
        _, g_u = eng.landmark_loss(verts, **SCALARS)
        eng.set_landmarks(ids_u[perm], w_u[perm])
        eng.set_landmark_targets(tg[0][:, :, perm], tg[1][:, :, perm], tg[2][:, perm], tg[3][:, perm])
        _, g_p = eng.landmark_loss(verts, **SCALARS)
        assert torch.equal(g_u, g_p) and g_u.any()
    finally:
        eng.clear_landmarks()
        eng.set_problems(world['cams'], world['gt'], world['conf'])
    one = make_engine(world['model'])
    try:
        use(one, c, rows=[32])
        L1, g1 = one.landmark_loss(verts[32:33], **SCALARS)
    finally:
        one.close()
    assert torch.equal(L1[0].cpu(), L[32].cpu()) and torch.equal(g1[0].cpu(), g[32].cpu())


# ------------------------------------------------------------------------------------------------ (c) the closure
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
    eng, x, c = world['eng'], world['x'], case(world, 4, 65)
    try:
        use(eng, c, world['gt'], world['conf'])
        verts, _ = eng.vertices(x, flags=flags)
        L_op, g_op = eng.landmark_loss(verts, **SCALARS)
        L_ref = _np(L_op).astype(np.float64)
        g_ref = _np(eng.vertices_backward(x, grad_verts=g_op, flags=flags)).astype(np.float64)
        w = _weight(eng, x, L_ref, 32, flags)
        eng.set_landmark_term(**SCALARS)
        r = _evaluate(eng, x, w, flags)
        L_at = _np(eng.landmark_loss(r['verts'], need_grad=False, **SCALARS)[0])
        o_sparse = eng.closure(x, _stage(w, flags | _lib.F_SPARSE_VERTS))
        assert np.array_equal(_np(o_sparse['loss']), r['loss']) and np.array_equal(_np(o_sparse['grad']), r['grad'])
    finally:
        eng.clear_landmarks()
    assert np.array_equal(r['S'], L_at)                                   # L_j is exactly the op at the trial point's vertices
    for j in c['live']:
        pen, pen_ref = float(r['loss'][j]) - float(r['loss0'][j]), w * w * L_ref[j]
        gp = r['grad'][j].astype(np.float64) - r['grad0'][j].astype(np.float64)
        gp_ref = w * w * g_ref[j]
        e_g = np.abs(gp - gp_ref).max() / np.abs(gp_ref).max()
        if j in (0, ONE, 31, 32):
            print('flags %d problem %d: L %.7g | pen %.7g ref %.7g (loss %.7g) | grad err/max %.2e (max %.4g)'
                  % (flags, j, r['S'][j], pen, pen_ref, r['loss'][j], e_g, np.abs(gp_ref).max()))
        assert L_ref[j] > 0
        assert abs(pen - pen_ref) <= LOSS_RTOL * float(r['loss'][j]), j
        assert e_g <= GRAD_TOL, j
    z = list(ZERO)                                                        # all confidences zero: the closure without the term
    assert not r['S'][z].any()
    assert np.array_equal(r['loss'][z], r['loss0'][z]) and np.array_equal(r['grad'][z], r['grad0'][z])
    assert not np.array_equal(r['loss'][32], r['loss0'][32])


# ------------------------------------------------------------------------------------------------ (d), (e) the fit
def _three(world, L=65, seed=21, with3d=True, **options):
    """A fresh engine with the three problems, a table of L landmarks and targets of its own."""
    rows = list(ROWS3)
    eng = make_engine(world['model'], **options)
    eng.set_problems(world['cams'], world['gt'][rows], world['conf'][rows])
    _set3(eng, world, L, seed, with3d)
    return eng, world['x'][rows].copy()


def _set3(eng, world, L, seed, with3d=True):
    ids, w = make_table(L, eng.nv, seed=L)
    tg = make_targets(world['verts_t'][list(ROWS3)], ids, w, world['cams'], seed=seed, zero=(2,), one=None)
    eng.set_landmarks(ids, w)
    eng.set_landmark_targets(*(tg if with3d else tg[:2]))


def _w3(eng, x):
    L = _np(eng.landmark_loss(eng.vertices(x)[0], need_grad=False, **SCALARS)[0]).astype(np.float64)
    return _weight(eng, x, L, 0)


def test_chained_rounds_evaluate_the_closures_function(world):
    eng, x = _three(world)
    try:
        w = _w3(eng, x)
        eng.set_landmark_term(**SCALARS)
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
        # two stages, the first without the term: a single-launch lead phase, then chained rounds
        xf2, st2 = eng.fit(x, [_stage(0.0), _stage(w)], **FIT_KW)
        print('two-stage fit: passes %s, closures %s' % (st2['passes'], _np(st2['n_closure'])))
        assert st2['passes']['run'] > 0                       # the lead phase's passes: it ran as the single launch
        assert st2['passes']['missed'] == 0 and st2['passes']['timed_out'] == 0
        assert torch.isfinite(xf2).all() and torch.isfinite(st2['final_loss']).all()
        # the problem whose confidences are all zero against the same stages with the term off.  A cleared term refuses a
        # weight > 0 (MVFIT_E_STATE), so the second stage's is 0 there; and only round_mode = 1 runs both fits through the
        # same kernels
        eng.set_options(round_mode=1)
        xa, sta = eng.fit(x, [_stage(0.0), _stage(w)], **FIT_KW)
        eng.clear_landmark_term()
        xb, stb = eng.fit(x, [_stage(0.0), _stage(0.0)], **FIT_KW)
        assert torch.equal(xa[2], xb[2]) and torch.equal(sta['final_loss'][2], stb['final_loss'][2])
        assert torch.equal(sta['n_closure'][2], stb['n_closure'][2])
        assert not torch.equal(xa[0], xb[0])
    finally:
        eng.close()


def test_the_round_graph_follows_the_targets(world):
    eng, x = _three(world)
    try:
        w = _w3(eng, x)
        eng.set_landmark_term(**SCALARS)
        first, _ = eng.fit(x, [_stage(w)], **FIT_KW)
        builds = eng.round_graph_info()['builds']
        _set_targets_only(eng, world, 65, 22)                               # the same sizes: other targets in the same buffers
        got = {'same': eng.fit(x, [_stage(w)], **FIT_KW)}
        assert eng.round_graph_info()['builds'] == builds                    # the captured graph was kept
        _set3(eng, world, 6, 23)                                             # another L (a new table clears the term)
        eng.set_landmark_term(**SCALARS)
        got['L6'] = eng.fit(x, [_stage(w)], **FIT_KW)
        _set3(eng, world, 6, 23, with3d=False)                               # without the 3-D part
        eng.set_landmark_term(**SCALARS)
        got['2d'] = eng.fit(x, [_stage(w)], **FIT_KW)
    finally:
        eng.close()
    for name, (L, seed, with3d) in {'same': (65, 22, True), 'L6': (6, 23, True), '2d': (6, 23, False)}.items():
        fresh, xs = _three(world, L, seed, with3d)
        try:
            fresh.set_landmark_term(**SCALARS)
            ref, st_ref = fresh.fit(xs, [_stage(w)], **FIT_KW)
        finally:
            fresh.close()
        out, st_got = got[name]
        assert torch.equal(out.cpu(), ref.cpu()) and torch.equal(st_got['final_loss'].cpu(), st_ref['final_loss'].cpu()), name
        assert torch.equal(st_got['n_closure'].cpu(), st_ref['n_closure'].cpu()), name
    second = got['same'][0]
    assert not torch.equal(second[:2].cpu(), first[:2].cpu())
    assert torch.equal(second[2].cpu(), first[2].cpu())                  # (all confidences zero: the targets do not reach it)
    assert not torch.equal(got['L6'][0][:2].cpu(), got['2d'][0][:2].cpu())


def _set_targets_only(eng, world, L, seed):
    ids, w = make_table(L, eng.nv, seed=L)
    tg = make_targets(world['verts_t'][list(ROWS3)], ids, w, world['cams'], seed=seed, zero=(2,), one=None)
    eng.set_landmark_targets(*tg)


# ------------------------------------------------------------------------------------------------ (f) what it is for
def test_foot_landmarks_turn_the_ankles(world):
    model, cams = world['model'], syn.make_camera_ring(8)
    n = 4
    lbs = np.asarray(model['lbs_weights'])
    ids = np.concatenate([np.argsort(-lbs[:, j])[:3] for j in (7, 8)]).astype(np.int32)     # the six vertices the ankles move most
    rng = np.random.default_rng(77)
    x_true = pack_params(B=n, **syn.make_frames(n, seed0=700))
    x_true[:, 13 + 18:13 + 24] = rng.normal(0.0, 0.5, (n, 6)).astype(np.float32)             # both ankles, rotated in the truth
    eng = make_engine(model)
    try:
        eng.set_problems(cams, np.zeros((n, 8, 17, 2), np.float32), np.zeros((n, 8, 17), np.float32))
        verts_true, joints = eng.vertices(x_true)
        gt, conf = syn.make_observations(_np(joints), cams, seed=12)
        eng.set_problems(cams, gt, conf)
        feet = _np(verts_true)[:, ids]
        xy = syn.project_points(feet, *cams).astype(np.float32)
        cf = np.ones(xy.shape[:-1], np.float32)
        cf[3] = 0.0                                                                           # a problem without foot points
        x0 = _perturbed(x_true, 5)
        x0[:, 13 + 18:13 + 24] = 0.0
        stages = stage_weights(1536.0)
        xk, _ = eng.fit(x0, stages)

        def foot_error(x):
            p = _np(eng.vertices(x)[0])[:, ids]
            return np.linalg.norm(syn.project_points(p, *cams) - xy, axis=-1).mean(axis=(1, 2))
        e0 = foot_error(xk)
        eng.set_landmarks(ids)
        eng.set_landmark_targets(xy, cf)
        xr, rep = lmk.refine_fit(eng, xk, dict(stages[-1], coll_loss_weight=0.5))
        e1 = foot_error(xr)
        print('foot reprojection error, px: keypoints only %s, with the landmark term %s, accepted %s' % (e0, e1, rep['accepted']))
        assert (rep['after'] <= rep['before']).all()                     # no problem's objective rose
        assert (e1[:3] < e0[:3]).all()
        assert torch.equal(xr[3].cpu(), xk[3].cpu()) or rep['accepted'][3]
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ (g) the contract
def test_contract(world):
    eng, x, cams, verts = world['eng'], world['x'], world['cams'], world['verts']
    faces = world['model']['faces']
    c = case(world, 4, 65)
    ids, w = c['ids'], c['w']
    xy, conf, xyz, conf3 = c['tg']
    fp = lambda a: a.ctypes.data_as(_lib._fp)
    try:
        # no table, no targets: everything refuses
        with pytest.raises(MvFitError, match='error -3: mvfit_landmark_loss'):
            eng.landmark_loss(verts)
        with pytest.raises(MvFitError, match='error -3: mvfit_set_landmark_term'):
            eng.set_landmark_term()
        assert eng._lib.mvfit_set_landmark_targets(eng._ctx, fp(xy), fp(conf), None, None) == -3
        with pytest.raises(MvFitError, match='error -3'):                  # no term: a weight > 0 is refused
            eng.closure(x, _stage(1.0))
        # the table
        with pytest.raises(MvFitError, match='error -1: mvfit_set_landmarks: L = 257'):
            eng.set_landmarks(np.zeros(257, np.int32))
        for bad_id in (-1, eng.nv):
            bad = ids.copy()
            bad[5, 0] = bad_id
            with pytest.raises(MvFitError, match='error -1: mvfit_set_landmarks: vertex id'):
                eng.set_landmarks(bad, w)
        for bad_w in (float('nan'), float('inf')):
            bad = w.copy()
            bad[5, 0] = bad_w
            with pytest.raises(MvFitError, match='error -1: mvfit_set_landmarks: weight'):
                eng.set_landmarks(ids, bad)
        eng.set_landmarks(ids, w)
        with pytest.raises(MvFitError, match='error -3: mvfit_landmark_loss'):          # a table without targets
            eng.landmark_loss(verts)
        # the targets
        assert eng._lib.mvfit_set_landmark_targets(eng._ctx, fp(xy), None, None, None) == -1
        assert eng._lib.mvfit_set_landmark_targets(eng._ctx, fp(xy), fp(conf), fp(xyz), None) == -1
        assert eng._lib.mvfit_set_landmark_targets(eng._ctx, fp(xy), fp(conf), None, fp(conf3)) == -1
        eng.set_landmark_targets(xy, conf, xyz, conf3)
        L0 = eng.landmark_loss(verts, need_grad=False, **SCALARS)[0]
        for bad_c in (-0.5, float('nan'), float('inf')):                   # a refused set leaves the one in place
            bad = conf.copy()
            bad[7, 1, 3] = bad_c
            with pytest.raises(MvFitError, match='error -1: mvfit_set_landmark_targets: conf'):
                eng.set_landmark_targets(xy, bad, xyz, conf3)
            bad3 = conf3.copy()
            bad3[7, 3] = bad_c
            with pytest.raises(MvFitError, match='error -1: mvfit_set_landmark_targets: conf3'):
                eng.set_landmark_targets(xy, conf, xyz, bad3)
        assert torch.equal(eng.landmark_loss(verts, need_grad=False, **SCALARS)[0], L0)
        # the op's arguments
        out = torch.empty(B, device=eng.device)
        assert eng._lib.mvfit_landmark_loss(eng._ctx, None, 100.0, 0.0, 0.0, out.data_ptr(), None) == -1
        assert eng._lib.mvfit_landmark_loss(eng._ctx, verts.data_ptr(), 100.0, 0.0, 0.0, None, None) == -1
        for bad in ((-1.0, 0.0, 0.0), (1.0, -1.0, 0.0), (1.0, 0.0, float('nan')), (float('inf'), 0.0, 0.0)):
            with pytest.raises(MvFitError, match='error -1: mvfit_landmark_loss'):
                eng.landmark_loss(verts, *bad)
            with pytest.raises(MvFitError, match='error -1: mvfit_set_landmark_term'):
                eng.set_landmark_term(*bad)
        eng.set_landmark_term(**SCALARS)
        eng.closure(x, _stage(1.0))
        with pytest.raises(MvFitError, match='error -4'):                   # samples: not kept by this term
            eng._check(eng._lib.mvfit_sdf_term_read(eng._ctx, torch.empty(B, eng.nv, 4, device=eng.device).data_ptr(), None))
        # one term slot: the other setters refuse while this term is on ...
        with pytest.raises(MvFitError, match='error -3: mvfit_set_sdf'):
            eng.set_sdf(faces, num_faces=1, grid_size=32)
        with pytest.raises(MvFitError, match='error -3: mvfit_set_scene_obstacles'):
            eng.set_scene_obstacles(verts, [B], grid_size=8)
        masks = torch.zeros(1, 8, 8, dtype=torch.uint8, device=eng.device)
        masks[0, 2:6, 2:6] = 1
        eng.set_silhouettes(masks, np.zeros(1, np.int32), tuple(a[:1] for a in cams))
        with pytest.raises(MvFitError, match='error -3: mvfit_set_silhouette_term'):
            eng.set_silhouette_term()
        T = torch.zeros(B, 1, eng.nv, 3, device=eng.device)
        eng.set_vertex_targets(T, np.ones((B, 1), np.float32))
        with pytest.raises(MvFitError, match='error -3: mvfit_set_vertex_target_term'):
            eng.set_vertex_target_term()
        pts = np.zeros((B, 4, 3), np.float32)
        eng.set_scans(pts)
        with pytest.raises(MvFitError, match='error -3: mvfit_set_scan_term'):
            eng.set_scan_term()
        with pytest.raises(MvFitError, match='error -3: mvfit_set_term_mix'):
            eng.set_term_mix(silhouette=0.5, vertex_targets=0.5)
        # ... and this one while one of them is configured
        eng.clear_landmark_term()
        for on, off in ((eng.set_silhouette_term, eng.clear_silhouette_term), (eng.set_vertex_target_term, eng.clear_vertex_target_term),
                        (eng.set_scan_term, eng.clear_scan_term),
                        (lambda: eng.set_term_mix(silhouette=0.5, vertex_targets=0.5), eng.clear_term_mix),
                        (lambda: eng.set_sdf(faces, num_faces=1, grid_size=32), lambda: eng.set_sdf(None)),
                        (lambda: eng.set_scene_obstacles(verts, [B], grid_size=8), eng.clear_scene_obstacles)):
            on()
            with pytest.raises(MvFitError, match='error -3: mvfit_set_landmark_term'):
                eng.set_landmark_term()
            off()
        eng.clear_silhouettes(); eng.clear_vertex_targets(); eng.clear_scans()
        # clearing the targets switches the term off; no targets, no term; the table stays
        eng.set_landmark_term()
        eng.clear_landmark_targets()
        with pytest.raises(MvFitError, match='error -3'):
            eng.closure(x, _stage(1.0))
        with pytest.raises(MvFitError, match='error -3: mvfit_set_landmark_term'):
            eng.set_landmark_term()
        eng.set_landmark_targets(xy, conf)
        eng.set_landmark_term()
        # a new table clears targets and term
        eng.set_landmarks(ids, w)
        with pytest.raises(MvFitError, match='error -3: mvfit_landmark_loss'):
            eng.landmark_loss(verts)
        with pytest.raises(MvFitError, match='error -3'):
            eng.closure(x, _stage(1.0))
        # another B clears the targets and the term and keeps the table
        eng.set_landmark_targets(xy, conf)
        eng.set_landmark_term()
        eng.closure(x, _stage(1.0))
        eng.set_problems(cams, world['gt'][:2], world['conf'][:2])
        with pytest.raises(MvFitError, match='error -3'):
            eng.closure(x[:2], _stage(1.0))
        with pytest.raises(MvFitError, match='error -3'):
            eng.fit(x[:2], [_stage(1.0)])
        with pytest.raises(MvFitError, match='error -3: mvfit_landmark_loss: no targets'):
            eng.landmark_loss(verts[:2])
        eng.set_landmark_targets(xy[:2], conf[:2])                          # (the table is still there)
        assert torch.isfinite(eng.landmark_loss(verts[:2])[0]).all()
        # clearing the table clears everything
        eng.set_landmark_term()
        eng.clear_landmarks()
        with pytest.raises(MvFitError, match='error -3: mvfit_landmark_loss: no landmark table'):
            eng.landmark_loss(verts[:2])
        with pytest.raises(MvFitError, match='error -3'):
            eng.closure(x[:2], _stage(1.0))
        # without problems
        bare = make_engine(world['model'])
        try:
            bare.set_landmarks(ids, w)                                      # (the table needs none)
            assert bare._lib.mvfit_set_landmark_targets(bare._ctx, fp(xy), fp(conf), None, None) == -3
            with pytest.raises(MvFitError, match='error -3'):
                bare.set_landmark_term()
        finally:
            bare.close()
    finally:
        eng.set_sdf(None)
        eng.clear_scene_obstacles()
        eng.clear_silhouettes()
        eng.clear_vertex_targets()
        eng.clear_scans()
        eng.clear_landmarks()
        eng.set_problems(cams, world['gt'], world['conf'])
