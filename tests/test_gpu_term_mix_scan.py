"""GPU: the scan share of the term mix (mvfit_term_mix::scan; term_mix.hip's three-operand cotangent kernel between
scan_loss.hip's gated round kernels and vertex_backward.hip's gated pull-back) in closure() and in fit()'s chained rounds.

The world is that of tests/test_gpu_term_mix.py - full body model, 4 views, B = 34 problems (rows 32 and 33 lie past one
32-problem chunk; n = 20670 floats per problem are 11 workgroups of the cotangent kernel, the last one partial), masks for
bodies 0, 31, 32, 33, K = 4 targets, 17 scenes of two - with the scan set of tests/test_gpu_scan_term.py beside it: Pmax = 257
points (one past a 256-point workgroup) per body, counts 257, 64, 1 and 0 among them.  Rows 1 and 5 have count 0, row 2 has
points whose weights are all 0; problem 5 has no other component either.
References: the single terms through their own setters, MvFit.scan_loss / silhouette_loss / vertex_target_loss at the closure's
vertices and the NumPy restatement tests/term_mix_scan_oracle.py.  Bounds: LOSS_RTOL / GRAD_TOL (tests/scene_sdf_cases.py) for
sums of separately evaluated closures; chained rounds against the closure 1e-6; everything else bit for bit."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from mvsmplfitting_amd import _lib
from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import MvFitError, pack_params
from tests import term_mix_oracle as tm
from tests import term_mix_scan_oracle as tms
from tests.gpu_helpers import make_engine
from tests.helpers import body_model
from tests.scene_sdf_cases import GRAD_TOL, LOSS_RTOL
from tests.test_gpu_scan_term import _scan_points
from tests.test_gpu_term_mix import (B, BETAS, FIT_KW, IMAGES, KW, OFFSET, SIL, SIZES, SIZES3, V, WITH_IMAGES, _bits, _cams, _k4, _mask_set, _np,
                                     _perturbed, _render, _same, _stage)

pytestmark = pytest.mark.gpu

PMAX = 257
SCAN = dict(scan_w_s2m=1.0, scan_w_m2s=0.5, scan_sigma=0.05)
OP = dict(w_s2m=1.0, w_m2s=0.5, sigma=0.05)                             # the same scalars as the op and the single term take them
ZERO = (1, 5)                           # count 0
NO_WEIGHT = 2                           # 100 points, every weight 0
FREE = ZERO + (NO_WEIGHT,)
ROWS3 = (32, 33, 5)                     # the fit's problems: a scene of two with 257 and 64 points, and problem 5 with nothing
# (scene, silhouette, vertex targets, scan)
SHARE_SETS = [(0.5, 2.0, 0.25, 1.5), (0.0, 0.0, 0.25, 1.5), (0.5, 0.0, 0.0, 1.0), (0.0, 2.0, 0.0, 1.0)]
KEYS = ('scene', 'sil', 'vt', 'scan')


def _counts():
    c = np.random.default_rng(8).integers(2, PMAX, B).astype(np.int32)
    c[[0, 32]] = PMAX
    c[[31, 33]] = 64
    c[3] = 1
    c[list(ZERO)] = 0
    c[NO_WEIGHT] = 100
    return c


@pytest.fixture(scope='module')
def world():
    model = body_model()
    faces = np.asarray(model['faces'], np.int64)
    vpw = syn.make_vposer_decoder()
    eng = make_engine(model, vpw=vpw)
    cams, H, W = _cams()
    fr = syn.make_frames(B, seed0=5300, betas=BETAS)
    fr['scale'][:] = 1.08
    x_true = pack_params(B=B, **fr)
    for a, b in ((0, 1), (32, 33)):
        x_true[b, 82:85] = x_true[a, 82:85] + OFFSET
    x_true[2:32:2, 82] += 3.0
    eng.set_problems(cams, np.zeros((B, V, 17, 2), np.float32), np.zeros((B, V, 17), np.float32))
    _, joints = eng.vertices(x_true)
    gt, conf = syn.make_observations(_np(joints), cams, seed=3)
    eng.set_problems(cams, gt, conf)
    masks = _render(eng, x_true, IMAGES, H, W)
    x = x_true.copy()
    x[:, 0:10] = 0.0
    x[:, 85] = 1.0
    x[:, 82:85] += np.array([0.03, -0.02, 0.04], np.float32)
    x[:, 86:118] = np.random.default_rng(2).normal(0, 0.3, (B, 32)).astype(np.float32)
    T2 = torch.stack([eng.vertices(_perturbed(x, 10))[0], eng.vertices(_perturbed(x, 11))[0]], dim=1)
    a2 = np.random.default_rng(4).uniform(0.5, 1.5, (B, 2)).astype(np.float32)
    a2[[1, 5]] = 0.0
    T4, a4 = _k4(T2, a2)
    points = _scan_points(eng, faces, x, 12, PMAX)
    count = _counts()
    weights = np.random.default_rng(9).uniform(0.5, 2.0, (B, PMAX)).astype(np.float32)
    weights[:, 5::41] = 0.0
    weights[NO_WEIGHT] = 0.0
    w = dict(eng=eng, model=model, faces=faces, vpw=vpw, cams=cams, H=H, W=W, x=x, gt=gt, conf=conf, masks=masks, T=T4, a=a4,
             points=points, count=count, weights=weights, cache={})
    eng.set_silhouettes(*_mask_set(w, range(B)))
    eng.set_vertex_targets(T4, a4)
    eng.set_scans(points, count=count, weights=weights)
    yield w
    eng.close()


def test_the_world_reaches_the_shapes_it_is_built_for(world):
    c = world['count']
    assert {257, 64, 1, 0} <= set(c.tolist()) and not c[list(ZERO)].any() and PMAX == 256 + 1
    assert c[NO_WEIGHT] > 0 and not world['weights'][NO_WEIGHT].any()
    n = 3 * world['eng'].nv
    assert n == 20670 and -(-(n // 2) // 1024) == 11 and (n // 2) % 1024 != 0
    assert B > 32 and c[list(ROWS3)].tolist() == [257, 64, 0]


# ------------------------------------------------------------------------------------------------ 1. the cotangent kernel
def _operands(world):
    if 'ops' not in world['cache']:
        eng = world['eng']
        verts, _ = eng.vertices(world['x'])
        Ls, gs = eng.silhouette_loss(verts, **SIL)
        Lv, gv = eng.vertex_target_loss(verts)
        Lc, gc = eng.scan_loss(verts, **OP)
        assert Lc[0] > 0 and Ls[0] > 0 and Lv[0] > 0
        world['cache']['ops'] = ((gs, Ls), (gv, Lv), (gc, Lc))
    return world['cache']['ops']


LIVE_SUBSETS = [s for s in itertools.product((0, 1), repeat=3) if any(s)]
LAM = (2.0, 0.25, 1.5)


@pytest.mark.parametrize('dead', ['nan', 'null'])
@pytest.mark.parametrize('subset', LIVE_SUBSETS)
def test_the_cotangent_kernel_against_the_oracle(world, subset, dead):
    eng, ops = world['eng'], _operands(world)
    assert len(LIVE_SUBSETS) == 7
    lam = [LAM[i] * subset[i] for i in range(3)]
    nan_g, nan_L = torch.full_like(ops[0][0], float('nan')), torch.full_like(ops[0][1], float('nan'))
    args = []
    for i in range(3):
        gk, Lk = ops[i] if subset[i] else ((nan_g, nan_L) if dead == 'nan' else (None, None))
        args += [lam[i], gk, Lk]
    g, L = eng.term_mix_cotangent3(*args)
    ref = []
    for i in range(3):
        ref += [lam[i], _np(ops[i][0]), _np(ops[i][1])]
    g_ref, L_ref = tms.mix_cotangent3(*ref)
    assert np.isfinite(_np(g)).all()
    assert np.array_equal(_bits(_np(g)), _bits(g_ref)), subset
    assert np.array_equal(_bits(_np(L)), _bits(L_ref)), subset
    if subset[2] == 0:
        # the two-operand entry: the same bits
        g2, L2 = eng.term_mix_cotangent(*args[:6])
        assert torch.equal(g2, g) and torch.equal(L2, L)


def test_cotangent_buffers_at_addresses_4_mod_8(world):
    """each of the three operands, and the result, in turn at an address that is 4 mod 8: the 4-byte path, the same bits"""
    eng, ops = world['eng'], _operands(world)
    g, L = eng.term_mix_cotangent3(LAM[0], ops[0][0], ops[0][1], LAM[1], ops[1][0], ops[1][1], LAM[2], ops[2][0], ops[2][1])
    n = ops[0][0].numel()

    def off(t=None):
        flat = torch.empty(n + 1, device=eng.device)
        if t is not None:
            flat[1:] = t.reshape(-1)
        o = flat[1:].view(B, eng.nv, 3)
        assert o.data_ptr() % 8 == 4 and o.is_contiguous()
        return o

    for which in range(4):
        src = [off(ops[i][0]) if i == which else ops[i][0] for i in range(3)]
        assert all(s.data_ptr() % 8 == (4 if i == which else 0) for i, s in enumerate(src))
        out = off() if which == 3 else torch.empty_like(g)
        L_out = torch.empty(B, device=eng.device)
        eng._check(eng._lib.mvfit_term_mix_cotangent3(eng._ctx, LAM[0], src[0].data_ptr(), ops[0][1].data_ptr(), LAM[1], src[1].data_ptr(),
                                                      ops[1][1].data_ptr(), LAM[2], src[2].data_ptr(), ops[2][1].data_ptr(),
                                                      out.data_ptr(), L_out.data_ptr()))
        assert torch.equal(out, g) and torch.equal(L_out, L), which
    # a misaligned operand whose share is 0 does not take the kernel off the 8-byte path, and is not read
    nan = off(torch.full_like(g, float('nan')))
    g2, L2 = eng.term_mix_cotangent3(LAM[0], ops[0][0], ops[0][1], LAM[1], ops[1][0], ops[1][1], 0.0, nan, None)
    g2_ref, L2_ref = eng.term_mix_cotangent(LAM[0], ops[0][0], ops[0][1], LAM[1], ops[1][0], ops[1][1])
    assert torch.equal(g2, g2_ref) and torch.equal(L2, L2_ref)


# ------------------------------------------------------------------------------------------------ 2. the closure
def _closure(eng, x, w, flags):
    o = eng.closure(x, _stage(w, flags), want_grad=True, want_verts=True)
    return dict(loss=_np(o['loss']), grad=_np(o['grad']), verts=o['verts'])


def _singles(world, flags):
    """The closure at x without a term and with each single term on through its own setter (w = 1), once per flags."""
    key = ('singles', flags)
    if key in world['cache']:
        return world['cache'][key]
    eng, x = world['eng'], world['x']
    r = dict(none=_closure(eng, x, 0.0, flags))
    eng.set_scene_obstacles(r['none']['verts'], SIZES, **KW)
    try:
        r['scene'] = _closure(eng, x, 1.0, flags)
        r['S_sc'] = _np(eng.sdf_term_read()[1])
    finally:
        eng.clear_scene_obstacles()
    eng.set_silhouette_term(**SIL)
    try:
        r['sil'] = _closure(eng, x, 1.0, flags)
    finally:
        eng.clear_silhouette_term()
    eng.set_vertex_target_term()
    try:
        r['vt'] = _closure(eng, x, 1.0, flags)
    finally:
        eng.clear_vertex_target_term()
    eng.set_scan_term(**OP)
    try:
        r['scan'] = _closure(eng, x, 1.0, flags)
    finally:
        eng.clear_scan_term()
    world['cache'][key] = r
    return r


def _mix_on(eng, shares):
    eng.set_term_mix(scene=shares[0], silhouette=shares[1], vertex_targets=shares[2], scan=shares[3], **SIL, **SCAN)


def _mixed(world, flags, shares, w=1.0, eng=None, x=None, sizes=SIZES):
    """The closure with the mix on (obstacles frozen at x's vertices), its four parts and sums."""
    eng, x = eng or world['eng'], world['x'] if x is None else x
    v0, _ = eng.vertices(x, flags=flags)
    eng.set_scene_obstacles(v0, sizes, **KW)
    try:
        _mix_on(eng, shares)
        r = _closure(eng, x, w, flags)
        r['parts'] = _np(eng.term_mix_read(scan=True))
        r['parts3'] = _np(eng.term_mix_read())
        smp, S = eng.sdf_term_read()
        assert smp is None
        r['sums'] = _np(S)
    finally:
        eng.clear_term_mix()
        eng.clear_scene_obstacles()
    return r


@pytest.mark.parametrize('flags', [0, _lib.F_VPOSER])
@pytest.mark.parametrize('shares', SHARE_SETS)
def test_the_mix_is_the_weighted_sum_of_the_single_terms(world, flags, shares):
    eng = world['eng']
    s = _singles(world, flags)
    m = _mixed(world, flags, shares)
    # the parts are the terms' own numbers at the trial point's vertices, bit for bit; 0 for a share of 0
    L_scan = _np(eng.scan_loss(m['verts'], need_grad=False, **OP)[0])
    L_sil = _np(eng.silhouette_loss(m['verts'], need_grad=False, **SIL)[0])
    L_vt = _np(eng.vertex_target_loss(m['verts'], need_grad=False)[0])
    assert (L_scan[[0, 3, 31, 32, 33]] > 0).all() and not L_scan[list(FREE)].any()
    assert m['parts'].shape == (B, 4) and np.array_equal(_bits(m['parts'][:, :3]), _bits(m['parts3']))
    assert np.array_equal(_bits(m['parts'][:, 3]), _bits(L_scan))
    own = (tm.scene_part(s['S_sc']), L_sil, L_vt)
    for k in range(3):
        want = own[k] if shares[k] > 0 else np.zeros(B, np.float32)
        assert np.array_equal(_bits(m['parts'][:, k]), _bits(want)), k
    assert np.array_equal(_bits(m['sums']), _bits(tms.mix_parts_sum4(shares, m['parts'])))
    # penalty and gradient: the weighted sum of the single terms' pull-backs
    f64 = lambda a: a.astype(np.float64)
    l0, g0 = f64(s['none']['loss']), f64(s['none']['grad'])
    pen_ref = sum(lam * (f64(s[k]['loss']) - l0) for lam, k in zip(shares, KEYS))
    gp_ref = sum(lam * (f64(s[k]['grad']) - g0) for lam, k in zip(shares, KEYS))
    pen, gp = f64(m['loss']) - l0, f64(m['grad']) - g0
    e_l = np.abs(pen - pen_ref) / f64(m['loss'])
    gmax = np.abs(gp_ref).max(axis=1)
    live = gmax > 0
    e_g = np.abs(gp - gp_ref).max(axis=1)[live] / gmax[live]
    print('flags %d shares %s: penalty error / loss worst %.2e (problem %d), gradient error / max worst %.2e (problem %d); '
          'penalties of 0, 1, 5, 32, 33: %s' % (flags, shares, e_l.max(), e_l.argmax(), e_g.max(), np.flatnonzero(live)[e_g.argmax()],
                                               pen[[0, 1, 5, 32, 33]]))
    assert live[[0, 3, 31, 32, 33]].all() and pen_ref[32] > 0
    assert (e_l <= LOSS_RTOL).all()
    assert (e_g <= GRAD_TOL).all()
    # rows without participating points and without any other live component: the bits of the closure without a term
    assert not live[5] and not m['parts'][5].any() and m['sums'][5] == 0
    assert np.array_equal(_bits(m['loss'][5]), _bits(s['none']['loss'][5]))
    assert np.array_equal(_bits(m['grad'][5]), _bits(s['none']['grad'][5]))
    if shares[1] == 0:                                                   # (row 2 has no image and zero scan weights)
        quiet = [j for j in FREE if not (shares[0] > 0 and s['S_sc'][j] > 0) and not (shares[2] > 0 and L_vt[j] > 0)]
        assert 5 in quiet
        for j in quiet:
            assert np.array_equal(_bits(m['loss'][j]), _bits(s['none']['loss'][j])), j
            assert np.array_equal(_bits(m['grad'][j]), _bits(s['none']['grad'][j])), j
    assert not np.array_equal(m['loss'][32], s['none']['loss'][32])


def test_the_pass_through_mix_hands_the_scan_buffers_to_the_pull_back(world):
    """scene + scan with scan == 1: where the scene pays nothing (S_sc = 0, the merge is then exact) the record - loss and
    gradient - is bit for bit the single scan term's; where the scan pays nothing, the single scene term's"""
    s = _singles(world, 0)
    m = _mixed(world, 0, (0.5, 0.0, 0.0, 1.0))
    far = [j for j in range(B) if s['S_sc'][j] == 0 and j not in FREE]
    assert len(far) >= 20 and 31 in far and 3 in far
    for j in far:
        assert np.array_equal(_bits(m['loss'][j]), _bits(s['scan']['loss'][j])), j
        assert np.array_equal(_bits(m['grad'][j]), _bits(s['scan']['grad'][j])), j
    assert not np.array_equal(m['loss'][31], s['none']['loss'][31])
    m1 = _mixed(world, 0, (1.0, 0.0, 0.0, 1.0))
    assert s['S_sc'][1] > 0 and m1['parts'][1, 3] == 0
    assert np.array_equal(_bits(m1['loss'][1]), _bits(s['scene']['loss'][1]))
    assert np.array_equal(_bits(m1['grad'][1]), _bits(s['scene']['grad'][1]))


def test_a_scan_share_of_zero_is_never_read_and_the_old_mix_keeps_its_bits(world):
    """the mix without a scan share does not look at the scan set: a set of another size changes nothing, and neither does no
    set at all"""
    eng = world['eng']
    shares = (0.5, 2.0, 0.25, 0.0)
    ref = _mixed(world, 0, shares)
    try:
        eng.set_scans(np.ascontiguousarray(world['points'][:3, :100]), count=np.minimum(world['count'][:3], 100))
        got = _mixed(world, 0, shares)
        eng.clear_scans()
        bare = _mixed(world, 0, shares)
    finally:
        eng.set_scans(world['points'], count=world['count'], weights=world['weights'])
    for k in ('loss', 'grad', 'parts', 'sums'):
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), k
        assert np.array_equal(_bits(bare[k]), _bits(ref[k])), k
    assert not ref['parts'][:, 3].any()
    assert np.array_equal(_bits(ref['sums']), _bits(tm.mix_parts_sum(shares[:3], ref['parts3'])))


# ------------------------------------------------------------------------------------------------ 3. in the fit
def _sub_engine(world, rows, seed=12, **options):
    """A fresh engine with the problems ``rows``, their masks, targets and scan bodies (or other points of the same counts)."""
    rows = list(rows)
    eng = make_engine(world['model'], vpw=world['vpw'], **options)
    eng.set_problems(world['cams'], world['gt'][rows], world['conf'][rows])
    eng.set_silhouettes(*_mask_set(world, rows))
    eng.set_vertex_targets(world['T'][rows], world['a'][rows])
    x = world['x'][rows].copy()
    _set_scans(world, eng, x, rows, seed)
    return eng, x


def _set_scans(world, eng, x, rows, seed=12):
    p = world['points'][rows] if seed == 12 else _scan_points(eng, world['faces'], x, seed, PMAX)
    eng.set_scans(p, count=world['count'][rows], weights=world['weights'][rows])


def _freeze(eng, x, sizes=SIZES3):
    eng.set_scene_obstacles(eng.vertices(x)[0], sizes, **KW)


def _w3(eng, x):
    """w with w^2 = data term / the mix's sum of problem 0: neither drowns the other."""
    data = float(eng.closure(x, _stage(0.0), want_grad=False)['loss'][0])
    eng.closure(x, _stage(1.0), want_grad=False)
    return float(np.sqrt(data / float(eng.sdf_term_read()[1][0])))


def _fit(eng, x, stages):
    xf, st = eng.fit(x, stages, **FIT_KW)
    return xf.cpu(), st['final_loss'].cpu(), st['n_closure'].cpu()


def test_chained_rounds_evaluate_the_closures_function(world):
    eng, x = _sub_engine(world, ROWS3)
    try:
        _freeze(eng, x)
        _mix_on(eng, SHARE_SETS[0])
        w = _w3(eng, x)
        tr = eng.fit_trace(12)
        xf, st = eng.fit(x, [_stage(w)], **FIT_KW)
        tr = _np(tr).astype(np.float64)
        eng.fit_trace(0)
        assert st['passes']['run'] == 0                       # chained rounds from the first stage on
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
        assert torch.isfinite(xf).all() and torch.isfinite(st['final_loss']).all()
    finally:
        eng.close()


def test_a_problems_fit_is_the_same_alone_and_in_the_batch(world):
    """without a scene share a problem stands alone: silhouette + vertex targets + scan, problem 32 in the three and by itself"""
    shares = (0.0, 2.0, 0.25, 1.5)
    eng, x = _sub_engine(world, ROWS3)
    try:
        _mix_on(eng, shares)
        w = _w3(eng, x)
        three = _fit(eng, x, [_stage(w)])
    finally:
        eng.close()
    one, x1 = _sub_engine(world, ROWS3[:1])
    try:
        _mix_on(one, shares)
        alone = _fit(one, x1, [_stage(w)])
    finally:
        one.close()
    for a, b in zip(three, alone):
        assert torch.equal(a[:1], b)
    assert not torch.equal(three[0][0], torch.from_numpy(x[0]))


def test_the_round_graph_follows_the_scan_set_and_the_shares(world):
    eng, x = _sub_engine(world, ROWS3)
    builds, replays = [], []

    def fit():
        out = _fit(eng, x, [_stage(w)])
        info = eng.round_graph_info()
        builds.append(info['builds'])
        replays.append(info)
        return out
    try:
        _freeze(eng, x)
        _mix_on(eng, SHARE_SETS[0])
        w = _w3(eng, x)
        first = fit()
        again = fit()                                          # a second run replays the captured graph
        _set_scans(world, eng, x, list(ROWS3), seed=30)        # other points, the same (N, max_points): the graph is kept
        second = fit()
        other = (0.5, 2.0, 0.25, 0.75)                         # another scan share: rebuilt
        _mix_on(eng, other)
        third = fit()
        eng.set_term_mix(scene=other[0], silhouette=other[1], vertex_targets=other[2], scan=other[3], **SIL,
                         **dict(SCAN, scan_sigma=0.1))         # another scan scalar: rebuilt
        fourth = fit()
    finally:
        eng.close()
    print('round graphs after each fit:', builds, replays[-1])
    assert [n - m for m, n in zip([0] + builds, builds)] == [1, 0, 0, 1, 1], builds
    assert _same(first, again)
    assert not _same(first, second) and not _same(second, third) and not _same(third, fourth)
    # the re-set scan set on an engine that never saw the first one
    fresh, xs = _sub_engine(world, ROWS3, seed=30)
    try:
        _freeze(fresh, xs)
        _mix_on(fresh, SHARE_SETS[0])
        assert _same(second, _fit(fresh, xs, [_stage(w)]))
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------ 4. the contract
def test_contract(world):
    eng, x = world['eng'], world['x']
    scans = dict(count=world['count'], weights=world['weights'])
    both = dict(silhouette=1.0, scan=1.0)
    try:
        # the struct's size: the layout before the scan share is accepted and its scan fields are not looked at
        assert C.sizeof(_lib.TermMix) == 44 and _lib.TERM_MIX_SIZE_V1 == 28
        old = _lib.TermMix(28, 0.0, 1.0, 1.0, 0.5, 20.0, 1.0, float('nan'), -1.0, float('inf'), float('nan'))
        assert eng._lib.mvfit_set_term_mix(eng._ctx, C.byref(old)) == 0
        a = eng.closure(x, _stage(1.0))
        assert not _np(eng.term_mix_read(scan=True))[:, 3].any()
        eng.set_term_mix(silhouette=1.0, vertex_targets=1.0, **SIL)
        b = eng.closure(x, _stage(1.0))
        assert torch.equal(a['loss'], b['loss']) and torch.equal(a['grad'], b['grad'])
        eng.clear_term_mix()
        for size in (C.sizeof(_lib.TermMix) - 4, 24, 32, C.sizeof(_lib.TermMix) + 4, 0):
            bad = _lib.TermMix(size, 0.0, 1.0, 1.0, 0.5, 20.0, 1.0, 0.0, 1.0, 0.0, 0.0)
            assert eng._lib.mvfit_set_term_mix(eng._ctx, C.byref(bad)) == -1, size
        # off: the four-part read refuses
        with pytest.raises(MvFitError, match='error -3: mvfit_term_mix_read4'):
            eng.term_mix_read(scan=True)
        assert eng._lib.mvfit_term_mix_read4(eng._ctx, None) == -1
        # the shares count four; the scan scalars as in the term's own setter
        with pytest.raises(MvFitError, match='error -1: mvfit_set_term_mix'):
            eng.set_term_mix(scan=1.0)
        for kw in (dict(scan=-1.0), dict(scan=float('nan')), dict(scan_w_s2m=-1.0), dict(scan_w_m2s=float('inf')), dict(scan_sigma=-0.1),
                   dict(scan_sigma=float('nan')), dict(scan_w_s2m=0.0, scan_w_m2s=0.0)):
            with pytest.raises(MvFitError, match='error -1: mvfit_set_term_mix'):
                eng.set_term_mix(**dict(both, **kw))
        with pytest.raises(MvFitError, match='error -3'):                    # a refused call leaves the mix off
            eng.closure(x, _stage(1.0))
        # scan > 0 without a set, and with a set of another N
        eng.clear_scans()
        with pytest.raises(MvFitError, match='error -3: mvfit_set_term_mix: scan > 0 needs a scan set'):
            eng.set_term_mix(**both)
        eng.set_scans(world['points'][:3], count=world['count'][:3])
        with pytest.raises(MvFitError, match='error -1: mvfit_set_term_mix: the scan set holds 3 bodies'):
            eng.set_term_mix(**both)
        eng.set_scans(world['points'], **scans)
        # on: the scan term's own setter refuses, the op stays available and returns its own bits
        verts, _ = eng.vertices(x)
        L0 = eng.scan_loss(verts, need_grad=False, **OP)[0]
        eng.set_term_mix(**both, **SCAN)
        eng.closure(x, _stage(1.0))
        with pytest.raises(MvFitError, match='error -3: mvfit_set_scan_term'):
            eng.set_scan_term()
        assert torch.equal(eng.scan_loss(verts, need_grad=False, **OP)[0], L0)
        assert _np(eng.term_mix_read(scan=True))[0, 3] > 0
        # a replacing set of the same shape keeps the mix on; one of another N switches it off (MVFIT_E_ARG)
        eng.set_scans(world['points'], **scans)
        eng.closure(x, _stage(1.0))
        with pytest.raises(MvFitError, match='error -1: mvfit_set_scans: the set holds 3 bodies'):
            eng.set_scans(world['points'][:3], count=world['count'][:3])
        with pytest.raises(MvFitError, match='error -3'):
            eng.closure(x, _stage(1.0))
        with pytest.raises(MvFitError, match='error -3: mvfit_term_mix_read4'):
            eng.term_mix_read(scan=True)
        # clear_scans switches a mix with a scan share off ...
        eng.set_scans(world['points'], **scans)
        eng.set_term_mix(**both, **SCAN)
        eng.clear_scans()
        with pytest.raises(MvFitError, match='error -3'):
            eng.closure(x, _stage(1.0))
        # ... and leaves one without it on, as does every other scan call
        eng.set_scans(world['points'], **scans)
        eng.set_term_mix(silhouette=1.0, vertex_targets=1.0, **SIL)
        a = eng.closure(x, _stage(1.0))
        eng.clear_scans()
        eng.set_scans(world['points'][:3], count=world['count'][:3])
        b = eng.closure(x, _stage(1.0))
        assert torch.equal(a['loss'], b['loss']) and torch.equal(a['grad'], b['grad'])
        with pytest.raises(MvFitError, match='error -3: mvfit_set_scan_term'):
            eng.set_scan_term()
        # the op entry
        with pytest.raises(MvFitError, match='error -1: mvfit_term_mix_cotangent3'):
            eng.term_mix_cotangent3(0.0, None, None, 0.0, None, None, 0.0, None, None)
        with pytest.raises(MvFitError, match='error -1: mvfit_term_mix_cotangent3'):
            eng.term_mix_cotangent3(0.0, None, None, 0.0, None, None, 1.0, None, None)
        with pytest.raises(MvFitError, match='error -1: mvfit_term_mix_cotangent3'):
            eng.term_mix_cotangent3(0.0, None, None, 0.0, None, None, -1.0, None, None)
    finally:
        eng.clear_term_mix()
        eng.clear_scan_term()
        eng.set_scans(world['points'], **scans)
        world['cache'].clear()
