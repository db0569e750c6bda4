"""GPU: the scan loss (csrc/scan_loss.hip; include/mvfit.h:mvfit_set_scans / mvfit_scan_loss) against its float64 restatement
(tests/scan_oracle.py), the culled against the exhaustive search bit for bit, batch independence bit for bit, error codes.

Bounds.  delta = 8 * 2^-24 * max(|p|_inf, |V|_inf) is what rounding can move one coordinate of q - p; a point's m (the float64
m of the face the GPU chose, against the oracle's best) is held to 2 sqrt(m) delta + delta^2, the loss to the weighted sum of
those plus one float32 rounding of the result.  A point is ambiguous when the oracle sees a second face as near (1e-5 relative
+ 1e-7 absolute in distance) whose closest point lies elsewhere (> 1e-4): those are left out of the m check, at most 1 % may
be.  The reference gradient follows the faces the GPU chose (faces that share the nearest edge or vertex tie in exact
arithmetic; either gives the same gradient).  GRAD_TOL: the largest |g - g_ref|_inf / |g_ref|_inf measured over the cases of
this file on an MI355X was 5.41e-07 (3.6e-08 .. 5.41e-07 over the nine oracle cases, profiles/scan_loss.md); asserted at four
times that, rounded up to one digit: 3e-6.

Shapes: sub_model 700 (815 faces: two LDS tiles of 512, the second ragged; 88 vertices in no face) and 1001 (1399 faces);
257 points = two workgroups of 256, the second with one point; a body with no points between two with; one point alone; the
full model (13776 faces: 26 full tiles and one of 464)."""
import functools

import numpy as np
import pytest
import torch

from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import MvFit, MvFitError
from mvsmplfitting_amd.layer import BodyLayer
from mvsmplfitting_amd.scan import ScanLoss
from tests import scan_oracle as so
from tests.small_models import sub_model

pytestmark = pytest.mark.gpu

GRAD_TOL = 3e-6
COUNT = np.array([257, 0, 64], np.int32)


@functools.lru_cache(maxsize=None)
def model(nv, faces=None):
    """faces: None (the model's own), an int k (its first k faces), 'x13' (so.repeated_faces, 13 copies), 'pair' (faces 0 and
    1 replaced by (a, a, c) and (a, a, a), a and c corners of face 2) or 'line' (the two faces (a, a, c), (a, a, c))"""
    full = syn.make_body_model(skin_topk=4)
    m = full if nv is None else sub_model(full, nv)
    if faces is None:
        return m
    f = np.asarray(m['faces'], np.int32)
    a, c = f[2, 0], f[2, 2]
    if faces == 'x13':
        f = so.repeated_faces(f, 13)
    elif faces == 'pair':
        f = np.concatenate([[[a, a, c], [a, a, a]], f[2:]])
    elif faces == 'line':
        f = np.array([[a, a, c], [a, a, c]])
    else:
        f = f[:faces]
    return dict(m, faces=np.ascontiguousarray(f, np.int32))


@functools.lru_cache(maxsize=None)
def layer(nv, faces=None):
    return BodyLayer(model(nv, faces))


def posed(nv, B, seed0):
    """vertices [B,Nv,3] float32 tensor of the model at make_frames poses (translation included)"""
    fr = syn.make_frames(B, seed0=seed0)
    t = {k: torch.from_numpy(v) for k, v in fr.items()}
    with torch.no_grad():
        out = layer(nv)(t['betas'], t['global_orient'], t['body_pose'], transl=t['transl'], scale=t['scale'])
    return out.vertices.contiguous()


def surface_samples(verts, faces, P, noise, rng):
    """P barycentric samples of the faces of verts [Nv,3] plus Gaussian noise"""
    f = faces[rng.integers(0, len(faces), P)]
    u = rng.random((P, 2))
    flip = u.sum(axis=1) > 1
    u[flip] = 1.0 - u[flip]
    a, b, c = verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]]
    return a + u[:, :1] * (b - a) + u[:, 1:] * (c - a) + rng.normal(0, noise, (P, 3))


FAR_AT = 10 + 30 * np.arange(8)                           # rows of body 0 that far=True moves away; none has weight 0


@functools.lru_cache(maxsize=None)
def world(nv, noise, count=tuple(COUNT.tolist()), pmax=257, seed=5, faces=None, shift=None, scale=1.0, far=False):
    """faces: the face list of model(nv, faces); the points are samples of it ('pair' and 'line': of the model's own faces).
    shift, scale: bodies and points become (x + shift) * scale in float64 before they are rounded to float32.  far: the rows
    FAR_AT of body 0 become so.far_points of the body, 5 to 50 units (times scale) away."""
    mesh = np.asarray(model(nv, faces)['faces'], np.int64)
    sampled = np.asarray(model(nv)['faces'], np.int64) if faces in ('pair', 'line') else mesh
    N = len(count)
    verts = posed(nv, N, 4100 + N)
    v64 = verts.cpu().numpy().astype(np.float64)
    move = lambda x: x if shift is None and scale == 1.0 else (x + np.asarray(shift or (0.0, 0.0, 0.0))) * scale
    rng = np.random.default_rng(seed)
    points = np.stack([move(surface_samples(v64[n], sampled, pmax, noise, rng)).astype(np.float32) for n in range(N)])
    weights = rng.uniform(0.5, 2.0, (N, pmax)).astype(np.float32)
    weights[:, 5::41] = 0.0
    if shift is not None or scale != 1.0:
        verts = torch.from_numpy(move(v64).astype(np.float32)).to(verts.device)
        v64 = verts.cpu().numpy().astype(np.float64)
    if far:
        points[0, FAR_AT] = so.far_points(v64[0], mesh, len(FAR_AT), lo=5.0 * scale, hi=50.0 * scale)[0].astype(np.float32)
    return dict(nv=nv, variant=faces, faces=mesh, verts=verts, v64=v64, points=points, count=np.asarray(count, np.int32),
                weights=weights)


def run(w, search='auto', **kw):
    eng = layer(w['nv'], w.get('variant')).engine
    eng.set_scans(w['points'], w['count'], w['weights'])
    try:
        loss, g, nf, npt = eng.scan_loss(w['verts'], return_nearest=True, search=search, **kw)
        torch.cuda.synchronize()
    finally:
        eng.clear_scans()
    return loss.cpu().numpy(), g.cpu().numpy(), nf.cpu().numpy(), npt.cpu().numpy()


def check_against_oracle(w, w_s2m, w_m2s, sigma, grad_tol=GRAD_TOL, found=None):
    """-> the oracle's own result (its winners, regions and ambiguity flags), with the GPU's (loss, g, nearest_face,
    nearest_point) under 'gpu' and the gradient error under 'grad_err'.  found: the 'found' of an earlier call for the same
    bodies, faces and participating points (the weights may differ in size), to skip the oracle's search."""
    loss, g, nf, npt = run(w, w_s2m=w_s2m, w_m2s=w_m2s, sigma=sigma)
    pts64 = w['points'].astype(np.float64)
    free = so.evaluate(w['v64'], w['faces'], pts64, w['count'], w['weights'], w_s2m=w_s2m, w_m2s=w_m2s, sigma=sigma,
                       found=found if w_s2m > 0 else None)
    part = free['part']
    # a point takes part and has a winner (the oracle reports -1 only where every face's m is NaN: repeated indices)
    assert ((nf >= 0) == (part & (free['nearest_face'] >= 0))).all() if w_s2m > 0 else (nf == -1).all()
    scale = max(np.abs(pts64[part]).max() if part.any() else 0.0, np.abs(w['v64']).max())
    ref = so.evaluate(w['v64'], w['faces'], pts64, w['count'], w['weights'], w_s2m=w_s2m, w_m2s=w_m2s, sigma=sigma,
                      face_override=nf, found=free['found'] if w_s2m > 0 else None)
    bound = np.zeros(len(loss))
    if w_s2m > 0:
        share = free['ambiguous'][part].mean()
        print('ambiguous share %.4f, regions %s' % (share, np.bincount(free['region'][nf >= 0], minlength=7).tolist()))
        assert share <= 0.01
        ok = part & ~free['ambiguous']
        dm = ref['m_s'] - free['m_s']                       # float64 m of the GPU's face against the oracle's best
        lim = so.m_bound(free['m_s'], scale)
        print('max dm / bound %.3g' % (np.abs(dm[ok]) / lim[ok]).max())
        assert (np.abs(dm[ok]) <= lim[ok]).all()
        bound += w_s2m * (w['weights'] * lim * part).sum(axis=1)
    if w_m2s > 0:
        has = w['count'] > 0
        assert (npt[has] >= 0).all() and (npt[~has] == -1).all()
        for n in np.flatnonzero(has):
            d = w['v64'][n] - pts64[n, npt[n]]
            lim = so.m_bound(free['m_m'][n], scale)
            assert part[n, npt[n]].all() and (np.abs((d * d).sum(axis=1) - free['m_m'][n]) <= lim).all()
            assert (npt[n] == free['nearest_point'][n]).mean() > 0.99
            bound[n] += w_m2s * lim.sum()
    else:
        assert (npt == -1).all()
    dl = np.abs(loss - ref['loss'])
    print('loss', loss, 'ref', ref['loss'], 'dl / bound', dl / np.maximum(bound + 2.0 ** -24 * np.abs(ref['loss']), 1e-300))
    assert (dl <= bound + 2.0 ** -24 * np.abs(ref['loss'])).all()
    err = np.abs(g - ref['grad']).max() / np.abs(ref['grad']).max()
    print('gradient error %.3g, over its bound %.3g' % (err, err / grad_tol))
    free['gpu'], free['grad_err'], free['grad_ref'] = (loss, g, nf, npt), err, ref['grad']
    assert err <= grad_tol
    return free


def test_the_models_are_the_ones_the_cases_are_sized_for():
    m = model(700)
    assert len(m['faces']) == 815 and 700 - len(np.unique(m['faces'])) == 88
    assert len(model(1001)['faces']) == 1399 and len(model(None)['faces']) == 13776


@pytest.mark.parametrize('noise', [0.005, 0.03])
@pytest.mark.parametrize('nv', [700, 1001])
def test_both_terms_against_the_oracle(nv, noise):
    w = world(nv, noise)
    free = check_against_oracle(w, 1.0, 1.0, 0.0)
    if noise == 0.03:                                     # every region branch ran
        assert set(free['region'][free['part']].tolist()) == set(range(7))


def test_term_s_alone_and_term_m_alone():
    w = world(700, 0.03)
    check_against_oracle(w, 0.7, 0.0, 0.0)
    check_against_oracle(w, 0.0, 1.3, 0.0)


def test_the_robust_form():
    check_against_oracle(world(1001, 0.03), 1.0, 0.5, 0.02)


def test_one_point():
    check_against_oracle(world(700, 0.005, count=(1,), pmax=1), 1.0, 1.0, 0.0)


def test_the_full_model_with_ragged_face_tiles():
    check_against_oracle(world(None, 0.005, count=(1024, 1000), pmax=1024), 1.0, 1.0, 0.0)


def same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
               for x, y in zip(a, b))


@pytest.mark.parametrize('nv,noise', [(700, 0.03), (1001, 0.005)])
def test_culled_and_exhaustive_search_and_two_runs_give_the_same_bits(nv, noise):
    w = world(nv, noise)
    for kw in (dict(w_s2m=1.0, w_m2s=1.0, sigma=0.0), dict(w_s2m=1.0, w_m2s=0.0, sigma=0.05)):
        a = run(w, search='auto', **kw)
        assert same_bits(a, run(w, search='exhaustive', **kw))
        assert same_bits(a, run(w, search='auto', **kw))


def test_the_full_model_culled_and_exhaustive_give_the_same_bits():
    w = world(None, 0.03, count=(1024, 1000), pmax=1024)
    assert same_bits(run(w, search='auto', w_s2m=1.0, w_m2s=1.0), run(w, search='exhaustive', w_s2m=1.0, w_m2s=1.0))


def test_a_body_alone_and_at_another_batch_position_gives_the_same_bits():
    w = world(700, 0.03)
    whole = run(w, w_s2m=1.0, w_m2s=1.0)
    for n in (0, 2):
        alone = dict(w, verts=w['verts'][n:n + 1].contiguous(), points=w['points'][n:n + 1], count=w['count'][n:n + 1],
                     weights=w['weights'][n:n + 1])
        assert same_bits(run(alone, w_s2m=1.0, w_m2s=1.0), [x[n:n + 1] for x in whole])
    order = [2, 0, 1]
    moved = dict(w, verts=w['verts'][order].contiguous(), points=w['points'][order], count=w['count'][order],
                 weights=w['weights'][order])
    assert same_bits(run(moved, w_s2m=1.0, w_m2s=1.0), [x[order] for x in whole])


def test_a_body_without_points_pays_exactly_nothing():
    w = world(700, 0.03)
    loss, g, nf, npt = run(w, w_s2m=1.0, w_m2s=0.0)
    assert loss[1] == 0.0 and not g[1].any() and (nf[1] == -1).all()
    assert loss[0] > 0 and g[0].any()
    loss, g, nf, npt = run(w, w_s2m=1.0, w_m2s=1.0)
    assert loss[1] == 0.0 and not g[1].any() and (npt[1] == -1).all()


def test_a_nan_in_a_point_that_takes_no_part_changes_no_bit():
    w = world(1001, 0.005)
    clean = run(w, w_s2m=1.0, w_m2s=1.0)
    pts = w['points'].copy()
    pts[2, 64:] = np.nan                                  # beyond count
    pts[1] = np.nan                                       # count 0
    pts[:, 5::41] = np.nan                                # weight 0
    assert same_bits(clean, run(dict(w, points=pts), w_s2m=1.0, w_m2s=1.0))


def test_unweighted_set_and_a_second_set_of_the_same_size():
    w = world(700, 0.005)
    eng = layer(700).engine
    eng.set_scans(w['points'], w['count'])
    a = eng.scan_loss(w['verts'], w_s2m=1.0, w_m2s=1.0)
    eng.set_scans(torch.from_numpy(w['points']).to(eng.device), w['count'], np.ones_like(w['weights']))
    b = eng.scan_loss(w['verts'], w_s2m=1.0, w_m2s=1.0)
    eng.clear_scans()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ref = so.evaluate(w['v64'], w['faces'], w['points'].astype(np.float64), w['count'], None, w_s2m=1.0, w_m2s=1.0)
    assert np.allclose(a[0].cpu().numpy(), ref['loss'], rtol=1e-4)


def test_the_module_through_the_body_layer():
    w = world(700, 0.03)
    lay = layer(700)
    fr = {k: torch.from_numpy(v).to(lay.engine.device) for k, v in syn.make_frames(3, seed0=4103).items()}
    betas, scale = fr['betas'].clone().requires_grad_(True), fr['scale'].clone().requires_grad_(True)
    mod = ScanLoss(engine=lay.engine, points=w['points'], count=w['count'], weights=w['weights'], w_s2m=1.0, w_m2s=0.5)
    try:
        out = lay(betas, fr['global_orient'], fr['body_pose'], transl=fr['transl'], scale=scale)
        loss = mod(out.vertices)
        loss.sum().backward()
        direct, g = lay.engine.scan_loss(out.vertices.detach(), w_s2m=1.0, w_m2s=0.5)
        assert torch.equal(loss.detach(), direct)
        want = lay.engine.vertices_backward(torch.cat([betas.detach(), fr['global_orient'], fr['body_pose'], fr['transl'],
                                                       scale.detach(), torch.zeros(3, 32, device=g.device)], dim=1), g)
        assert torch.equal(betas.grad, want[:, :10]) and torch.equal(scale.grad, want[:, 85:86])
        assert betas.grad[0].abs().max() > 0 and not betas.grad[1].any()
    finally:
        lay.engine.clear_scans()


def test_error_codes():
    w = world(700, 0.005)
    eng = layer(700).engine
    with pytest.raises(MvFitError, match='-4|no scan set'):
        eng.scan_loss(w['verts'])
    with pytest.raises(MvFitError, match='count'):
        eng.set_scans(w['points'], [257, 258, 0])
    with pytest.raises(MvFitError, match='count'):
        eng.set_scans(w['points'], [257, -1, 0])
    bad = w['weights'].copy()
    bad[0, 3] = -1.0
    with pytest.raises(MvFitError, match='weights'):
        eng.set_scans(w['points'], w['count'], bad)
    bad[0, 3] = np.inf
    with pytest.raises(MvFitError, match='weights'):
        eng.set_scans(w['points'], w['count'], bad)
    bad[0, 3] = 1.0
    bad[2, 100] = -1.0                                    # beyond count[2] = 64: never read
    eng.set_scans(w['points'], w['count'], bad)
    try:
        with pytest.raises(MvFitError, match='num_bodies'):
            eng.scan_loss(w['verts'][:2].contiguous())
        for kw in (dict(w_s2m=-1.0), dict(w_m2s=float('nan')), dict(sigma=-1.0), dict(sigma=float('inf'))):
            with pytest.raises(MvFitError, match='finite'):
                eng.scan_loss(w['verts'], **kw)
        with pytest.raises(MvFitError, match='search'):
            eng.scan_loss(w['verts'], search='fast')
        loss, g = eng.scan_loss(w['verts'], need_grad=False)
        assert g is None and loss[0] > 0
    finally:
        eng.clear_scans()
    with pytest.raises(MvFitError, match='no scan set'):
        eng.scan_loss(w['verts'])
    no_faces = dict(model(700), faces=None)
    with MvFit(no_faces) as e:
        with pytest.raises(MvFitError, match='faces'):
            e.set_scans(w['points'], w['count'])
