"""GPU: the scan loss (csrc/scan_loss.hip) past the sizes and inputs of tests/test_gpu_scan_loss.py, with that file's helpers
and bounds: more points than one LDS tile of term M (2048) and more than 64 loss partials a body, a workspace used again, face
counts at the edges of the face tile (512) and past one seed tile (2048 seeds = 16384 faces), bodies far from the origin and
scaled down, points far from the body, points exactly on vertices (known answers without a tolerance), faces with a repeated
index, and weights scaled by powers of two and by 1 / count.

E5's tolerance.  The case shifted by (512, -300, 40) has a bound of its own, measured as GRAD_TOL was: |g - g_ref|_inf /
|g_ref|_inf on an MI355X was 2.54e-08 (sigma = 0, where the eight far points are most of |g_ref|_inf) and 1.49e-07 (sigma =
0.05, which takes them out) (profiles/scan_loss.md); asserted at four times the larger, rounded up to one digit: 6e-7.  It
is no larger than near the origin because p - a of nearby fp32 numbers is exact and everything after it is small.  The
scaled-down case keeps GRAD_TOL (measured 2.38e-08 and 1.13e-06: at sigma = 0.05 * 2^-6 the gradient itself is small against
the accumulator's unit, which the weights' exponent does not touch)."""
import numpy as np
import pytest

from mvsmplfitting_amd.engine import MvFit
from tests import scan_oracle as so
from tests.test_gpu_scan_loss import (FAR_AT, GRAD_TOL, check_against_oracle, layer, model, posed, run, same_bits, world)

pytestmark = pytest.mark.gpu

E5_SHIFT = (512.0, -300.0, 40.0)
E5_SHIFT_TOL = 6e-7                                        # measured; see the module docstring
_found = {}                                                # the oracle's search of a world, kept between tests


# ------------------------------------------------------------------------------------------- E1: points on the vertices
def first_equal(points, v):
    """per row of v the lowest i with points[i] == v[j] in all three coordinates, -1 without one"""
    first = {}
    for i, key in enumerate(map(tuple, (points + 0.0).tolist())):
        first.setdefault(key, i)
    return np.array([first.get(key, -1) for key in map(tuple, (v + 0.0).tolist())])


@pytest.fixture(scope='module')
def body_on_its_vertices():
    verts = posed(None, 1, 4101)
    v = verts[0].cpu().numpy()
    faces = np.asarray(model(None)['faces'], np.int64)
    assert len(np.unique(faces)) == len(v) == 6890         # every vertex lies in a face
    zero = so.lowest_zero_face(v.astype(np.float64), v.astype(np.float64), faces)
    assert (zero >= 0).all()
    return verts, v, faces, zero


@pytest.mark.parametrize('order', ['forward', 'reversed', 'doubled'])
def test_points_on_the_vertices_past_one_point_tile_exactly(body_on_its_vertices, order):
    verts, v, faces, zero = body_on_its_vertices
    nv = len(v)
    src = {'forward': np.arange(nv), 'reversed': np.arange(nv)[::-1],
           'doubled': np.concatenate([np.arange(nv), np.arange(2048, nv)])}[order]   # 2048.. once more behind: ties across tiles
    pts = np.ascontiguousarray(v[src])
    w = dict(nv=None, faces=faces, verts=verts, v64=v.astype(np.float64)[None], points=pts[None],
             count=np.array([len(pts)], np.int32), weights=np.ones((1, len(pts)), np.float32))
    assert len(pts) > 3 * 2048 and len(pts) % 2048 != 0    # three full tiles of 2048 and a ragged one at the least
    got = run(w, search='auto', w_s2m=1.0, w_m2s=1.0, sigma=0.0)
    loss, g, nf, npt = got
    assert loss.view(np.uint32)[0] == 0 and not g.view(np.uint32).any()
    want = first_equal(pts, v)
    distinct = first_equal(v, v) == np.arange(nv)
    assert distinct.mean() > 0.99
    if order == 'forward':
        assert (want[distinct] == np.arange(nv)[distinct]).all()
    elif order == 'reversed':
        assert (want[distinct] == (nv - 1 - np.arange(nv))[distinct]).all()
    else:
        assert (want[distinct] == np.arange(nv)[distinct]).all() and (want < nv).all()
    assert np.array_equal(npt[0], want)
    assert np.array_equal(nf[0], zero[src])
    assert same_bits(got, run(w, search='exhaustive', w_s2m=1.0, w_m2s=1.0, sigma=0.0))


# ------------------------------------------------------------------------------- E2: point tiles against the oracle
def test_three_bodies_across_the_point_tile_edge_against_the_oracle():
    w = world(700, 0.005, count=(2048, 2049, 4097), pmax=4097)
    jv = int(w['faces'][0, 0])
    pts = w['points'].copy()
    pts[1, 2048] = w['verts'][1, jv].cpu().numpy()         # the only point of body 1's ragged tile sits on a vertex
    assert w['weights'][1, 2048] > 0
    free = check_against_oracle(dict(w, points=pts), 1.0, 1.0, 0.0)
    npt = free['gpu'][3]
    assert npt[1, jv] == 2048 and (npt[1] == 2048).any()
    assert npt[0].max() < 2048 and npt[2].max() >= 2048


# ------------------------------------------------------------------- E3: 65 partials a body, a workspace used again
def e3_world():
    return world(700, 0.005, count=(16385, 1), pmax=16385)


def set_and_evaluate(eng, w, **kw):
    eng.set_scans(w['points'], w['count'], w['weights'])
    out = eng.scan_loss(w['verts'], return_nearest=True, **kw)
    return [x.cpu().numpy() for x in out]


def test_sixty_five_partials_a_body_against_the_oracle():
    w = e3_world()
    assert -(-w['points'].shape[1] // 256) == 65
    _found['e3'] = check_against_oracle(w, 1.0, 0.5, 0.0, found=_found.get('e3'))['found']


def test_a_workspace_used_again_holds_nothing_of_the_set_before():
    kw = dict(w_s2m=1.0, w_m2s=0.5, sigma=0.0)
    first = e3_world()
    second = world(700, 0.005, count=(300, 16385), pmax=16385, seed=6)
    third = world(700, 0.005, count=(64, 257), pmax=257, seed=7)
    eng = layer(700).engine
    try:
        set_and_evaluate(eng, first, **kw)
        again = set_and_evaluate(eng, second, **kw)        # the same (N, Pmax): the buffers stay
        smaller = set_and_evaluate(eng, third, **kw)       # a smaller set after a larger one
    finally:
        eng.clear_scans()
    for used, w in ((again, second), (smaller, third)):
        with MvFit(model(700)) as fresh:
            assert same_bits(used, set_and_evaluate(fresh, w, **kw))
    assert again[0][0] > 0 and again[0][1] > 0


# ------------------------------------------------------------------------- E4: face-count edges, the second seed tile
@pytest.mark.parametrize('nv,faces', [(700, 512), (1001, 1024), (700, 1), (1001, 'x13')])
def test_face_counts_at_the_tile_edges_and_past_one_seed_tile(nv, faces):
    """one face tile exactly, two exactly (of sub-model 1001: 700 has 815 faces only), one face, and 18187 faces"""
    w = world(nv, 0.03, faces=faces)
    nf = len(w['faces'])
    assert nf == (13 * 1399 if faces == 'x13' else faces)
    if faces == 'x13':
        assert -(-nf // 8) > 2048                          # the seeds need a second LDS tile
    for kw in (dict(w_s2m=1.0, w_m2s=1.0, sigma=0.0), dict(w_s2m=1.0, w_m2s=0.0, sigma=0.05)):
        assert same_bits(run(w, search='auto', **kw), run(w, search='exhaustive', **kw))
    check_against_oracle(w, 1.0, 1.0, 0.0)


# ---------------------------------------------------------------------- E5: away from the origin, points far away
def e5_world(case):
    return world(1001, 0.03, far=True, **(dict(shift=E5_SHIFT) if case == 'shifted' else dict(scale=2.0 ** -6)))


@pytest.mark.parametrize('case', ['shifted', 'scaled'])
def test_bodies_away_from_the_origin_and_points_far_from_the_body(case):
    w = e5_world(case)
    size = 1.0 if case == 'shifted' else 2.0 ** -6
    far = np.sqrt(so.scan_to_mesh(w['points'][0, FAR_AT].astype(np.float64), w['v64'][0], w['faces'])['m'])
    print('far points at', far / size)
    assert (far >= 4.99 * size).all() and (far <= 50.01 * size).all()
    tol = E5_SHIFT_TOL if case == 'shifted' else GRAD_TOL
    for key, kw in (('plain', dict(w_s2m=1.0, w_m2s=0.5, sigma=0.0)), ('robust', dict(w_s2m=1.0, w_m2s=0.0, sigma=0.05 * size))):
        assert same_bits(run(w, search='auto', **kw), run(w, search='exhaustive', **kw))
        free = check_against_oracle(w, kw['w_s2m'], kw['w_m2s'], kw['sigma'], grad_tol=tol, found=_found.get(case))
        _found[case] = free['found']
        print('E5 %s %s: gradient error %.3g' % (case, key, free['grad_err']))


# ------------------------------------------------------------------------------- E6: faces with a repeated index
def test_two_faces_with_a_repeated_index_among_the_others():
    w = world(700, 0.03, faces='pair')
    f = w['faces']
    assert f[0, 0] == f[0, 1] != f[0, 2] and f[1, 0] == f[1, 1] == f[1, 2]
    for kw in (dict(w_s2m=1.0, w_m2s=1.0, sigma=0.0), dict(w_s2m=1.0, w_m2s=0.0, sigma=0.05)):
        assert same_bits(run(w, search='auto', **kw), run(w, search='exhaustive', **kw))
    check_against_oracle(w, 1.0, 1.0, 0.0)


def test_a_point_without_a_winner_reports_none_and_pays_exactly_nothing():
    w = world(700, 0.03, faces='line')
    a, c = w['faces'][0, 0], w['faces'][0, 2]
    kw = dict(w_s2m=1.0, w_m2s=0.0, sigma=0.0)
    got = run(w, search='auto', **kw)
    assert same_bits(got, run(w, search='exhaustive', **kw))
    free = check_against_oracle(w, 1.0, 0.0, 0.0)
    loss, g, nf, npt = got
    ap = w['points'].astype(np.float64) - w['v64'][:, a][:, None, :]
    d2 = (ap * (w['v64'][:, c] - w['v64'][:, a])[:, None, :]).sum(axis=-1)       # ac . ap: > 0 makes m NaN (include/mvfit.h)
    none, some = free['part'] & (d2 > 0), free['part'] & (d2 <= 0)
    assert none.sum() > 20 and some.sum() > 20
    assert (nf[none] == -1).all() and (nf[some] == 0).all()
    dropped = w['weights'].copy()
    dropped[none] = 0.0                                    # without them: the same loss and gradient bits
    other = run(dict(w, weights=dropped), search='auto', **kw)
    assert same_bits(got[:2], other[:2])
    touched = np.flatnonzero(np.abs(g).sum(axis=(0, 2)))
    assert set(touched.tolist()) == {int(a)}               # every winner's closest point is vertex a


# -------------------------------------------------------------------------------------------- E7: the weights' scale
@pytest.mark.parametrize('which', ['small', 'e3'])
def test_weights_scaled_by_a_power_of_two_scale_every_bit(which):
    w = world(700, 0.005) if which == 'small' else e3_world()
    kw = dict(w_s2m=1.0, w_m2s=0.0, sigma=0.0)
    base = run(w, **kw)
    for k in (10, 24, 40):
        got = run(dict(w, weights=np.ldexp(w['weights'], -k)), **kw)
        assert same_bits(got[:2], [np.ldexp(base[0], -k), np.ldexp(base[1], -k)]), k
        assert same_bits(got[2:], base[2:]), k


@pytest.mark.parametrize('w_m2s', [1.0, 0.0])
@pytest.mark.parametrize('which', ['small', 'e3'])
def test_weights_of_one_over_count_against_the_oracle(which, w_m2s):
    """With both terms on, term M's gradient (which no weight scales) is most of |g_ref|_inf and hides term S's rounding, and
    so does a body of few points beside one of many.  Term S alone is held to GRAD_TOL body by body as well: the same
    quantity over a part of the batch, so the same bound."""
    w = world(700, 0.005) if which == 'small' else e3_world()
    weights = (w['weights'] / np.maximum(w['count'], 1)[:, None]).astype(np.float32)
    free = check_against_oracle(dict(w, weights=weights), 1.0, w_m2s, 0.0, found=_found.get(which))
    _found[which] = free['found']
    if w_m2s == 0.0:
        g, ref = free['gpu'][1], free['grad_ref']
        for n in np.flatnonzero(w['count'] > 0):
            err = np.abs(g[n] - ref[n]).max() / np.abs(ref[n]).max()
            print('body %d (%d points): gradient error %.3g, over its bound %.3g' % (n, w['count'][n], err, err / GRAD_TOL))
            assert err <= GRAD_TOL


def test_one_weight_of_one_among_weights_of_two_to_the_minus_twenty():
    w = world(700, 0.005, count=(257,), pmax=257)
    weights = np.full_like(w['weights'], 2.0 ** -20)
    weights[0, 0] = 1.0
    check_against_oracle(dict(w, weights=weights), 1.0, 0.0, 0.0)
