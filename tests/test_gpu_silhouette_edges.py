"""GPU: the silhouette term past one search chunk, one LDS tile and one instance group (csrc/silhouette.hip: SIL_CHUNK = 512
contour points per workgroup, SIL_VT = 3456 vertices per tile, 64 partials per trip of sil_ordered_sum;
csrc/silhouette_occlusion.hip: OCC_GROUP = 512 instances per pass), on the cases of tests/silhouette_edge_cases.py, whose reach
tests/test_silhouette_edge_cases_cpu.py proves on the oracles: images that keep exactly 1, 511 .. 513, 1024, 1025, 0, 1536,
1537 and 32769 contour points (65 chunks), bodies of 701, 3456, 3457 and 6890 vertices, ties inside one 16-byte read, across
two reads and across the tile boundary, a body with one valid vertex, an image whose body lies behind its camera, and a
scene of twelve bodies in 48 images: 576 instances.

References: tests/silhouette_oracle.py and tests/silhouette_occlusion_oracle.py at the vertices the engine made.  Bounds, the
project's own (tests/scene_sdf_cases.py): fields, contour lists, maps, flags, hidden bytes and winners exactly, loss within
LOSS_RTOL = 1e-5 relative, gradient within GRAD_TOL = 2e-4 of max |g_ref| per call."""
import numpy as np
import pytest
import torch

from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import stage_weights
from tests import silhouette_edge_cases as ec
from tests import silhouette_occlusion_oracle as oo
from tests import silhouette_oracle as so
from tests.gpu_helpers import make_engine
from tests.scene_sdf_cases import GRAD_TOL, LOSS_RTOL

pytestmark = pytest.mark.gpu

NV = 3457
V4 = 4


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _ring(V=V4):
    R, t, f, c = syn.make_camera_ring(V, radius=4.0)
    return R, t, (f * np.float32(256 / 2048.0)).astype(np.float32), np.tile(np.float32([128.0, 96.0]), (V, 1))


@pytest.fixture(scope='module')
def worlds():
    """get(nv): one engine per vertex count with three problems set, the posed bodies and a cache of oracle answers."""
    made = {}

    def get(nv):
        if nv not in made:
            eng = make_engine(ec.model(nv))
            x = ec.params()
            eng.set_problems(_ring(), np.zeros((ec.N, V4, 17, 2), np.float32), np.zeros((ec.N, V4, 17), np.float32))
            made[nv] = dict(eng=eng, nv=nv, x=x, verts=_np(eng.vertices(x)[0]), cams=ec.arc_cameras(), ref={})
        return made[nv]

    yield get
    for w in made.values():
        w['eng'].close()


def _reference(w, stride, name):
    if (stride, name) not in w['ref']:
        w['ref'][(stride, name)] = so.evaluate(ec.prepared(stride), w['verts'], ec.IMAGE_BODY, w['cams'], **ec.SETTINGS[name])
    return w['ref'][(stride, name)]


def _check(eng, verts, ref, label, **kw):
    """One evaluation against the oracle's dict at the project's bounds; prints each figure before it asserts."""
    loss, g, win = eng.silhouette_loss(verts, return_winner=True, **kw)
    loss_only, none = eng.silhouette_loss(verts, need_grad=False, **kw)              # acc == nullptr: the same loss bits
    bits = _np(loss)
    loss, g, win = bits.astype(np.float64), _np(g).astype(np.float64), _np(win)
    scale = np.abs(ref['g']).max()
    lerr = np.abs(loss - ref['loss']) / np.maximum(np.abs(ref['loss']), 1e-300)
    gerr = np.abs(g - ref['g']).max() / scale
    print('EDGE %s: winners differ %d of %d | loss %s rel err %s | grad err / max %.3g (max |g| %.4g)'
          % (label, int((win != ref['winner']).sum()), len(win), loss, lerr, gerr, scale))
    assert np.array_equal(win, ref['winner'])
    assert scale > 0 and np.isfinite(loss).all() and np.isfinite(g).all()
    for n in np.flatnonzero(ref['loss'] == 0):                                      # a body without a contribution: exactly 0
        assert loss[n] == 0 and not g[n].any()
    assert (np.abs(loss - ref['loss']) <= LOSS_RTOL * np.abs(ref['loss'])).all()
    assert (np.abs(g - ref['g']) <= GRAD_TOL * scale).all()
    assert none is None and np.array_equal(_bits(_np(loss_only)), _bits(bits))
    return loss, g, win


# ---- 1. chunk edges against the oracle
@pytest.mark.parametrize('stride', [1, 3])
@pytest.mark.parametrize('nv', ec.NVS)
def test_exact_count_masks_prepare_as_the_oracle_does(worlds, nv, stride):
    eng = worlds(nv)['eng']
    masks, want = ec.exact_count_masks(), ec.prepared(stride)
    eng.set_silhouettes(masks, ec.IMAGE_BODY, worlds(nv)['cams'], contour_stride=stride)
    field, first, xy = (_np(t) for t in eng.silhouettes())
    assert tuple(np.diff(first)) == ec.KEPT[stride]
    assert np.array_equal(first, want['first']) and np.array_equal(xy, want['xy'])
    assert np.array_equal(_bits(field), _bits(want['fields'])), int((field != want['fields']).sum())
    assert not field[6].any() and not field[10].any() and field[0].max() > 500


LOSS_CASES = [(NV, s, k) for s in (1, 3) for k in ec.SETTINGS] + [(nv, s, 'sigma20') for nv in (701, 3456, 6890) for s in (1, 3)]


@pytest.mark.parametrize('nv,stride,name', LOSS_CASES, ids=['%d-stride%d-%s' % c for c in LOSS_CASES])
def test_loss_gradient_and_winners_at_the_chunk_edges(worlds, nv, stride, name):
    w = worlds(nv)
    ref = _reference(w, stride, name)
    if nv == NV and ec.SETTINGS[name]['w_out'] > 0:
        assert (ref['winner'] >= 3456).any()                                        # the one-vertex second tile wins points
    w['eng'].set_silhouettes(ec.exact_count_masks(), ec.IMAGE_BODY, w['cams'], contour_stride=stride)
    loss, _, _ = _check(w['eng'], w['verts'], ref, '%d stride %d %s' % (nv, stride, name), **ec.SETTINGS[name])
    assert loss[0] > 0 and loss[2] > 0 and loss[1] == 0


# ---- 2. ties, one valid vertex, a body behind its camera
def _tie(w, kind):
    nv, prep = w['nv'], ec.prepared(1)
    jw = ec.most_winning(_reference(w, 1, 'sigma20')['winner'], prep['first'], ec.IMAGE_BODY, nv)
    verts, tied = ec.tie_world(w['verts'], jw, kind)
    ref = so.evaluate(prep, verts, ec.IMAGE_BODY, w['cams'], **ec.SETTINGS['sigma20'])
    for body, (lower, higher) in tied.items():                                      # the case is what its name says
        won = ec.wins(ref['winner'], prep['first'], ec.IMAGE_BODY, body, nv)
        print('%d %s body %d: vertex %d wins %d points, its copies %s win %s'
              % (nv, kind, body, lower, won[lower], higher, won[higher]))
        assert won[lower] >= 100 and not won[higher].any()
    w['eng'].set_silhouettes(ec.exact_count_masks(), ec.IMAGE_BODY, w['cams'])
    _check(w['eng'], verts, ref, '%d tie %s' % (nv, kind), **ec.SETTINGS['sigma20'])


@pytest.mark.parametrize('kind', sorted(ec.TIES))
def test_equal_distances_go_to_the_lowest_vertex(worlds, kind):
    _tie(worlds(NV), kind)


@pytest.mark.parametrize('kind', ec.TIES_701)
def test_equal_distances_go_to_the_lowest_vertex_in_an_odd_tile(worlds, kind):
    _tie(worlds(701), kind)


def test_one_valid_vertex_collects_every_point(worlds):
    w = worlds(NV)
    verts = ec.single_valid(w['verts'], 3456)
    ref = so.evaluate(ec.prepared(1), verts, ec.IMAGE_BODY, w['cams'], **ec.SETTINGS['sigma20'])
    assert (ref['winner'] == 3456).all() and len(ref['winner']) == sum(ec.KEPT[1])
    w['eng'].set_silhouettes(ec.exact_count_masks(), ec.IMAGE_BODY, w['cams'])
    _, g, win = _check(w['eng'], verts, ref, '%d one valid vertex' % NV, **ec.SETTINGS['sigma20'])
    assert (win == 3456).all() and not g[:, :3456].any() and np.abs(g[:, 3456]).max() > 0


def test_an_image_whose_body_lies_behind_its_camera_adds_exactly_nothing(worlds):
    w = worlds(NV)
    eng, first = w['eng'], ec.prepared(1)['first']
    cams = ec.all_behind(w['cams'], ec.BIG_IMAGE)
    ref = so.evaluate(ec.prepared(1), w['verts'], ec.IMAGE_BODY, cams, **ec.SETTINGS['sigma20'])
    assert (ref['winner'][first[ec.BIG_IMAGE]:first[ec.BIG_IMAGE + 1]] == -1).all()
    eng.set_silhouettes(ec.exact_count_masks(), ec.IMAGE_BODY, cams)
    loss, g = eng.silhouette_loss(w['verts'], **ec.SETTINGS['sigma20'])
    _check(eng, w['verts'], ref, '%d image %d behind its camera' % (NV, ec.BIG_IMAGE), **ec.SETTINGS['sigma20'])
    keep = np.array([i for i in range(len(ec.IMAGE_BODY)) if i != ec.BIG_IMAGE])
    eng.set_silhouettes(ec.exact_count_masks()[keep], ec.IMAGE_BODY[keep], tuple(a[keep] for a in cams))
    loss_r, g_r = eng.silhouette_loss(w['verts'], **ec.SETTINGS['sigma20'])
    assert torch.equal(loss, loss_r) and torch.equal(g, g_r) and float(loss[ec.BIG_BODY]) > 0


# ---- 3. independence at the edges
def test_the_65_chunk_body_alone_in_a_larger_batch_and_twice(worlds):
    w = worlds(NV)
    eng, masks, cams = w['eng'], ec.exact_count_masks(), w['cams']
    v = torch.from_numpy(w['verts']).to(eng.device)
    kw = ec.SETTINGS['sigma20']
    eng.set_silhouettes(masks, ec.IMAGE_BODY, cams)
    loss, g, win = eng.silhouette_loss(v, return_winner=True, **kw)
    loss_b, g_b, win_b = eng.silhouette_loss(v, return_winner=True, **kw)
    assert torch.equal(loss, loss_b) and torch.equal(g, g_b) and torch.equal(win, win_b)
    b = ec.BIG_BODY
    pick = np.flatnonzero(ec.IMAGE_BODY == b)
    assert ec.BIG_IMAGE in pick
    eng.set_silhouettes(masks[pick], np.zeros(len(pick), np.int32), tuple(a[pick] for a in cams))
    loss_1, g_1 = eng.silhouette_loss(v[b:b + 1], **kw)
    assert torch.equal(loss_1[0], loss[b]) and torch.equal(g_1[0], g[b]) and g_1.abs().max() > 0
    eng.set_silhouettes(masks[pick], np.full(len(pick), 3, np.int32), tuple(a[pick] for a in cams))
    loss_4, g_4 = eng.silhouette_loss(torch.cat([v[:1], v[:1], v[1:2], v[b:b + 1]]), **kw)
    assert torch.equal(loss_4[3], loss[b]) and torch.equal(g_4[3], g[b]) and not g_4[:3].any() and not loss_4[:3].any()


# ---- 4. the occluder freeze past its first instance group
@pytest.fixture(scope='module')
def occ():
    eng = make_engine(ec.model(ec.OCC_NV))
    x = ec.occ_params()
    xe = x.copy()
    xe[:, 82:85] += ec.OCC_SHIFT
    cams5, pc = ec.occ_cameras()
    eng.set_problems(cams5, np.zeros((ec.OCC_N, 5, 17, 2), np.float32), np.zeros((ec.OCC_N, 5, 17), np.float32))
    verts, verts_e = eng.vertices(x)[0], eng.vertices(xe)[0]
    # the masks: per image the pixels where its body is the visible one of the twelve (the modal body_id render)
    everyone = list(range(ec.OCC_N))
    _, bid = eng.render_scene(verts, None, np.zeros((ec.OCC_M, ec.OCC_H, ec.OCC_W, 3), np.uint8), [everyone] * ec.OCC_M,
                              ec.OCC_VIEW, body_id=True)
    masks = (bid == torch.as_tensor(ec.OCC_BODY, device=bid.device, dtype=bid.dtype)[:, None, None]).to(torch.uint8)
    faces = np.asarray(ec.model(ec.OCC_NV)['faces'])
    w = dict(eng=eng, verts=verts, verts_e=verts_e, pc=pc, masks=masks, faces=faces, prep=so.prepare(_np(masks), 1))
    w['z_occ'], w['z_own'] = oo.freeze(_np(verts), faces, ec.OCC_BODY, pc, ec.OCC_SCENE, ec.OCC_H, ec.OCC_W)
    w['flags'] = oo.point_flags(_np(masks), w['prep']['first'], w['prep']['xy'], w['z_occ'], w['z_own'])
    yield w
    eng.close()


def _freeze(w, images=slice(None)):
    eng = w['eng']
    eng.set_silhouettes(w['masks'][images], ec.OCC_BODY[images], tuple(a[images] for a in w['pc']))
    eng.set_silhouette_occluders(w['verts'], ec.OCC_SCENE, margin=ec.OCC_MARGIN)
    return tuple(_np(t) for t in eng.silhouette_occluders())


def test_576_instances_freeze_as_the_oracle_does(occ):
    eng, first = occ['eng'], occ['prep']['first']
    assert len(ec.instances(ec.OCC_BODY, ec.OCC_SCENE)) == 576
    z_occ, z_own, flag = _freeze(occ)
    assert np.array_equal(_np(eng.silhouettes()[2]), occ['prep']['xy'])
    hidden = _np(eng.silhouette_hidden(occ['verts_e']))
    r_hidden = oo.hidden_bytes(_np(occ['verts_e']), ec.OCC_BODY, occ['pc'], occ['z_occ'], ec.OCC_MARGIN)
    print('contour per image %s\nflagged per image %s\nhidden per image %s'
          % (np.diff(first).tolist(), [int(occ['flags'][first[i]:first[i + 1]].sum()) for i in range(ec.OCC_M)],
             r_hidden.sum(1).tolist()))
    for i in range(ec.OCC_M):
        assert np.array_equal(_bits(z_occ[i]), _bits(occ['z_occ'][i])), i
        assert np.array_equal(_bits(z_own[i]), _bits(occ['z_own'][i])), i
    assert np.array_equal(flag, occ['flags'])
    assert np.array_equal(hidden, r_hidden)
    # the world reaches both groups: the straddling image 42 and the close-up images behind it
    assert occ['flags'].any() and not occ['flags'].all()
    assert r_hidden[42].any() and r_hidden[:42].any() and r_hidden[43:].any()
    assert occ['flags'][:first[42]].any() and occ['flags'][first[43]:].any()
    assert np.isfinite(occ['z_occ'][43:]).any() and np.isfinite(occ['z_own'][43:]).any()
    # a re-freeze returns the same bytes
    eng.set_silhouette_occluders(occ['verts'], ec.OCC_SCENE, margin=ec.OCC_MARGIN)
    again = tuple(_np(t) for t in eng.silhouette_occluders())
    assert np.array_equal(_bits(again[0]), _bits(z_occ)) and np.array_equal(_bits(again[1]), _bits(z_own))
    assert np.array_equal(again[2], flag)


def test_two_passes_give_what_the_halves_give_in_one_pass_each(occ):
    first = occ['prep']['first']
    z_occ, z_own, flag = _freeze(occ)
    for lo, hi in ((0, 24), (24, 48)):
        assert len(ec.instances(ec.OCC_BODY[lo:hi], ec.OCC_SCENE)) == 288
        h_occ, h_own, h_flag = _freeze(occ, slice(lo, hi))
        assert np.array_equal(_bits(h_occ), _bits(z_occ[lo:hi])) and np.array_equal(_bits(h_own), _bits(z_own[lo:hi]))
        assert np.array_equal(h_flag, flag[first[lo]:first[hi]]) and h_flag.any()


@pytest.mark.parametrize('sigma', [0.0, 20.0])
def test_the_occluded_search_with_an_odd_tile_against_the_oracle(occ, sigma):
    eng = occ['eng']
    ref = oo.occluded(_np(occ['masks']), 1, _np(occ['verts']), occ['faces'], ec.OCC_BODY, occ['pc'], ec.OCC_SCENE, ec.OCC_MARGIN,
                      eval_vertices=_np(occ['verts_e']), sigma=sigma)
    assert (ref['winner'] == -2).any() and (ref['winner'] >= 0).any() and ref['hidden'].any()
    _freeze(occ)
    _check(eng, occ['verts_e'], ref, 'occluded 701 sigma %g' % sigma, sigma=sigma)


# ---- 5. the gated instantiations at the same edges
def _stage(w):
    return dict(stage_weights(1536.0)[3], coll_loss_weight=float(w))


def test_closure_adds_w2_L_at_the_chunk_and_tile_edges():
    sigma = 20.0
    cams = _ring()
    x = ec.params()
    x_true = x.copy()
    x_true[:, 0:10] = np.random.default_rng(5).normal(0, 1.0, (ec.N, 10)).astype(np.float32)
    x_true[:, 82:85] -= np.float32([0.03, -0.02, 0.04])
    eng = make_engine(ec.model(NV))
    try:
        eng.set_problems(cams, np.zeros((ec.N, V4, 17, 2), np.float32), np.zeros((ec.N, V4, 17), np.float32))
        gt, conf = syn.make_observations(_np(eng.vertices(x_true)[1]), cams, seed=3)
        eng.set_problems(cams, gt, conf)
        eng.set_silhouettes(ec.exact_count_masks(), ec.IMAGE_BODY, ec.arc_cameras())
        verts = eng.vertices(x)[0]
        L, g = eng.silhouette_loss(verts, sigma=sigma)
        L_ref, g_ref = _np(L).astype(np.float64), _np(eng.vertices_backward(x, grad_verts=g)).astype(np.float64)
        data = float(eng.closure(x, _stage(0.0), want_grad=False)['loss'][ec.BIG_BODY])
        w = float(np.sqrt(data / L_ref[ec.BIG_BODY]))
        eng.set_silhouette_term(sigma=sigma)
        o1 = eng.closure(x, _stage(w), want_grad=True)
        S = _np(eng.sdf_term_read()[1])
        o0 = eng.closure(x, _stage(0.0), want_grad=True)
        loss1, loss0 = _np(o1['loss']), _np(o0['loss'])
        grad1, grad0 = _np(o1['grad']), _np(o0['grad'])
        for j in (0, 2):
            pen, pen_ref = float(loss1[j]) - float(loss0[j]), w * w * L_ref[j]
            gp = grad1[j].astype(np.float64) - grad0[j].astype(np.float64)
            gp_ref = w * w * g_ref[j]
            e_s = abs(float(S[j]) - L_ref[j]) / L_ref[j]
            e_g = np.abs(gp - gp_ref).max() / np.abs(gp_ref).max()
            print('EDGE gated problem %d: w %.4g L %.7g ref %.7g rel %.2e | pen %.7g ref %.7g (loss %.7g) | '
                  'grad err/max %.2e (max %.4g)'
                  % (j, w, S[j], L_ref[j], e_s, pen, pen_ref, loss1[j], e_g, np.abs(gp_ref).max()))
            assert L_ref[j] > 0
            assert e_s <= 1e-5
            assert abs(pen - pen_ref) <= LOSS_RTOL * float(loss1[j])
            assert e_g <= GRAD_TOL
        assert S[1] == 0 and np.array_equal(loss1[1], loss0[1]) and np.array_equal(grad1[1], grad0[1])
    finally:
        eng.close()
