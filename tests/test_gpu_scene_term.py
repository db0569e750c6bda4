"""GPU: the collision term of a fit against frozen obstacles (mvfit_set_scene_obstacles; scene_sdf.hip:
scene_entries_kernel -> sdf_term.hip: sdf_pullback_kernel) at the closure level.

Two scenes of sizes (2, 3) of full bodies with small random shape and pose, 4 views, G = 32, robustifier 0.05, weight 1.
Scene 1's pair is offset by golden case d's translation (0.13, 0.02, 0.07) - both bodies reach into the other's field; scene
2 is the same pair plus a third body 3 m away, which must get exactly zero.  The references: MvFit.scene_sdf_loss (itself
checked against the reference's SDFLoss in tests/test_gpu_scene_sdf.py) at the freeze point, the NumPy restatement
tests/scene_sdf_oracle.py on the stored fields away from it; gradients go through MvFit.vertices_backward.  Bounds: the
project's own (tests/scene_sdf_cases.py) - LOSS_RTOL = 1e-5, GRAD_TOL = 2e-4 of max; fields and independence bit for bit."""
import numpy as np
import pytest
import torch

from mvsmplfitting_amd import _lib
from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import MvFitError, stage_weights
from tests import scene_sdf_oracle as so
from tests.gpu_helpers import make_engine
from tests.helpers import body_model
from tests.scene_sdf_cases import GRAD_TOL, LOSS_RTOL

pytestmark = pytest.mark.gpu

V, G, ROB, SF, W = 4, 32, 0.05, 0.2, 1.0
SIZES = (2, 3)
OFFSET = np.array([0.13, 0.02, 0.07], np.float32)         # golden case d's translation
KW = dict(grid_size=G, scale_factor=SF, robustifier=ROB)


def _np(t):
    return t.detach().cpu().numpy()


def _params():
    """x[5,118]: bodies 0, 1 = the pair; 2, 3 = the same pair; 4 = a body 3 m away."""
    rng = np.random.default_rng(77)
    pair = np.zeros((2, 118), np.float32)
    pair[:, 0:10] = rng.normal(0, 0.3, (2, 10))
    pair[:, 10:82] = rng.normal(0, 0.05, (2, 72))
    pair[:, 85] = 1.0
    pair[1, 82:85] = OFFSET
    far = np.zeros((1, 118), np.float32)
    far[:, 0:10] = rng.normal(0, 0.3, (1, 10))
    far[:, 10:82] = rng.normal(0, 0.05, (1, 72))
    far[:, 85] = 1.0
    far[0, 82:85] = (3.0, 0.0, 0.0)
    return np.concatenate([pair, pair, far]).astype(np.float32)


def _stage(w=W, flags=0):
    return dict(stage_weights(1536.0, flags=flags)[3], coll_loss_weight=w)


def _problems(eng, x, cams, flags=0):
    """Observations of the bodies at x (noisy projections of their keypoints); leaves the problems set."""
    B = x.shape[0]
    eng.set_problems(cams, np.zeros((B, V, 17, 2), np.float32), np.zeros((B, V, 17), np.float32))
    _, joints = eng.vertices(x, flags=flags)
    gt, conf = syn.make_observations(_np(joints), cams, seed=3)
    eng.set_problems(cams, gt, conf)
    return gt, conf


def _evaluate(eng, x, flags=0):
    """closure with the term (and its sums), closure without it."""
    o1 = eng.closure(x, _stage(flags=flags), want_grad=True, want_verts=True)
    smp, S = eng.sdf_term_read()
    assert smp is None
    o0 = eng.closure(x, _stage(0.0, flags=flags), want_grad=True)
    f64 = lambda t: _np(t).astype(np.float64)
    return dict(loss=f64(o1['loss']), grad=f64(o1['grad']), verts=_np(o1['verts']), S=_np(S), loss0=f64(o0['loss']),
                grad0=f64(o0['grad']), loss_bits=_np(o1['loss']), grad_bits=_np(o1['grad']), loss0_bits=_np(o0['loss']),
                grad0_bits=_np(o0['grad']))


@pytest.fixture(scope='module')
def world():
    """The engine with the five problems set, the obstacles frozen at their vertices, and the op's own numbers there."""
    model = body_model()
    cams = syn.make_camera_ring(V)
    eng = make_engine(model)
    x = _params()
    gt, conf = _problems(eng, x, cams)
    v0, _ = eng.vertices(x)
    loss_op, g_op, phi_op = eng.scene_sdf_loss(v0, model['faces'], scene_sizes=SIZES, return_phi=True, **KW)
    eng.set_scene_obstacles(v0, SIZES, **KW)
    at = _evaluate(eng, x)
    yield dict(eng=eng, model=model, cams=cams, x=x, gt=gt, conf=conf, v0=v0, loss_op=_np(loss_op).astype(np.float64),
               g_op=g_op, phi_op=_np(phi_op), at=at)
    eng.close()


def _check_term(r, rows, S_ref, g_ref):
    """Problems ``rows`` of an evaluation r against S_ref[j] and the pulled-back d S_j / d params g_ref[j] (float64)."""
    for j in rows:
        pen, pen_ref = r['loss'][j] - r['loss0'][j], (W * S_ref[j]) ** 2
        gp, gp_ref = r['grad'][j] - r['grad0'][j], 2.0 * W * W * S_ref[j] * g_ref[j]
        e_s = abs(r['S'][j] - S_ref[j]) / max(abs(S_ref[j]), 1e-30)
        e_g = np.abs(gp - gp_ref).max() / max(np.abs(gp_ref).max(), 1e-30)
        print('problem %d: S %.7g ref %.7g rel %.2e | pen %.7g ref %.7g (loss %.7g) | grad err/max %.2e (max %.4g)'
              % (j, r['S'][j], S_ref[j], e_s, pen, pen_ref, r['loss'][j], e_g, np.abs(gp_ref).max()))
        assert S_ref[j] > 0, 'the case does not exercise the term'
        assert e_s <= LOSS_RTOL
        assert abs(pen - pen_ref) <= LOSS_RTOL * r['loss'][j]
        assert e_g <= GRAD_TOL


def test_frozen_fields_are_the_ops_fields_bit_for_bit(world):
    eng = world['eng']
    phi, box = eng.scene_obstacles()
    assert tuple(phi.shape) == (5, G, G, G)
    assert np.array_equal(_np(phi), world['phi_op']), np.count_nonzero(_np(phi) != world['phi_op'])
    assert np.count_nonzero(world['phi_op']) > 0
    c, s = so.boxes(_np(world['v0']), SF)
    assert np.array_equal(_np(box)[:, :3], c) and np.array_equal(_np(box)[:, 3], s)
    # a re-freeze at the same vertices changes nothing
    eng.set_scene_obstacles(world['v0'], SIZES, **KW)
    again = _evaluate(eng, world['x'])
    for k in ('S', 'loss_bits', 'grad_bits'):
        assert np.array_equal(again[k], world['at'][k]), k


def test_at_the_freeze_point_the_term_is_the_ops_loss_and_gradient(world):
    eng, at = world['eng'], world['at']
    first = np.concatenate([[0], np.cumsum(SIZES)])
    for s, P in enumerate(SIZES):
        total = at['S'][first[s]:first[s + 1]].astype(np.float64).sum() / P ** 2
        print('scene %d: sum S / P^2 = %.7g, op %.7g' % (s, total, world['loss_op'][s]))
        assert world['loss_op'][s] > 0
        assert abs(total - world['loss_op'][s]) <= LOSS_RTOL * world['loss_op'][s]
    # each problem: pen_j = (w S_j)^2, and d S_j / d v_j = P^2 g_op[j] pulled back through the body
    pp = torch.tensor([4.0, 4.0, 9.0, 9.0, 9.0], device=eng.device)[:, None, None]
    g_ref = _np(eng.vertices_backward(world['x'], grad_verts=world['g_op'] * pp)).astype(np.float64)
    c, sc_ = so.boxes(_np(world['v0']), SF)
    S_ref = _oracle_S(world, at['verts'], c, sc_)[0]                # each S_j on its own: the restatement on the op's fields
    _check_term(at, [0, 1, 2, 3], S_ref, g_ref)


def _oracle_S(world, verts, c, s):
    """S_j and d S_j / d v_j [5,Nv,3] (float64) from the stored fields and the boxes (c, s) of the freeze vertices."""
    first = np.concatenate([[0], np.cumsum(SIZES)])
    S, dS = np.zeros(5), np.zeros(verts.shape, np.float64)
    for sidx in range(len(SIZES)):
        for j in range(first[sidx], first[sidx + 1]):
            for i in range(first[sidx], first[sidx + 1]):
                if i == j:
                    continue
                p, dp = so.sample(world['phi_op'][i], so.local_coords(verts[j], c[i], s[i]))
                dp = dp / np.float64(s[i])
                q = p / ROB
                fr = q * q
                dp = dp * (2.0 * q / ROB / (fr + 1.0) ** 2)[:, None]
                S[j] += (fr / (fr + 1.0)).sum()
                dS[j] += dp
    return S, dS


def test_away_from_the_freeze_point_the_term_samples_the_frozen_fields(world):
    eng = world['eng']
    x = world['x'].copy()
    x[1, 82:85] += np.array([0.02, 0.0, 0.0], np.float32)           # body 1: 2 cm, and a perturbed pose
    x[1, 13:82] += np.random.default_rng(5).normal(0, 0.02, 69).astype(np.float32)
    eng.set_scene_obstacles(world['v0'], SIZES, **KW)
    r = _evaluate(eng, x)
    c, s = so.boxes(_np(world['v0']), SF)
    S_ref, dS = _oracle_S(world, r['verts'], c, s)
    g_ref = _np(eng.vertices_backward(x, grad_verts=torch.tensor(dS, dtype=torch.float32))).astype(np.float64)
    assert S_ref[1] != pytest.approx(float(world['at']['S'][1]), rel=1e-3), 'the move changes the term'
    _check_term(r, [0, 1, 2, 3], S_ref, g_ref)
    # the obstacles did not move: body 0 still samples body 1's field where it was frozen
    assert r['S'][0] == world['at']['S'][0] and np.array_equal(r['grad_bits'][0], world['at']['grad_bits'][0])


def test_a_body_out_of_reach_pays_exactly_nothing(world):
    at = world['at']
    assert at['S'][4] == 0.0
    assert np.array_equal(at['loss_bits'][4], at['loss0_bits'][4]) and np.array_equal(at['grad_bits'][4], at['grad0_bits'][4])
    # and the pair next to it pays what the same pair pays alone (their observations differ, the term does not)
    assert np.array_equal(at['S'][2:4], at['S'][0:2])


def test_a_scenes_numbers_do_not_depend_on_the_batch(world):
    eng, at = world['eng'], world['at']
    try:
        # alone, B = 2
        eng.set_problems(world['cams'], world['gt'][:2], world['conf'][:2])
        v, _ = eng.vertices(world['x'][:2])
        eng.set_scene_obstacles(v, [2], **KW)
        alone = _evaluate(eng, world['x'][:2])
        # as the second scene of a B = 5 call
        order = [2, 3, 4, 0, 1]
        eng.set_problems(world['cams'], world['gt'][order], world['conf'][order])
        v, _ = eng.vertices(world['x'][order])
        eng.set_scene_obstacles(v, [3, 2], **KW)
        second = _evaluate(eng, world['x'][order])
        for k in ('S', 'loss_bits', 'grad_bits'):
            assert np.array_equal(alone[k], at[k][:2]), k
            assert np.array_equal(second[k][3:5], at[k][:2]), k
    finally:
        eng.set_problems(world['cams'], world['gt'], world['conf'])
        eng.set_scene_obstacles(world['v0'], SIZES, **KW)


def test_contract(world):
    eng, x = world['eng'], world['x']
    faces = world['model']['faces']
    try:
        with pytest.raises(MvFitError, match='error -1: mvfit_set_scene_obstacles'):
            eng.set_scene_obstacles(world['v0'], [2, 2], **KW)             # sizes that do not add up to B
        eng.closure(x, _stage(), want_grad=False)                          # a refused call changes nothing: the obstacles stand
        assert np.array_equal(_np(eng.sdf_term_read()[1]), world['at']['S'])
        with pytest.raises(MvFitError, match='error -3: mvfit_set_sdf'):
            eng.set_sdf(faces, num_faces=1, grid_size=32)
        with pytest.raises(MvFitError, match='error -4'):                  # samples: not kept by the scene term
            eng._check(eng._lib.mvfit_sdf_term_read(eng._ctx, torch.empty(5, eng.nv, 4, device=eng.device).data_ptr(), None))
        eng.clear_scene_obstacles()
        with pytest.raises(MvFitError, match='error -3'):                  # neither term
            eng.closure(x, _stage())
        with pytest.raises(MvFitError, match='error -3'):
            eng.fit(x, [_stage()])
        eng.set_sdf(faces, num_faces=1, grid_size=32)
        with pytest.raises(MvFitError, match='error -3: mvfit_set_scene_obstacles'):
            eng.set_scene_obstacles(world['v0'], SIZES, **KW)
        eng.set_sdf(None)
        # another B clears the obstacles
        eng.set_scene_obstacles(world['v0'], SIZES, **KW)
        eng.closure(x, _stage())
        eng.set_problems(world['cams'], world['gt'][:2], world['conf'][:2])
        with pytest.raises(MvFitError, match='error -3'):
            eng.closure(x[:2], _stage())
    finally:
        eng.set_sdf(None)
        eng.set_problems(world['cams'], world['gt'], world['conf'])
        eng.set_scene_obstacles(world['v0'], SIZES, **KW)


def test_with_vposer_the_terms_gradient_lands_in_the_embedding(world):
    model, cams = world['model'], world['cams']
    flags = _lib.F_VPOSER
    eng = make_engine(model, vpw=syn.make_vposer_decoder())
    try:
        x = world['x'][:2].copy()
        x[:, 13:82] = 0.0
        x[:, 86:118] = np.random.default_rng(9).normal(0, 0.3, (2, 32)).astype(np.float32)
        _problems(eng, x, cams, flags=flags)
        v, _ = eng.vertices(x, flags=flags)
        _, g_op, _ = eng.scene_sdf_loss(v, model['faces'], scene_sizes=[2], **KW)
        eng.set_scene_obstacles(v, [2], **KW)
        r = _evaluate(eng, x, flags=flags)
        g_ref = _np(eng.vertices_backward(x, grad_verts=g_op * 4.0, flags=flags)).astype(np.float64)
        for j in range(2):
            gp, gp_ref = r['grad'][j] - r['grad0'][j], 2.0 * W * W * float(r['S'][j]) * g_ref[j]
            print('problem %d: S %.7g, embedding gradient max %.4g, err/max %.2e'
                  % (j, r['S'][j], np.abs(gp_ref[86:118]).max(), np.abs(gp - gp_ref).max() / np.abs(gp_ref).max()))
            assert r['S'][j] > 0 and np.abs(gp_ref[86:118]).max() > 0
            assert not np.any(gp[13:82]), 'body_pose is not optimised with VPoser'
            assert np.abs(gp - gp_ref).max() <= GRAD_TOL * np.abs(gp_ref).max()
    finally:
        eng.close()
