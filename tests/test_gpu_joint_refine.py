"""GPU: joint_refine.refine_joint - scene collision, silhouettes and temporal smoothing in ONE fit per sweep - on 2 persons x 3
frames x 4 views of the full body model: a 384 x 512 camera ring, keypoints with 2 px noise, masks rendered from the truth,
the persons 0.25 m apart.  Start: the staged keypoint fit of every (frame, person) on its own.

The comparison: the three single refinements run one after another from the same start (scene_fit.refine_scenes, then
silhouette.refine_fit, then temporal.smooth_sequences), each with the weight that gives its term the factor it has in the
mix (a single term adds w_k^2 * term, so w_k = w sqrt(share_k)).  Weights, chosen once from the terms' magnitudes at a keypoint
fit so that each weighs about as much as the data term (~1e3) and not tuned afterwards: S_sc^2 and L_sil ~1e4 there (w^2 share
~0.05 .. 0.1), L_vt ~ 6890 vertices x (1 cm)^2 ~ 1 (w^2 share ~ 500): w = 0.3, shares 0.5 / 1 / 5000.

Measured on an MI355X (sums over the six problems, everything frozen at the point):
                 keypoint fit   joint     in a row: after scene   after silhouettes   after temporal
    sum S_sc^2   822542         438381    0                       753437              771386
    sum L_sil    227297         68510.7   3.03527e+06             10718.5             217934
    sum L_vt     90.468         19.9302   94.8008                 84.6943             0.700904
    joint E      79094          35065                                                 56928.5
Each single refinement is best at its own component right after it ran and is undone by the next one: in a row, only the last
term (temporal) ends low, 28 times below the joint fit's, while the joint fit ends 1.8 and 3.2 times below on the other two.
"No worse than 1.05 x in every component" therefore does not hold for the component refined last, and the assertions are the
energy statements: E never rises, a sweep is accepted, and the joint energy of the joint result is below that of the three
fits in a row."""
import numpy as np
import pytest
import torch

from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import MvFit, pack_params, stage_weights
from mvsmplfitting_amd.joint_refine import refine_joint
from mvsmplfitting_amd.scene_fit import refine_scenes
from mvsmplfitting_amd.silhouette import refine_fit
from mvsmplfitting_amd.temporal import smooth_sequences
from tests.helpers import body_model

pytestmark = pytest.mark.gpu

V, F, P = 4, 3, 2
N = F * P                                           # frame-major: problem n = f * P + p
SIZES = [P] * F
PERSON, FRAME = np.tile(np.arange(P), F), np.repeat(np.arange(F), P)
W = 0.3
SHARES = dict(scene=0.5, silhouette=1.0, temporal=5000.0)
SCENE_KW = dict(grid_size=32, scale_factor=0.2, robustifier=0.05)


def _np(t):
    return t.detach().cpu().numpy()


def _cams():
    R, t, f, c = syn.make_camera_ring(V, radius=4.0)
    Wd, Hd = 512, 384
    f = (f * np.float32(Wd / 2048.0)).astype(np.float32)
    c = np.tile(np.array([Wd / 2.0, Hd / 2.0], np.float32), (V, 1))
    return (R, t, f, c), Hd, Wd


def _truth():
    """A smooth motion: each person's pose and position drift a little from frame to frame."""
    x = np.zeros((F, P, 118), np.float32)
    for p in range(P):
        fr = syn.make_frames(1, seed0=900 + p)
        x0 = pack_params(B=1, **fr)[0]
        drift = np.random.default_rng(950 + p).normal(0, 0.02, 72).astype(np.float32)
        for f in range(F):
            x[f, p] = x0
            x[f, p, 10:82] += f * drift
            x[f, p, 82:85] = (0.25 * p - 0.125 + 0.02 * f, 0.0, 0.01 * f)
    return x.reshape(N, 118)


def _stage(w):
    return dict(stage_weights(1536.0)[-1], coll_loss_weight=float(w))


@pytest.fixture(scope='module')
def world():
    eng = MvFit(body_model())
    cams, H, Wd = _cams()
    x_true = _truth()
    eng.set_problems(cams, np.zeros((N, V, 17, 2), np.float32), np.zeros((N, V, 17), np.float32))
    v_true, joints = eng.vertices(x_true)
    gt, conf = syn.make_observations(_np(joints), cams, seed=3)
    eng.set_problems(cams, gt, conf)
    prob, view = np.repeat(np.arange(N), V).astype(np.int32), np.tile(np.arange(V), N).astype(np.int32)
    _, fid = eng.render_overlay(v_true, None, np.zeros((N * V, H, Wd, 3), np.uint8), prob, view, face_id=True)
    masks = (fid >= 0).to(torch.uint8)
    per_image = tuple(a[view] for a in cams)
    x0 = x_true.copy()
    x0[:, 0:10] = 0.0
    x0[:, 10:82] = 0.0
    x0[:, 82:85] += np.array([0.03, -0.02, 0.04], np.float32)
    x_kp, _ = eng.fit(x0, stage_weights(1536.0))
    yield dict(eng=eng, x_kp=x_kp, mask_set=(masks, prob, per_image))
    eng.close()


def _components(eng, x):
    """The three unweighted components at x, everything frozen at x, summed over the problems: [sum S_sc^2, sum L_sil, sum
    L_vt]; and the joint energy there."""
    x, rep = refine_joint(eng, x, _stage(W), shares=SHARES, scene_sizes=SIZES, seq_id=PERSON, frame_idx=FRAME, sweeps=0, **SCENE_KW)
    return rep['parts0'].sum(axis=0), float(rep['E0'].sum())


def test_one_fit_with_three_terms_against_three_fits_in_a_row(world):
    eng, x_kp = world['eng'], world['x_kp']
    eng.set_silhouettes(*world['mask_set'])
    try:
        start, E_start = _components(eng, x_kp)
        xj, rep = refine_joint(eng, x_kp, _stage(W), shares=SHARES, scene_sizes=SIZES, seq_id=PERSON, frame_idx=FRAME, sweeps=3,
                               **SCENE_KW)
        assert rep['group'].tolist() == [0] * N                       # the tracks link the three scenes
        E = [rep['E0']] + [sw['E'] for sw in rep['sweeps']]
        print('joint: E %s, accepted %s, closures %s' % ([float(e[0]) for e in E], [sw['accepted'].tolist() for sw in rep['sweeps']],
                                                        [int(sw['n_closure'].max()) for sw in rep['sweeps']]))
        for a, b in zip(E, E[1:]):
            assert (b <= a).all()
        assert any(sw['accepted'].any() for sw in rep['sweeps'])
        assert E[-1][0] < E[0][0]
        joint, E_joint = _components(eng, xj)
        # the three single refinements, one after another, from the same start
        xs, _ = refine_scenes(eng, x_kp, SIZES, _stage(W * np.sqrt(SHARES['scene'])), sweeps=3, **SCENE_KW)
        after_scene, _ = _components(eng, xs)
        xs, _ = refine_fit(eng, xs, _stage(W * np.sqrt(SHARES['silhouette'])))
        after_sil, _ = _components(eng, xs)
        xs, _ = smooth_sequences(eng, xs, _stage(W * np.sqrt(SHARES['temporal'])), PERSON, FRAME, sweeps=3)
        serial, E_serial = _components(eng, xs)
    finally:
        eng.clear_silhouettes()
    names = ('sum S_sc^2', 'sum L_sil', 'sum L_vt')
    for k, name in enumerate(names):
        print('%-11s keypoint fit %.6g | joint %.6g | in a row: after scene %.6g, after silhouettes %.6g, after temporal %.6g'
              % (name, start[k], joint[k], after_scene[k], after_sil[k], serial[k]))
    print('joint energy: keypoint fit %.6g | joint %.6g | in a row %.6g' % (E_start, E_joint, E_serial))
    assert E_start == float(E[0][0]) and E_joint == float(E[-1][0])           # (the report's own numbers, re-evaluated)
    assert E_joint < E_serial
    assert (joint < start).all()                                              # every component fell from the keypoint fit's
