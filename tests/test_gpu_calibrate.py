"""GPU: calibrate.refine_rig on a synthetic capture - a ring of 4 cameras, 8 frames, 2 px noise, views 1-3 turned by about a
degree and moved by about 3 % of the ring's radius; the start point is the staged fit under the wrong rig.  The accept rule, the
anchor, a forced rejected sweep, the refusals; and the closure's data term against the sum of the views' energies."""
import numpy as np
import pytest
import torch

from mvsmplfitting_amd import _lib, calibrate
from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import MvFit, pack_cameras, stage_weights, unpack_cameras
from oracle import closure_np as cn
from tests import camera_refine_oracle as co
from tests.helpers import body_model

pytestmark = pytest.mark.gpu
B, V, RADIUS = 8, 4, 4.0


@pytest.fixture(scope='module')
def capture():
    model = body_model()
    cams = syn.make_camera_ring(V, radius=RADIUS)
    orc = cn.ClosureOracle(model, np.float64)
    fr = syn.make_frames(B, seed0=40)
    kp = np.stack([orc.body(dict({k: fr[k][b] for k in fr}, use_vposer=False), want_cache=False)['joints'] for b in range(B)])
    gt, conf = syn.make_observations(kp, cams, seed=7, noise_px=2.0)
    true = pack_cameras(cams)
    rng = np.random.default_rng(21)
    wrong = true.copy()
    for v in range(1, V):
        ax, sh = rng.normal(size=3), rng.normal(size=3)
        d = np.concatenate([ax * np.deg2rad(1.0) / np.linalg.norm(ax), sh * 0.03 * RADIUS / np.linalg.norm(sh), np.zeros(3)])
        wrong[v] = co.step(true[v], d)
    wrong = pack_cameras(unpack_cameras(wrong, np.float32))               # a rig as a camera file in float32 would give it
    stages = stage_weights(1536.0)
    eng = MvFit(model)
    eng.set_problems(unpack_cameras(wrong, np.float32), gt, conf)
    x0 = np.zeros((B, 118), np.float32)
    x0[:, 85] = 1.0
    xf, _ = eng.fit(x0, stages)
    yield dict(eng=eng, gt=gt, conf=conf, true=true, wrong=wrong, stage=stages[-1], xf=xf)
    eng.close()


def _rig_errors(c15, true):
    R, t, _, _ = unpack_cameras(c15)
    Rt, tt, _, _ = unpack_cameras(true)
    centre = np.array([np.linalg.norm(-R[v].T @ t[v] + Rt[v].T @ tt[v]) for v in range(1, len(R))])
    angle = np.array([co.rot_angle(R[v], Rt[v]) for v in range(1, len(R))])
    return centre.mean(), np.rad2deg(angle.mean())


def test_sweeps_lower_the_energy_and_keep_the_anchor(capture):
    c = capture
    x, cams, rep = calibrate.refine_rig(c['eng'], c['xf'], c['stage'], c['wrong'], c['gt'], c['conf'], sweeps=3, anchor=0)
    E = [rep['E0']] + [s['E'] for s in rep['sweeps']]
    before, after = _rig_errors(c['wrong'], c['true']), _rig_errors(cams, c['true'])
    print('E: %s, accepted %s' % (E, [s['accepted'] for s in rep['sweeps']]))
    print('mean camera-centre error of views 1-3: %.4f -> %.4f m; mean rotation error %.3f -> %.3f degrees' % (before[0], after[0], before[1], after[1]))
    print('statuses of the last sweep %s, iterations %s' % (rep['sweeps'][-1]['report'][:, 4], rep['sweeps'][-1]['report'][:, 2]))
    assert rep['sweeps'][0]['accepted']
    assert all(b <= a for a, b in zip(E, E[1:])) and E[-1] < E[0]
    assert np.array_equal(cams[0].view(np.uint64), c['wrong'][0].view(np.uint64))
    assert rep['sweeps'][0]['report'][0, 4] == 3 and (rep['sweeps'][0]['report'][1:, 4] != 3).all()
    assert rep['loss'].shape == (B,) and abs(rep['loss'].sum() - E[-1]) <= 1e-9 * E[-1]
    assert x.shape == (B, 118) and np.array_equal(x.cpu().numpy(), rep['sweeps'][-1]['params'])
    assert np.array_equal(cams, rep['sweeps'][-1]['cams']) and rep['sweeps'][-1]['n_closure'].shape == (B,)
    # the engine holds the returned rig
    loss = c['eng'].closure(x, c['stage'], want_grad=False)['loss'].cpu().numpy().astype(np.float64)
    assert np.array_equal(loss, rep['loss'])
    # anchor=None: every view moves
    x2, cams2, rep2 = calibrate.refine_rig(c['eng'], c['xf'], c['stage'], c['wrong'], c['gt'], c['conf'], sweeps=1, anchor=None)
    assert (rep2['sweeps'][0]['report'][:, 4] != 3).all() and rep2['sweeps'][0]['E'] <= rep2['E0']


def test_a_rejected_sweep_changes_nothing(capture, monkeypatch):
    c = capture
    eng = c['eng']
    eng.set_problems(unpack_cameras(c['wrong'], np.float32), c['gt'], c['conf'])
    loss0 = eng.closure(c['xf'], c['stage'], want_grad=False)['loss'].cpu().numpy()

    def worse(params, stages, **kw):
        return torch.as_tensor(params).to(eng.device) + 0.3, dict(n_closure=torch.zeros(B, dtype=torch.int32))
    monkeypatch.setattr(eng, 'fit', worse)
    x, cams, rep = calibrate.refine_rig(eng, c['xf'], c['stage'], c['wrong'], c['gt'], c['conf'], sweeps=3, anchor=0)
    assert len(rep['sweeps']) == 1 and not rep['sweeps'][0]['accepted'] and rep['sweeps'][0]['E'] == rep['E0']
    assert np.array_equal(x.cpu().numpy().view(np.uint32), c['xf'].cpu().numpy().view(np.uint32))
    assert np.array_equal(cams.view(np.uint64), c['wrong'].view(np.uint64))
    assert np.array_equal(eng.closure(c['xf'], c['stage'], want_grad=False)['loss'].cpu().numpy(), loss0)


def test_refusals(capture):
    c = capture
    with pytest.raises(ValueError, match='F_USE_3D'):
        calibrate.refine_rig(c['eng'], c['xf'], dict(c['stage'], flags=_lib.F_USE_3D), c['wrong'], c['gt'], c['conf'])
    R, t, f, cc = unpack_cameras(c['wrong'], np.float32)
    per_problem = tuple(np.tile(a[None], (B,) + (1,) * a.ndim) for a in (R, t, f, cc))
    with pytest.raises(ValueError, match='per-problem'):
        calibrate.refine_rig(c['eng'], c['xf'], c['stage'], per_problem, c['gt'], c['conf'])


def test_data_term_is_the_sum_of_the_views(capture):
    """With every prior weight 0 and no VPoser the closure loss is the data term alone: sum_b loss = sum_v E_v to 1e-5
    relative, the project's loss tolerance for the float32 closure."""
    c = capture
    eng = c['eng']
    eng.set_problems(unpack_cameras(c['wrong'], np.float32), c['gt'], c['conf'])
    stage = dict(data_weight=500.0 / 1536.0, body_pose_weight=0.0, shape_weight=0.0, bending_prior_weight=0.0, rho=100.0, flags=0)
    out = eng.closure(c['xf'], stage, want_grad=False, want_joints=True)
    total = float(out['loss'].cpu().numpy().astype(np.float64).sum())
    E = eng.camera_normal_eqs(out['joints'], c['wrong'], rho=100.0, data_weight=stage['data_weight'], need_grad=False)['E']
    views = float(E.cpu().numpy().sum())
    print('sum_b loss %.9e, sum_v E_v %.9e, relative %.2e' % (total, views, abs(total - views) / views))
    assert abs(total - views) <= 1e-5 * views
