"""GPU: the skeleton-keypoint model (model_type 'smpl', pose_format 'coco17'; include/mvfit.h: kp_regressor NULL) - 12 of the
17 keypoints are posed skeleton joints (the translation column of the chained transforms, + transl), 5 are face vertices.
Against the reference's own 'smpl' module (goldens of tools/make_golden_smpl_coco17.py) and the float64 restatement of
tests/smpl_oracle.py, through every path that contains the closure."""
import os

import numpy as np
import pytest

from mvsmplfitting_amd import _lib
from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import MvFitError, stage_weights as eng_stage_weights
from oracle import closure_np as cn
from tests.gpu_helpers import flags_for, from118, make_engine, to118
from tests.helpers import CASES, GOLD, stage_weights
from tests.smpl_oracle import SmplClosureOracle

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-5
VERT_ATOL = 1e-4
GRAD_RTOL = 2e-4
SMPL_CASES = ['l2_s0_v8', 'l2_top4_v8', 'gmm_s2_v8', 'vp_s0_v8', 'l2_3d_v8', 'l2_angle_drop_v8']


def smpl_model(skin_topk=None):
    return syn.make_body_model(0, skin_topk=skin_topk, model_type='smpl')


def load_smpl_case(name):
    cfg = CASES[name]
    g = dict(np.load(os.path.join(GOLD, 'closure_smpl_%s.npz' % name)))
    model = smpl_model(cfg.get('skin_topk'))
    assert abs(syn.model_checksum(model) - float(g['model_checksum'])) < 1e-6 * float(g['model_checksum'])
    vpw = syn.make_vposer_decoder(**cfg['vp']) if cfg['use_vposer'] else None
    gmm = syn.make_gmm() if cfg['prior'] == 'gmm' else None
    w = g['wts']
    wts = dict(data_weight=float(w[0]), body_pose_weight=float(w[1]), shape_weight=float(w[2]),
               bending_prior_weight=float(w[3]), rho=float(w[4]))
    return cfg, g, model, vpw, gmm, wts, (g['cam_R'], g['cam_t'], g['cam_f'], g['cam_c'])


# 1 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sparse', [False, True])
@pytest.mark.parametrize('name', SMPL_CASES)
def test_smpl_closure_matches_reference_golden(name, sparse):
    cfg, g, model, vpw, gmm, wts, cams = load_smpl_case(name)
    eng = make_engine(model, vpw, gmm)
    B = g['x'].shape[0]
    eng.set_problems(cams, g['gt_xy'], g['conf'])
    if 'joints3d' in g:
        eng.set_joints3d(g['joints3d'][:, :, :3], g['joints3d'][:, :, 3])
    x = np.stack([to118(g['x'][b], cfg['use_vposer']) for b in range(B)]).astype(np.float32)
    out = eng.closure(x, dict(wts, flags=flags_for(cfg) | (_lib.F_SPARSE_VERTS if sparse else 0)),
                      want_grad=True, want_verts=True, want_joints=True)
    loss = out['loss'].cpu().numpy().astype(np.float64)
    grad = out['grad'].cpu().numpy().astype(np.float64)
    joints = out['joints'].cpu().numpy().astype(np.float64)
    assert np.all(np.abs(loss - g['loss64']) <= LOSS_RTOL * np.abs(g['loss64'])), (loss, g['loss64'])
    assert np.abs(joints - g['joints64']).max() < VERT_ATOL
    if not sparse:
        verts = out['verts'].cpu().numpy().astype(np.float64)
        assert np.abs(verts[:2] - g['verts64_as32']).max() < VERT_ATOL
    for b in range(B):
        gm, gr = from118(grad[b], cfg['use_vposer']), g['grad64'][b]
        assert np.abs(gm - gr).max() <= GRAD_RTOL * np.abs(gr).max(), (name, b, np.abs(gm - gr).max(), np.abs(gr).max())
    eng.close()


# 2 ----------------------------------------------------------------------------------------------------------------------
def test_smpl_closure_batch32_against_float64_restatement():
    """32 frames x 8 views; loss / gradient / keypoints / vertices vs tests/smpl_oracle.py (checked against the goldens on
    the CPU: tests/test_smpl_joints_cpu.py)."""
    model = smpl_model()
    cams = syn.make_camera_ring(8)
    orc = SmplClosureOracle(model)
    B = 32
    fr = syn.make_frames(B, seed0=1000)
    kps = np.asarray([orc.body(dict({k: fr[k][b] for k in fr}, use_vposer=False), want_cache=False)['joints'] for b in range(B)])
    gt, conf = syn.make_observations(kps, cams, seed=99)
    conf = conf * syn.COCO17_JOINT_WEIGHTS
    rng = np.random.default_rng(17)
    x86 = rng.normal(0, 0.15, (B, 86))
    x86[:, 85] = 1.0 + rng.normal(0, 0.05, B)
    x = np.stack([to118(x86[b], False) for b in range(B)]).astype(np.float32)
    wts = stage_weights(2)
    eng = make_engine(model)
    eng.set_problems(cams, gt, conf)
    ref = [orc.closure(x[b, :86].astype(np.float64), cams, gt[b], conf[b], wts) for b in range(B)]
    for sparse in (False, True):
        out = eng.closure(x, dict(wts, flags=_lib.F_SPARSE_VERTS if sparse else 0), want_verts=True, want_joints=True)
        loss = out['loss'].cpu().numpy().astype(np.float64)
        grad = out['grad'].cpu().numpy().astype(np.float64)
        joints = out['joints'].cpu().numpy().astype(np.float64)
        for b in range(B):
            L, g, o = ref[b]
            assert abs(loss[b] - L) <= LOSS_RTOL * abs(L), (sparse, b, loss[b], L)
            assert np.abs(joints[b] - o['joints']).max() < VERT_ATOL
            assert np.abs(grad[b, :86] - g).max() <= GRAD_RTOL * np.abs(g).max(), (sparse, b)
            if not sparse:
                assert np.abs(out['verts'][b].cpu().numpy() - o['vertices']).max() < VERT_ATOL
    eng.close()


# 3 ----------------------------------------------------------------------------------------------------------------------
def test_smpl_vertices_joints_match_golden():
    """mvfit_vertices: the skeleton keypoints from the skinning transforms of the pose block, the face keypoints from the
    vertex buffer."""
    cfg, g, model, vpw, gmm, wts, cams = load_smpl_case('l2_s0_v8')
    eng = make_engine(model)
    B = g['x'].shape[0]
    eng.set_problems(cams, g['gt_xy'], g['conf'])
    x = np.stack([to118(g['x'][b], False) for b in range(B)]).astype(np.float32)
    verts, joints = eng.vertices(x)
    assert np.abs(joints.cpu().numpy().astype(np.float64) - g['joints64']).max() < VERT_ATOL
    assert np.abs(verts.cpu().numpy()[:2].astype(np.float64) - g['verts64_as32']).max() < VERT_ATOL
    eng.close()


# 4 ----------------------------------------------------------------------------------------------------------------------
N_STEP = 35


def tol(k, n=N_STEP, lo=2e-5, hi=3e-3):
    return lo * (hi / lo) ** (min(k, n - 1) / (n - 1))


@pytest.mark.parametrize('sparse', [False, True])
def test_smpl_fit_follows_reference_fp32_trajectory(sparse):
    g = dict(np.load(os.path.join(GOLD, 'fit_smpl_l2.npz')))
    eng = make_engine(smpl_model())
    B = g['x0'].shape[0]
    eng.set_problems((g['cam_R'], g['cam_t'], g['cam_f'], g['cam_c']), g['gt_xy'], g['conf'])
    x0 = np.stack([to118(g['x0'][b], False) for b in range(B)]).astype(np.float32)
    stages = eng_stage_weights(1536.0, flags=_lib.F_SPARSE_VERTS if sparse else 0)
    tr = eng.fit_trace(120)
    xf, st = eng.fit(x0, stages)
    tr = tr.cpu().numpy().astype(np.float64)
    eng.fit_trace(0)
    final = st['final_loss'].cpu().numpy().astype(np.float64)
    for b in range(B):
        n = min(N_STEP, int(g['ncl32'][b][0]), int(g['ncl'][b][0]))
        worst = 0.0
        for k in range(n):
            ex = np.abs(from118(tr[b, k, :118], False) - g['trace32'][b][k, :-1]).max()
            el = abs(tr[b, k, 118] - g['trace32'][b][k, -1]) / abs(g['trace32'][b][k, -1])
            worst = max(worst, ex / tol(k), el / tol(k))
        assert worst <= 1.0, (b, worst)
        assert final[b] <= 1.05 * max(float(g['final'][b]), float(g['final32'][b])), (b, final[b])
    eng.close()


# 5, 6 -------------------------------------------------------------------------------------------------------------------
def _async_setup(B, skin_topk=4, **options):
    g = dict(np.load(os.path.join(GOLD, 'fit_smpl_l2.npz')))
    eng = make_engine(smpl_model(skin_topk), **options)
    rng = np.random.default_rng(3)
    gt = np.repeat(g['gt_xy'][:1], B, 0) + rng.normal(0, 3.0, (B,) + g['gt_xy'].shape[1:]).astype(np.float32)
    eng.set_problems((g['cam_R'], g['cam_t'], g['cam_f'], g['cam_c']), gt, np.repeat(g['conf'][:1], B, 0))
    x0 = np.zeros((B, 118), np.float32)
    x0[:, 85] = 1.0
    x0[:, :86] += rng.normal(0, 0.02, (B, 86)).astype(np.float32)
    return eng, x0


@pytest.mark.parametrize('resident', [-1, 0])
def test_smpl_async_fit_equals_objective_vertices_only_fit(resident):
    eng, x0 = _async_setup(33)
    eng.set_options(resident_pass=resident)
    xa, sa = eng.fit(x0, eng_stage_weights(1536.0, flags=0))
    xs, ss = eng.fit(x0, eng_stage_weights(1536.0, flags=_lib.F_SPARSE_VERTS))
    assert sa['passes']['run'] > 0 and ss['passes']['run'] == 0
    assert sa['passes']['missed'] == 0 and sa['passes']['timed_out'] == 0, sa['passes']
    assert np.array_equal(xa.cpu().numpy(), xs.cpu().numpy())
    assert np.array_equal(sa['final_loss'].cpu().numpy(), ss['final_loss'].cpu().numpy())
    assert np.array_equal(sa['n_closure'].cpu().numpy(), ss['n_closure'].cpu().numpy())
    assert np.isfinite(sa['final_loss'].cpu().numpy()).all()
    eng.close()


def test_smpl_chained_rounds_end_on_the_fits_of_the_single_launch():
    eng, x0 = _async_setup(16)
    stages = eng_stage_weights(1536.0, flags=0)
    xa, sa = eng.fit(x0, stages)
    eng.set_options(round_mode=1)
    xc, sc = eng.fit(x0, stages)
    assert sc['passes'] == dict(run=0, skipped=0, missed=0, timed_out=0)
    fa, fc = sa['final_loss'].cpu().numpy().astype(np.float64), sc['final_loss'].cpu().numpy().astype(np.float64)
    na, nc = sa['n_closure'].cpu().numpy(), sc['n_closure'].cpu().numpy()
    rel = np.abs(fa - fc) / np.abs(fc)
    assert np.isfinite(fa).all() and np.isfinite(fc).all()
    assert np.median(rel) <= 2e-3 and rel.max() <= 5e-2, rel
    assert 0.7 * nc.sum() <= na.sum() <= 1.3 * nc.sum(), (na, nc)
    eng.close()


# 7 ----------------------------------------------------------------------------------------------------------------------
def test_smpl_work_queue_equals_sub_batches_at_160():
    res = {}
    for wq in (1, 0):
        eng, x0 = _async_setup(160, work_queue=wq)
        xf, st = eng.fit(x0, eng_stage_weights(1536.0, flags=0))
        assert st['passes']['run'] > 0 and st['passes']['missed'] == 0 and st['passes']['timed_out'] == 0, st['passes']
        res[wq] = (xf.cpu().numpy(), st['n_closure'].cpu().numpy(), st['final_loss'].cpu().numpy())
        eng.close()
    for k in range(3):
        assert np.array_equal(res[1][k], res[0][k]), k
    assert np.isfinite(res[1][2]).all()


# 8 ----------------------------------------------------------------------------------------------------------------------
def test_smpl_vposer_and_sdf_fits_end_finite():
    g = dict(np.load(os.path.join(GOLD, 'fit_smpl_l2.npz')))
    cams = (g['cam_R'], g['cam_t'], g['cam_f'], g['cam_c'])
    model = smpl_model(4)
    x0 = np.zeros((2, 118), np.float32)
    x0[:, 85] = 1.0
    eng = make_engine(model, syn.make_vposer_decoder())
    eng.set_problems(cams, g['gt_xy'], g['conf'])
    xf, st = eng.fit(x0, eng_stage_weights(1536.0, flags=_lib.F_VPOSER))
    assert np.isfinite(st['final_loss'].cpu().numpy()).all() and np.isfinite(xf.cpu().numpy()).all()
    eng.close()
    eng = make_engine(model)
    eng.set_problems(cams, g['gt_xy'], g['conf'])
    eng.set_sdf(model['faces'], num_faces=1, grid_size=32)
    xf, st = eng.fit(x0, eng_stage_weights(1536.0, coll_w=[0.0, 0.0, 0.01, 0.05]))
    assert np.isfinite(st['final_loss'].cpu().numpy()).all() and np.isfinite(xf.cpu().numpy()).all()
    eng.close()


# 9 ----------------------------------------------------------------------------------------------------------------------
def test_smpl_hip_keypoints_with_zero_weight_do_not_change_the_closure():
    cfg, g, model, vpw, gmm, wts, cams = load_smpl_case('l2_s0_v8')
    assert np.all(g['conf'][:, :, 11:13] == 0.0)                  # the COCO-17 joint weights (data_parser.py:353-356)
    eng = make_engine(model)
    B = g['x'].shape[0]
    x = np.stack([to118(g['x'][b], False) for b in range(B)]).astype(np.float32)
    outs = []
    for shift in (0.0, 57.0):
        gt = g['gt_xy'].copy()
        gt[:, :, 11:13] += shift
        eng.set_problems(cams, gt, g['conf'])
        o = eng.closure(x, dict(wts, flags=0), want_grad=True)
        outs.append((o['loss'].cpu().numpy(), o['grad'].cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    eng.close()


def test_smpl_fit_folder_coco17_on_the_demo(tmp_path):
    from mvsmplfitting_amd import batch
    data = os.path.join(GOLD, 'demo_data')
    out = batch.fit_folder(smpl_model(4), os.path.join(data, 'keypoints'), os.path.join(data, '3DOH50K_Parameters.txt'),
                           str(tmp_path / 'results'), pose_format='coco17')
    assert out
    for serial, r in out.items():
        assert all(os.path.isfile(f) for f in r['files']) and len(r['files']) == len(r['frames'])
        assert np.isfinite(r['final_loss']).all()


def test_smpl_rest_keypoints_and_init_guess_match_reference():
    """init_guess.py:41-44 takes J_regressor . rest vertices for 'smpl'; the engine's rest keypoints are the posed joints
    at zero pose - the same points (the regressor's rows sum to 1) to rounding, hence the reference's initial guess."""
    from mvsmplfitting_amd import init_guess as ig
    gd = dict(np.load(os.path.join(GOLD, 'demo_fit_smpl.npz')))
    ref = dict(np.load(os.path.join(GOLD, 'init_guess_smpl_ref.npz')))
    model = smpl_model()
    eng = make_engine(model)
    kp6 = gd['keypoints'].reshape(6, 17, 3).astype(np.float32)
    for name in ('views6', 'views3', 'views6_fixscale', 'single0'):
        v = list(ref[name + '/views'])
        fs = float(ref[name + '/fixed_scale'])
        eng.set_problems((gd['cam_R'][v], gd['cam_t'][v], gd['cam_f'][v], gd['cam_c'][v]),
                         kp6[v][None, :, :, :2], kp6[v][None, :, :, 2])
        out = ig.init_guess_batch(eng, gd['extris'][v], gd['intris'][v], kp6[v][None], est_scale=fs < 0,
                                  fixed_scale=None if fs < 0 else fs)
        assert np.abs(out['transl'][0].cpu().numpy() - ref[name + '/transl']).max() < 1e-4 * max(1.0, np.abs(ref[name + '/transl']).max()), name
        assert np.abs(out['global_orient'][0].cpu().numpy() - ref[name + '/global_orient']).max() < 1e-4, name
        assert abs(float(out['scale'][0]) - float(ref[name + '/scale'])) < 1e-4 * abs(float(ref[name + '/scale'])), name
    eng.close()


# 10 ---------------------------------------------------------------------------------------------------------------------
def test_joint_map_range_is_checked_in_both_modes():
    bad = dict(smpl_model(), joint_map=syn.COCO17_JOINT_MAP.copy())
    bad['joint_map'][3] = 29
    with pytest.raises(MvFitError):
        make_engine(bad)
    ok = dict(smpl_model(), joint_map=syn.COCO17_JOINT_MAP.copy())
    ok['joint_map'][3] = 28
    make_engine(ok).close()
    lsp = syn.make_body_model(0)
    bad = dict(lsp, joint_map=syn.LSP_JOINT_MAP.copy())
    bad['joint_map'][3] = 19
    with pytest.raises(MvFitError):
        make_engine(bad)
