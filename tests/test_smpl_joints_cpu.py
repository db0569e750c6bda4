"""CPU: the skeleton-keypoint model kind (model_type 'smpl', pose_format 'coco17') on the host side - the synthetic model,
model_arrays on the reference's own 'smpl' module, the pose-format / model-kind check of the batch driver - and the
float64 restatement tests/smpl_oracle.py against the reference goldens it stands in for on the GPU tests."""
import os

import numpy as np
import pytest

from mvsmplfitting_amd import batch
from mvsmplfitting_amd import synthetic as syn
from oracle import closure_np as cn
from tests.helpers import CASES, GOLD, body_model
from tests.smpl_oracle import SmplClosureOracle

DATA = os.path.join(GOLD, 'demo_data')


def test_synthetic_smpl_model():
    m = syn.make_body_model(0, model_type='smpl')
    lsp = syn.make_body_model(0)
    assert m['kp_regressor'] is None
    # smpl_to_annotation('smpl', 'coco17') (reference code/utils/utils.py:444-449)
    assert np.array_equal(m['joint_map'], [24, 25, 26, 27, 28, 16, 17, 18, 19, 20, 21, 1, 2, 4, 5, 7, 8])
    assert np.array_equal(syn.COCO17_JOINT_WEIGHTS, [1] * 11 + [0, 0] + [1] * 4)
    for k in ('v_template', 'shapedirs', 'posedirs', 'J_regressor', 'parents', 'lbs_weights', 'face_vertex_ids', 'faces'):
        assert np.array_equal(m[k], lsp[k]), k
    with pytest.raises(ValueError):
        syn.make_body_model(0, model_type='smplx')
    with pytest.raises(ValueError):
        syn.make_body_model(0, model_type='smpl', kp_regressor=syn.make_lsp_regressor())


@pytest.mark.parametrize('name', ['l2_s0_v8', 'l2_top4_v8', 'gmm_s2_v8', 'vp_s0_v8', 'l2_3d_v8', 'l2_angle_drop_v8'])
def test_float64_restatement_matches_reference_goldens(name):
    cfg = CASES[name]
    g = dict(np.load(os.path.join(GOLD, 'closure_smpl_%s.npz' % name)))
    model = syn.make_body_model(0, skin_topk=cfg.get('skin_topk'), model_type='smpl')
    assert abs(syn.model_checksum(model) - float(g['model_checksum'])) < 1e-6 * float(g['model_checksum'])
    vpw = syn.make_vposer_decoder(**cfg['vp']) if cfg['use_vposer'] else None
    gmm = syn.gmm_constants(syn.make_gmm(), np.float64) if cfg['prior'] == 'gmm' else None
    orc = SmplClosureOracle(model, vposer=vpw, gmm=gmm)
    cams = (g['cam_R'], g['cam_t'], g['cam_f'], g['cam_c'])
    w = dict(zip(['data_weight', 'body_pose_weight', 'shape_weight', 'bending_prior_weight', 'rho'], g['wts']))
    prior = cn.PRIOR_GMM if cfg['prior'] == 'gmm' else cn.PRIOR_L2
    for b in range(g['x'].shape[0]):
        j3 = (g['joints3d'][b][:, :3], g['joints3d'][b][:, 3]) if 'joints3d' in g else None
        L, G, o = orc.closure(g['x'][b], cams, g['gt_xy'][b], g['conf'][b], w, use_vposer=cfg['use_vposer'], prior=prior,
                              joints3d=j3)
        assert abs(L - g['loss64'][b]) <= 1e-12 * abs(g['loss64'][b])
        assert np.abs(G - g['grad64'][b]).max() <= 1e-12 * np.abs(g['grad64'][b]).max()
        assert np.abs(o['joints'] - g['joints64'][b]).max() < 1e-12


def test_skeleton_joints_are_not_a_regression_of_the_posed_vertices():
    """Why the keypoints need their own forward: J_regressor . posed vertices misses the posed joints away from zero pose,
    and equals them at zero pose (what init_guess.py:41-44 takes: the rest keypoints)."""
    m = syn.make_body_model(0, model_type='smpl')
    orc = SmplClosureOracle(m)
    p = dict(betas=np.zeros(10), global_orient=np.zeros(3), body_pose=np.zeros(69), transl=np.zeros(3), scale=1.3,
             use_vposer=False)
    o = orc.body(p)
    sk = orc.kp_joint >= 0
    assert np.abs((orc.JR @ o['vertices'])[orc.kp_joint[sk]] - o['joints'][sk]).max() < 1e-6       # (float32 rows sum to 1 to rounding)
    p['body_pose'] = np.random.default_rng(0).normal(0, 0.3, 69)
    o = orc.body(p)
    assert np.abs((orc.JR @ o['vertices'])[orc.kp_joint[sk]] - o['joints'][sk]).max() > 1e-3


def test_model_arrays_of_the_reference_smpl_module():
    from oracle import ref_import as ri
    if not ri.available():
        pytest.skip('reference tree not present')
    import torch
    from mvsmplfitting_amd import fitting
    sys_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools')
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_golden_smpl_coco17', os.path.join(sys_path, 'make_golden_smpl_coco17.py'))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    model = syn.make_body_model(0, model_type='smpl')
    smpl = mg.smpl_module(model, 'float32', False)
    assert not hasattr(smpl, 'joint_regressor')
    arr = fitting.model_arrays(smpl)
    assert arr['kp_regressor'] is None
    assert np.array_equal(arr['joint_map'], model['joint_map'])
    assert np.array_equal(arr['face_vertex_ids'], model['face_vertex_ids'])
    for k in ('v_template', 'J_regressor', 'lbs_weights', 'shapedirs', 'posedirs'):
        assert np.array_equal(arr[k], model[k]), k
    assert isinstance(smpl.v_template, torch.Tensor)


@pytest.mark.parametrize('fmt,kind', [('lsp14', 'smpl'), ('coco17', 'smpllsp'), ('coco25', 'smpl')])
def test_fit_folder_rejects_a_format_the_model_kind_does_not_map(fmt, kind, tmp_path):
    model = syn.make_body_model(0, model_type='smpl') if kind == 'smpl' else body_model()
    with pytest.raises(ValueError):
        batch.fit_folder(model, os.path.join(DATA, 'keypoints'), os.path.join(DATA, '3DOH50K_Parameters.txt'),
                         str(tmp_path / 'r'), pose_format=fmt)
    assert not (tmp_path / 'r').exists()
