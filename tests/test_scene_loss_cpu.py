"""CPU: SceneSDFLoss (mvsmplfitting_amd/scene_loss.py) over a stand-in engine built on the restatement
(tests/scene_sdf_oracle.py:OracleEngine): gradient routing, per-scene scaling, dtype handling, argument checks."""
import numpy as np
import pytest
import torch

from mvsmplfitting_amd.scene_loss import SceneSDFLoss
from tests import scene_sdf_cases as sc
from tests import scene_sdf_oracle as so


def _module(c, eng=None):
    return SceneSDFLoss(c['faces'], grid_size=c['grid_size'], robustifier=c['robustifier'], engine=eng or so.OracleEngine())


def test_one_scene_gives_a_scalar_and_the_translation_gradient_is_the_row_sum_of_the_vertex_gradient():
    c = sc.case('a')
    eng = so.OracleEngine()
    v = torch.tensor(c['vertices'], requires_grad=True)
    t = torch.tensor(c['translation'], requires_grad=True)
    loss = _module(c, eng)(v, t, scale_factor=c['scale_factor'])
    assert loss.dim() == 0
    loss.backward()
    sc.check(c, loss.item(), v.grad.numpy(), t.grad.numpy())
    assert torch.allclose(t.grad, v.grad.sum(dim=1), rtol=1e-5, atol=1e-7)
    assert eng.calls == [dict(sizes=(3,), grid_size=16, scale_factor=0.2, robustifier=None)]


def test_scene_sizes_give_one_loss_per_scene_and_grad_out_scales_each_scenes_bodies():
    c = sc.case('a')
    v = torch.tensor(np.concatenate([c['vertices'][:1], c['vertices'], c['vertices'][:2]]), requires_grad=True)
    t = torch.tensor(np.concatenate([c['translation'][:1], c['translation'], c['translation'][:2]]), requires_grad=True)
    loss = _module(c)(v, t, scene_sizes=[1, 3, 2])
    assert tuple(loss.shape) == (3,) and loss[0].item() == 0.0 and loss[1].item() == pytest.approx(c['loss'], rel=1e-5)
    w = torch.tensor([5.0, 2.0, -3.0])
    (loss * w).sum().backward()
    assert not v.grad[0].any() and not t.grad[0].any()
    assert np.abs(v.grad[1:4].numpy() - 2.0 * c['g_vertices']).max() <= 2.0 * sc.GRAD_TOL * c['g_max']
    pair = so.scene_loss(c['vertices'][:2], c['translation'][:2], c['faces'], 16, 0.2, None, sdf=so.OracleEngine().sdf)
    assert np.abs(v.grad[4:].numpy() + 3.0 * pair['g_vertices']).max() <= 1e-5 * np.abs(pair['g_vertices']).max() * 3.0
    assert np.abs(t.grad[4:].numpy() + 3.0 * pair['g_translation']).max() <= 1e-5 * np.abs(pair['g_translation']).max() * 3.0


def test_a_single_body_gives_zero_loss_and_zero_gradients():
    c = sc.case('a')
    v = torch.tensor(c['vertices'][:1], requires_grad=True)
    t = torch.tensor(c['translation'][:1], requires_grad=True)
    loss = _module(c)(v, t)
    loss.backward()
    assert loss.item() == 0.0 and not v.grad.any() and not t.grad.any()


def test_float64_inputs_get_float64_gradients():
    c = sc.case('a')
    v = torch.tensor(c['vertices'], dtype=torch.float64, requires_grad=True)
    t = torch.tensor(c['translation'], dtype=torch.float64, requires_grad=True)
    _module(c)(v, t).backward()
    assert v.grad.dtype == torch.float64 and t.grad.dtype == torch.float64
    sc.check(c, c['loss'], v.grad.numpy(), t.grad.numpy())


def test_arguments_are_validated():
    c = sc.case('a')
    m = _module(c)
    v, t = torch.tensor(c['vertices']), torch.tensor(c['translation'])
    for sizes in ([2, 2], [3, 0], [], [4, -1]):
        with pytest.raises(ValueError):
            m(v, t, scene_sizes=sizes)
    with pytest.raises(ValueError):
        m(v, t[:2])
    with pytest.raises(ValueError):
        m(v[0], t)
    with pytest.raises(ValueError):
        SceneSDFLoss(c['faces'].reshape(-1), engine=so.OracleEngine())
    with pytest.raises(ValueError):
        SceneSDFLoss(c['faces'])
