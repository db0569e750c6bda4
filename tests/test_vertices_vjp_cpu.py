"""CPU: the goldens of mvfit_vertices_backward (tests/golden/vertices_vjp_ref.npz, the reference's own float64 autograd
through its body module, tools/make_golden_vjp.py) against the float64 hand-derived VJP the GPU tests use
(tests/vjp_helpers.py: the closure oracle's adjoint with every loss weight 0) - which ties that oracle to the reference -
and BodyLayer's packing and gradient routing on a CPU stand-in engine (tests/layer_stand_in.py)."""
import os

import numpy as np
import pytest
import torch

from mvsmplfitting_amd import _lib
from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.layer import BodyLayer, ModelOutput
from tests import vjp_helpers as vh
from tests.helpers import GOLD
from tests.layer_stand_in import LinearEngine

ORACLE_RTOL = 1e-10


def _gold():
    return dict(np.load(os.path.join(GOLD, 'vertices_vjp_ref.npz')))


@pytest.mark.parametrize('name', sorted(vh.CONFIGS))
def test_golden_vjp_matches_the_float64_oracle(name):
    g = _gold()
    cfg = vh.CONFIGS[name]
    model, vpw = vh.model_for(cfg), vh.vposer_for(cfg)
    assert abs(syn.model_checksum(model) - float(g['model_checksum_' + name])) < 1e-6 * float(g['model_checksum_' + name])
    assert int(g[name + '/seed']) == cfg['seed']
    xs = g[name + '/x'].astype(np.float64)
    np.testing.assert_array_equal(xs, vh.random_points(cfg['seed'], vh.B_GOLD, cfg['vposer']))
    orc = vh.VjpOracle(model, vpw)
    for mode in vh.MODES:
        gv, gj = vh.cotangents(cfg['seed'], vh.B_GOLD, model['v_template'].shape[0], mode)
        ck = float(g['%s/checksum_%s' % (name, mode)])
        assert abs(vh.cotangent_checksum(gv, gj) - ck) <= 1e-12 * ck, 'regenerated cotangents drifted'
        ref = g['%s/grad64_%s' % (name, mode)]
        for b in range(vh.B_GOLD):
            mine = orc.vjp(xs[b], None if gv is None else gv[b], None if gj is None else gj[b], cfg['vposer'])
            err = np.abs(mine - ref[b]).max()
            assert err <= ORACLE_RTOL * np.abs(ref[b]).max(), (name, mode, b, err)


def test_golden_file_is_small():
    assert os.path.getsize(os.path.join(GOLD, 'vertices_vjp_ref.npz')) < 256 * 1024


# ---------------------------------------------------------------------------------------------------------------- layer
def _inputs(B, dtype=torch.float32, seed=0):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=dtype).requires_grad_(True)
    return dict(betas=r(B, 10), global_orient=r(B, 3), body_pose=r(B, 69), transl=r(B, 3), scale=r(B, 1))


def test_layer_output_shapes_and_fields():
    eng = LinearEngine()
    layer = BodyLayer(None, engine=eng)
    inp = _inputs(4)
    out = layer(**inp, return_full_pose=True)
    assert isinstance(out, ModelOutput)
    assert out._fields == ('vertices', 'joints', 'full_pose', 'betas', 'global_orient', 'body_pose')
    assert tuple(out.vertices.shape) == (4, 5, 3) and tuple(out.joints.shape) == (4, 17, 3)
    assert tuple(out.full_pose.shape) == (4, 72)
    assert out.betas is inp['betas'] and out.global_orient is inp['global_orient'] and out.body_pose is inp['body_pose']
    torch.testing.assert_close(out.full_pose, torch.cat([inp['global_orient'], inp['body_pose']], 1), rtol=0, atol=0)
    assert layer(**inp).full_pose is None
    x = eng.last_x
    for name, (a, b) in dict(betas=(0, 10), global_orient=(10, 13), body_pose=(13, 82), transl=(82, 85), scale=(85, 86)).items():
        torch.testing.assert_close(x[:, a:b], inp[name].detach(), rtol=0, atol=0)
    assert torch.all(x[:, 86:] == 0) and eng.last_flags == 0


def test_layer_routes_each_slot_of_the_flat_gradient_to_its_input():
    eng = LinearEngine()
    layer = BodyLayer(None, engine=eng)
    inp = _inputs(3, dtype=torch.float64, seed=1)
    out = layer(**inp, return_full_pose=True)
    gen = torch.Generator().manual_seed(7)
    Wv = torch.randn(3, 5, 3, generator=gen, dtype=torch.float32)
    Wj = torch.randn(3, 17, 3, generator=gen, dtype=torch.float32)
    ((out.vertices * Wv).sum() + (out.joints * Wj).sum()).backward()
    g = (Wv.reshape(3, -1) @ eng.Mv + Wj.reshape(3, -1) @ eng.Mj).double()
    for name, (a, b) in dict(betas=(0, 10), global_orient=(10, 13), body_pose=(13, 82), transl=(82, 85), scale=(85, 86)).items():
        assert inp[name].grad.dtype == torch.float64, name
        torch.testing.assert_close(inp[name].grad, g[:, a:b], rtol=1e-6, atol=1e-5)
    assert eng.backward_calls == [(True, True, 0)]


def test_layer_full_pose_is_differentiable_without_vposer():
    eng = LinearEngine()
    layer = BodyLayer(None, engine=eng)
    inp = _inputs(2, seed=3)
    out = layer(**inp, return_full_pose=True)
    out.full_pose.sum().backward()
    assert torch.all(inp['global_orient'].grad == 1) and torch.all(inp['body_pose'].grad == 1)
    assert eng.backward_calls == []                 # nothing flowed into the vertices node


def test_layer_defaults_and_only_joints_cotangent():
    eng = LinearEngine()
    layer = BodyLayer(None, engine=eng)
    betas = torch.randn(2, 10, requires_grad=True)
    go = torch.randn(2, 3, requires_grad=True)
    bp = torch.randn(2, 69)
    out = layer(betas, go, bp)
    x = eng.last_x
    assert torch.all(x[:, 82:85] == 0) and torch.all(x[:, 85] == 1) and torch.all(x[:, 86:] == 0)
    out.joints.sum().backward()
    assert eng.backward_calls == [(False, True, 0)]
    g = torch.ones(2, 51) @ eng.Mj
    torch.testing.assert_close(betas.grad, g[:, 0:10])
    torch.testing.assert_close(go.grad, g[:, 10:13])


def test_layer_vposer_slots():
    eng = LinearEngine()
    layer = BodyLayer(None, engine=eng)
    z = torch.randn(3, 32, requires_grad=True)
    betas = torch.randn(3, 10, requires_grad=True)
    go = torch.randn(3, 3, requires_grad=True)
    out = layer(betas, go, pose_embedding=z, scale=torch.full((3,), 1.5), return_full_pose=True)
    x = eng.last_x
    assert eng.last_flags == _lib.F_VPOSER
    assert torch.all(x[:, 13:82] == 0) and torch.all(x[:, 85] == 1.5)
    torch.testing.assert_close(x[:, 86:118], z.detach(), rtol=0, atol=0)
    # body_pose / full_pose: the decoded pose, no gradient
    dec = eng.full_pose(x)
    torch.testing.assert_close(out.full_pose, dec, rtol=0, atol=0)
    torch.testing.assert_close(out.body_pose, dec[:, 3:], rtol=0, atol=0)
    assert not out.body_pose.requires_grad and not out.full_pose.requires_grad
    out.vertices.sum().backward()
    g = torch.ones(3, 15) @ eng.Mv
    torch.testing.assert_close(z.grad, g[:, 86:118])
    torch.testing.assert_close(betas.grad, g[:, 0:10])
    assert eng.backward_calls == [(True, False, _lib.F_VPOSER)]


def test_layer_sets_problems_only_when_the_batch_changes():
    eng = LinearEngine()
    layer = BodyLayer(None, engine=eng)
    for B in (2, 2, 5, 5, 2):
        layer(**_inputs(B))
    assert eng.set_problems_calls == [2, 5, 2]


def test_layer_rejects_an_embedding_without_vposer():
    layer = BodyLayer(None, engine=LinearEngine(has_vposer=False))
    with pytest.raises(ValueError):
        layer(torch.zeros(1, 10), torch.zeros(1, 3), pose_embedding=torch.zeros(1, 32))
