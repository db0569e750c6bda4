"""GPU: SceneSDFLoss (mvsmplfitting_amd/scene_loss.py) composed with BodyLayer - the collision loss between two bodies
reaches shape, pose and translation, with the gradients mvfit_vertices_backward gives when fed the op's g_vertices."""
import numpy as np
import pytest
import torch

from mvsmplfitting_amd.layer import BodyLayer
from mvsmplfitting_amd.scene_loss import SceneSDFLoss
from tests.helpers import body_model

pytestmark = pytest.mark.gpu


def test_collision_loss_between_two_bodies_reaches_shape_pose_and_translation():
    model = body_model()
    layer = BodyLayer(model)
    eng, dev = layer.engine, layer.engine.device
    coll = SceneSDFLoss(model['faces'], grid_size=32, robustifier=0.05, engine=eng)
    rng = np.random.default_rng(3)
    leaf = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev, requires_grad=True)
    betas, orient = leaf(rng.normal(0, 0.5, (2, 10))), leaf(rng.normal(0, 0.05, (2, 3)))
    pose, transl = leaf(rng.normal(0, 0.05, (2, 69))), leaf([[0.0, 0.0, 0.0], [0.14, 0.03, 0.06]])
    out = layer(betas, orient, pose)
    loss = coll(out.vertices, transl)
    assert loss.dim() == 0 and float(loss.detach()) > 0
    loss.backward()
    # the same numbers from the two ops
    v = (out.vertices.detach() + transl.detach()[:, None]).contiguous()
    l_op, g_op, _ = eng.scene_sdf_loss(v, model['faces'], grid_size=32, robustifier=0.05)
    assert float(l_op[0]) == float(loss.detach()) and g_op.abs().max() > 0
    x = torch.cat([betas, orient, pose, torch.zeros(2, 3, device=dev), torch.ones(2, 1, device=dev),
                   torch.zeros(2, 32, device=dev)], dim=1).detach().contiguous()
    gx = eng.vertices_backward(x, g_op)
    assert torch.equal(betas.grad, gx[:, 0:10]) and betas.grad.abs().max() > 0
    assert torch.equal(orient.grad, gx[:, 10:13])
    assert torch.equal(pose.grad, gx[:, 13:82]) and pose.grad.abs().max() > 0
    gt = g_op.sum(dim=1)
    assert (transl.grad - gt).abs().max() <= 1e-5 * gt.abs().max() and gt.abs().max() > 0
    # one small step against the translation gradient lowers the loss
    with torch.no_grad():
        t2 = transl - 1e-3 * transl.grad / transl.grad.norm()
        lower = coll(out.vertices.detach(), t2)
    print('loss %.7g -> %.7g' % (float(loss.detach()), float(lower)))
    assert float(lower) < float(loss.detach())
    eng.close()
