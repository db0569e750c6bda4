"""The scene collision loss between fitted bodies as a differentiable PyTorch module: the reference's multi-person
interpenetration loss (SDFLoss, reference sdf/sdf/sdf_loss.py:7-99) on the HIP kernels (include/mvfit.h:mvfit_scene_sdf_loss).

It composes with the differentiable body model:

    layer = BodyLayer(model_arrays)
    coll = SceneSDFLoss(model_arrays['faces'], grid_size=32, robustifier=0.05, engine=layer.engine)
    out = layer(betas, global_orient, body_pose)                 # the P bodies of one scene, without translation
    loss = coll(out.vertices, transl)
    loss.backward()                       # -> betas.grad, global_orient.grad, body_pose.grad, transl.grad

``vertices + translation[:, None]`` is done in torch, so autograd produces the translation gradient (the row sums of the
vertex gradient) and casts gradients back to the inputs' dtype and device; one autograd node maps the translated vertices to
the loss.  The forward call already computes the gradient and the node keeps it; backward scales it by the scene's incoming
gradient.  Once differentiable: there is no double backward.

Semantics (as the unmodified reference executes): every body of a scene is kept - the reference's isolation filter is a
bitwise complement of a uint8 mask and never removes one - and the divisor is P^2; a scene of one body gives 0.
"""
from __future__ import annotations

import numpy as np
import torch
from torch.autograd.function import once_differentiable


class SceneSDFFunction(torch.autograd.Function):
    """v[N,Nv,3] float32 (translation added) -> loss[S] on module's engine; backward = grad_out[scene of body] * g_vertices."""

    @staticmethod
    def forward(ctx, v, module, scale_factor, sizes):
        loss, g, _ = module.engine.scene_sdf_loss(v.detach(), module.faces, scene_sizes=sizes, grid_size=module.grid_size,
                                                  scale_factor=scale_factor, robustifier=module.robustifier, need_grad=True)
        ctx.save_for_backward(g)
        ctx.sizes = sizes
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        g, = ctx.saved_tensors
        per_body = torch.repeat_interleave(grad_out.to(g.dtype), torch.as_tensor(ctx.sizes, device=grad_out.device))
        return per_body[:, None, None] * g, None, None, None


class SceneSDFLoss(torch.nn.Module):
    """SDFLoss(faces, grid_size, robustifier) of the reference, batched over scenes, on the GPU.

    faces: [F,3] integer array or tensor (all F faces are voxelised); engine: an object with MvFit's scene_sdf_loss and
    device to use instead of building one (a BodyLayer's engine, or a stand-in in tests).  Without one the module builds an
    MvFit of its own on ``model`` (the model_arrays-style dict MvFit takes)."""

    def __init__(self, faces, grid_size=32, robustifier=None, engine=None, model: dict | None = None, device: int = 0):
        super().__init__()
        if engine is None:
            if model is None:
                raise ValueError('SceneSDFLoss needs engine= (an MvFit, e.g. BodyLayer(...).engine) or model=')
            from .engine import MvFit
            engine = MvFit(model, device=device)
        self.engine = engine
        f = faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else np.asarray(faces)
        if f.ndim != 2 or f.shape[1] != 3:
            raise ValueError('faces must be [F, 3], got %r' % (f.shape,))
        self.register_buffer('faces', torch.tensor(f.astype(np.int32)))
        self.grid_size = int(grid_size)
        self.robustifier = robustifier

    def forward(self, vertices, translation, scale_factor=0.2, scene_sizes=None):
        """vertices[N,Nv,3], translation[N,3] (the reference's arguments).  One scene of N bodies -> a 0-d loss; with
        scene_sizes (bodies per scene, in order, adding up to N) -> loss[S]."""
        dev = self.engine.device
        vertices = torch.as_tensor(vertices)
        translation = torch.as_tensor(translation)
        if vertices.dim() != 3 or vertices.shape[2] != 3:
            raise ValueError('vertices must be [N, Nv, 3], got %r' % (tuple(vertices.shape),))
        N = int(vertices.shape[0])
        if tuple(translation.shape) != (N, 3):
            raise ValueError('translation must be [%d, 3], got %r' % (N, tuple(translation.shape)))
        if scene_sizes is None:
            sizes = (N,)
        else:
            sizes = tuple(int(n) for n in scene_sizes)
            if len(sizes) == 0 or any(n < 1 for n in sizes):
                raise ValueError('scene_sizes must list at least one body per scene, got %r' % (sizes,))
            if sum(sizes) != N:
                raise ValueError('scene_sizes %r do not add up to the %d bodies' % (sizes, N))
        v = vertices + translation.unsqueeze(dim=1)
        v = v.to(device=dev, dtype=torch.float32)
        loss = SceneSDFFunction.apply(v, self, float(scale_factor), sizes)
        return loss[0] if scene_sizes is None else loss
