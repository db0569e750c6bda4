"""The body model as a differentiable PyTorch module: SMPL.forward (reference code/smplx/body_models_scale.py:327-412) on the
HIP kernels, with its reverse mode (include/mvfit.h: mvfit_vertices / mvfit_vertices_backward).

Any term a caller writes on ``out.vertices`` or ``out.joints`` gets its gradient with respect to the inputs:

    layer = BodyLayer(model_arrays)
    out = layer(betas, global_orient, body_pose, transl=transl)
    loss = my_term(out.vertices, out.joints)
    loss.backward()                     # -> betas.grad, global_orient.grad, body_pose.grad, transl.grad

The inputs are packed into the flat parameter vector x[B,118] of the C ABI with ``torch.cat`` (so autograd routes the
gradient of x back to each input, cast back to its dtype and device); one autograd node maps x to (vertices, joints).
Once differentiable: there is no double backward.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib

ModelOutput = namedtuple('ModelOutput', ['vertices', 'joints', 'full_pose', 'betas', 'global_orient', 'body_pose'])

# widths of the flat parameter vector's blocks, in order (include/mvfit.h; engine.SL)
_WIDTHS = (('betas', 10), ('global_orient', 3), ('body_pose', 69), ('transl', 3), ('scale', 1), ('pose_embedding', 32))
assert sum(w for _, w in _WIDTHS) == _lib.D


class VerticesFunction(torch.autograd.Function):
    """x[B,118] float32 -> (vertices[B,Nv,3], joints[B,17,3]) on layer's engine; backward = mvfit_vertices_backward."""

    @staticmethod
    def forward(ctx, x, layer, flags):
        layer._ensure_batch(x.shape[0])
        verts, joints = layer.engine.vertices(x.detach(), flags)
        ctx.save_for_backward(x)
        ctx.layer, ctx.flags = layer, flags
        ctx.set_materialize_grads(False)            # an output that receives no gradient: NULL cotangent, not zeros
        return verts, joints

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_verts, grad_joints):
        x, = ctx.saved_tensors
        if grad_verts is None and grad_joints is None:
            return None, None, None
        ctx.layer._ensure_batch(x.shape[0])
        g = ctx.layer.engine.vertices_backward(x.detach(), grad_verts, grad_joints, ctx.flags)
        return g, None, None


class BodyLayer(torch.nn.Module):
    """SMPL with its gradient, on the GPU.

    model: the model_arrays-style dict MvFit takes (synthetic.make_body_model, or real SMPL arrays; kp_regressor None =
    model_type 'smpl'); vposer: the decoder weight dict (optional); options: mvfit_options fields; engine: an object with
    MvFit's interface to use instead of building one (tests).

    The layer owns its MvFit.  The C ABI sizes its work per batch (mvfit_set_problems); the layer calls it whenever B
    changes, with one placeholder view at zero confidence (no observation enters either direction)."""

    def __init__(self, model: dict, vposer: dict | None = None, device: int = 0, options: dict | None = None, engine=None):
        super().__init__()
        if engine is None:
            from .engine import MvFit
            engine = MvFit(model, vposer=vposer, device=device, options=options)
        self.engine = engine
        self.has_vposer = vposer is not None or bool(getattr(engine, 'has_vposer', False))

    def _ensure_batch(self, B: int):
        if self.engine.B == B:
            return
        cams = (np.eye(3, dtype=np.float32)[None], np.array([[0.0, 0.0, 10.0]], np.float32), np.array([1000.0], np.float32),
                np.array([[512.0, 512.0]], np.float32))
        self.engine.set_problems(cams, np.zeros((B, 1, 17, 2), np.float32), np.zeros((B, 1, 17), np.float32))

    def forward(self, betas, global_orient, body_pose=None, transl=None, scale=None, pose_embedding=None,
                return_full_pose=False):
        """betas[B,10], global_orient[B,3], body_pose[B,69] (or None with pose_embedding), transl[B,3] (default 0),
        scale[B,1] or [B] (default 1), pose_embedding[B,32] (VPoser: the body pose is decoded from it).

        Returns ModelOutput(vertices[B,Nv,3], joints[B,17,3], full_pose[B,72] or None, betas, global_orient, body_pose).
        With VPoser, body_pose and full_pose are the decoded pose (mvfit_full_pose) and carry no gradient - the gradient
        reaches the embedding through vertices and joints.  Without VPoser, full_pose is global_orient | body_pose (cat)."""
        dev = self.engine.device
        B = int(betas.shape[0])
        use_vp = pose_embedding is not None
        if use_vp and not self.has_vposer:
            raise ValueError('pose_embedding given but the layer has no VPoser decoder')
        if not use_vp and body_pose is None:
            raise ValueError('body_pose is required without pose_embedding')

        def f32(t, width, default=0.0):
            if t is None:
                return torch.full((B, width), default, device=dev, dtype=torch.float32)
            t = torch.as_tensor(t)
            return t.to(device=dev, dtype=torch.float32).reshape(B, width)
        parts = dict(betas=f32(betas, 10), global_orient=f32(global_orient, 3),
                     body_pose=f32(None if use_vp else body_pose, 69), transl=f32(transl, 3), scale=f32(scale, 1, 1.0),
                     pose_embedding=f32(pose_embedding, 32))
        x = torch.cat([parts[n] for n, _ in _WIDTHS], dim=1)
        flags = _lib.F_VPOSER if use_vp else 0
        vertices, joints = VerticesFunction.apply(x, self, flags)
        if use_vp:
            decoded = self.engine.full_pose(x.detach(), flags)
            out_body_pose = decoded[:, 3:]
            full_pose = decoded if return_full_pose else None
        else:
            out_body_pose = body_pose
            full_pose = torch.cat([parts['global_orient'], parts['body_pose']], dim=1) if return_full_pose else None
        return ModelOutput(vertices, joints, full_pose, betas, global_orient, out_body_pose)
