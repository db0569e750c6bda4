"""TESTS ONLY - a CPU stand-in for the engine BodyLayer drives (mvsmplfitting_amd/layer.py): vertices and joints are fixed
linear maps of the flat parameters x[B,118], so the layer's packing, unpacking and gradient routing can be checked
without a GPU.  It records what the layer handed it."""
import numpy as np
import torch

from mvsmplfitting_amd import _lib


class LinearEngine:
    def __init__(self, nv=5, seed=0, has_vposer=True):
        rng = np.random.default_rng(seed)
        self.nv = nv
        self.B = 0
        self.device = torch.device('cpu')
        self.has_vposer = has_vposer
        self.Mv = torch.tensor(rng.standard_normal((nv * 3, _lib.D)), dtype=torch.float32)
        self.Mj = torch.tensor(rng.standard_normal((17 * 3, _lib.D)), dtype=torch.float32)
        self.set_problems_calls = []
        self.last_x = None
        self.last_flags = None
        self.backward_calls = []

    def set_problems(self, cams, gt_xy, w_conf):
        assert gt_xy.shape[1:] == (1, 17, 2) and not np.any(w_conf), 'one placeholder view at zero confidence'
        self.B = int(gt_xy.shape[0])
        self.set_problems_calls.append(self.B)

    def vertices(self, x, flags=0):
        assert x.dtype == torch.float32 and tuple(x.shape) == (self.B, _lib.D)
        self.last_x, self.last_flags = x.clone(), flags
        return (x @ self.Mv.T).reshape(self.B, self.nv, 3), (x @ self.Mj.T).reshape(self.B, 17, 3)

    def vertices_backward(self, x, grad_verts=None, grad_joints=None, flags=0):
        self.backward_calls.append((grad_verts is not None, grad_joints is not None, flags))
        g = torch.zeros(self.B, _lib.D)
        if grad_verts is not None:
            g = g + grad_verts.reshape(self.B, -1) @ self.Mv
        if grad_joints is not None:
            g = g + grad_joints.reshape(self.B, -1) @ self.Mj
        return g

    def full_pose(self, x, flags=0):
        """'decoded' pose: a map of the embedding slots only (stands in for the VPoser decoder)."""
        return torch.cat([x[:, 10:13], x[:, 86:109].repeat(1, 3)], dim=1)
