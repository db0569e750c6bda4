"""TESTS ONLY - stand-ins for the engine and the body layer, as far as silhouette.refine_shape drives them.

QuadEngine's "silhouette loss" of body b is |v_b - target_b|^2 (gradient 2 (v_b - target_b)); StubLayer's "body" is
vertices = scale * template + betas[:3] + transl.  Every engine call is recorded."""
from collections import namedtuple

import torch

Out = namedtuple('Out', ['vertices', 'joints'])


class QuadEngine:
    def __init__(self, target):
        self.device = torch.device('cpu')
        self.target = torch.as_tensor(target, dtype=torch.float32)
        self.masks = None
        self.calls = []

    def set_silhouettes(self, masks, image_body, cams, contour_stride=1):
        self.masks = masks
        self.calls.append('set')

    def clear_silhouettes(self):
        self.masks = None
        self.calls.append('clear')

    def silhouette_loss(self, vertices, w_in=1.0, w_out=1.0, sigma=0.0, need_grad=True, return_winner=False):
        assert self.masks is not None, 'no mask set'
        self.calls.append('loss')
        r = vertices.detach() - self.target
        return (r * r).sum(dim=(1, 2)), 2.0 * r


class StubLayer:
    def __init__(self, engine, template):
        self.engine = engine
        self.template = torch.as_tensor(template, dtype=torch.float32)

    def __call__(self, betas, global_orient, body_pose=None, transl=None, scale=None):
        v = scale[:, :, None] * self.template[None] + betas[:, None, :3] + transl[:, None, :]
        return Out(v, v[:, :1].expand(-1, 17, -1))
