"""TESTS ONLY - stand-ins for the engine and the body layer, as far as scan.ScanLoss and scan.refine_to_scan drive them.

QuadScanEngine's "scan loss" of body b is |v_b - target_b|^2 (gradient 2 (v_b - target_b)); StubLayer's "body" is
vertices = scale * template + betas[:3] + transl.  Every engine call is recorded."""
from collections import namedtuple

import torch

Out = namedtuple('Out', ['vertices', 'joints'])


class QuadScanEngine:
    def __init__(self, target):
        self.device = torch.device('cpu')
        self.target = torch.as_tensor(target, dtype=torch.float32)
        self.scans = None
        self.calls = []

    def set_scans(self, points, count=None, weights=None):
        self.scans = (points, count, weights)
        self.calls.append('set')

    def clear_scans(self):
        self.scans = None
        self.calls.append('clear')

    def scan_loss(self, vertices, w_s2m=1.0, w_m2s=0.0, sigma=0.0, need_grad=True, return_nearest=False, search='auto'):
        assert self.scans is not None, 'no scan set'
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
