"""TESTS ONLY - a scripted stand-in for mvsmplfitting_amd.engine.MvFit, as far as scene_fit.refine_scenes drives it.

Nothing is computed: a problem's closure loss is the first entry of its parameter row, its "vertices" are that entry
repeated, the collision loss of a scene is the sum of its rows' second entries, and fit() returns the next array of a
script, whatever it is given.  Every call is recorded, so a test can read the order of the calls and what was frozen."""
import numpy as np
import torch


class ScriptedEngine:
    def __init__(self, B, script, fail_at=None):
        self.device = torch.device('cpu')
        self.B = B
        self.faces = np.zeros((1, 3), np.int32)
        self.script = [np.asarray(s, np.float32) for s in script]
        self.fail_at = fail_at            # the fit with this index raises
        self.n_fit = 0
        self.obstacles = None             # what set_scene_obstacles froze last (None: cleared)
        self.calls = []

    def vertices(self, params, flags=0):
        x = torch.as_tensor(params)
        self.calls.append(('vertices', x[:, 0].tolist()))
        return x[:, :1, None].repeat(1, 4, 3).contiguous(), None

    def set_scene_obstacles(self, vertices, scene_sizes, grid_size=32, scale_factor=0.2, robustifier=None):
        self.obstacles = dict(at=vertices[:, 0, 0].tolist(), sizes=list(scene_sizes), grid_size=grid_size,
                              scale_factor=scale_factor, robustifier=robustifier)
        self.calls.append(('set_scene_obstacles', self.obstacles['at']))

    def clear_scene_obstacles(self):
        self.obstacles = None
        self.calls.append(('clear_scene_obstacles', None))

    def closure(self, params, weights, want_grad=True, want_verts=False, want_joints=False):
        assert self.obstacles is not None and float(weights['coll_loss_weight']) > 0
        x = torch.as_tensor(params)
        assert self.obstacles['at'] == x[:, 0].tolist(), 'the objective is judged with the obstacles frozen at its own point'
        self.calls.append(('closure', x[:, 0].tolist()))
        return dict(loss=x[:, 0].clone())

    def scene_sdf_loss(self, vertices, faces, scene_sizes=None, grid_size=32, scale_factor=0.2, robustifier=None,
                       need_grad=True, return_phi=False):
        first = np.concatenate([[0], np.cumsum(scene_sizes)])
        v = vertices[:, 0, 0]
        self.calls.append(('scene_sdf_loss', v.tolist()))
        return torch.stack([v[first[s]:first[s + 1]].sum() * 0.5 for s in range(len(scene_sizes))]), None, None

    def fit(self, params, stages, **kw):
        assert self.obstacles is not None and len(stages) == 1
        self.calls.append(('fit', dict(at=torch.as_tensor(params)[:, 0].tolist(), frozen=self.obstacles['at'], kw=kw)))
        k = self.n_fit
        self.n_fit += 1
        if self.fail_at == k:
            raise RuntimeError('scripted failure')
        out = torch.as_tensor(params).clone()
        out[:, 0] = torch.as_tensor(self.script[k])
        out[:, 1] += 1.0                  # a fit always moves the row: a reverted row is recognisable
        return out, dict(n_closure=torch.full((self.B,), 7 + k, dtype=torch.int32))
