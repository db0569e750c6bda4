"""TESTS ONLY - a stand-in for the engine as far as silhouette.refine_fit_occluded (and the refine_fit inside it) drives it.

The "objective" of problem j is |x_j - goal_j|^2; fit() adds the next entry of ``moves`` ([B,118] each) to the rows, so a
test scripts which rows improve in which sweep; a ``None`` entry makes fit() raise.  Every call is recorded, with the
vertices the occluders were frozen at."""
import numpy as np
import torch


class ScriptedEngine:
    def __init__(self, goal, moves, images_per_body=2, nv=4, points_per_image=3):
        self.device = torch.device('cpu')
        self.goal = torch.as_tensor(goal, dtype=torch.float32)
        self.B = int(self.goal.shape[0])
        self.moves = list(moves)
        self.nv, self.M, self.ppi = nv, self.B * images_per_body, points_per_image
        self.calls, self.frozen = [], []
        self.term = self.occluders = False
        self.last = None

    # the model: vertex k of problem j = x_j[:3] + k
    def vertices(self, x):
        v = x[:, None, :3] + torch.arange(self.nv, dtype=x.dtype)[None, :, None]
        return v, v[:, :1].expand(-1, 17, -1)

    def set_silhouette_occluders(self, vertices, body_scene, margin=0.02):
        self.calls.append('freeze')
        self.frozen.append((vertices.clone(), np.asarray(body_scene).copy(), float(margin)))
        self.occluders = True

    def clear_silhouette_occluders(self):
        self.calls.append('clear_occluders')
        self.occluders = False

    def round_graph_info(self, drop=False):
        self.calls.append('drop_graph' if drop else 'graph_info')
        return dict(builds=0, occluder_buffers=(0, 0, 0))

    def silhouettes(self):
        first = torch.arange(self.M + 1, dtype=torch.int32) * self.ppi
        return torch.zeros(self.M, 2, 2), first, torch.zeros(self.M * self.ppi, 2, dtype=torch.int32)

    def silhouette_occluders(self):
        assert self.occluders
        flag = torch.zeros(self.M * self.ppi, dtype=torch.uint8)
        flag[::2] = 1                            # points 0, 2, 4, ...: image i has 2 or 1 flagged points in turn
        return torch.zeros(self.M, 2, 2), torch.zeros(self.M, 2, 2), flag

    def silhouette_hidden(self, vertices):
        assert self.occluders
        h = torch.zeros(self.M, self.nv, dtype=torch.uint8)
        h[:, :len(self.frozen)] = 1              # sweep s hides s vertices per image
        return h

    def set_silhouette_term(self, w_in=1.0, w_out=1.0, sigma=0.0):
        self.calls.append('term_on')
        self.term = True

    def clear_silhouette_term(self):
        self.calls.append('term_off')
        self.term = False

    def closure(self, x, stage, want_grad=True):
        assert self.term and self.occluders, 'judged outside the frozen maps'
        self.last = ((torch.as_tensor(x) - self.goal) ** 2).sum(dim=1)
        return dict(loss=self.last)

    def sdf_term_read(self):
        return None, 0.5 * self.last

    def fit(self, x, stages, **kw):
        self.calls.append('fit')
        move = self.moves.pop(0)
        if move is None:
            raise RuntimeError('scripted failure')
        return x + torch.as_tensor(move, dtype=x.dtype), dict(n_closure=torch.ones(self.B, dtype=torch.int32))
