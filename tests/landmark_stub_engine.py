"""TESTS ONLY - stand-ins for the engine as far as landmarks.LandmarkLoss, landmarks.refine_fit and fit_folder(landmarks=) drive
it.

QuadLandmarkEngine's "landmark loss" of problem b is |v_b - target_b|^2 (gradient 2 (v_b - target_b)).  LandmarkFolderEngine is
the CPU stub engine of the folder tests with the landmark calls recorded: its fit returns its input - or, with the term on,
the input with the translation moved by ``step`` - and its closure with the term on returns 10 - x[:, 82] - x[:, 83], so a
positive step lowers every objective and a negative one raises it."""
import numpy as np
import torch

from tests.stub_engine import StubMvFit


class QuadLandmarkEngine:
    def __init__(self, target):
        self.device = torch.device('cpu')
        self.target = torch.as_tensor(target, dtype=torch.float32)
        self.table = self.targets = None
        self.calls = []

    def set_landmarks(self, vertex_ids, weights=None):
        self.table = (np.asarray(vertex_ids), None if weights is None else np.asarray(weights))
        self.targets = None
        self.calls.append('table')

    def set_landmark_targets(self, xy, conf, xyz=None, conf3=None):
        assert self.table is not None, 'no table'
        self.targets = (xy, conf, xyz, conf3)
        self.calls.append('targets')

    def landmark_loss(self, vertices, rho=100.0, w3d=0.0, rho3d=0.0, need_grad=True):
        assert self.targets is not None, 'no targets'
        self.calls.append(('loss', rho, w3d, rho3d))
        r = vertices.detach() - self.target
        return (r * r).sum(dim=(1, 2)), 2.0 * r


class LandmarkFolderEngine(StubMvFit):
    def __init__(self, model, step=0.25):
        super().__init__(model)
        self.nv = int(np.asarray(model['v_template']).shape[0])
        self.step = float(step)
        self.log = []
        self.table = self.targets = None
        self.term = None

    def set_problems(self, cams, gt_xy, w_conf):
        super().set_problems(cams, gt_xy, w_conf)
        self.log.append(['set_problems', [self.B, self.V]])

    def set_landmarks(self, vertex_ids, weights=None):
        self.table = (np.asarray(vertex_ids).copy(), np.asarray(weights).copy())
        self.log.append(['set_landmarks', int(self.table[0].shape[0])])

    def clear_landmarks(self):
        self.table = self.targets = self.term = None
        self.log.append(['clear_landmarks'])

    def set_landmark_targets(self, xy, conf, xyz=None, conf3=None):
        assert self.table is not None
        self.targets = (np.asarray(xy).copy(), np.asarray(conf).copy())
        self.log.append(['set_landmark_targets', list(self.targets[0].shape)])

    def set_landmark_term(self, rho=100.0, w3d=0.0, rho3d=0.0):
        assert self.targets is not None
        self.term = (rho, w3d, rho3d)
        self.log.append(['set_landmark_term', rho])

    def clear_landmark_term(self):
        self.term = None
        self.log.append(['clear_landmark_term'])

    def closure(self, params, weights, want_grad=True, want_verts=False, want_joints=False):
        x = torch.as_tensor(params).to(torch.float64)
        self.log.append(['closure', float(weights.get('coll_loss_weight', 0.0))])
        assert self.term is not None
        self._S = torch.full((x.shape[0],), 2.0)
        return dict(loss=10.0 - x[:, 82] - x[:, 83])

    def sdf_term_read(self):
        return None, self._S

    def fit(self, params, stages, **kw):
        self.log.append(['fit', len(stages), float(stages[-1].get('coll_loss_weight', 0.0))])
        x = torch.as_tensor(params).clone()
        if self.term is not None:
            x[:, 82] += self.step
        return x, dict(final_loss=torch.zeros(x.shape[0]), n_closure=torch.zeros(x.shape[0], dtype=torch.int32),
                       n_iter=torch.zeros(x.shape[0], dtype=torch.int32))
