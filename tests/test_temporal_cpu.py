"""CPU: temporal.neighbour_table, the host logic of temporal.smooth_sequences against a small engine defined here (quadratic
per-problem closures, vertices linear in the parameters: every number below can be computed directly), and the argument
checks of fit_folder(temporal=...)."""
import numpy as np
import pytest
import torch

from mvsmplfitting_amd import batch
from mvsmplfitting_amd.temporal import neighbour_table, smooth_sequences
from tests.helpers import body_model

STAGE = dict(data_weight=1.0, body_pose_weight=1.0, shape_weight=1.0, bending_prior_weight=1.0, coll_loss_weight=0.7)


# ------------------------------------------------------------------------------------------------ neighbour_table
def test_two_interleaved_sequences():
    seq = [7, 3, 7, 3, 7, 3]
    frm = [0, 0, 1, 1, 2, 2]
    nbr, a = neighbour_table(seq, frm)
    assert nbr.dtype == np.int64 and a.dtype == np.float32 and nbr.shape == a.shape == (6, 2)
    assert nbr.tolist() == [[-1, 2], [-1, 3], [0, 4], [1, 5], [2, -1], [3, -1]]
    assert a.tolist() == [[0, 1], [0, 1], [1, 1], [1, 1], [1, 0], [1, 0]]


def test_a_gap_breaks_the_chain_and_the_order_of_the_problems_is_free():
    # frames 4, 5, 7, 8 of one sequence, listed out of order: 5 and 7 are not neighbours
    nbr, a = neighbour_table([0, 0, 0, 0], [8, 4, 7, 5])
    assert nbr.tolist() == [[2, -1], [-1, 3], [-1, 0], [1, -1]]
    assert a.tolist() == [[1, 0], [0, 1], [0, 1], [1, 0]]


def test_single_frame_sequences_have_no_neighbours():
    nbr, a = neighbour_table(['a', 'b', 'c'], [5, 5, 6])
    assert (nbr == -1).all() and not a.any()


def test_a_duplicate_frame_raises():
    with pytest.raises(ValueError, match='both frame 1 of sequence 0'):
        neighbour_table([0, 1, 0, 0], [0, 1, 1, 1])
    with pytest.raises(ValueError):
        neighbour_table([0, 1], [0])


# ------------------------------------------------------------------------------------------------ smooth_sequences
NV = 2
MIX = (np.eye(6) + 0.25 * np.random.default_rng(1).normal(size=(6, 6)))


class QuadraticEngine:
    """f_j(x) = ||x_j[:6] - c_j||^2, vertices_j = (x_j[:6] MIX) as [2,3]; the term as the real engine states it.
    fit(): the exact minimiser of every frozen problem, unless ``moves`` holds a callable for the sweep (x -> x')."""

    def __init__(self, centres, moves=()):
        self.c = np.asarray(centres, np.float64)
        self.B, self.nv, self.device = len(self.c), NV, torch.device('cpu')
        self.moves = list(moves)
        self.targets = self.weights = None
        self.term = False
        self.n_fit = self.n_set = 0
        self.L = None

    def vertices(self, x, flags=0):
        u = torch.as_tensor(np.asarray(x))[:, :6].double()
        return (u @ torch.as_tensor(MIX)).reshape(self.B, NV, 3), None

    def set_vertex_targets(self, targets, weights):
        assert tuple(targets.shape) == (self.B, 2, NV, 3)
        self.targets, self.weights = targets.detach().clone().double().numpy(), np.asarray(weights, np.float64).copy()
        self.n_set += 1

    def clear_vertex_targets(self):
        self.targets = self.weights = None
        self.term = False

    def set_vertex_target_term(self):
        assert self.targets is not None
        self.term = True

    def clear_vertex_target_term(self):
        self.term = False

    def _L(self, x):
        v = self.vertices(x)[0].numpy()
        return np.array([sum(self.weights[j, k] * ((v[j] - self.targets[j, k]) ** 2).sum() for k in range(2) if self.weights[j, k] > 0)
                         for j in range(self.B)], np.float64)

    def closure(self, x, stage, want_grad=True):
        assert self.term and not want_grad
        u = np.asarray(torch.as_tensor(np.asarray(x))[:, :6].double())
        self.L = self._L(x)
        return dict(loss=torch.as_tensor(((u - self.c) ** 2).sum(1) + stage['coll_loss_weight'] ** 2 * self.L))

    def sdf_term_read(self):
        return None, torch.as_tensor(self.L)

    def fit(self, x, stages, **kw):
        assert self.term and len(stages) == 1
        k, self.n_fit = self.n_fit, self.n_fit + 1
        x = torch.as_tensor(np.asarray(x)).clone()
        if k < len(self.moves) and self.moves[k] is not None:
            out = self.moves[k](x.clone())
            if isinstance(out, Exception):
                raise out
        else:
            w2 = stages[0]['coll_loss_weight'] ** 2
            out = x.clone()
            for j in range(self.B):
                A, b = np.eye(6), self.c[j].copy()
                for t in range(2):
                    if self.weights[j, t] > 0:
                        A += w2 * self.weights[j, t] * MIX @ MIX.T
                        b += w2 * self.weights[j, t] * MIX @ self.targets[j, t].reshape(6)
                out[j, :6] = torch.as_tensor(np.linalg.solve(A, b), dtype=out.dtype)
        return out, dict(n_closure=torch.full((self.B,), 5 + k, dtype=torch.int32))


SEQ = np.array([0, 1, 0, 1, 0, 1, 0])           # sequence 0: problems 0, 2, 4, 6; sequence 1: 1, 3, 5
FRM = np.array([0, 0, 1, 1, 2, 2, 3])


def _world(seed=0):
    rng = np.random.default_rng(seed)
    c = rng.normal(size=(7, 6))
    x0 = np.zeros((7, 118), np.float64)
    x0[:, :6] = c + 0.3 * rng.normal(size=(7, 6))
    x0[:, 6] = 1.0                              # (a column no fit touches)
    return c, x0


def _joint_energy(c, x, w):
    """sum_j f_j + w^2 sum_pairs ||V_{t+1} - V_t||^2 and the pair sums, per sequence, computed directly."""
    x = np.asarray(x, np.float64)
    v = x[:, :6] @ MIX
    E, sm = np.zeros(2), np.zeros(2)
    for s in range(2):
        rows = np.flatnonzero(SEQ == s)
        rows = rows[np.argsort(FRM[rows])]
        sm[s] = sum(((v[rows[i + 1]] - v[rows[i]]) ** 2).sum() for i in range(len(rows) - 1))
        E[s] = ((x[rows, :6] - c[rows]) ** 2).sum() + w * w * sm[s]
    return E, sm


def test_the_half_bookkeeping_gives_the_joint_energy():
    c, x0 = _world()
    w = STAGE['coll_loss_weight']
    eng = QuadraticEngine(c)
    x, rep = smooth_sequences(eng, torch.as_tensor(x0), STAGE, SEQ, FRM, sweeps=3)
    E0, sm0 = _joint_energy(c, x0, w)
    assert rep['sequences'].tolist() == [0, 1]
    assert np.allclose(rep['E0'], E0, rtol=1e-12, atol=0) and np.allclose(rep['smooth0'], sm0, rtol=1e-12, atol=0)
    assert np.array_equal(rep['params0'], x0)
    assert len(rep['sweeps']) == 3 and eng.n_fit == 3
    prev = E0
    for k, sw in enumerate(rep['sweeps']):
        Ek, smk = _joint_energy(c, sw['params'], w)
        assert np.allclose(sw['E'], Ek, rtol=1e-12, atol=0) and np.allclose(sw['smooth'], smk, rtol=1e-12, atol=0)
        # the exact Jacobi sweep of a quadratic chain energy is monotone
        assert sw['accepted'].all() and (sw['E'] < prev).all()
        assert sw['n_closure'].tolist() == [5 + k] * 7
        prev = sw['E']
    assert np.array_equal(x.numpy(), rep['sweeps'][-1]['params'])
    assert (rep['sweeps'][-1]['smooth'] < sm0).all()
    # loss [B]: the frozen problems at the result; they count every pair twice
    assert rep['loss'].shape == (7,)
    E, sm = _joint_energy(c, x.numpy(), w)
    assert np.allclose([rep['loss'][SEQ == s].sum() for s in range(2)], E + w * w * sm, rtol=1e-12, atol=0)
    # all accepted: one freeze at the start and one per sweep
    assert eng.n_set == 4
    assert not eng.term and eng.targets is None


def test_a_rejected_sequence_reverts_exactly_and_is_refrozen():
    c, x0 = _world(1)
    w = STAGE['coll_loss_weight']

    def worsen_one(x):                 # sequence 0 gets its minimiser, sequence 1 is pushed away from everything
        good = QuadraticEngine(c)
        good.targets, good.weights, good.term = eng.targets, eng.weights, True
        out, _ = good.fit(x, [STAGE])
        out[SEQ == 1, :6] = x[SEQ == 1, :6] + 3.0
        return out

    eng = QuadraticEngine(c, moves=[worsen_one])
    x, rep = smooth_sequences(eng, x0.astype(np.float32), STAGE, SEQ, FRM, sweeps=2)
    s0, s1 = rep['sweeps']
    assert s0['accepted'].tolist() == [True, False]
    x0f = x0.astype(np.float32)
    assert np.array_equal(s0['params'][SEQ == 1], x0f[SEQ == 1])                      # bit for bit
    assert not np.array_equal(s0['params'][SEQ == 0], x0f[SEQ == 0])
    assert s0['E'][1] == rep['E0'][1] and s0['smooth'][1] == rep['smooth0'][1] and s0['E'][0] < rep['E0'][0]
    E, _ = _joint_energy(c, s0['params'], w)
    assert np.allclose(s0['E'], E, rtol=1e-6)
    # freezes: start, after sweep 0's fit, the re-freeze at the kept rows, after sweep 1's fit
    assert eng.n_set == 4 and eng.n_fit == 2
    assert s1['accepted'].all()
    assert np.array_equal(x.numpy(), s1['params'])


def test_it_stops_when_nothing_was_accepted():
    c, x0 = _world(2)

    def worsen(x):
        x[:, :6] += 2.0
        return x

    x0 = x0.astype(np.float32)              # (an array goes in as float32, like every parameter array of the engine)
    eng = QuadraticEngine(c, moves=[worsen, worsen, worsen])
    x, rep = smooth_sequences(eng, x0, STAGE, SEQ, FRM, sweeps=5)
    assert eng.n_fit == 1 and len(rep['sweeps']) == 1 and not rep['sweeps'][0]['accepted'].any()
    assert np.array_equal(x.numpy(), x0) and np.array_equal(rep['sweeps'][0]['E'], rep['E0'])
    assert not eng.term and eng.targets is None
    # the sweep limit
    eng = QuadraticEngine(c)
    smooth_sequences(eng, x0, STAGE, SEQ, FRM, sweeps=1)
    assert eng.n_fit == 1


def test_the_engine_is_left_clean_when_something_raises():
    c, x0 = _world(3)
    eng = QuadraticEngine(c, moves=[lambda x: RuntimeError('boom')])
    with pytest.raises(RuntimeError, match='boom'):
        smooth_sequences(eng, x0, STAGE, SEQ, FRM)
    assert not eng.term and eng.targets is None and eng.n_set == 1
    eng = QuadraticEngine(c)
    with pytest.raises(ValueError, match='coll_loss_weight'):
        smooth_sequences(eng, x0, dict(STAGE, coll_loss_weight=0.0), SEQ, FRM)
    with pytest.raises(ValueError, match='7 problems'):
        smooth_sequences(eng, x0, STAGE, SEQ[:6], FRM[:6])
    with pytest.raises(ValueError, match='both frame'):
        smooth_sequences(eng, x0, STAGE, np.zeros(7, int), np.zeros(7, int))
    assert eng.n_set == 0 and eng.n_fit == 0


# ------------------------------------------------------------------------------------------------ fit_folder
def test_fit_folder_temporal_argument_errors(tmp_path):
    """Raised before any engine is created (engine=None and no GPU here) and before any file is read."""
    model = body_model()
    run = lambda **kw: batch.fit_folder(model, str(tmp_path / 'none'), str(tmp_path / 'none.txt'), str(tmp_path / 'out'), **kw)
    with pytest.raises(ValueError, match="temporal: a dict with at least 'weight'"):
        run(temporal=True)
    with pytest.raises(ValueError, match="temporal: a dict with at least 'weight'"):
        run(temporal=dict(sweeps=2))
    with pytest.raises(ValueError, match='temporal: unknown keys .*wieght'):
        run(temporal=dict(weight=1.0, wieght=2.0))
    for bad in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError, match='temporal: weight must be > 0'):
            run(temporal=dict(weight=bad))
    with pytest.raises(ValueError, match='temporal: sweeps must be >= 1'):
        run(temporal=dict(weight=1.0, sweeps=0))
    with pytest.raises(ValueError, match='temporal and scene_collision'):
        run(temporal=dict(weight=1.0), scene_collision=dict(weight=1.0), persons='all')
    with pytest.raises(ValueError, match='temporal and silhouettes'):
        run(temporal=dict(weight=1.0), silhouettes=dict(mask_root=str(tmp_path), weight=1.0))
    with pytest.raises(ValueError, match='temporal and silhouettes'):
        run(temporal=dict(weight=1.0), silhouettes=dict(mask_root=str(tmp_path), weight=1.0), is_seq=False, persons=[0, 1])
    assert batch.check_temporal(dict(weight=2.0)) == dict(weight=2.0, sweeps=3)
    assert batch.check_temporal(dict(weight=2.0, sweeps=5))['sweeps'] == 5
