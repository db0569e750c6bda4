"""CPU: the host logic of joint_refine.refine_joint against a small engine defined here (quadratic per-problem closures,
vertices linear in the parameters, every term a squared distance: the joint energy can be computed directly), and the groups
the accept rule works on."""
import numpy as np
import pytest
import torch

from mvsmplfitting_amd.joint_refine import check_shares, problem_groups, refine_joint
from mvsmplfitting_amd.temporal import neighbour_table

STAGE = dict(data_weight=1.0, body_pose_weight=1.0, shape_weight=1.0, bending_prior_weight=1.0, coll_loss_weight=0.7)
SHARES = dict(scene=0.5, silhouette=2.0, temporal=0.25)
NV = 2
MIX = (np.eye(6) + 0.25 * np.random.default_rng(1).normal(size=(6, 6)))
# seven problems: scenes (0, 1), (2, 3), (4, 5), (6); problems 0 and 2 are frames 0 and 1 of sequence 'a' - they link the first
# two scenes - and 4, 6 single frames of their own
SIZES = [2, 2, 2, 1]
SEQ = np.array(['a', 'b', 'a', 'c', 'd', 'e', 'f'])
FRM = np.array([0, 0, 1, 0, 0, 0, 0])
GROUP = [0, 0, 0, 0, 1, 1, 2]


# ------------------------------------------------------------------------------------------------ groups and shares
def test_two_scenes_linked_by_a_sequence_form_one_group():
    nbr, _ = neighbour_table(SEQ, FRM)
    assert problem_groups(7, SIZES, nbr).tolist() == GROUP
    assert problem_groups(7, SIZES, None).tolist() == [0, 0, 1, 1, 2, 2, 3]
    assert problem_groups(7, None, nbr).tolist() == [0, 1, 0, 2, 3, 4, 5]
    assert problem_groups(3, None, None).tolist() == [0, 1, 2]
    # a chain through three scenes, listed so that a later problem joins two earlier groups
    nbr, _ = neighbour_table([0, 1, 2, 0, 3, 3], [0, 0, 0, 1, 0, 1])
    assert problem_groups(6, [2, 1, 2, 1], nbr).tolist() == [0, 0, 1, 0, 0, 0]


def test_shares():
    assert check_shares(dict(scene=1, temporal=2)) == (1.0, 0.0, 2.0)
    with pytest.raises(ValueError, match="unknown shares \\['silhouete'\\]"):
        check_shares(dict(scene=1, silhouete=1))
    with pytest.raises(ValueError, match='at least two shares'):
        check_shares(dict(scene=1))
    with pytest.raises(ValueError, match='at least two shares'):
        check_shares(dict(scene=1, temporal=0.0))
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='finite and >= 0'):
            check_shares(dict(scene=1, temporal=bad))


# ------------------------------------------------------------------------------------------------ refine_joint
class QuadraticEngine:
    """f_j(x) = ||x_j[:6] - c_j||^2, vertices_j = (x_j[:6] MIX) as [2,3].  The three parts of the mix, each a squared distance:
    S_sc,j^2 = sum over the other bodies i of j's scene of ||V_j - O_i||^2 (O: the frozen obstacles), L_sil,j = ||V_j - M_j||^2
    (M: the "mask set", the engine's own), L_vt,j = the vertex-target loss.  fit(): the exact minimiser of every frozen
    problem, unless ``moves`` holds a callable for the sweep (x -> x')."""

    def __init__(self, centres, masks, moves=()):
        self.c, self.M = np.asarray(centres, np.float64), np.asarray(masks, np.float64)
        self.B, self.nv, self.device = len(self.c), NV, torch.device('cpu')
        self.moves = list(moves)
        self.targets = self.weights = self.obst = self.sizes = self.mix = None
        self.n_fit = self.n_targets = self.n_obst = 0
        self.parts = None

    def vertices(self, x, flags=0):
        u = torch.as_tensor(np.asarray(x))[:, :6].double()
        return (u @ torch.as_tensor(MIX)).reshape(self.B, NV, 3), None

    def set_vertex_targets(self, targets, weights):
        assert tuple(targets.shape) == (self.B, 2, NV, 3)
        self.targets, self.weights = targets.detach().clone().double().numpy().reshape(self.B, 2, 6), np.asarray(weights, np.float64).copy()
        self.n_targets += 1

    def clear_vertex_targets(self):
        self.targets = self.weights = None
        if self.mix and self.mix[2] > 0:
            self.mix = None

    def set_scene_obstacles(self, v, sizes, grid_size=32, scale_factor=0.2, robustifier=None):
        assert sum(sizes) == self.B and (grid_size, scale_factor, robustifier) == (16, 0.3, 0.01)
        self.obst, self.sizes = v.detach().clone().double().numpy().reshape(self.B, 6), list(sizes)
        self.n_obst += 1

    def clear_scene_obstacles(self):
        self.obst = None
        if self.mix and self.mix[0] > 0:
            self.mix = None

    def set_term_mix(self, scene=0.0, silhouette=0.0, vertex_targets=0.0, w_in=1.0, w_out=1.0, sigma=0.0):
        assert (scene == 0 or self.obst is not None) and (vertex_targets == 0 or self.targets is not None)
        assert (w_in, w_out, sigma) == (1.0, 0.5, 3.0)
        self.mix = (scene, silhouette, vertex_targets)

    def clear_term_mix(self):
        self.mix = None

    def _anchors(self, j):
        """(weight, point [6]) of every squared distance problem j pays, weighted by the shares."""
        out = []
        if self.mix[0] > 0:
            first = np.concatenate([[0], np.cumsum(self.sizes)])
            s = np.searchsorted(first, j, side='right') - 1
            out += [(self.mix[0], self.obst[i], 0) for i in range(first[s], first[s + 1]) if i != j]
        if self.mix[1] > 0:
            out.append((self.mix[1], self.M[j], 1))
        if self.mix[2] > 0:
            out += [(self.mix[2] * self.weights[j, k], self.targets[j, k], 2) for k in range(2) if self.weights[j, k] > 0]
        return out

    def closure(self, x, stage, want_grad=True):
        assert self.mix is not None and not want_grad
        u = np.asarray(torch.as_tensor(np.asarray(x))[:, :6].double())
        v = u @ MIX
        self.parts = np.zeros((self.B, 3))
        pen = np.zeros(self.B)
        for j in range(self.B):
            for lam, p, kind in self._anchors(j):
                d = ((v[j] - p) ** 2).sum()
                pen[j] += lam * d
                self.parts[j, kind] += lam * d / self.mix[kind]
        return dict(loss=torch.as_tensor(((u - self.c) ** 2).sum(1) + stage['coll_loss_weight'] ** 2 * pen))

    def term_mix_read(self):
        assert self.mix is not None
        return torch.as_tensor(self.parts)

    def fit(self, x, stages, **kw):
        assert self.mix is not None and len(stages) == 1 and kw == dict(max_iter=9)
        k, self.n_fit = self.n_fit, self.n_fit + 1
        x = torch.as_tensor(np.asarray(x)).clone()
        if k < len(self.moves) and self.moves[k] is not None:
            out = self.moves[k](x.clone())
            if isinstance(out, Exception):
                raise out
        else:
            out = self.minimiser(x, stages[0])
        return out, dict(n_closure=torch.full((self.B,), 5 + k, dtype=torch.int32))

    def minimiser(self, x, stage):
        w2 = stage['coll_loss_weight'] ** 2
        out = x.clone()
        for j in range(self.B):
            A, b = np.eye(6), self.c[j].copy()
            for lam, p, _ in self._anchors(j):
                A += w2 * lam * MIX @ MIX.T
                b += w2 * lam * MIX @ p
            out[j, :6] = torch.as_tensor(np.linalg.solve(A, b), dtype=out.dtype)
        return out


KW = dict(shares=SHARES, scene_sizes=SIZES, seq_id=SEQ, frame_idx=FRM, grid_size=16, scale_factor=0.3, robustifier=0.01,
          w_in=1.0, w_out=0.5, sigma=3.0, max_iter=9)


def _world(seed=0):
    rng = np.random.default_rng(seed)
    c = rng.normal(size=(7, 6))
    masks = (c + 0.2 * rng.normal(size=(7, 6))) @ MIX
    x0 = np.zeros((7, 118), np.float64)
    x0[:, :6] = c + 0.3 * rng.normal(size=(7, 6))
    x0[:, 6] = 1.0                              # (a column no fit touches)
    return c, masks, x0


def _joint_energy(c, masks, x, w, shares=SHARES):
    """Per group: sum_j f_j + w^2 (l_sc * every ordered pair of a scene + l_sil * the mask distances + l_t * every unordered
    pair of consecutive frames), and the groups' unweighted parts as the frozen problems count them, computed directly."""
    x = np.asarray(x, np.float64)
    v = x[:, :6] @ MIX
    E, parts = np.zeros(3), np.zeros((3, 3))
    first = np.concatenate([[0], np.cumsum(SIZES)])
    for j in range(7):
        g = GROUP[j]
        s = np.searchsorted(first, j, side='right') - 1
        parts[g, 0] += sum(((v[j] - v[i]) ** 2).sum() for i in range(first[s], first[s + 1]) if i != j)
        parts[g, 1] += ((v[j] - masks[j]) ** 2).sum()
        E[g] += ((x[j, :6] - c[j]) ** 2).sum()
    pair = ((v[2] - v[0]) ** 2).sum()           # the one pair of consecutive frames: problems 0 and 2, both in group 0
    parts[0, 2] += 2 * pair
    lam = [shares.get(k, 0.0) for k in ('scene', 'silhouette', 'temporal')]
    E += w * w * (lam[0] * parts[:, 0] + lam[1] * parts[:, 1])
    E[0] += w * w * lam[2] * pair
    return E, parts


def test_the_bookkeeping_gives_the_joint_energy_and_it_never_rises():
    c, masks, x0 = _world()
    w = STAGE['coll_loss_weight']
    eng = QuadraticEngine(c, masks)
    x, rep = refine_joint(eng, torch.as_tensor(x0), STAGE, sweeps=3, **KW)
    E0, parts0 = _joint_energy(c, masks, x0, w)
    assert rep['group'].tolist() == GROUP and rep['shares'] == SHARES
    assert np.allclose(rep['E0'], E0, rtol=1e-12, atol=0) and np.allclose(rep['parts0'], parts0, rtol=1e-12, atol=0)
    assert np.array_equal(rep['params0'], x0)
    assert 1 <= len(rep['sweeps']) <= 3 and eng.n_fit == len(rep['sweeps'])
    prev = E0
    for k, sw in enumerate(rep['sweeps']):
        Ek, pk = _joint_energy(c, masks, sw['params'], w)
        assert np.allclose(sw['E'], Ek, rtol=1e-12, atol=0) and np.allclose(sw['parts'], pk, rtol=1e-12, atol=0)
        assert (sw['E'] <= prev).all() and (sw['E'][sw['accepted']] < prev[sw['accepted']]).all()
        assert np.array_equal(sw['E'][~sw['accepted']], prev[~sw['accepted']])
        assert sw['n_closure'].tolist() == [5 + k] * 7
        prev = sw['E']
    assert rep['sweeps'][0]['accepted'].all()           # the frozen problems' minimisers lower every group's energy here
    assert np.array_equal(x.numpy(), rep['sweeps'][-1]['params'])
    # loss [B] and parts_problem [B,3]: the frozen problems at the result
    E, parts = _joint_energy(c, masks, x.numpy(), w)
    got = np.array([rep['parts_problem'][np.array(GROUP) == g].sum(0) for g in range(3)])
    assert np.allclose(got, parts, rtol=1e-12, atol=0)
    loss = np.array([rep['loss'][np.array(GROUP) == g].sum() for g in range(3)])
    assert np.allclose(loss, E + 0.5 * w * w * SHARES['temporal'] * parts[:, 2], rtol=1e-12, atol=0)
    assert eng.mix is None and eng.targets is None and eng.obst is None


def test_two_parts_only():
    c, masks, x0 = _world(4)
    w = STAGE['coll_loss_weight']
    shares = dict(silhouette=1.5, temporal=0.5)
    eng = QuadraticEngine(c, masks)
    kw = dict(KW, shares=shares)
    kw.pop('scene_sizes')
    x, rep = refine_joint(eng, torch.as_tensor(x0), STAGE, sweeps=2, **kw)
    assert rep['group'].tolist() == [0, 1, 0, 2, 3, 4, 5] and eng.n_obst == 0
    v = x0[:, :6] @ MIX
    f = ((x0[:, :6] - c) ** 2).sum(1) + w * w * 1.5 * ((v - masks) ** 2).sum(1)
    pair = ((v[2] - v[0]) ** 2).sum()
    assert np.allclose(rep['E0'], [f[0] + f[2] + w * w * 0.5 * pair, f[1], f[3], f[4], f[5], f[6]], rtol=1e-12, atol=0)
    assert not rep['parts0'][:, 0].any()


def test_a_rejected_group_reverts_exactly_and_is_refrozen():
    c, masks, x0 = _world(1)

    def worsen_one(x):                 # groups 0 and 2 get their minimisers, group 1 (problems 4, 5) is pushed away
        out = eng.minimiser(x, STAGE)
        out[4:6, :6] = x[4:6, :6] + 3.0
        return out

    eng = QuadraticEngine(c, masks, moves=[worsen_one])
    x, rep = refine_joint(eng, x0.astype(np.float32), STAGE, sweeps=2, **KW)
    s0, s1 = rep['sweeps']
    assert s0['accepted'].tolist() == [True, False, True]
    x0f = x0.astype(np.float32)
    assert np.array_equal(s0['params'][4:6], x0f[4:6])                                # bit for bit
    assert not np.array_equal(s0['params'][:4], x0f[:4]) and not np.array_equal(s0['params'][6], x0f[6])
    assert s0['E'][1] == rep['E0'][1] and np.array_equal(s0['parts'][1], rep['parts0'][1])
    assert s0['E'][0] < rep['E0'][0] and s0['E'][2] < rep['E0'][2]
    E, parts = _joint_energy(c, masks, s0['params'], STAGE['coll_loss_weight'])
    assert np.allclose(s0['E'], E, rtol=1e-6) and np.allclose(s0['parts'], parts, rtol=1e-5)
    # freezes: start, after sweep 0's fit, the re-freeze at the kept rows, after sweep 1's fit
    assert eng.n_targets == 4 and eng.n_obst == 4 and eng.n_fit == 2
    assert np.array_equal(x.numpy(), s1['params'])


def test_it_stops_when_nothing_was_accepted():
    c, masks, x0 = _world(2)

    def worsen(x):
        x[:, :6] += 2.0
        return x

    x0 = x0.astype(np.float32)
    eng = QuadraticEngine(c, masks, moves=[worsen, worsen, worsen])
    x, rep = refine_joint(eng, x0, STAGE, sweeps=5, **KW)
    assert eng.n_fit == 1 and len(rep['sweeps']) == 1 and not rep['sweeps'][0]['accepted'].any()
    assert np.array_equal(x.numpy(), x0) and np.array_equal(rep['sweeps'][0]['E'], rep['E0'])
    assert eng.mix is None and eng.targets is None and eng.obst is None
    eng = QuadraticEngine(c, masks)                       # the sweep limit
    refine_joint(eng, x0, STAGE, sweeps=1, **KW)
    assert eng.n_fit == 1


def test_the_engine_is_left_clean_when_something_raises():
    c, masks, x0 = _world(3)
    eng = QuadraticEngine(c, masks, moves=[lambda x: RuntimeError('boom')])
    with pytest.raises(RuntimeError, match='boom'):
        refine_joint(eng, x0, STAGE, **KW)
    assert eng.mix is None and eng.targets is None and eng.obst is None and eng.n_targets == 1
    assert np.array_equal(eng.M, masks)                   # the mask set is the caller's
    eng = QuadraticEngine(c, masks)
    with pytest.raises(ValueError, match='coll_loss_weight'):
        refine_joint(eng, x0, dict(STAGE, coll_loss_weight=0.0), **KW)
    with pytest.raises(ValueError, match='at least two shares'):
        refine_joint(eng, x0, STAGE, **dict(KW, shares=dict(scene=1.0)))
    with pytest.raises(ValueError, match='needs scene_sizes'):
        refine_joint(eng, x0, STAGE, **dict(KW, scene_sizes=None))
    with pytest.raises(ValueError, match='do not add up'):
        refine_joint(eng, x0, STAGE, **dict(KW, scene_sizes=[2, 2]))
    with pytest.raises(ValueError, match='needs seq_id'):
        refine_joint(eng, x0, STAGE, **dict(KW, seq_id=None))
    with pytest.raises(ValueError, match='7 problems'):
        refine_joint(eng, x0, STAGE, **dict(KW, seq_id=SEQ[:6], frame_idx=FRM[:6]))
    assert eng.n_targets == 0 and eng.n_obst == 0 and eng.n_fit == 0
