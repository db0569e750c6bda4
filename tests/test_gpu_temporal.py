"""GPU: temporal.smooth_sequences on the engine - two interleaved sequences of six frames, four views.  The truth is a smooth
motion (translation and a few pose angles linear in t), the observations carry independent per-frame keypoint noise, the
start point is the independent staged fit of all twelve problems, and w balances the smoothing term against the data term
on that start point (w^2 = loss / L of a mid-sequence problem, as tests/test_gpu_silhouette_term.py's _weight).

Asserted are the directions only: every sequence accepted at least once, E and the pair sum below their start values, a
rejected sweep's rows bit-equal to the previous ones, the engine left without term and targets.  E, the pair sum and the
mean vertex error against the truth are printed (DESIGN section 7 quotes them); no threshold on those."""
import numpy as np
import pytest

from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import MvFitError, pack_params, stage_weights
from mvsmplfitting_amd.temporal import neighbour_table, smooth_sequences
from tests.gpu_helpers import make_engine
from tests.helpers import body_model

pytestmark = pytest.mark.gpu

V, S, F = 4, 2, 6
B = S * F
SEQ = np.tile(np.arange(S), F)                  # interleaved: problem j is frame j // S of sequence j % S
FRM = np.repeat(np.arange(F), S)


def _np(t):
    return t.detach().cpu().numpy()


def _truth():
    x = np.zeros((B, 118), np.float32)
    rng = np.random.default_rng(77)
    for s in range(S):
        base = pack_params(B=1, **syn.make_frames(1, seed0=7000 + s))[0]
        vel = rng.normal(0, 0.01, 3).astype(np.float32)                    # metres per frame
        joints = rng.choice(23, 4, replace=False)
        omega = rng.normal(0, 0.015, (4, 3)).astype(np.float32)             # radians per frame
        for t in range(F):
            row = base.copy()
            row[82:85] += t * vel
            for i, j in enumerate(joints):
                row[13 + 3 * j:16 + 3 * j] += t * omega[i]
            x[t * S + s] = row
    return x


def test_smoothing_lowers_the_joint_energy_and_the_jitter():
    model = body_model()
    cams = syn.make_camera_ring(V)
    x_true = _truth()
    eng = make_engine(model)
    try:
        eng.set_problems(cams, np.zeros((B, V, 17, 2), np.float32), np.zeros((B, V, 17), np.float32))
        v_true, joints = eng.vertices(x_true)
        gt, conf = syn.make_observations(_np(joints), cams, seed=9)
        eng.set_problems(cams, gt, conf)
        stages = stage_weights(1536.0)
        x0 = np.zeros((B, 118), np.float32)
        x0[:, 85] = 1.0
        xfit, _ = eng.fit(x0, stages)
        # the balancing rule on the start point, at a problem with both neighbours
        nbr, a = neighbour_table(SEQ, FRM)
        row = 2 * S
        assert (nbr[row] >= 0).all()
        v0, _ = eng.vertices(xfit)
        eng.set_vertex_targets(v0[np.maximum(nbr, 0)], a)
        L = _np(eng.vertex_target_loss(v0, need_grad=False)[0]).astype(np.float64)
        eng.clear_vertex_targets()
        data = float(eng.closure(xfit, stages[-1], want_grad=False)['loss'][row])
        w = float(np.sqrt(data / L[row]))
        stage = dict(stages[-1], coll_loss_weight=w)

        def vertex_error(x):
            v, _ = eng.vertices(x)
            return float((v - v_true).norm(dim=2).mean())

        x, rep = smooth_sequences(eng, xfit, stage, SEQ, FRM, sweeps=3)
        last = rep['sweeps'][-1]
        print('w %.5g (data %.5g, L %.5g at problem %d)' % (w, data, L[row], row))
        print('E      %s -> %s' % (rep['E0'], last['E']))
        print('smooth %s -> %s (truth %s)' % (rep['smooth0'], last['smooth'],
                                              [float(sum(((v_true[(t + 1) * S + s] - v_true[t * S + s]) ** 2).sum() for t in range(F - 1)))
                                               for s in range(S)]))
        print('mean vertex error against the truth %.5f m -> %.5f m' % (vertex_error(xfit), vertex_error(x)))
        for k, sw in enumerate(rep['sweeps']):
            print('sweep %d: accepted %s E %s smooth %s closures %s' % (k, sw['accepted'], sw['E'], sw['smooth'], sw['n_closure']))
        assert np.array_equal(rep['params0'], _np(xfit))
        assert np.allclose(rep['smooth0'], [0.5 * L[SEQ == s].sum() for s in range(S)], rtol=1e-12)
        assert np.stack([sw['accepted'] for sw in rep['sweeps']]).any(axis=0).all()
        assert (last['E'] < rep['E0']).all()
        assert (last['smooth'] < rep['smooth0']).all()
        prev_x, prev_E = rep['params0'], rep['E0']
        for sw in rep['sweeps']:
            for s in range(S):
                if sw['accepted'][s]:
                    assert sw['E'][s] < prev_E[s]
                else:
                    assert np.array_equal(sw['params'][SEQ == s], prev_x[SEQ == s]) and sw['E'][s] == prev_E[s]
            prev_x, prev_E = sw['params'], sw['E']
        assert np.array_equal(_np(x), last['params'])
        # the engine is left with no term and no targets
        with pytest.raises(MvFitError, match='error -3'):
            eng.closure(x, stage)
        with pytest.raises(MvFitError, match='error -3: mvfit_vertex_target_loss'):
            eng.vertex_target_loss(v0)
    finally:
        eng.close()
