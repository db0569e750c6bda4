"""CPU: the host logic of scene_fit.refine_scenes against a scripted engine (tests/scene_stub_engine.py) - accept, reject,
revert, stop, the obstacles cleared on the way out - and the argument checks of fit_folder(scene_collision=...)."""
import numpy as np
import pytest
import torch

from mvsmplfitting_amd import batch
from mvsmplfitting_amd.scene_fit import refine_scenes
from tests.scene_stub_engine import ScriptedEngine

SIZES = [2, 1]
STAGE = dict(data_weight=1.0, body_pose_weight=1.0, shape_weight=1.0, bending_prior_weight=1.0, coll_loss_weight=0.5)


def _x0():
    x = np.zeros((3, 118), np.float32)
    x[:, 0] = [5.0, 5.0, 3.0]             # J = (10, 3)
    return x


def test_accept_reject_revert_and_stop():
    # sweep 0: scene 0 falls 10 -> 8 (accepted), scene 1 rises 3 -> 4 (rejected)
    # sweep 1: scene 0 rises 8 -> 9 (rejected), scene 1 falls 3 -> 2 (accepted)
    # sweep 2: scene 0 stays at 8 (not strictly lower: rejected), scene 1 rises: nothing accepted, stop
    eng = ScriptedEngine(3, [[4, 4, 4], [5, 4, 2], [4, 4, 2.5], [0, 0, 0]])
    x, rep = refine_scenes(eng, _x0(), SIZES, STAGE, sweeps=5, grid_size=16, robustifier=0.1, max_iter=11)
    assert eng.n_fit == 3 and len(rep['sweeps']) == 3
    assert rep['J0'].tolist() == [10.0, 3.0]
    assert [s['J'].tolist() for s in rep['sweeps']] == [[8.0, 3.0], [8.0, 2.0], [8.0, 2.0]]
    assert [s['accepted'].tolist() for s in rep['sweeps']] == [[True, False], [False, True], [False, False]]
    assert rep['collision0'].tolist() == [5.0, 1.5]
    assert [s['collision'].tolist() for s in rep['sweeps']] == [[4.0, 1.5], [4.0, 1.0], [4.0, 1.0]]
    assert [s['n_closure'].tolist() for s in rep['sweeps']] == [[7] * 3, [8] * 3, [9] * 3]
    assert x[:, 0].tolist() == [4.0, 4.0, 2.0] and rep['loss'].tolist() == [4.0, 4.0, 2.0]
    # a rejected scene's rows are the previous rows exactly: each scene was moved by exactly one accepted fit
    assert x[:, 1].tolist() == [1.0, 1.0, 1.0]
    # every fit starts from the kept rows with the obstacles frozen there
    fits = [d for n, d in eng.calls if n == 'fit']
    assert [f['at'] for f in fits] == [[5.0, 5.0, 3.0], [4.0, 4.0, 3.0], [4.0, 4.0, 2.0]]
    assert all(f['at'] == f['frozen'] and f['kw'] == dict(max_iter=11) for f in fits)
    assert eng.obstacles is None and eng.calls[-1][0] == 'clear_scene_obstacles'


def test_the_sweep_limit_stops_it_and_the_freeze_arguments_are_passed_on():
    eng = ScriptedEngine(3, [[4, 4, 2], [3, 3, 1], [2, 2, 0]])
    seen = []
    orig = eng.set_scene_obstacles
    eng.set_scene_obstacles = lambda *a, **kw: (seen.append(kw), orig(*a, **kw))[1]
    x, rep = refine_scenes(eng, torch.tensor(_x0()), SIZES, STAGE, sweeps=2, grid_size=16, scale_factor=0.3, robustifier=0.1)
    assert eng.n_fit == 2 and [s['J'].tolist() for s in rep['sweeps']] == [[8.0, 2.0], [6.0, 1.0]]
    assert all(s['accepted'].all() for s in rep['sweeps'])
    assert all(kw == dict(grid_size=16, scale_factor=0.3, robustifier=0.1) for kw in seen)
    # all scenes accepted: no re-freeze between the sweeps - initial, then one per sweep
    assert len(seen) == 3
    assert eng.obstacles is None


def test_J_is_non_increasing_whatever_the_fit_returns():
    rng = np.random.default_rng(0)
    eng = ScriptedEngine(3, rng.uniform(0, 6, (6, 3)))
    _, rep = refine_scenes(eng, _x0(), SIZES, STAGE, sweeps=6)
    J = np.stack([rep['J0']] + [s['J'] for s in rep['sweeps']])
    assert np.all(np.diff(J, axis=0) <= 0)
    for k, s in enumerate(rep['sweeps']):
        assert np.array_equal(s['accepted'], J[k + 1] < J[k])


def test_the_obstacles_are_cleared_when_something_raises():
    eng = ScriptedEngine(3, [[4, 4, 4], [0, 0, 0]], fail_at=1)
    with pytest.raises(RuntimeError, match='scripted failure'):
        refine_scenes(eng, _x0(), SIZES, STAGE)
    assert eng.obstacles is None and eng.calls[-1][0] == 'clear_scene_obstacles'


def test_bad_arguments():
    eng = ScriptedEngine(3, [])
    with pytest.raises(ValueError, match='coll_loss_weight'):
        refine_scenes(eng, _x0(), SIZES, dict(STAGE, coll_loss_weight=0.0))
    with pytest.raises(ValueError, match='add up'):
        refine_scenes(eng, _x0(), [2, 2], STAGE)
    assert eng.calls == []


@pytest.mark.parametrize('kw,match', [(dict(persons=0, scene_collision=dict(weight=1.0)), 'persons'),
                                      (dict(persons='all', is_seq=True, scene_collision=dict(weight=1.0)), 'is_seq'),
                                      (dict(persons='all', scene_collision=dict(sweeps=2)), 'weight')])
def test_fit_folder_refuses_what_the_refinement_cannot_do(tmp_path, kw, match):
    from tests.helpers import body_model
    with pytest.raises(ValueError, match=match):
        batch.fit_folder(body_model(), str(tmp_path / 'keypoints'), str(tmp_path / 'cams.txt'), str(tmp_path / 'out'),
                         engine=object(), **kw)
