"""CPU: the landmark term's host side up to the engine - io_formats.read_people_extra, landmarks.load_table /
targets_from_people / LandmarkLoss / refine_fit, batch.check_landmarks (every ValueError is raised before any engine work) and
the fit_folder(landmarks=...) path, through the stand-ins of tests/landmark_stub_engine.py."""
import json
import os

import numpy as np
import pytest
import torch

from mvsmplfitting_amd import batch
from mvsmplfitting_amd import io_formats as iof
from mvsmplfitting_amd import landmarks as lmk
from tests.helpers import GOLD, body_model
from tests.landmark_stub_engine import LandmarkFolderEngine, QuadLandmarkEngine

TABLE = os.path.join(GOLD, 'landmarks_halpe_feet_smpl.json')
DATA = os.path.join(GOLD, 'demo_data')
CAMS = os.path.join(DATA, '3DOH50K_Parameters.txt')


def _feet(frame, cam, person):
    """the nine rows 17-25 a test file appends to an entry: distinct numbers per (frame, camera, person, row)"""
    rows = np.zeros((9, 3), np.float32)
    rows[:, 0] = 1000.0 * frame + 100.0 * cam + 10.0 * person + np.arange(9)
    rows[:, 1] = rows[:, 0] + 0.5
    rows[:, 2] = 0.75
    return rows


def make_folder(root, people=1, frames=2, rows26=True, person_ids=None):
    """The demo serial under root/keypoints with ``people`` entries per file and ``frames`` frames; rows26: every entry has 26
    rows, the last nine _feet(frame, camera, entry)."""
    src = os.path.join(DATA, 'keypoints', '0000')
    for c, cam in enumerate(sorted(os.listdir(src))):
        with open(os.path.join(src, cam, '00001_keypoints.json')) as f:
            data = json.load(f)
        os.makedirs(os.path.join(root, 'keypoints', '0000', cam))
        for k in range(frames):
            entries = []
            for p in range(people):
                kp = list(data['people'][0]['pose_keypoints_2d'])
                if rows26:
                    kp += [float(v) for v in _feet(k, c, p).reshape(-1)]
                e = dict(pose_keypoints_2d=kp)
                if person_ids is not None:
                    e['person_id'] = int(person_ids[p])
                entries.append(e)
            with open(os.path.join(root, 'keypoints', '0000', cam, '%05d_keypoints.json' % (k + 1)), 'w') as f:
                json.dump(dict(data, people=entries), f)
    return os.path.join(str(root), 'keypoints')


# ---------------------------------------------------------------------------------------------- the readers
def test_read_people_extra(tmp_path):
    keyp = make_folder(tmp_path / 'a', people=2, person_ids=[7, 3])
    path = os.path.join(keyp, '0000', 'Camera02', '00002_keypoints.json')
    rows = [20, 21, 22, 23, 24, 25]
    got = iof.read_people_extra(path, rows)
    assert sorted(got) == [3, 7]
    assert np.array_equal(got[7], _feet(1, 2, 0)[3:]) and np.array_equal(got[3], _feet(1, 2, 1)[3:])
    assert got[7].dtype == np.float32 and got[7].shape == (6, 3)
    by_index = iof.read_people_extra(path, rows, by_index=True)
    assert sorted(by_index) == [0, 1] and np.array_equal(by_index[0], got[7])
    # rows past the file's: confidence 0; read_people and read_keypoints keep their 17 rows
    far = iof.read_people_extra(path, [25, 26, 40])
    assert np.array_equal(far[7][0], _feet(1, 2, 0)[8]) and not far[7][1:].any()
    assert iof.read_people(path)[7].shape == (17, 3) and iof.read_keypoints(path)[0].shape == (17, 3)
    keyp17 = make_folder(tmp_path / 'b', rows26=False)
    short = iof.read_people_extra(os.path.join(keyp17, '0000', 'Camera00', '00001_keypoints.json'), rows)
    assert sorted(short) == [0] and short[0].shape == (6, 3) and not short[0].any()
    with pytest.raises(ValueError, match='negative row'):
        iof.read_people_extra(path, [-1])


def test_load_table():
    t = lmk.load_table(TABLE)
    assert t['names'] == ['LBigToe', 'RBigToe', 'LSmallToe', 'RSmallToe', 'LHeel', 'RHeel']
    assert t['keypoint_index'].tolist() == [20, 21, 22, 23, 24, 25]
    assert t['vertex_ids'].shape == (6, 4) and t['vertex_ids'].dtype == np.int32 and t['weights'].dtype == np.float32
    assert np.array_equal(t['weights'], np.tile(np.array([1, 0, 0, 0], np.float32), (6, 1)))
    assert (t['vertex_ids'][:, 0] < 6890).all() and len(set(t['vertex_ids'][:, 0].tolist())) == 6
    with open(TABLE) as f:
        assert set(json.load(f)) == {'names', 'keypoint_index', 'vertex_ids', 'weights'}            # data only
    d = lmk.load_table(dict(vertex_ids=[5, 9]))
    assert d['vertex_ids'][:, 0].tolist() == [5, 9] and d['weights'][:, 0].tolist() == [1.0, 1.0]
    assert d['keypoint_index'].tolist() == [-1, -1] and d['names'] == ['landmark_0', 'landmark_1']
    m = lmk.load_table(dict(vertex_ids=[[1, 2], [3]], weights=[[0.25, 0.75], [1.0]]))
    assert m['vertex_ids'].tolist() == [[1, 2, 0, 0], [3, 0, 0, 0]] and m['weights'][0].tolist() == [0.25, 0.75, 0.0, 0.0]
    for bad, msg in ((dict(), 'vertex_ids'), (dict(vertex_ids=[]), 'outside'), (dict(vertex_ids=[[1, 2]]), 'weights are needed'),
                     (dict(vertex_ids=[[1, 2, 3, 4, 5]], weights=[[1, 1, 1, 1, 1]]), '1 to 4'),
                     (dict(vertex_ids=[[1]], weights=[[1.0, 2.0]]), 'shape of vertex_ids'),
                     (dict(vertex_ids=[[-1]], weights=[[1.0]]), 'negative'), (dict(vertex_ids=[1], colour='red'), 'unknown keys'),
                     (dict(vertex_ids=[1], weights=[[float('nan')]]), 'finite'), (dict(vertex_ids=[1, 2], names=['a']), 'one entry')):
        with pytest.raises(ValueError, match=msg):
            lmk.load_table(bad)


def test_targets_from_people():
    a = np.array([[1, 2, 0.5], [3, 4, 0.0], [5, 6, 1.0]], np.float32)
    b = a + 10
    xy, conf = lmk.targets_from_people([[a, None], [b, a]], 3)
    assert xy.shape == (2, 2, 3, 2) and conf.shape == (2, 2, 3) and xy.dtype == np.float32
    assert np.array_equal(conf[0, 0], [0.5, 0.0, 1.0]) and not conf[0, 1].any()
    assert np.array_equal(xy[0, 0, [0, 2]], a[[0, 2], :2]) and np.isnan(xy[0, 0, 1]).all() and np.isnan(xy[0, 1]).all()
    assert np.array_equal(xy[1, 0], b[:, :2]) and np.array_equal(conf[1, 0], b[:, 2])
    with pytest.raises(ValueError, match='rows of shape'):
        lmk.targets_from_people([[a[:2]]], 3)
    with pytest.raises(ValueError, match='lists 1 views'):
        lmk.targets_from_people([[a, a], [a]], 3)


# ---------------------------------------------------------------------------------------------- the option
def test_check_landmarks():
    cfg = batch.check_landmarks(dict(weight=2.0, table=TABLE), 6890)
    assert cfg['rho'] == 100.0 and cfg['weight'] == 2.0 and cfg['table']['keypoint_index'].tolist() == list(range(20, 26))
    assert batch.check_landmarks(dict(weight=1, table=TABLE, rho=0.0), 6890)['rho'] == 0.0


def test_fit_folder_landmarks_argument_errors(tmp_path):
    model = body_model()
    run = lambda **kw: batch.fit_folder(model, str(tmp_path / 'none'), str(tmp_path / 'none.txt'), str(tmp_path / 'out'), **kw)
    ok = dict(weight=1.0, table=TABLE)
    for bad, msg in ((dict(table=TABLE), "at least 'weight'"), (dict(weight=1.0), "at least 'weight'"), ('feet', "at least 'weight'"),
                     (dict(ok, colour=1), 'unknown keys'), (dict(ok, weight=0.0), 'weight must be > 0'),
                     (dict(ok, weight=-1.0), 'weight must be > 0'), (dict(ok, rho=-1.0), 'rho must be'),
                     (dict(ok, table=dict(vertex_ids=[6890], keypoint_index=[20])), 'names vertex 6890'),
                     (dict(ok, table=dict(vertex_ids=[1])), 'keypoint_index')):
        with pytest.raises(ValueError, match=msg):
            run(landmarks=bad)
    with pytest.raises(ValueError, match='is_seq'):
        run(landmarks=ok, is_seq=True)
    with pytest.raises(ValueError, match='refine_cameras with landmarks'):
        run(landmarks=ok, refine_cameras=dict())
    others = dict(scene_collision=dict(weight=1.0), silhouettes=dict(weight=1.0, mask_root='m'), temporal=dict(weight=1.0),
                  scans=dict(weight=1.0, root='s'),
                  joint=dict(weight=1.0, silhouettes=dict(share=1.0, mask_root='m'), temporal=dict(share=1.0)))
    for name, arg in others.items():
        with pytest.raises(ValueError, match='landmarks and %s both use' % name):
            run(landmarks=ok, persons='all', **{name: arg})


# ---------------------------------------------------------------------------------------------- module and refine_fit
def test_landmark_loss_module_is_one_autograd_node():
    target = torch.arange(2 * 5 * 3, dtype=torch.float32).reshape(2, 5, 3) * 0.1
    eng = QuadLandmarkEngine(target)
    xy, conf = np.zeros((2, 3, 2, 2), np.float32), np.ones((2, 3, 2), np.float32)
    loss = lmk.LandmarkLoss(eng, dict(vertex_ids=[0, 4]), xy, conf, rho=50.0)
    assert eng.calls == ['table', 'targets'] and eng.table[0].shape == (2, 4)
    v = torch.zeros(2, 5, 3, requires_grad=True)
    out = loss(v * 2.0)
    (out * torch.tensor([1.0, 3.0])).sum().backward()
    assert eng.calls[-1] == ('loss', 50.0, 0.0, 0.0)
    assert torch.allclose(out, (target ** 2).sum(dim=(1, 2)))
    assert torch.allclose(v.grad, 2.0 * torch.tensor([1.0, 3.0])[:, None, None] * 2.0 * (-target))
    with pytest.raises(ValueError, match='hold 3 bodies'):
        loss(torch.zeros(3, 5, 3))
    with pytest.raises(ValueError, match='come together'):
        lmk.LandmarkLoss(eng, dict(vertex_ids=[0]), xy, conf, xyz=np.zeros((2, 1, 3)))
    with pytest.raises(ValueError, match='rho'):
        lmk.LandmarkLoss(eng, dict(vertex_ids=[0]), xy, conf, rho=-1.0)


@pytest.mark.parametrize('step,accepted', [(0.25, True), (-0.25, False)])
def test_refine_fit_keeps_a_row_only_if_its_objective_fell(step, accepted):
    eng = LandmarkFolderEngine(body_model(), step=step)
    eng.table, eng.targets = 'table', 'targets'
    x0 = torch.zeros(3, 118)
    x0[:, 82] = torch.tensor([0.0, 1.0, 2.0])
    out, rep = lmk.refine_fit(eng, x0, dict(coll_loss_weight=0.5), rho=40.0)
    assert [c[0] for c in eng.log] == ['set_landmark_term', 'closure', 'fit', 'closure', 'clear_landmark_term']
    assert eng.log[0] == ['set_landmark_term', 40.0] and eng.term is None
    assert rep['accepted'].tolist() == [accepted] * 3
    assert torch.equal(out, x0 + (torch.eye(118)[82] * step if accepted else 0.0))
    assert np.array_equal(rep['before'], 10.0 - x0[:, 82].numpy()) and np.array_equal(rep['loss'], rep['after'])
    assert np.array_equal(rep['after'], rep['before'] - (step if accepted else 0.0))
    assert set(rep) == {'before', 'after', 'accepted', 'landmark_before', 'landmark_after', 'n_closure', 'loss'}
    with pytest.raises(ValueError, match='coll_loss_weight > 0'):
        lmk.refine_fit(eng, x0, dict(coll_loss_weight=0.0))


# ---------------------------------------------------------------------------------------------- fit_folder(landmarks=)
def _run(tmp, name, folder_kw, **kw):
    model = body_model()
    eng = LandmarkFolderEngine(model)
    keyp = make_folder(os.path.join(str(tmp), name), **folder_kw)
    out = batch.fit_folder(model, keyp, CAMS, os.path.join(str(tmp), name, 'out'), engine=eng, **kw)
    return eng, out['0000']


def test_fit_folder_landmarks_single_person(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **kw: None)
    timing = {}
    eng, out = _run(tmp_path, 'with', dict(frames=2), landmarks=dict(weight=0.375, table=TABLE, rho=60.0), timing=timing)
    base, ref = _run(tmp_path, 'without', dict(frames=2))
    # after the keypoint fit: table, targets, term on, J(x0), the fit with the term, J(x'), term off, table gone
    first = eng.log.index(['set_landmarks', 6])
    assert eng.log[first - 1][0] == 'fit'
    assert eng.log[first:first + 8] == [['set_landmarks', 6], ['set_landmark_targets', [2, 6, 6, 2]], ['set_landmark_term', 60.0],
                                        ['closure', 0.375], ['fit', 1, 0.375], ['closure', 0.375], ['clear_landmark_term'],
                                        ['clear_landmarks']]
    fits = [c for c in eng.log if c[0] == 'fit']
    assert fits[-1] == ['fit', 1, 0.375] and fits[0][1] == 4
    rep = out['landmark_report']
    assert rep['accepted'].tolist() == [True, True] and rep['targets'].tolist() == [36, 36]
    assert 'landmark' in timing
    moved = ref['params'].copy()
    moved[:, 82] += 0.25
    assert np.array_equal(out['params'], moved)
    assert np.array_equal(out['final_loss'], rep['loss'].astype(np.float32))
    assert len(out['files']) == 2 and all(os.path.exists(f) for f in out['files'])
    assert not [c for c in base.log if 'landmark' in c[0]]


def test_fit_folder_landmarks_follow_the_person_ids(tmp_path):
    eng, out = _run(tmp_path, 'ids', dict(people=2, frames=2, person_ids=[7, 3]), persons='all',
                    landmarks=dict(weight=1.0, table=TABLE))
    assert out['problem_person'].tolist() == [3, 7, 3, 7] and out['problem_frame'].tolist() == [0, 0, 1, 1]
    assert ['set_landmark_targets', [4, 6, 6, 2]] in eng.log
    # the targets the engine was handed: problem n = (frame, id), view v -> rows 20..25 of that id's entry in that file
    seen = _last_targets(tmp_path, 'ids2', dict(people=2, frames=2, person_ids=[7, 3]), persons='all')
    for n, (f, pid) in enumerate([(0, 3), (0, 7), (1, 3), (1, 7)]):
        for v in range(6):
            want = _feet(f, v, {7: 0, 3: 1}[pid])[3:]
            assert np.array_equal(seen[0][n, v], want[:, :2]) and np.array_equal(seen[1][n, v], want[:, 2])
    # persons=[7]: the one id
    seen = _last_targets(tmp_path, 'ids3', dict(people=2, frames=1, person_ids=[7, 3]), persons=[7])
    assert seen[0].shape == (1, 6, 6, 2) and np.array_equal(seen[0][0, 4], _feet(0, 4, 0)[3:, :2])


def _last_targets(tmp, name, folder_kw, **kw):
    got = {}

    class Keep(LandmarkFolderEngine):
        def set_landmark_targets(self, xy, conf, xyz=None, conf3=None):
            got['t'] = (np.asarray(xy).copy(), np.asarray(conf).copy())
            super().set_landmark_targets(xy, conf, xyz, conf3)
    model = body_model()
    keyp = make_folder(os.path.join(str(tmp), name), **folder_kw)
    batch.fit_folder(model, keyp, CAMS, os.path.join(str(tmp), name, 'out'), engine=Keep(model), landmarks=dict(weight=1.0, table=TABLE),
                     **kw)
    return got['t']


def test_files_with_17_rows_are_not_refitted(tmp_path):
    eng, out = _run(tmp_path, 'short', dict(frames=2, rows26=False), landmarks=dict(weight=1.0, table=TABLE))
    base, ref = _run(tmp_path, 'short_ref', dict(frames=2, rows26=False))
    assert not [c for c in eng.log if 'landmark' in c[0] or c[0] == 'closure'] and eng.log == base.log
    assert np.array_equal(out['params'], ref['params']) and np.array_equal(out['final_loss'], ref['final_loss'])
    rep = out['landmark_report']
    assert rep['loss'] is None and not rep['accepted'].any() and not rep['targets'].any()
