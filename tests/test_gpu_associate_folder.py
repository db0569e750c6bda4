"""GPU: fit_folder(persons='all', associate=True) on a three-person serial whose files list the people in a shuffled,
per-file order (3 persons with their own shape a metre apart, 4 views, 3 frames, exact projected keypoints; person 1 is not
detected by view 2 in frame 1, person 2 is absent from frame 2; one file carries a false positive): the association
restores the identities and the fit is, bit for bit, the fit of the ordered folder."""
import json

import numpy as np
import pytest

from mvsmplfitting_amd import batch
from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import MvFit
from tests.helpers import body_model

pytestmark = pytest.mark.gpu

V, F, P = 4, 3, 3
BASE = np.array([[-1.1, 0.0, 0.0], [0.0, 0.0, 0.1], [1.1, 0.0, -0.1]], np.float32)
PROBLEMS = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1)]          # (frame, person) of the ordered folder
FALSE_POSITIVE = (0, 1)                                                             # (frame, view) of the extra entry


def _truth():
    """xgt [F, P, 118]: each person their own betas, a pose per frame, standing a metre apart."""
    x = np.zeros((F, P, 118), np.float32)
    for p in range(P):
        betas = np.random.default_rng(300 + p).normal(0, 0.5, 10).astype(np.float32)
        fr = syn.make_frames(F, seed0=50 + 100 * p, betas=betas)
        for k, (a, b) in dict(betas=(0, 10), global_orient=(10, 13), body_pose=(13, 82), transl=(82, 85), scale=(85, 86)).items():
            x[:, p, a:b] = fr[k]
        x[:, p, 82:85] = BASE[p] + 0.3 * x[:, p, 82:85]
    return x


def _write_folder(root, name, entries):
    """entries[(f, v)] = [[17, 3] rows in file order]"""
    for v in range(V):
        d = root / name / 's0' / ('Camera%02d' % v)
        d.mkdir(parents=True)
        for f in range(F):
            people = [dict(pose_keypoints_2d=[float(x) for x in k2.reshape(-1)]) for k2 in entries[(f, v)]]
            with open(d / ('%05d_keypoints.json' % f), 'w') as fh:
                json.dump(dict(version=1.0, people=people), fh)
    return str(root / name)


@pytest.fixture(scope='module')
def scene(tmp_path_factory):
    root = tmp_path_factory.mktemp('associate')
    model = body_model()
    cams = syn.make_camera_ring(V)
    xgt = _truth()
    with MvFit(model) as eng:
        eng.set_problems(cams, np.zeros((F * P, V, 17, 2), np.float32), np.zeros((F * P, V, 17), np.float32))
        _, joints = eng.vertices(xgt.reshape(F * P, 118))
    uv = syn.project_points(joints.cpu().numpy(), *cams).reshape(F, P, V, 17, 2)
    cam_R, cam_t, cam_f, cam_c = (np.asarray(a, np.float64) for a in cams)
    with open(root / 'cams.txt', 'w') as fh:
        for v in range(V):
            fh.write('%d\n' % v)
            K = np.array([[cam_f[v], 0, cam_c[v, 0]], [0, cam_f[v], cam_c[v, 1]], [0, 0, 1]])
            for r in K:
                fh.write(' '.join('%.10f' % x for x in r) + '\n')
            fh.write('0 0\n')
            for r in np.hstack([cam_R[v], cam_t[v][:, None]]):
                fh.write(' '.join('%.10f' % x for x in r) + '\n')
    rng = np.random.default_rng(2024)
    ordered, shuffled, who = {}, {}, {}
    for f in range(F):
        for v in range(V):
            rows = []
            for p in range(P if f < 2 else 2):                      # frame 2 lists two persons only
                k2 = np.concatenate([uv[f, p, v], np.ones((17, 1))], 1)
                if (f, p, v) == (1, 1, 2):
                    k2[:] = 0                                       # person 1 is not detected by view 2 in frame 1
                rows.append((p, k2))
            ordered[(f, v)] = [k2 for _, k2 in rows]
            if (f, v) == FALSE_POSITIVE:
                rows.append((-1, np.concatenate([rng.uniform([0, 0], [2048, 1536], (17, 2)), np.ones((17, 1))], 1)))
            perm = rng.permutation(len(rows))
            shuffled[(f, v)] = [rows[i][1] for i in perm]
            who[(f, v)] = [rows[i][0] for i in perm]                # the true person of every entry, -1: nobody
    assert any(who[(f, v)][:2] != [0, 1] for f in range(F) for v in range(V))
    return dict(root=root, ordered=_write_folder(root, 'ordered', ordered), shuffled=_write_folder(root, 'shuffled', shuffled),
                who=who, cams=str(root / 'cams.txt'), model=model, xgt=xgt)


def _fit(scene, eng, keyp, name, **kw):
    return batch.fit_folder(scene['model'], scene[keyp], scene['cams'], str(scene['root'] / name), engine=eng, **kw)['s0']


@pytest.fixture(scope='module')
def ordered_fit(scene):
    """The ordered folder fitted without association: computed once, read by both tests."""
    with MvFit(scene['model']) as eng:
        return _fit(scene, eng, 'ordered', 'plain', persons='all')


def _nearest(out, xgt):
    return [int(np.argmin(np.linalg.norm(out['params'][n, 82:85][None] - xgt[f, :, 82:85], axis=1)))
            for n, f in enumerate(out['problem_frame'].tolist())]


def test_association_restores_the_identities_and_the_fit(scene, ordered_fit):
    xgt, who = scene['xgt'], scene['who']
    with MvFit(scene['model']) as eng:
        timing = {}
        out = _fit(scene, eng, 'shuffled', 'assoc', persons='all', associate=True, timing=timing)
    want = ordered_fit
    rep = out['association']
    assert out['persons'] == [0, 1, 2] and rep['num_clusters'].tolist() == [3, 3, 2]
    assert rep['params'] == dict(max_cost=0.05, min_joints=6, min_views=2, max_move=0.5, max_gap=5)
    assert timing['associate'] > 0 and set(timing) == {'read', 'associate', 'init_guess', 'fit', 'write'}
    print('associate: %.1f ms of %.1f ms' % (1e3 * timing['associate'], 1e3 * sum(timing.values())))
    # every detection's track is one true person, every person one track; only the false positive has none
    person_of = {}
    lost = []
    for f in range(F):
        for v in range(V):
            for k in range(int(rep['count'][f, v])):
                p, t = who[(f, v)][rep['slot'][f, v, k]], int(rep['track_ids'][f, v, k])
                if t < 0:
                    lost.append((f, v, p))
                else:
                    assert person_of.setdefault(t, p) == p, (f, v, k, t, p)
    assert lost == [FALSE_POSITIVE + (-1,)] and rep['unassigned'] == 1
    assert sorted(person_of) == [0, 1, 2] and sorted(person_of.values()) == [0, 1, 2]
    # the problems are those of the ordered folder, each nearest to its own person's truth ...
    got_rows = [(f, person_of[t]) for f, t in zip(out['problem_frame'].tolist(), out['problem_person'].tolist())]
    assert sorted(got_rows) == PROBLEMS
    assert list(zip(want['problem_frame'].tolist(), want['problem_person'].tolist())) == PROBLEMS
    assert _nearest(out, xgt) == [p for _, p in got_rows]
    # ... and fitted to the same bits: the same keypoint rows went in, and a problem does not depend on its position
    at = [got_rows.index(r) for r in PROBLEMS]
    for k in ('params', 'final_loss', 'n_closure', 'views_per_frame'):
        assert np.array_equal(out[k][at], want[k]), k


def test_without_association_the_shuffled_folder_crosses_identities(scene, ordered_fit):
    """What the feature is for: entry k of one view is not entry k of the next."""
    who = scene['who']
    _, _, mask = batch.load_serial_people(batch.list_frames(scene['shuffled'])[0][2], V)
    chimeras = [(f, k) for f in range(F) for k in range(3)
                if len({who[(f, v)][k] for v in range(V) if k < len(who[(f, v)]) and who[(f, v)][k] >= 0 and mask[f, k, v]}) > 1]
    assert chimeras
    with MvFit(scene['model']) as eng:
        crossed = _fit(scene, eng, 'shuffled', 'crossed', persons='all')
    clean = ordered_fit
    worst = {(f, k): float(crossed['final_loss'][n]) for n, (f, k) in
             enumerate(zip(crossed['problem_frame'].tolist(), crossed['problem_person'].tolist()))}
    print('final loss, ordered folder: max %.4g; shuffled folder without associate: %s' % (clean['final_loss'].max(), worst))
    # a problem whose views show different persons cannot be fitted as well as any real person
    assert all(worst[c] > 10.0 * float(clean['final_loss'].max()) for c in chimeras if c in worst)
    assert any(c in worst for c in chimeras)
