"""CPU: the association contracts in their NumPy restatement (tests/associate_oracle.py), the host modules of
mvsmplfitting_amd/associate.py and the ``associate`` argument errors of fit_folder."""
import json

import numpy as np
import pytest

from mvsmplfitting_amd import associate as assoc
from mvsmplfitting_amd import batch
from mvsmplfitting_amd import synthetic as syn
from tests import associate_oracle as ao
from tests.helpers import body_model

MAX_COST = assoc.DEFAULTS['max_cost']
INF = np.inf


def test_decisive_scene_is_recovered_and_is_decisive():
    s = ao.decisive_scene(syn.make_camera_ring(4))
    assert MAX_COST == 0.05
    cost, labels, num = ao.associate(s['kp'], s['count'], s['K'], s['E'], max_cost=MAX_COST)
    truth = s['truth'][0].reshape(-1)
    assert s['count'][0].tolist() == [3, 4, 2, 3] and (truth == -1).sum() == 16 - 12 + 1       # empty slots + the false positive
    # decisive: every true pair far below the threshold, every false pair far above - labels never hinge on rounding
    V, N = s['kp'].shape[1:3]
    view = np.repeat(np.arange(V), N)
    valid = (np.arange(N)[None] < s['count'][0][:, None]).reshape(-1)
    cross = valid[:, None] & valid[None, :] & (view[:, None] != view[None, :])
    true = cross & (truth[:, None] == truth[None, :]) & (truth[:, None] >= 0)
    print('true pairs: max %.4f m; false pairs: min %.4f m' % (cost[0][true].max(), cost[0][cross & ~true].min()))
    assert true.sum() == 2 * (6 + 3 + 6)
    assert cost[0][true].max() < MAX_COST / 2
    assert cost[0][cross & ~true].min() > 2 * MAX_COST
    assert np.array_equal(cost[0], cost[0].T) and np.all(np.isinf(cost[0][~cross]))
    assert num[0] == 3
    assert ao.same_partition(labels[0], s['truth'][0])
    # numbered in ascending order of the smallest member
    lab = labels[0].reshape(-1)
    firsts = [int(np.flatnonzero(lab == c)[0]) for c in range(3)]
    assert firsts == sorted(firsts)


def test_tie_goes_to_the_lexicographically_smallest_pair():
    # three views, one detection each; 0 and 1 are different persons, 2 is exactly as close to both
    c = np.array([[INF, 1.0, 0.01],
                  [1.0, INF, 0.01],
                  [0.01, 0.01, INF]])
    labels, n = ao.cluster(c, np.ones(3, bool), MAX_COST, 2)
    assert labels.tolist() == [0, -1, 0] and n == 1                 # (0, 2) before (1, 2); then L({0, 2}, 1) = 1.0
    # the second index decides between pairs with the same first one
    c = np.full((4, 4), INF)
    for a, b, x in ((0, 1, 0.02), (0, 2, 0.02), (1, 2, 1.0), (0, 3, 1.0), (1, 3, 1.0), (2, 3, 1.0)):
        c[a, b] = c[b, a] = x
    labels, n = ao.cluster(c, np.ones(4, bool), MAX_COST, 2)
    assert labels.tolist() == [0, 0, -1, -1] and n == 1


def test_complete_linkage_does_not_chain_through_a_middle_detection():
    # view 0: a of person P, view 1: m between the two, view 2: b of person Q
    c = np.array([[INF, 0.03, 0.2],
                  [0.03, INF, 0.04],
                  [0.2, 0.04, INF]])
    labels, n = ao.cluster(c, np.ones(3, bool), MAX_COST, 2)
    assert labels.tolist() == [0, 0, -1] and n == 1                 # single linkage would give [0, 0, 0]
    # cannot-link: two detections of one view (+inf between them) never end in one cluster, however close to a third
    c = np.array([[INF, INF, 0.01],
                  [INF, INF, 0.02],
                  [0.01, 0.02, INF]])
    labels, n = ao.cluster(c, np.ones(3, bool), MAX_COST, 2)
    assert labels.tolist() == [0, -1, 0] and n == 1


def _walk(F, starts, steps):
    return np.stack([np.asarray(starts, float) + f * np.asarray(steps, float) for f in range(F)])      # [F, C, 3]


def test_tracks_persist_under_a_permutation_of_the_clusters():
    F = 6
    c = _walk(F, [[0, 0, 0], [2, 0, 0], [4, 0, 0]], [[0.1, 0, 0], [0, 0.1, 0], [0, 0, -0.1]])
    rng = np.random.default_rng(3)
    perm = [np.arange(3)] + [rng.permutation(3) for _ in range(F - 1)]
    shuffled = np.stack([c[f][perm[f]] for f in range(F)])
    ids = assoc.track_clusters(shuffled, np.ones((F, 3), bool))
    assert np.array_equal(ids, np.stack(perm))


@pytest.mark.parametrize('gap, same', [(5, True), (6, False)])
def test_an_absent_person_keeps_their_id_for_max_gap_frames(gap, same):
    F = 2 + gap
    c = np.zeros((F, 2, 3))
    c[:, 1] = [3.0, 0, 0]
    valid = np.ones((F, 2), bool)
    valid[1:1 + gap, 1] = False                                     # person 1 is away for `gap` frames
    ids = assoc.track_clusters(c, valid, max_move=0.5, max_gap=5)
    assert np.all(ids[:, 0] == 0) and ids[0, 1] == 1 and np.all(ids[1:1 + gap, 1] == -1)
    assert ids[-1, 1] == (1 if same else 2)


def test_a_newcomer_gets_the_next_id():
    c = np.zeros((3, 3, 3))
    c[:, 1], c[:, 2] = [2.0, 0, 0], [0, 0, 5.0]
    valid = np.ones((3, 3), bool)
    valid[0, 2] = False
    ids = assoc.track_clusters(c, valid)
    assert ids.tolist() == [[0, 1, -1], [0, 1, 2], [0, 1, 2]]


def test_two_persons_passing_each_other_keep_their_ids():
    # 0.3 m apart (inside max_move = 0.5 of each other), each moving 0.1 m per frame: less than half the separation
    F = 8
    c = _walk(F, [[-0.35, 0, 0.15], [0.35, 0, -0.15]], [[0.1, 0, 0], [-0.1, 0, 0]])
    assert np.linalg.norm(c[:, 0] - c[:, 1], axis=1).min() < 0.5
    flip = np.arange(F) % 2 == 1                                    # the cluster order alternates
    c[flip] = c[flip][:, ::-1]
    ids = assoc.track_clusters(c, np.ones((F, 2), bool), max_move=0.5)
    assert np.array_equal(ids[:, 0], np.where(flip, 1, 0)) and np.array_equal(ids[:, 1], np.where(flip, 0, 1))


def _write(path, people):
    with open(path, 'w') as fh:
        json.dump(dict(version=1.0, people=people), fh)


def _entry(seed, person_id=None, zero=False):
    k = np.random.default_rng(seed).uniform(1, 100, (17, 3)).astype(np.float32)
    if zero:
        k[:] = 0
    e = dict(pose_keypoints_2d=[float(x) for x in k.reshape(-1)])
    if person_id is not None:
        e['person_id'] = person_id
    return e, k


def test_load_serial_detections(tmp_path):
    (e0, k0), (e1, k1), (ez, _), (e2, k2) = _entry(0, 7), _entry(1, 3), _entry(2, 5, zero=True), _entry(3, 0)
    _write(tmp_path / 'a.json', [e0, ez, e1])                      # person_id 7, (all zero), 3: file order counts
    _write(tmp_path / 'b.json', [e2])
    frames = [('00000', [str(tmp_path / 'a.json'), None]), ('00001', [str(tmp_path / 'b.json'), str(tmp_path / 'a.json')])]
    det, count, slot = assoc.load_serial_detections(frames, 2)
    assert det.shape == (2, 2, 2, 17, 3) and det.dtype == np.float32
    assert count.tolist() == [[2, 0], [1, 2]]
    assert slot.tolist() == [[[0, 2], [-1, -1]], [[0, -1], [0, 2]]]
    assert np.array_equal(det[0, 0, 0], k0) and np.array_equal(det[0, 0, 1], k1) and np.array_equal(det[1, 0, 0], k2)
    assert np.array_equal(det[1, 1], det[0, 0]) and not det[0, 1].any() and not det[1, 0, 1].any()
    _write(tmp_path / 'many.json', [_entry(10 + i)[0] for i in range(17)])
    with pytest.raises(ValueError, match='many.json'):
        assoc.load_serial_detections([('00000', [str(tmp_path / 'many.json'), None])], 2)
    _write(tmp_path / 'ok.json', [_entry(10 + i)[0] for i in range(16)] + [ez])
    assert assoc.load_serial_detections([('00000', [str(tmp_path / 'ok.json'), None])], 2)[1].tolist() == [[16, 0]]


def test_cluster_keypoints_rows():
    det = np.arange(1 * 3 * 2 * 17 * 3, dtype=np.float32).reshape(1, 3, 2, 17, 3)
    labels = np.array([[[1, 0], [0, -1], [-1, 1]]])
    rows, kp, member = assoc.cluster_keypoints(det, labels, [2])
    assert rows.tolist() == [[0, 0], [0, 1]] and member.tolist() == [[True, True, False], [True, False, True]]
    assert np.array_equal(kp[0, 0], det[0, 0, 1]) and np.array_equal(kp[0, 1], det[0, 1, 0]) and not kp[0, 2].any()
    assert np.array_equal(kp[1, 0], det[0, 0, 0]) and np.array_equal(kp[1, 2], det[0, 2, 1])


def test_fit_folder_associate_argument_errors(tmp_path):
    """Raised before any engine is created (engine=None and no GPU here) and before any file is read."""
    model = body_model()
    run = lambda **kw: batch.fit_folder(model, str(tmp_path / 'none'), str(tmp_path / 'none.txt'), str(tmp_path / 'out'), **kw)
    with pytest.raises(ValueError, match='persons'):
        run(associate=True)
    with pytest.raises(ValueError, match='persons'):
        run(associate=dict(max_cost=0.1), persons=0)
    with pytest.raises(ValueError, match='max_cots'):
        run(associate=dict(max_cots=0.1), persons='all')
    with pytest.raises(ValueError, match='use_3d'):
        run(associate=True, persons='all', use_3d=True)
    with pytest.raises(ValueError, match='associate'):
        run(associate='yes', persons='all')
    assert assoc.check_params(True) == assoc.DEFAULTS and assoc.check_params(dict(max_gap=2))['max_gap'] == 2
