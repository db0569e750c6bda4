"""CPU: io_formats.read_people / read_people3d (which entry of a keypoint file is which person) and
batch.load_serial_people on a ragged tree."""
import json

import numpy as np
import pytest

from mvsmplfitting_amd import batch
from mvsmplfitting_amd import io_formats as iof


def _kp(seed, zero=False):
    a = np.random.default_rng(seed).uniform(1, 100, (17, 3)).astype(np.float32)
    if zero:
        a[:] = 0
    return a


def _write(path, entries):
    """entries: [(keypoints [17,3], person_id or None, joints3d [17,4] or None)]"""
    people = []
    for kp, pid, j3 in entries:
        p = {'pose_keypoints_2d': [float(v) for v in kp.reshape(-1)]}
        if pid is not None:
            p['person_id'] = pid
        if j3 is not None:
            p['pose_keypoints_3d'] = [float(v) for v in j3.reshape(-1)]
        people.append(p)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps({'version': 1.3, 'people': people}))
    return str(path)


def test_index_files(tmp_path):
    a, b = _kp(1), _kp(2)
    p = _write(tmp_path / 'a.json', [(a, None, None), (b, None, None)])
    got = iof.read_people(p)
    assert sorted(got) == [0, 1] and np.array_equal(got[0], a) and np.array_equal(got[1], b)
    assert got[0].dtype == np.float32 and got[0].shape == (17, 3)
    # read_keypoints stays the list it was
    old = iof.read_keypoints(p)
    assert len(old) == 2 and np.array_equal(old[1], b)


def test_id_files(tmp_path):
    a, b = _kp(1), _kp(2)
    got = iof.read_people(_write(tmp_path / 'a.json', [(a, 7, None), (b, 2, None)]))
    assert sorted(got) == [2, 7] and np.array_equal(got[7], a) and np.array_equal(got[2], b)


def test_mixed_files_fall_back_to_the_index(tmp_path):
    a, b = _kp(1), _kp(2)
    got = iof.read_people(_write(tmp_path / 'a.json', [(a, 7, None), (b, None, None)]))
    assert sorted(got) == [0, 1] and np.array_equal(got[0], a)
    # a non-integer id is no id
    got = iof.read_people(_write(tmp_path / 'b.json', [(a, 'x', None), (b, 3, None)]))
    assert sorted(got) == [0, 1]


def test_all_zero_entries_are_absent(tmp_path):
    a, b = _kp(1), _kp(2)
    got = iof.read_people(_write(tmp_path / 'a.json', [(a, None, None), (_kp(0, zero=True), None, None), (b, None, None)]))
    assert sorted(got) == [0, 2] and np.array_equal(got[2], b)
    # coordinates without any confidence: absent too
    c = _kp(3)
    c[:, 2] = 0
    assert sorted(iof.read_people(_write(tmp_path / 'b.json', [(c, None, None), (b, None, None)]))) == [1]
    assert iof.read_people(_write(tmp_path / 'c.json', [])) == {}


def test_duplicate_ids_name_the_file(tmp_path):
    p = _write(tmp_path / 'dup.json', [(_kp(1), 4, None), (_kp(2), 4, None)])
    with pytest.raises(ValueError, match='dup.json'):
        iof.read_people(p)
    # an absent duplicate is no duplicate
    assert sorted(iof.read_people(_write(tmp_path / 'ok.json', [(_kp(1), 4, None), (_kp(0, zero=True), 4, None)]))) == [4]


def test_people3d_by_the_same_rule(tmp_path):
    j = np.random.default_rng(5).uniform(-1, 1, (17, 4)).astype(np.float32)
    j[:, 3] = 1
    got = iof.read_people3d(_write(tmp_path / 'a.json', [(_kp(1), 5, None), (_kp(2), 9, j)]))
    assert sorted(got) == [9] and np.array_equal(got[9], j) and got[9].shape == (17, 4)
    got = iof.read_people3d(_write(tmp_path / 'b.json', [(_kp(1), None, None), (_kp(2), None, j)]))
    assert sorted(got) == [1]


def test_load_serial_people_on_a_ragged_tree(tmp_path):
    """3 cameras, 2 frames, persons 0 / 1 / 2 by index: person 1 is missing from camera 1 in frame 0 (all-zero entry),
    person 2 from frame 1 altogether (shorter lists), and camera 2 has no file for frame 1."""
    root = tmp_path / 'keypoints' / 's'
    kp = {(f, p, v): _kp(100 * f + 10 * p + v) for f in range(2) for p in range(3) for v in range(3)}
    zero = _kp(0, zero=True)
    for v in range(3):
        e0 = [(kp[0, p, v], None, None) for p in range(3)]
        if v == 1:
            e0[1] = (zero, None, None)
        _write(root / ('Camera%02d' % v) / '00001_keypoints.json', e0)
        if v != 2:
            _write(root / ('Camera%02d' % v) / '00002_keypoints.json', [(kp[1, p, v], None, None) for p in range(2)])
    (serial, cams, frames), = batch.list_frames(str(tmp_path / 'keypoints'))
    ids, arr, mask = batch.load_serial_people(frames, 3)
    assert ids == [0, 1, 2] and arr.shape == (2, 3, 3, 17, 3) and arr.dtype == np.float32 and mask.shape == (2, 3, 3)
    want = np.ones((2, 3, 3), bool)
    want[0, 1, 1] = False          # the all-zero entry
    want[1, 2, :] = False          # person 2 is not in frame 1
    want[1, :, 2] = False          # camera 2 has no file for frame 1
    assert np.array_equal(mask, want)
    for f in range(2):
        for p in range(3):
            for v in range(3):
                assert np.array_equal(arr[f, p, v], kp[f, p, v] if want[f, p, v] else zero), (f, p, v)
    # person 0's slice is what load_serial reads
    old, old_mask = batch.load_serial(frames, 3, return_mask=True)
    assert np.array_equal(arr[:, 0], old) and np.array_equal(mask[:, 0], old_mask)
