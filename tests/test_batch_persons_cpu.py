"""CPU: fit_folder(persons=...) host logic with the recording stub engine (tests/stub_engine.py) on a copy of the demo
folder whose files list the demo person twice."""
import json
import os
import pickle
import shutil
import warnings

import numpy as np
import pytest

from mvsmplfitting_amd import batch
from mvsmplfitting_amd.engine import stage_weights
from tests.helpers import GOLD, body_model
from tests.stub_engine import StubMvFit

DATA = os.path.join(GOLD, 'demo_data')
CAMS = os.path.join(DATA, '3DOH50K_Parameters.txt')
STAGES = stage_weights(1536.0)[:1]           # one stage: the host logic is under test, not the fit


@pytest.fixture(scope='module')
def doubled(tmp_path_factory):
    """The demo folder with every file's person listed twice."""
    root = tmp_path_factory.mktemp('doubled')
    shutil.copytree(os.path.join(DATA, 'keypoints'), root / 'keypoints')
    for d, _, files in os.walk(root / 'keypoints'):
        for fn in files:
            if fn.endswith('_keypoints.json'):
                with open(os.path.join(d, fn)) as f:
                    data = json.load(f)
                data['people'] = [data['people'][0], dict(data['people'][0])]
                with open(os.path.join(d, fn), 'w') as f:
                    json.dump(data, f)
    return str(root / 'keypoints')


def _run(keyp, out, **kw):
    model = body_model()
    return batch.fit_folder(model, keyp, CAMS, str(out), engine=StubMvFit(model), stages=STAGES, **kw)['0000']


def _files(folder):
    return sorted(os.path.relpath(os.path.join(d, f), folder) for d, _, fs in os.walk(folder) for f in fs)


def _bytes(path):
    with open(path, 'rb') as f:
        return f.read()


def test_all_writes_one_file_per_person_with_equal_content(doubled, tmp_path):
    out = _run(doubled, tmp_path / 'all', persons='all', save_meshes=True)
    assert out['persons'] == [0, 1]
    assert out['problem_frame'].tolist() == [0, 0] and out['problem_person'].tolist() == [0, 1]
    assert out['params'].shape == (2, 118) and out['final_loss'].shape == (2,)
    assert _files(tmp_path / 'all') == sorted([os.path.join('0000', '00001', '000.pkl'), os.path.join('0000', '00001', '001.pkl'),
                                               os.path.join('meshes', '0000', '00001', '000.obj'),
                                               os.path.join('meshes', '0000', '00001', '001.obj')])
    assert out['files'] == [str(tmp_path / 'all' / '0000' / '00001' / ('%03d.pkl' % p)) for p in (0, 1)]
    assert _bytes(out['files'][0]) == _bytes(out['files'][1])
    assert np.array_equal(out['params'][0], out['params'][1])
    with open(out['files'][1], 'rb') as f:
        res = pickle.load(f)
    assert set(res) == {'betas', 'global_orient', 'transl', 'scale', 'loss', 'pose_embedding', 'body_pose', 'pose'}
    # ... and it is what the single-person path writes for that person
    single = _run(doubled, tmp_path / 'single')
    assert _bytes(single['files'][0]) == _bytes(out['files'][0])


def test_person_zero_is_the_path_without_the_argument(doubled, tmp_path):
    a = _run(doubled, tmp_path / 'a')
    b = _run(doubled, tmp_path / 'b', persons=0)
    assert _files(tmp_path / 'a') == _files(tmp_path / 'b') == [os.path.join('0000', '00001', '000.pkl')]
    assert _bytes(a['files'][0]) == _bytes(b['files'][0])
    assert sorted(a) == sorted(b) and 'problem_person' not in b
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), k


def test_one_other_person(doubled, tmp_path):
    out = _run(doubled, tmp_path / 'one', persons=[1])
    assert _files(tmp_path / 'one') == [os.path.join('0000', '00001', '001.pkl')]
    assert out['persons'] == [1] and out['problem_person'].tolist() == [1]
    same = _run(doubled, tmp_path / 'int', persons=1)
    assert _files(tmp_path / 'int') == [os.path.join('0000', '00001', '001.pkl')]
    assert _bytes(same['files'][0]) == _bytes(out['files'][0])


def test_absent_persons_warn_and_bad_arguments_raise(doubled, tmp_path):
    model = body_model()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        out = batch.fit_folder(model, doubled, CAMS, str(tmp_path / 'none'), engine=StubMvFit(model), stages=STAGES, persons=[5])
    assert out == {} and any(issubclass(x.category, RuntimeWarning) for x in w)
    assert _files(tmp_path / 'none') == []
    with pytest.raises(ValueError):
        batch.fit_folder(model, doubled, CAMS, str(tmp_path / 'x'), engine=StubMvFit(model), persons='everyone')
    with pytest.raises(ValueError):
        batch.fit_folder(model, doubled, CAMS, str(tmp_path / 'x'), engine=StubMvFit(model), persons=[0, 1],
                         fix_scale={0: 1.0})
