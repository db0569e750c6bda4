"""CPU: fit_folder's per-serial pipeline on its two paths (persons=0, and persons= a list or 'all').

The engine call log of every case is compared with tests/golden/fit_folder_calls.json; each refinement option, alone, must
reach its function with the path's problems and tracks; check_scene_collision and JOINT_PARTS are held to their literals.
The fixture is what `record_logs` returned when fit_folder still held the pipeline once per path; since then one line has
left it on purpose: the single path's set_joints3d before an is_seq chain over annotated frames (sequence.fit_sequences
sets the targets of every step itself).  To record it again: json.dump(record_logs(<empty folder>), ..., indent=1)."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

from mvsmplfitting_amd import batch
from tests.helpers import GOLD, body_model
from tests.stub_engine import StubMvFit

DATA = os.path.join(GOLD, 'demo_data')
CAMS = os.path.join(DATA, '3DOH50K_Parameters.txt')
CALLS = os.path.join(GOLD, 'fit_folder_calls.json')


class RecordingEngine(StubMvFit):
    """The stub engine with a fit that returns its input (zero losses and counts): the host logic is under test.  ``log``
    holds every call made on the engine: [method] plus [B, V] for set_problems and the number of stages for fit."""

    def __init__(self, model):
        super().__init__(model)
        self.nv = int(np.asarray(model['v_template']).shape[0])
        self.log = []

    def set_problems(self, cams, gt_xy, w_conf):
        super().set_problems(cams, gt_xy, w_conf)
        self.log.append(['set_problems', [self.B, self.V]])

    def fit(self, params, stages, **kw):
        self.log.append(['fit', len(stages)])
        x = torch.as_tensor(params).clone()
        return x, dict(final_loss=torch.zeros(x.shape[0]), n_closure=torch.zeros(x.shape[0], dtype=torch.int32),
                       n_iter=torch.zeros(x.shape[0], dtype=torch.int32))


def _logged(name):
    def call(self, *a, **kw):
        self.log.append([name])
        return getattr(StubMvFit, name)(self, *a, **kw)
    call.__name__ = name
    return call


for _name in ('set_joints3d', 'vertices', 'full_pose', 'triangulate', 'depth_guess', 'umeyama'):
    setattr(RecordingEngine, _name, _logged(_name))


def make_folder(root, people=1, frames=1, annotated=()):
    """A copy of the demo serial under root/keypoints: every file lists the demo person ``people`` times, the demo frame
    stands ``frames`` times, and the frames (0-based) in ``annotated`` carry a 'pose_keypoints_3d' entry per person."""
    j3 = np.concatenate([np.random.default_rng(3).normal(size=(17, 3)) * 0.3 + [0.0, 0.0, 3.0], np.ones((17, 1))], 1)
    src = os.path.join(DATA, 'keypoints', '0000')
    for cam in sorted(os.listdir(src)):
        with open(os.path.join(src, cam, '00001_keypoints.json')) as f:
            data = json.load(f)
        os.makedirs(os.path.join(root, 'keypoints', '0000', cam))
        for k in range(frames):
            person = dict(data['people'][0])
            if k in annotated:
                person['pose_keypoints_3d'] = [float(v) for v in j3.reshape(-1)]
            with open(os.path.join(root, 'keypoints', '0000', cam, '%05d_keypoints.json' % (k + 1)), 'w') as f:
                json.dump(dict(data, people=[dict(person) for _ in range(people)]), f)
    return os.path.join(str(root), 'keypoints')


# case -> (people per file, frames, annotated frames, fit_folder arguments)
CASES = {
    'default': (1, 1, (), dict()),
    'persons_0': (1, 1, (), dict(persons=0)),
    'persons_all': (2, 1, (), dict(persons='all')),
    'persons_1': (2, 1, (), dict(persons=[1])),
    'two_fixed_scales': (2, 1, (), dict(persons='all', fix_scale={0: 1.0, 1: 1.1})),
    'is_seq_single': (1, 3, (), dict(is_seq=True)),
    'is_seq_persons': (2, 3, (), dict(is_seq=True, persons='all')),
    'mixed_3d_single': (1, 2, (0,), dict(use_3d=True)),
    'mixed_3d_persons': (2, 2, (0,), dict(use_3d=True, persons='all')),
    'meshes_single': (1, 2, (), dict(save_meshes=True)),
    'meshes_persons': (2, 2, (), dict(save_meshes=True, persons='all')),
    'is_seq_3d_single':(1, 3, (0, 1, 2), dict(is_seq=True, use_3d=True)),
    'is_seq_3d_persons': (2, 3, (0, 1, 2), dict(is_seq=True, use_3d=True, persons='all')),
}


def run_case(name, tmp, **more):
    people, frames, annotated, kw = CASES[name]
    model = body_model()
    eng = RecordingEngine(model)
    keyp = make_folder(os.path.join(str(tmp), name), people, frames, annotated)
    out = batch.fit_folder(model, keyp, CAMS, os.path.join(str(tmp), name, 'out'), engine=eng, **dict(kw, **more))
    return eng, out['0000']


def record_logs(tmp):
    return {name: run_case(name, tmp)[0].log for name in CASES}


@pytest.mark.parametrize('name', sorted(CASES))
def test_the_engine_sees_the_recorded_calls(name, tmp_path):
    with open(CALLS) as f:
        want = json.load(f)
    assert sorted(want) == sorted(CASES)
    eng, _ = run_case(name, tmp_path)
    assert eng.log == want[name]


def test_the_cases_take_the_branches_they_are_named_for(tmp_path):
    """Two guess groups, both 3-D groups and the chain's warm steps are in the recorded logs at all."""
    with open(CALLS) as f:
        want = json.load(f)
    assert want['two_fixed_scales'].count(['umeyama']) == 2 and want['persons_all'].count(['umeyama']) == 1
    for name in ('mixed_3d_single', 'mixed_3d_persons'):
        assert want[name].count(['fit', 4]) == 2 and want[name].count(['set_joints3d']) == 1
    for name in ('is_seq_single', 'is_seq_persons'):
        assert [c for c in want[name] if c[0] == 'fit'] == [['fit', 4], ['fit', 2], ['fit', 2]]


# ---------------------------------------------------------------------------------------------- the refinements
WEIGHT = 0.375
# option -> (patched function, fit_folder argument, report key, timing key)
OPTIONS = {
    'scene_collision': ('refine_scenes', dict(weight=WEIGHT), 'scene_report', 'refine'),
    'silhouettes': ('refine_serial_silhouettes', dict(weight=WEIGHT, mask_root='masks'), 'silhouette_report', 'silhouette'),
    'scans': ('refine_serial_scans', dict(weight=WEIGHT, root='scans'), 'scan_report', 'scan'),
    'temporal': ('smooth_sequences', dict(weight=WEIGHT), 'temporal_report', 'temporal'),
    'joint': ('refine_serial_joint', dict(weight=WEIGHT, silhouettes=dict(share=1.0, mask_root='masks'), temporal=dict(share=1.0)),
              'joint_report', 'joint'),
    'refine_cameras': ('refine_serial_cameras', dict(), 'camera_report', 'cameras'),
}
OPTION_FUNCTIONS = [v[0] for v in OPTIONS.values()]


# (scene_collision exists on the multi-person path only: a ValueError otherwise, tests/test_scene_refine_cpu.py)
@pytest.mark.parametrize('option,multi', [(o, m) for o in OPTIONS for m in (False, True) if m or o != 'scene_collision'],
                         ids=lambda v: v if isinstance(v, str) else ('persons' if v else 'single'))
def test_an_option_alone_reaches_its_refinement(option, multi, tmp_path, monkeypatch):
    seen = []

    def recorder(name):
        def call(eng, xf, *a, **kw):
            seen.append((name, a, kw))
            report = dict(loss=np.zeros(xf.shape[0], np.float32))
            return (xf, report, 'the cameras') if name == 'refine_serial_cameras' else (xf, report)
        return call
    for name in OPTION_FUNCTIONS:
        monkeypatch.setattr(batch, name, recorder(name))
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **kw: None)      # (timing= on an engine without a device)
    func, arg, report_key, timing_key = OPTIONS[option]
    timing = {}
    eng, out = run_case('mixed_3d_persons' if multi else 'mixed_3d_single', tmp_path, use_3d=False, timing=timing,
                        **{option: arg})
    assert [s[0] for s in seen] == [func]
    _, a, kw = seen[0]
    F = 2
    if multi:
        problems, seq_id, frame_idx, sizes = [(0, 0), (0, 1), (1, 0), (1, 1)], [0, 1, 0, 1], [0, 0, 1, 1], [2, 2]
    else:
        problems, seq_id, frame_idx, sizes = [(f, None) for f in range(F)], [0] * F, list(range(F)), None
    last = batch.stage_weights(1536.0, flags=0)[-1]
    if option == 'scene_collision':
        assert a[0] == sizes and a[1] == dict(last, coll_loss_weight=WEIGHT) and kw == {}
    elif option == 'silhouettes':
        stage, cfg, serial, cams, frames, probs, rig, nv = a
        assert stage == last and cfg['weight'] == WEIGHT and probs == problems and nv == eng.nv
    elif option == 'scans':
        stage, cfg, serial, cams, frames, probs, rig = a
        assert stage == last and cfg['weight'] == WEIGHT and probs == problems
    elif option == 'temporal':
        assert a[0] == dict(last, coll_loss_weight=WEIGHT) and kw == dict(sweeps=3)
        assert np.asarray(a[1]).tolist() == seq_id and np.asarray(a[2]).tolist() == frame_idx
    elif option == 'joint':
        stage, cfg, serial, cams, frames, probs, rig, nv, scene_sizes, sid, fidx = a
        assert stage == last and cfg['weight'] == WEIGHT and probs == problems and nv == eng.nv
        assert scene_sizes == sizes and np.asarray(sid).tolist() == seq_id and np.asarray(fidx).tolist() == frame_idx
    else:
        stage, cfg, serial, rig, gt_xy, conf, intris, result_folder = a
        assert stage == last and cfg == batch.CAMERA_REFINE_DEFAULTS and gt_xy.shape == (len(problems), 6, 17, 2)
        assert out['cameras'] == 'the cameras'
    if option in ('silhouettes', 'scans', 'joint'):
        assert serial == '0000' and cams == ['Camera%02d' % v for v in range(6)] and [f[0] for f in frames] == ['00001', '00002']
        assert all(type(f) is int and (p is None or type(p) is int) for f, p in probs)
    assert report_key in out and set(out) & {v[2] for v in OPTIONS.values()} == {report_key}
    assert np.array_equal(out['final_loss'], np.zeros(len(problems), np.float32))
    assert timing_key in timing and set(timing) == {'read', 'init_guess', 'fit', 'write', timing_key}


# ---------------------------------------------------------------------------------------------- the option checks
def test_check_scene_collision_messages():
    ok = dict(weight=1.0)
    for args, match in (((ok, False, False), 'it needs persons= a list of ids'),
                        ((ok, True, True), 'scene_collision is not available with is_seq=True'),
                        (('x', False, True), "a dict with at least 'weight'"),
                        ((dict(sweeps=2), False, True), "a dict with at least 'weight'"),
                        ((dict(weight=1.0, grid=3), False, True), r"scene_collision: unknown keys \['grid'\]")):
        with pytest.raises(ValueError, match=match):
            batch.check_scene_collision(*args)
    # in the order of the inline checks: the path, then is_seq, then the dict, then its keys
    with pytest.raises(ValueError, match='it needs persons='):
        batch.check_scene_collision('x', True, False)
    with pytest.raises(ValueError, match='is_seq=True'):
        batch.check_scene_collision('x', True, True)
    with pytest.raises(ValueError, match="at least 'weight'"):
        batch.check_scene_collision(dict(grid=3), False, True)
    batch.check_scene_collision(dict(weight=1.0, sweeps=3, grid_size=32, robustifier=0.05, scale_factor=0.2), False, True)
    assert 'check_scene_collision' in batch.__all__


def test_joint_parts_are_the_literals():
    assert batch.JOINT_PARTS == dict(
        scene_collision=dict(grid_size=32, robustifier=0.05, scale_factor=0.2),
        silhouettes=dict(w_in=1.0, w_out=1.0, sigma=0.0, contour_stride=1, downscale=1, max_mask_bytes=2 ** 31),
        temporal=dict(),
        scans=dict(root=None, depth_root=None, w_s2m=1.0, w_m2s=0.0, sigma=0.05, max_points=8192, stride=1, mask_root=None))
    assert list(batch.JOINT_PARTS) == ['scene_collision', 'silhouettes', 'temporal', 'scans']
