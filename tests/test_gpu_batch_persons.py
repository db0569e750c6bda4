"""GPU: fit_folder(persons=...) on a synthetic three-person serial written in the reference's file formats: 3 persons with
their own shape a metre apart, 4 views, 3 frames, exact projected keypoints; person 1 is missing from view 2 in frame 1
(all-zero entry), person 2 from frame 2 altogether."""
import json
import os
import pickle

import numpy as np
import pytest

from mvsmplfitting_amd import batch
from mvsmplfitting_amd import io_formats as iof
from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import SCENE_PALETTE, MvFit
from tests.helpers import body_model

pytestmark = pytest.mark.gpu

V, F, P = 4, 3, 3
BASE = np.array([[-1.1, 0.0, 0.0], [0.0, 0.0, 0.1], [1.1, 0.0, -0.1]], np.float32)
PROBLEMS = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1)]          # (frame, person), as fit_folder orders them


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


@pytest.fixture(scope='module')
def scene(tmp_path_factory):
    root = tmp_path_factory.mktemp('persons')
    model = body_model()
    cams = syn.make_camera_ring(V)
    xgt = _truth()
    with MvFit(model) as eng:
        eng.set_problems(cams, np.zeros((F * P, V, 17, 2), np.float32), np.zeros((F * P, V, 17), np.float32))
        _, joints = eng.vertices(xgt.reshape(F * P, 118))
    joints = joints.cpu().numpy()
    uv = syn.project_points(joints, *cams).reshape(F, P, V, 17, 2)
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
    for v in range(V):
        d = root / 'keypoints' / 's0' / ('Camera%02d' % v)
        d.mkdir(parents=True)
        for f in range(F):
            people = []
            for p in range(P if f < 2 else 2):                      # frame 2 lists two persons only
                k2 = np.concatenate([uv[f, p, v], np.ones((17, 1))], 1)
                if (f, p, v) == (1, 1, 2):
                    k2[:] = 0                                       # person 1 is not detected by view 2 in frame 1
                people.append(dict(pose_keypoints_2d=[float(x) for x in k2.reshape(-1)]))
            with open(d / ('%05d_keypoints.json' % f), 'w') as fh:
                json.dump(dict(version=1.0, people=people), fh)
    return dict(root=root, keyp=str(root / 'keypoints'), cams=str(root / 'cams.txt'), model=model, xgt=xgt, rig=cams)


def _fit(scene, eng, name, **kw):
    return batch.fit_folder(scene['model'], scene['keyp'], scene['cams'], str(scene['root'] / name), engine=eng, **kw)['s0']


def _tree(folder):
    return sorted(os.path.relpath(os.path.join(d, f), folder) for d, _, fs in os.walk(folder) for f in fs)


def _same_bytes(a, b):
    with open(a, 'rb') as fa, open(b, 'rb') as fb:
        return fa.read() == fb.read()


def test_all_persons_are_independent_problems(scene):
    xgt = scene['xgt']
    with MvFit(scene['model']) as eng:
        out = _fit(scene, eng, 'all', persons='all', save_meshes=True)
        assert list(zip(out['problem_frame'].tolist(), out['problem_person'].tolist())) == PROBLEMS
        assert out['persons'] == [0, 1, 2] and out['params'].shape == (8, 118)
        want = sorted(os.path.join(sub, 's0', '%05d' % f, '%03d.%s' % (p, ext)) for f, p in PROBLEMS
                      for sub, ext in (('', 'pkl'), ('meshes', 'obj')))
        assert _tree(scene['root'] / 'all') == [os.path.normpath(w) for w in want]
        assert out['views_per_frame'].tolist() == [4, 4, 4, 4, 3, 4, 4, 4]
        assert np.all(np.isfinite(out['final_loss']))
        # identities are not crossed: every fitted root translation is nearest to its own person's
        for n, (f, p) in enumerate(PROBLEMS):
            d = np.linalg.norm(out['params'][n, 82:85][None] - xgt[f, :, 82:85], axis=1)
            assert int(np.argmin(d)) == p, (f, p, d)
        # each row is, bit for bit, the row that person gets when fitted alone
        for p in range(P):
            solo = _fit(scene, eng, 'solo%d' % p, persons=[p])
            rows = [n for n, (_, q) in enumerate(PROBLEMS) if q == p]
            assert solo['problem_person'].tolist() == [p] * len(rows)
            assert solo['problem_frame'].tolist() == [PROBLEMS[n][0] for n in rows]
            for k in ('params', 'final_loss', 'n_closure'):
                assert np.array_equal(solo[k], out[k][rows]), (p, k)
            for n, path in zip(rows, solo['files']):
                assert os.path.basename(path) == '%03d.pkl' % p and _same_bytes(path, out['files'][n])
        # person 0 mode is the call without the argument, files included
        a, b = _fit(scene, eng, 'plain'), _fit(scene, eng, 'zero', persons=0)
        assert _tree(scene['root'] / 'plain') == _tree(scene['root'] / 'zero') == [
            os.path.join('s0', '%05d' % f, '000.pkl') for f in range(F)]
        assert sorted(a) == sorted(b) and 'problem_person' not in a
        for k in ('params', 'final_loss', 'n_closure', 'init'):
            assert np.array_equal(a[k], b[k]), k
        for x, y in zip(a['files'], b['files']):
            assert _same_bytes(x, y)


def test_sequence_mode_chains_each_person_over_their_own_frames(scene):
    with MvFit(scene['model']) as eng:
        out = _fit(scene, eng, 'seq_all', persons='all', is_seq=True)
        assert list(zip(out['problem_frame'].tolist(), out['problem_person'].tolist())) == PROBLEMS     # no (2, 2)
        assert _tree(scene['root'] / 'seq_all') == sorted(os.path.join('s0', '%05d' % f, '%03d.pkl' % p) for f, p in PROBLEMS)
        assert np.all(np.isfinite(out['final_loss'])) and np.all(np.isfinite(out['params']))
        # every chain starts cold at the person's first frame
        assert all(out['restarted'][n] for n, (f, _) in enumerate(PROBLEMS) if f == 0)
        for p in (0, 1):
            solo = _fit(scene, eng, 'seq_solo%d' % p, persons=[p], is_seq=True)
            rows = [n for n, (_, q) in enumerate(PROBLEMS) if q == p]
            for k in ('params', 'final_loss', 'n_closure', 'restarted'):
                assert np.array_equal(solo[k], out[k][rows]), (p, k)


def test_save_images_draws_every_person_of_the_frame(scene):
    pytest.importorskip('PIL')
    yy, xx = np.mgrid[0:1536, 0:2048]
    for v in range(V):
        d = scene['root'] / 'images' / 's0' / ('Camera%02d' % v)
        d.mkdir(parents=True, exist_ok=True)
        base = np.stack([(xx * 255 // 2047), (yy * 255 // 1535), np.full_like(xx, 40 * v)], -1).astype(np.uint8)
        for f in range(F):
            iof.save_image(str(d / ('%05d.jpg' % f)), base)
    palette = np.asarray(SCENE_PALETTE, np.float32)
    with MvFit(scene['model']) as eng:
        out = _fit(scene, eng, 'img', persons='all', save_images=True)
        assert out['images'] == [str(scene['root'] / 'img' / 'images' / 's0' / ('%05d' % f) / ('Camera%02d.jpg' % v))
                                 for f in range(F) for v in range(V)]
        assert all(os.path.isfile(p) for p in out['images'])
        x = out['params'].copy()
        for n, path in enumerate(out['files']):
            with open(path, 'rb') as fh:
                x[n, 13:82] = pickle.load(fh)['body_pose'][0]
        eng.set_problems(scene['rig'], np.zeros((8, V, 17, 2), np.float32), np.zeros((8, V, 17), np.float32))
        verts, joints = eng.vertices(x, flags=0)
        two_visible = False
        for f in range(F):
            rows = [n for n, (g, _) in enumerate(PROBLEMS) if g == f]
            cols = palette[[PROBLEMS[n][1] % 7 for n in rows]]
            imgs = np.stack([iof.read_image(str(scene['root'] / 'images' / 's0' / ('Camera%02d' % v) / ('%05d.jpg' % f)))
                             for v in range(V)])
            want, bid = eng.render_scene(verts, joints, imgs, [rows] * V, list(range(V)), colors=np.tile(cols, (V, 1)),
                                         body_id=True)
            want, bid = want.cpu().numpy(), bid.cpu().numpy()
            for v in range(V):
                got = iof.read_image(out['images'][f * V + v])
                assert got.shape == (1536, 2048, 3)
                mad = np.abs(got.astype(np.int16) - want[v].astype(np.int16)).mean()
                print('frame %d view %d: mean absolute difference %.3f, bodies visible %s'
                      % (f, v, mad, sorted(set(np.unique(bid[v]).tolist()) - {-1})))
                assert mad < 2.0, (f, v, mad)
                two_visible |= len(set(np.unique(bid[v]).tolist()) - {-1}) >= 2
        assert two_visible
