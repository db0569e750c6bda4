"""GPU: fit_folder(persons='all', silhouettes=dict(..., occlusion=...)) on one frame of two full bodies seen by a ring of four
192 x 256 cameras: person 0 stands in front of person 1 in view 0, behind them in view 2 and beside them in views 1 and 3.
Keypoints are projected exactly from the truth; the masks are the body_id of mvfit_render_scene at the truth (modal: a mask
lacks what the person in front covers), written as PNG `<frame>_<id:03d>.png`.

Two sweeps, the default.  refine_fit_occluded drops the captured round graph before the second sweep, so that its fit runs
on a graph of its own (a default-length fit that replays a graph captured before the maps changed is
not reproducible from engine to engine); the two engines compared here have the same history of calls."""
import json
import pickle

import numpy as np
import pytest

from mvsmplfitting_amd import batch
from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import MvFit, MvFitError, stage_weights
from mvsmplfitting_amd.silhouette import refine_fit_occluded
from tests.helpers import body_model

pytestmark = pytest.mark.gpu

V, P, H, W = 4, 2, 192, 256
OFFSET = np.array([[0.1, 0.0, 0.4], [0.0, 0.0, -0.4]], np.float32)
WEIGHT, OCC = 0.05, dict(margin=0.02, sweeps=2)


def _truth():
    x = np.zeros((P, 118), np.float32)
    for p in range(P):
        fr = syn.make_frames(1, seed0=7300 + 100 * p)
        for k, (a, b) in dict(global_orient=(10, 13), body_pose=(13, 82)).items():
            x[p, a:b] = fr[k][0]
        x[p, 85] = 1.0
        x[p, 82:85] = OFFSET[p]
    return x


def test_folder_with_occlusion_equals_the_driver_by_hand(tmp_path):
    from PIL import Image
    model = body_model()
    R, t, _, _ = syn.make_camera_ring(V, radius=4.0)
    cams = (R, t, np.full(V, 300.0, np.float32), np.tile(np.array([W / 2.0, H / 2.0], np.float32), (V, 1)))
    xgt = _truth()
    eng = MvFit(model)
    try:
        eng.set_problems(cams, np.zeros((P, V, 17, 2), np.float32), np.zeros((P, V, 17), np.float32))
        verts, joints = eng.vertices(xgt)
        uv = syn.project_points(joints.cpu().numpy(), *cams)                 # [P, V, 17, 2]
        _, bid = eng.render_scene(verts, None, np.zeros((V, H, W, 3), np.uint8), [[0, 1]] * V, list(range(V)), body_id=True)
        bid = bid.cpu().numpy()
        cam_R, cam_t, cam_f, cam_c = (np.asarray(a, np.float64) for a in cams)
        with open(tmp_path / 'cams.txt', 'w') as fh:
            for v in range(V):
                fh.write('%d\n' % v)
                K = np.array([[cam_f[v], 0, cam_c[v, 0]], [0, cam_f[v], cam_c[v, 1]], [0, 0, 1]])
                for r in K:
                    fh.write(' '.join('%.10f' % x for x in r) + '\n')
                fh.write('0 0\n')
                for r in np.hstack([cam_R[v], cam_t[v][:, None]]):
                    fh.write(' '.join('%.10f' % x for x in r) + '\n')
        for v in range(V):
            d = tmp_path / 'keypoints' / 's0' / ('Camera%02d' % v)
            d.mkdir(parents=True)
            people = [dict(pose_keypoints_2d=[float(x) for x in np.concatenate([uv[p, v], np.ones((17, 1))], 1).reshape(-1)])
                      for p in range(P)]
            with open(d / '00000_keypoints.json', 'w') as fh:
                json.dump(dict(version=1.0, people=people), fh)
        keyp, cam_file, root = str(tmp_path / 'keypoints'), str(tmp_path / 'cams.txt'), tmp_path / 'masks'
        serial, cam_names, frames = batch.list_frames(keyp)[0]
        masks = np.zeros((P, V, H, W), np.uint8)
        for p in range(P):
            for v, cam in enumerate(cam_names):
                masks[p, v] = (bid[v] == p) * 255
                path = batch.mask_path(str(root), serial, cam, frames[0][0], p)
                (root / serial / cam).mkdir(parents=True, exist_ok=True)
                Image.fromarray(masks[p, v], 'L').save(path)
        full = [(bid[v] == 1).sum() for v in range(V)]
        print('person 1 visible pixels per view: %s' % full)
        assert full[0] < 0.8 * min(full[1], full[3])                        # covered in view 0

        def fit(name, engine=eng, **kw):
            return batch.fit_folder(model, keyp, cam_file, str(tmp_path / name), engine=engine, persons='all', **kw)['s0']

        # two engines with the same history - a keypoint fit, then the refinement: a fit's bits may depend on which of the
        # engine's buffers earlier calls have made.  By hand first: the problems are still set as fit_folder set them
        eng.close()
        eng = MvFit(model)
        base = fit('plain', engine=eng)
        ex, it = batch.iof.load_camera_para(cam_file)
        ex, it = np.asarray(ex[:V], np.float64), np.asarray(it[:V], np.float64)
        rig = (ex[:, :3, :3].astype(np.float32), ex[:, :3, 3].astype(np.float32), it[:, 0, 0].astype(np.float32),
               it[:, :2, 2].astype(np.float32))
        view = np.tile(np.arange(V), P)
        eng.set_silhouettes(masks.reshape(P * V, H, W), np.repeat(np.arange(P), V).astype(np.int32), tuple(a[view] for a in rig))
        stage = dict(stage_weights(1536.0)[-1], coll_loss_weight=WEIGHT)
        hand, hrep = refine_fit_occluded(eng, base['params'], stage, [0, 0], **OCC)
        eng.clear_silhouettes()
        eng.close()
        eng = MvFit(model)
        out = fit('occluded', engine=eng, silhouettes=dict(mask_root=str(root), weight=WEIGHT, occlusion=OCC))
        rep = out['silhouette_report']
        for s in rep['sweeps']:
            print('sweep: accepted %s hidden %s flagged %s' % (s['accepted'], s['hidden'], s['flagged']))
        assert len(rep['sweeps']) == 2
        assert rep['images'] == [(n, v) for n in range(P) for v in range(V)] and rep['mask_size'] == (H, W)
        s0 = rep['sweeps'][0]
        # images are (person, view): person 1 stands behind person 0 in view 0, person 0 behind person 1 in view 2 (the camera
        # opposite), and nobody hides anybody in the side views
        assert s0['hidden'][V + 0] > 0 and s0['flagged'][V + 0] > 0 and s0['hidden'][2] > 0 and s0['flagged'][2] > 0
        assert s0['hidden'][0] == 0 and s0['hidden'][V + 2] == 0
        assert not s0['hidden'][[1, 3, V + 1, V + 3]].any()
        # the engine is left clean: no occluders, no term, no mask set
        with pytest.raises(MvFitError, match='error -3'):
            eng.silhouette_occluders()
        with pytest.raises(MvFitError, match='error -3'):
            eng.set_silhouette_term()
        print('by hand against the folder: max |difference| of the parameters %.3g; sweeps by hand: %s'
              % (np.abs(hand.cpu().numpy() - np.asarray(out['params'])).max(), [s['accepted'].tolist() for s in hrep['sweeps']]))
        for s in hrep['sweeps']:
            print('by hand sweep: accepted %s hidden %s flagged %s' % (s['accepted'], s['hidden'], s['flagged']))
        for k in ('before', 'after', 'silhouette_before', 'silhouette_after', 'n_closure'):
            print('by hand %s %s | folder %s' % (k, hrep[k], rep[k]))
        assert np.array_equal(hand.cpu().numpy(), np.asarray(out['params']))
        assert len(hrep['sweeps']) == len(rep['sweeps'])
        for a, b in zip(hrep['sweeps'], rep['sweeps']):
            assert np.array_equal(a['accepted'], b['accepted']) and np.array_equal(a['hidden'], b['hidden']) and np.array_equal(a['flagged'], b['flagged'])
        assert len(out['files']) == P
        for k, path in enumerate(out['files']):
            with open(path, 'rb') as f:
                res = pickle.load(f)
            assert np.array_equal(res['betas'][0], hand[k, :10].cpu().numpy())
            assert float(res['loss']) == float(out['final_loss'][k])
        # the option on the single-person path, and an unknown key
        with pytest.raises(ValueError, match='persons='):
            batch.fit_folder(model, keyp, cam_file, str(tmp_path / 'x'), engine=eng,
                             silhouettes=dict(mask_root=str(root), weight=WEIGHT, occlusion=OCC))
        with pytest.raises(ValueError, match='occlusion'):
            fit('y', engine=eng, silhouettes=dict(mask_root=str(root), weight=WEIGHT, occlusion=dict(depth=1)))
    finally:
        eng.close()
