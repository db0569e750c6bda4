"""TEST INFRASTRUCTURE - writes tests/golden/reference_checks.npz: what the REFERENCE's own functions return on the seeded
inputs of the CPU tests that compare against it, so that those tests run wherever the repository is checked out:

  tests/test_oracle_vs_reference.py   closure (loss, gradient, vertices, joints) of RefProblem.eval_closure, float64,
                                      with and without VPoser and with the 3-D joint term; utils/recompute3D.recompute3D
  tests/test_umeyama.py               utils/umeyama.umeyama on the seeded point sets
  tests/test_io_formats.py            utils.load_camera_para / utils.data_parser.read_keypoints on the seeded files
  tests/test_reference_seams.py       the parameter names of FittingMonitor.create_fitting_closure / run_fitting

Run in the build container (needs the reference tree):

    python -m oracle.make_golden_reference_checks      ->  tests/golden/reference_checks.npz
"""
import inspect
import os
import pathlib
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_import as ri                      # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
OUT = os.path.join(GOLD, 'reference_checks.npz')


def main():
    assert ri.available(), 'needs the reference tree'
    from tests import test_io_formats as tio, test_oracle_vs_reference as tov, test_umeyama as tum
    ref = ri.load()
    out = {}
    for use_vp in (False, True):
        _, model, cams, gt, cf, x, wts, vpw = tov.closure_inputs(use_vp)
        rp = ri.RefProblem(model, cams, gt[0], cf[0], 'float64', use_vposer=use_vp, vposer_weights=vpw)
        for k, v in zip(('L', 'g', 'verts', 'joints'), rp.eval_closure(x, wts)):
            out['closure_vp%d_%s' % (use_vp, k)] = np.asarray(v, np.float64)
    _, model, cams, gt, cf, x, wts, j3 = tov.closure_3d_inputs()
    rp = ri.RefProblem(model, cams, gt[0], cf[0], 'float64', joints3d=j3)
    for k, v in zip(('L', 'g'), rp.eval_closure(x, wts)):
        out['closure_3d_%s' % k] = np.asarray(v, np.float64)
    from oracle import make_golden_triangulate as mg
    from utils.recompute3D import recompute3D
    for V, B, seed in tov.TRIANGULATION_CASES:
        extris, intris, kps = mg.make_case(V, B, seed)
        out['recompute3d_%d_%d_%d' % (V, B, seed)] = np.stack(
            [recompute3D(list(extris), list(intris), [kps[b, v][None].copy() for v in range(V)]) for b in range(B)])
    from utils.umeyama import umeyama as ref_umeyama
    for est in (True, False):
        for i, (src, dst) in enumerate(tum._cases()):
            r, t, s = ref_umeyama(src.copy(), dst.copy(), est)
            out['umeyama_%d_%d_r' % (est, i)], out['umeyama_%d_%d_t' % (est, i)] = np.asarray(r), np.asarray(t)
            out['umeyama_%d_%d_s' % (est, i)] = np.float64(s)
    with tempfile.TemporaryDirectory() as d:
        cam, _, _, kj, _ = tio._write_fixture(pathlib.Path(d), V=4)
        out['camera_extris'], out['camera_intris'] = (np.asarray(a) for a in ref.utils.load_camera_para(str(cam)))
        import importlib
        dp = importlib.import_module('utils.data_parser')
        out['keypoints'] = np.stack(dp.read_keypoints(str(kj), use_hands=False, use_face=False).keypoints)
    ref_cls = type(ref.fitting.FittingMonitor(maxiters=1))     # the class is wrapped by @torch.no_grad() (fitting.py:36)
    for name in ('create_fitting_closure', 'run_fitting'):
        out['signature_' + name] = np.array(list(inspect.signature(getattr(ref_cls, name)).parameters))
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, sorted(out))


if __name__ == '__main__':
    main()
