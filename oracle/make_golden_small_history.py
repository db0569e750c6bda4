"""TEST INFRASTRUCTURE - end quality of the staged fit at a small L-BFGS history, recorded from the project's own oracle.

Writes tests/golden/fit_small_history.npz: for both problems of tests/golden/fit_l2.npz and every history in HISTORIES, the
final loss and the closure count of the oracle's staged fit (oracle/closure_np.py under oracle/lbfgs_np.py, the four stages of
engine.stage_weights(1536.0), a fresh optimiser per stage) - once in float64 and once in float32.  At history 4 such a fit
takes 600 to 1600 L-BFGS iterations, i.e. the ring's head goes round; too slow to compute in a test
(10-25 s per problem and precision), so it is recorded.  tests/test_gpu_lbfgs_history.py holds the device fit against it.

    python -m oracle.make_golden_small_history
"""
import os

import numpy as np

from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import stage_weights
from oracle import closure_np as cn
from oracle import lbfgs_np as ln

GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden')
HISTORIES = (4, 8)
SEGMENTS = [(0, 10), (10, 13), (13, 82), (82, 85), (85, 86)]
WKEYS = ('data_weight', 'body_pose_weight', 'shape_weight', 'bending_prior_weight', 'rho')


def oracle_fit(orc, dtype, cams, gt_xy, conf, x0, history):
    """-> final loss, closures, L-BFGS iterations and accepted pairs (summed over the stages)."""
    x = np.asarray(x0, dtype)
    final, ncl, nit, pairs = None, 0, 0, 0
    for st in stage_weights(1536.0):
        wts = {k: st[k] for k in WKEYS}
        opt = ln.LbfgsOracle(x, lambda xx, wts=wts: orc.closure(xx, cams, gt_xy, conf, wts)[:2], history=history, dtype=dtype)
        prev, losses = ln.run_fitting(opt, segments=SEGMENTS)
        final = prev if prev is not None else losses[-1]
        x = opt.x.copy()
        ncl += opt.func_evals; nit += opt.n_iter; pairs += opt.n_pairs
    return float(final), ncl, nit, pairs


def main():
    g = dict(np.load(os.path.join(GOLD, 'fit_l2.npz')))
    lsp = np.load(os.path.join(GOLD, 'lsp_regressor.npz'))
    model = syn.make_body_model(0, skin_topk=None, kp_regressor=(lsp['rows'], lsp['cols'], lsp['vals']))
    cams = (g['cam_R'], g['cam_t'], g['cam_f'], g['cam_c'])
    B = g['x0'].shape[0]
    out = dict(histories=np.array(HISTORIES, np.int32), model_checksum=np.array(syn.model_checksum(model)))
    for name, dtype in (('64', np.float64), ('32', np.float32)):
        orc = cn.ClosureOracle(model, dtype)
        res = np.array([[oracle_fit(orc, dtype, cams, g['gt_xy'][b], g['conf'][b], g['x0'][b], h) for b in range(B)]
                        for h in HISTORIES])
        out['final' + name] = res[:, :, 0]                       # [history, problem]
        out['ncl' + name] = res[:, :, 1].astype(np.int32)
        out['n_iter' + name] = res[:, :, 2].astype(np.int32)
        out['n_pairs' + name] = res[:, :, 3].astype(np.int32)
        print('float' + name, 'final', res[:, :, 0], 'closures', res[:, :, 1], 'iterations', res[:, :, 2], 'pairs', res[:, :, 3])
    np.savez_compressed(os.path.join(GOLD, 'fit_small_history.npz'), **out)


if __name__ == '__main__':
    main()
