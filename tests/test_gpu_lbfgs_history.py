"""GPU: the L-BFGS history ring step by step once pairs are evicted and the ring wraps, at histories other than 100.

The ring has LB_HIST = 100 slots whatever mvfit_lbfgs_opts::history is: the pair count alone decides the insertion slot
((hist_head + hist_len - 1) % 100) and hist_head advances with every pair accepted at a full history - so at history < 100 the
new pair's slot is NOT the evicted pair's.  lbfgs_advance, lb_fast_accept, the Gram update of lb_direction_block and the packed
R^-1 of lb_direction_compact each depend on which slot is the oldest.  Four views of it:

  1. float64 KAT kernel (the production lbfgs_round, both direction forms), quad / gmof at history 1 ... 8: the free run against
     the oracle at the same history, every closure (the oracle is stable there: a 1e-15 change of x0 moves it by <= 2e-13);
  2. the same kernel on the chained Rosenbrock objective through 117-263 accepted pairs - insertion slot and head past 99 -
     replayed by the oracle along the device's own trace (tests/lbfgs_follow.py; tolerance and the numbers behind it:
     tests/test_lbfgs_follow_cpu.py);
  3. the float32 production kernels (single launch: compact direction, ring in LDS; chained step kernel: Gram matrices in
     global memory) at history 2 and 4 against the oracle over the first outer step, evictions from closure 5-9 on, with the
     tolerance schedule of tests/test_gpu_trajectory.py - the float32 ORACLE must stay inside the same envelope (measured as
     fractions of it: 0.044 (problem 0, history 2), 0.10 (0, 4), 0.18 (1, 4), and 0.31 for (1, 2) without its closure 16, see
     SKIP_ROWS); tests/test_lbfgs_follow_cpu.py pins this and the two eviction mutants against the envelope on the CPU;
  4. end quality of the staged production fit at history 4 and 8 (589 to 1589 pairs over the four stages of the oracle's fits: the
     head goes round the ring) next to the oracle's recorded fits (oracle/make_golden_small_history.py)."""
import functools
import os

import numpy as np
import pytest

from mvsmplfitting_amd import _lib
from mvsmplfitting_amd.engine import MvFitError, lbfgs_kat, stage_weights as eng_stage_weights
from oracle import lbfgs_np as ln
from tests import lbfgs_follow as lf
from tests.gpu_helpers import from118, make_engine, to118
from tests.helpers import GOLD, body_model, oracle_for
from tests.test_gpu_trajectory import N_STEP, tol

pytestmark = pytest.mark.gpu
KIND = dict(quad=0, rosen=1, gmof=2)
FORMS = ['two_loop', 'compact']
WKEYS = ('data_weight', 'body_pose_weight', 'shape_weight', 'bending_prior_weight', 'rho')


def _kat(kind, D, form, **kw):
    _, x0 = ln.kat_objective(kind, D)
    return lbfgs_kat(KIND[kind] | (0x100 if form == 'compact' else 0), D, [0, 10, 13, D], x0, **kw)


# ------------------------------------------------------------------------------------------- 0. the options are checked
@pytest.mark.parametrize('history', [0, 101])
def test_history_outside_the_ring_is_refused(history):
    """history <= 0 puts the first pair into a negative slot, history > 100 runs past the ring: both entry points that run
    the optimiser refuse them before anything is launched."""
    with pytest.raises(MvFitError, match=r'failed: -1$'):                      # MVFIT_E_ARG, not MVFIT_E_HIP (-2) after a launch
        _kat('quad', 49, 'two_loop', history=history)
    g = dict(np.load(os.path.join(GOLD, 'fit_l2.npz')))
    eng = make_engine(body_model())
    try:
        eng.set_problems((g['cam_R'], g['cam_t'], g['cam_f'], g['cam_c']), g['gt_xy'], g['conf'])
        x0 = np.stack([to118(x, False) for x in g['x0']]).astype(np.float32)
        with pytest.raises(MvFitError, match=r'error -1: bad lbfgs options'):
            eng.fit(x0, eng_stage_weights(1536.0), history=history)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------- 1. free run, small history
@functools.lru_cache(maxsize=None)
def _oracle_free_run(kind, D, history):
    fn, x0 = ln.kat_objective(kind, D)
    opt = ln.LbfgsOracle(x0, fn, history=history)
    prev, _ = ln.run_fitting(opt, segments=lf.SEGMENTS + [(13, D)])
    return opt, prev


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('history', [1, 2, 3, 5, 8])
@pytest.mark.parametrize('D', [49, 86])
@pytest.mark.parametrize('kind', ['quad', 'gmof'])
def test_device_lbfgs_follows_oracle_at_small_history(kind, D, history, form):
    """33-57 closures, n_iter - history evictions from iteration history + 1 on; the tolerances of
    test_gpu_lbfgs.py::test_device_lbfgs_follows_reference, over every closure."""
    opt, prev = _oracle_free_run(kind, D, history)
    assert opt.n_pairs > history, 'the case never evicts'
    xf, trace, ncl, final = _kat(kind, D, form, history=history, max_trace=80)
    assert ncl == len(opt.trace) <= 80, (ncl, len(opt.trace))
    for i, (x, f) in enumerate(opt.trace):
        assert np.abs(trace[i][:D] - x).max() < 1e-7, (kind, D, history, i, np.abs(trace[i][:D] - x).max())
        assert abs(trace[i][D] - f) <= 1e-7 * max(1.0, abs(f)), (kind, D, history, i)
    assert np.abs(xf - opt.x).max() < 1e-9
    assert abs(final - prev) < 1e-8


# ------------------------------------------------------------------------------------------- 2. replay through the wrap
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('D,history', lf.ROSEN_CASES)
def test_device_lbfgs_replayed_through_eviction_and_wrap(D, history, form):
    xf, trace, ncl, final = _kat('rosen', D, form, history=history, max_trace=400)
    assert ncl == len(trace) < 400, ncl                     # every closure of the run was recorded
    fo = lf.replay(trace, D, history)
    dev = np.array(fo.dev)
    print('rosen D=%d history=%d %s: %d closures, %d pairs, worst deviation %.2g (closure %d)'
          % (D, history, form, ncl, fo.n_pairs, dev.max(), int(dev.argmax())))
    over = np.nonzero(dev > lf.TOL)[0]
    assert over.size == 0, (D, history, form, int(over[0]), dev[over[:5]])
    for i in range(len(fo.trace)):
        f = fo.trace[i][1]                                  # the oracle's objective at the device's trial point
        assert abs(trace[i][D] - f) <= 1e-12 * max(1.0, abs(f)), (D, history, form, i, trace[i][D], f)
    assert lf.check_replay(fo, trace, D, history) <= lf.TOL


# ------------------------------------------------------------------------------------------- 3. the float32 production kernels
@functools.lru_cache(maxsize=None)
def _fit_problem():
    g = dict(np.load(os.path.join(GOLD, 'fit_l2.npz')))
    return g, (g['cam_R'], g['cam_t'], g['cam_f'], g['cam_c'])


def first_step(history, dtype=np.float64, cls=ln.LbfgsOracle):
    """(x, loss) of every closure of ONE step() of the oracle ``cls`` at the first stage's weights, per problem."""
    g, cams = _fit_problem()
    wts = {k: eng_stage_weights(1536.0)[0][k] for k in WKEYS}
    orc = oracle_for(body_model(), None, None, dtype)
    per_problem = []
    for b in range(g['x0'].shape[0]):
        opt = cls(g['x0'][b], lambda x, b=b: orc.closure(x, cams, g['gt_xy'][b], g['conf'][b], wts)[:2],
                  history=history, dtype=dtype)
        opt.step()
        assert opt.n_pairs > history, 'no eviction inside the first outer step'
        per_problem.append(np.array([np.concatenate([np.asarray(x, np.float64), [f]]) for x, f in opt.trace]))
    return per_problem


@functools.lru_cache(maxsize=None)
def _oracle_first_step(history):
    """[float64, float32] first steps of the clean oracle."""
    return [first_step(history, np.float64), first_step(history, np.float32)]


# Closures of the first outer step that are NOT compared, per (problem, history): where the float32 ORACLE alone is outside the
# envelope, the row cannot tell a device fault from float32 rounding.  Problem 1 at history 2, closure 16 only: a far line-search
# trial on a steep flank (loss 12034 between 10247 and 9558) where the float32 oracle's loss is 4.4e-4 (relative) from the float64
# oracle's - 2.06 x the envelope - and its x 0.53 x.  The other 33 closures of that case are compared: the float32 oracle is at
# 0.31 x at closure 14, 0.22 x at closure 15, 0.21 x at closure 17 and below 0.03 x from closure 18 on.
SKIP_ROWS = {(1, 2): {16}}


def compared_rows(b, history, *traces):
    n = min([N_STEP] + [len(t) for t in traces])
    return [k for k in range(n) if k not in SKIP_ROWS.get((b, history), ())]


def worst(rows, ref, ks):
    """max over k in ks of err(k) / tol(k): x absolute, loss relative (tests/test_gpu_trajectory.py)."""
    return max(max(np.abs(rows[k, :-1] - ref[k, :-1]).max(), abs(rows[k, -1] - ref[k, -1]) / abs(ref[k, -1])) / tol(k)
               for k in ks)


@pytest.mark.parametrize('round_mode', [0, 1])
@pytest.mark.parametrize('history', [2, 4])
@pytest.mark.parametrize('sparse', [False, True])
def test_fp32_fit_follows_oracle_through_evictions(sparse, history, round_mode):
    """Three kernels: the asynchronous single-launch fit (flags 0, round_mode 0), the chained step kernel (flags 0, round_mode 1)
    and the single-launch fit on the sparse vertices (F_SPARSE_VERTS, which takes that kernel in either round_mode)."""
    g, cams = _fit_problem()
    ref64, ref32 = _oracle_first_step(history)
    B = g['x0'].shape[0]
    eng = make_engine(body_model(), round_mode=round_mode)
    eng.set_problems(cams, g['gt_xy'], g['conf'])
    x0 = np.stack([to118(g['x0'][b], False) for b in range(B)]).astype(np.float32)
    tr = eng.fit_trace(40)
    xf, st = eng.fit(x0, eng_stage_weights(1536.0, flags=_lib.F_SPARSE_VERTS if sparse else 0), history=history)
    tr = tr.cpu().numpy().astype(np.float64)
    eng.fit_trace(0)
    ncl = st['n_closure'].cpu().numpy()
    eng.close()
    for b in range(B):
        ks = compared_rows(b, history, ref64[b], ref32[b])
        n = ks[-1] + 1
        assert n >= 30 and ncl[b] >= n, (b, n, ncl[b])                   # evictions begin at closure 5-9
        w32 = worst(ref32[b], ref64[b], ks)
        assert w32 <= 1.0, 'the float32 oracle itself leaves the envelope: problem %d history %d, %.3g' % (b, history, w32)
        rows = np.array([np.concatenate([from118(tr[b, k, :118], False), [tr[b, k, 118]]]) for k in range(n)])
        assert np.isfinite(rows).all()
        w = worst(rows, ref64[b], ks)
        print('problem %d history %d sparse %d round_mode %d: %d of %d closures, device %.3g and float32 oracle %.3g of the envelope'
              % (b, history, sparse, round_mode, len(ks), n, w, w32))
        assert w <= 1.0, (b, history, sparse, round_mode, w,
                          [(k, float(worst(rows, ref64[b], [k]))) for k in ks if worst(rows, ref64[b], [k]) > 1.0][:5])


# ------------------------------------------------------------------------------------------- 4. end quality past the wrap
SMALL = dict(np.load(os.path.join(GOLD, 'fit_small_history.npz')))


@pytest.mark.parametrize('round_mode', [0, 1])
@pytest.mark.parametrize('hi', range(len(SMALL['histories'])))
def test_device_fit_against_oracle_fit_at_small_history(hi, round_mode):
    history = int(SMALL['histories'][hi])
    g, cams = _fit_problem()
    B = g['x0'].shape[0]
    eng = make_engine(body_model(), round_mode=round_mode)
    eng.set_problems(cams, g['gt_xy'], g['conf'])
    x0 = np.stack([to118(g['x0'][b], False) for b in range(B)]).astype(np.float32)
    xf, st = eng.fit(x0, eng_stage_weights(1536.0), history=history)
    final = st['final_loss'].cpu().numpy().astype(np.float64)
    ncl = st['n_closure'].cpu().numpy()
    eng.close()
    ref_final = np.maximum(SMALL['final64'][hi], SMALL['final32'][hi])
    ref_lo = np.minimum(SMALL['ncl64'][hi], SMALL['ncl32'][hi])
    ref_hi = np.maximum(SMALL['ncl64'][hi], SMALL['ncl32'][hi])
    print('history %d round_mode %d: final %s (oracle %s / %s), closures %s (oracle %s / %s)'
          % (history, round_mode, final, SMALL['final64'][hi], SMALL['final32'][hi], ncl, SMALL['ncl64'][hi], SMALL['ncl32'][hi]))
    assert np.all(np.isfinite(final))
    assert np.all(final <= 1.05 * ref_final), (final, ref_final)
    assert np.all(ncl > 0.4 * ref_lo) and np.all(ncl < 2.5 * ref_hi), (ncl, ref_lo, ref_hi)
