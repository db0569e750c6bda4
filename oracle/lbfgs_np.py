"""TEST INFRASTRUCTURE - NumPy restatement of the reference optimiser loop.

Restates, for a generic ``evalfn(x) -> (loss, grad)``:
  * ``LBFGS.step`` with strong-Wolfe line search  (reference code/optimizers/lbfgs_ls.py:256-445)
  * ``_strong_Wolfe`` / ``_cubic_interpolate``     (lbfgs_ls.py:39-167, 11-36)
  * ``FittingMonitor.run_fitting``                 (reference code/utils/fitting.py:71-142)
with the production settings of ``create_optimizer`` (optim_factory.py:50-52:
lr, max_iter=maxiters, max_eval=max_iter*5//4, tolerance_grad=1e-5,
tolerance_change=1e-9, history_size=100).

Pinned against the reference optimiser itself on analytic objectives
(tests/test_lbfgs_oracle.py; golden trajectories tests/golden/lbfgs_kat.npz).
The checker for the device L-BFGS; never imported by the shipped package.
"""
from __future__ import annotations

import math

import numpy as np


def cubic_interpolate(x1, f1, g1, x2, f2, g2, bounds=None, tag=None):
    """lbfgs_ls.py:11-36.  ``tag``: called with the name of every branch taken (see TAGS); no effect on the value."""
    tag = tag or (lambda name: None)
    if bounds is not None:
        lo, hi = bounds
    else:
        lo, hi = (x1, x2) if x1 <= x2 else (x2, x1)
    d1 = g1 + g2 - 3 * (f1 - f2) / (x1 - x2)
    d2s = d1 * d1 - g1 * g2
    if d2s >= 0:
        d2 = math.sqrt(d2s)
        if x1 <= x2:
            tag('cubic_x1_le_x2')
            mp = x2 - (x2 - x1) * ((g2 + d2 - d1) / (g2 - g1 + 2 * d2))
        else:
            tag('cubic_x1_gt_x2')
            mp = x1 - (x1 - x2) * ((g1 + d2 - d1) / (g1 - g2 + 2 * d2))
        if lo > mp:
            tag('cubic_clamp_lo')
        elif hi < mp:
            tag('cubic_clamp_hi')
        return min(max(mp, lo), hi)
    tag('cubic_bisect_bounds' if bounds is not None else
        'cubic_bisect_unbounded' if x1 <= x2 else 'cubic_bisect_unbounded_x1_gt_x2')
    return (lo + hi) / 2.0


# Every branch the oracle can report in ``LbfgsOracle.branches``, by the function that takes it.
TAGS = (
    # cubic_interpolate (:32-37)
    'cubic_x1_le_x2', 'cubic_x1_gt_x2', 'cubic_clamp_lo', 'cubic_clamp_hi',
    'cubic_bisect_bounds', 'cubic_bisect_unbounded', 'cubic_bisect_unbounded_x1_gt_x2',
    # _strong_wolfe, bracket phase (:84-107): Armijo / f_new >= f_prev failure at it = 0, 1, >= 2; Wolfe met at the first trial
    # point (the candidate of the device's lb_fast_accept), after one, after two or more extrapolations; gtd_new >= 0
    'bracket_fail_it0', 'bracket_fail_it1', 'bracket_fail_it2p', 'wolfe_first', 'wolfe_it1', 'wolfe_it2p', 'bracket_gtd_pos',
    'extrapolate', 'max_ls',
    # zoom phase (:110-138)
    'zoom_skipped', 'zoom_progress', 'zoom_insuf_set', 'zoom_clamp_insuf0', 'zoom_clamp_insuf1', 'zoom_clamp_max', 'zoom_clamp_min',
    'zoom_high_replaced', 'zoom_reordered', 'zoom_wolfe', 'zoom_swap', 'zoom_low_replaced',
    'zoom_end_max_iter', 'zoom_end_width',
    # step (:147-202); exit_*_first: the same stop test right behind a line search that ended at its first trial point
    'exit_grad0', 'first_iter', 'pair_accepted', 'pair_evicted', 'pair_rejected', 'pair_rejected_empty', 'exit_gtd',
    'exit_max_iter', 'exit_max_eval', 'exit_tol_grad', 'exit_step_small', 'exit_loss_change',
    'exit_max_iter_first', 'exit_max_eval_first', 'exit_tol_grad_first', 'exit_step_small_first', 'exit_loss_change_first',
    # run_fitting (:214-225)
    'fit_nonfinite', 'fit_ftol', 'fit_gtol', 'fit_maxiters',
)


class LbfgsOracle:
    """State persists across ``step`` calls exactly like ``optimizer.state`` does."""

    YS_MIN = 1e-10                     # curvature pairs with y.s at or below it are rejected (lbfgs_ls.py:323)

    def __init__(self, x0, evalfn, lr=1.0, max_iter=30, history=100, tol_grad=1e-5,
                 tol_change=1e-9, dtype=np.float64):
        self.x = np.array(x0, dtype)
        self.evalfn = evalfn
        self.lr, self.max_iter, self.history = lr, max_iter, history
        self.max_eval = max_iter * 5 // 4
        self.tol_grad, self.tol_change = tol_grad, tol_change
        self.n_iter = 0
        self.func_evals = 0
        self.d = self.t = self.H = self.prev_g = self.prev_loss = None
        self.dirs, self.stps, self.ro = [], [], []
        self.n_pairs = 0               # accepted (s, y) pairs so far, evicted ones included
        self.last_grad = None          # .grad left by the last closure call (gtol test reads it)
        self.trace = []                # (x_trial, loss) of every closure call
        self.exits = []                # why each step() ended: 'grad0', 'gtd' (:379-380, with n_iter), 'ls' (:419-434)
        self.branches = []             # (index of the last closure call, tag of TAGS) of every branch taken, in order
        self._ls_first = False         # the last line search ended at its first trial point

    def _tag(self, name):
        self.branches.append((len(self.trace) - 1, name))

    # The decisions of the line search and of step() that a wrong implementation is most likely to get wrong, as methods:
    # tests/test_lbfgs_branch_cases_cpu.py derives wrong oracles from them.
    def _cubic(self, *a, **kw):
        return cubic_interpolate(*a, tag=self._tag, **kw)

    def _extrapolation_bounds(self, t, t_prev):
        """:96-97"""
        return t + 0.01 * (t - t_prev), t * 10

    def _max_ls_bracket_start(self, t_prev):
        """:107 - the bracket of an exhausted bracket phase starts at 0, not at the last but one trial"""
        return 0.0

    def _zoom_trial(self, t, br, insuf):
        """:112-123 - the sufficient-progress rule; returns (t, insuf)"""
        eps = 0.1 * (max(br) - min(br))
        if min(max(br) - t, t - min(br)) < eps:
            if insuf or t >= max(br) or t <= min(br):
                self._tag('zoom_clamp_insuf%d' % insuf)
                if abs(t - max(br)) < abs(t - min(br)):
                    self._tag('zoom_clamp_max')
                    t = max(br) - eps
                else:
                    self._tag('zoom_clamp_min')
                    t = min(br) + eps
                insuf = False
            else:
                self._tag('zoom_insuf_set')
                insuf = True
        else:
            self._tag('zoom_progress')
            insuf = False
        return t, insuf

    def _zoom_swap(self, gtd_new, br, bf, bg, bgtd, low, high):
        """:134-136 - the old low end becomes the high end"""
        if gtd_new * (br[high] - br[low]) >= 0:
            self._tag('zoom_swap')
            br[high] = br[low]; bf[high] = bf[low]; bg[high] = bg[low]
            bgtd[high] = bgtd[low]

    def _grad_small_after_search(self, g):
        """:197"""
        return np.abs(g).max() <= self.tol_grad

    def _eval(self, x):
        f, g = self.evalfn(x)
        f = float(f)
        self.last_grad = np.array(g, self.x.dtype)
        self.func_evals += 1
        self.trace.append((x.copy(), f))
        return f, self.last_grad.copy()

    def _evict(self):
        """Drop the oldest pair (lbfgs_ls.py:325-329)."""
        self.dirs.pop(0); self.stps.pop(0); self.ro.pop(0)

    def _strong_wolfe(self, t, d, f, g, gtd, c1=1e-4, c2=0.9, max_ls=25):
        """lbfgs_ls.py:39-167; obj_func(x,t,d) evaluates at x + t d (lbfgs_ls.py:249-254)."""
        tol, max_iter = self.tol_change, self.max_iter
        x = self.x
        d_norm = np.abs(d).max()
        f_new, g_new = self._eval(x + t * d)
        evals = 1
        gtd_new = float(g_new @ d)
        t_prev, f_prev, g_prev, gtd_prev = 0.0, f, g.copy(), gtd
        done = False
        it = 0
        br = None
        while it < max_ls:
            if f_new > (f + c1 * t * gtd) or (it > 1 and f_new >= f_prev):
                self._tag('bracket_fail_it%s' % (it if it < 2 else '2p'))
                br = [t_prev, t]; bf = [f_prev, f_new]; bg = [g_prev, g_new.copy()]
                bgtd = [gtd_prev, gtd_new]
                break
            if abs(gtd_new) <= -c2 * gtd:
                self._tag('wolfe_first' if it == 0 else 'wolfe_it1' if it == 1 else 'wolfe_it2p')
                br = [t]; bf = [f_new]; bg = [g_new]; bgtd = [gtd_new]
                done = True
                break
            if gtd_new >= 0:
                self._tag('bracket_gtd_pos')
                br = [t_prev, t]; bf = [f_prev, f_new]; bg = [g_prev, g_new.copy()]
                bgtd = [gtd_prev, gtd_new]
                break
            self._tag('extrapolate')
            min_step, max_step = self._extrapolation_bounds(t, t_prev)
            tmp = t
            t = self._cubic(t_prev, f_prev, gtd_prev, t, f_new, gtd_new,
                            bounds=(min_step, max_step))
            t_prev, f_prev, g_prev, gtd_prev = tmp, f_new, g_new.copy(), gtd_new
            f_new, g_new = self._eval(x + t * d)
            evals += 1
            gtd_new = float(g_new @ d)
            it += 1
        self._ls_first = done and it == 0
        if it == max_ls:
            self._tag('max_ls')
            br = [self._max_ls_bracket_start(t_prev), t]; bf = [f, f_new]; bg = [g, g_new]; bgtd = [gtd, gtd_new]
        insuf = False
        low, high = (0, 1) if bf[0] <= bf[-1] else (1, 0)
        if not done and it >= max_iter:
            self._tag('zoom_skipped')
        while not done and it < max_iter:
            t = self._cubic(br[0], bf[0], bgtd[0], br[1], bf[1], bgtd[1])
            t, insuf = self._zoom_trial(t, br, insuf)
            f_new, g_new = self._eval(x + t * d)
            evals += 1
            gtd_new = float(g_new @ d)
            it += 1
            if f_new > (f + c1 * t * gtd) or f_new >= bf[low]:
                self._tag('zoom_high_replaced')
                br[high] = t; bf[high] = f_new; bg[high] = g_new.copy(); bgtd[high] = gtd_new
                if ((0, 1) if bf[0] <= bf[1] else (1, 0)) != (low, high):
                    self._tag('zoom_reordered')
                low, high = (0, 1) if bf[0] <= bf[1] else (1, 0)
            else:
                if abs(gtd_new) <= -c2 * gtd:
                    self._tag('zoom_wolfe')
                    done = True
                else:
                    self._zoom_swap(gtd_new, br, bf, bg, bgtd, low, high)
                self._tag('zoom_low_replaced')
                br[low] = t; bf[low] = f_new; bg[low] = g_new.copy(); bgtd[low] = gtd_new
            if abs(br[1] - br[0]) * d_norm < tol:
                self._tag('zoom_end_width')
                break
            if not done and it >= max_iter:
                self._tag('zoom_end_max_iter')
        return bf[low], bg[low], br[low], evals

    def step(self):
        """lbfgs_ls.py:256-445.  Returns the loss at the START of the step (orig_loss)."""
        orig_loss, g = self._eval(self.x)
        loss = orig_loss
        cur_evals = 1
        if np.abs(g).max() <= self.tol_grad:
            self.exits.append(('grad0', self.n_iter))
            self._tag('exit_grad0')
            return orig_loss
        d, t, H = self.d, self.t, self.H
        n = 0
        while n < self.max_iter:
            n += 1
            self.n_iter += 1
            if self.n_iter == 1:
                self._tag('first_iter')
                d = -g
                self.dirs, self.stps, self.ro = [], [], []
                H = 1.0
            else:
                y = g - self.prev_g
                s = d * t
                ys = float(y @ s)
                if ys > self.YS_MIN:
                    self._tag('pair_accepted')
                    if len(self.dirs) == self.history:
                        self._tag('pair_evicted')
                        self._evict()
                    self.dirs.append(y); self.stps.append(s); self.ro.append(1.0 / ys)
                    self.n_pairs += 1
                    H = ys / float(y @ y)
                else:
                    self._tag('pair_rejected' if self.dirs else 'pair_rejected_empty')
                k = len(self.dirs)
                al = [0.0] * k
                q = -g
                for i in range(k - 1, -1, -1):
                    al[i] = float(self.stps[i] @ q) * self.ro[i]
                    q = q - al[i] * self.dirs[i]
                r = q * H
                for i in range(k):
                    be = float(self.dirs[i] @ r) * self.ro[i]
                    r = r + (al[i] - be) * self.stps[i]
                d = r
            self.prev_g = g.copy()
            self.prev_loss = loss
            if self.n_iter == 1:
                t = min(1.0, 1.0 / float(np.abs(g).sum())) * self.lr
            else:
                t = self.lr
            gtd = float(g @ d)
            if gtd > -self.tol_change:
                self.exits.append(('gtd', self.n_iter))
                self._tag('exit_gtd')
                break
            loss, g, t, ls_evals = self._strong_wolfe(t, d, loss, g, gtd)
            self.x = self.x + t * d
            cur_evals += ls_evals
            first = '_first' if self._ls_first else ''
            if n == self.max_iter:
                self._tag('exit_max_iter' + first)
                break
            if cur_evals >= self.max_eval:
                self._tag('exit_max_eval' + first)
                break
            if self._grad_small_after_search(g):
                self._tag('exit_tol_grad' + first)
                break
            if np.abs(d * t).max() <= self.tol_change:
                self._tag('exit_step_small' + first)
                break
            if abs(loss - self.prev_loss) < self.tol_change:
                self._tag('exit_loss_change' + first)
                break
        self.d, self.t, self.H = d, t, H
        return orig_loss


def run_fitting(opt: LbfgsOracle, maxiters=30, ftol=1e-9, gtol=1e-9, segments=None):
    """fitting.py:99-142.  ``segments``: list of (start, stop) of each parameter tensor in the
    flat vector - the gtol test is per tensor on abs(max(grad)) (fitting.py:115-116)."""
    prev = None
    losses = []
    D = opt.x.shape[0]
    segments = segments or [(0, D)]
    for n in range(maxiters):
        loss = opt.step()
        losses.append(loss)
        if math.isnan(loss) or math.isinf(loss):
            opt._tag('fit_nonfinite')
            break
        if n > 0 and prev is not None and ftol > 0:
            rel = (prev - loss) / max(abs(prev), abs(loss), 1.0)          # utils.py:348-349
            if rel <= ftol:
                opt._tag('fit_ftol')
                break
        if all(abs(opt.last_grad[a:b].max()) < gtol for a, b in segments):
            opt._tag('fit_gtol')
            break
        prev = loss
    else:
        opt._tag('fit_maxiters')
    return prev, losses


# ------------------------------------------------------------ analytic KAT objectives
def kat_objective(kind: str, D: int, seed: int = 0):
    """Deterministic test objectives shared with the device KAT kernel
    (mvsmplfitting_amd/csrc/fit_kernels.hip:kat_eval implements the same formulas).

    'quad'  : 0.5 * sum c_i (x_i - m_i)^2,   c_i = 1 + 99 * i/(D-1), m_i = sin(i)
    'rosen' : chained Rosenbrock  sum_{i<D-1} 100 (x_{i+1} - x_i^2)^2 + (1 - x_i)^2
    'gmof'  : sum_i 1e4 * r_i^2/(r_i^2 + 1e4) with r_i = 50*(x_i - m_i) + 20 sin(3 x_{(i+1)%D})
              plus 0.5*sum x_i^2  (non-convex, GMoF-like)
    'linear': c . x, c_i = 1 + i/D, start 0 (unbounded below; d2_square of every interpolation is 0 up to rounding)
    'wavy', 'wavy2' : sum_i 0.5 x_i^2 + a sin(b x_i), (a, b) of WAVY, start 0
    'steep' : -sum_i c_i x_i^4, 'steep2' : -sum_i c_i |x_i|^(31/16) by four square roots; start 1 + 0.5 cos(i)
              (unbounded below: the bracket phase of a line search runs out of its 25 extrapolations)
    'linear' and the kinds behind it sum in index order, like the device.
    Returns (fn(x)->(f,g), x0).
    """
    i = np.arange(D, dtype=np.float64)
    m = np.sin(i)
    if kind == 'quad':
        c = 1.0 + 99.0 * i / (D - 1)

        def fn(x):
            r = x - m
            return 0.5 * float((c * r * r).sum()), c * r
        return fn, np.zeros(D)
    if kind == 'rosen':
        def fn(x):
            a = x[1:] - x[:-1] ** 2
            b = 1.0 - x[:-1]
            f = float((100.0 * a * a + b * b).sum())
            g = np.zeros_like(x)
            g[:-1] += -400.0 * a * x[:-1] - 2.0 * b
            g[1:] += 200.0 * a
            return f, g
        return fn, np.full(D, -1.2) * np.cos(0.1 * i)
    if kind == 'gmof':
        rho2 = 1e4

        def fn(x):
            xn = np.roll(x, -1)
            r = 50.0 * (x - m) + 20.0 * np.sin(3.0 * xn)
            r2 = r * r
            f = float((rho2 * r2 / (r2 + rho2)).sum() + 0.5 * (x * x).sum())
            dr = 2.0 * r * rho2 * rho2 / (r2 + rho2) ** 2
            g = 50.0 * dr + np.roll(dr * 60.0 * np.cos(3.0 * xn), 1) + x
            return f, g
        return fn, 0.3 * np.cos(0.7 * i)
    if kind == 'linear':
        c = 1.0 + i / D

        def fn(x):
            return float(np.cumsum(c * x)[-1]), c.copy()
        return fn, np.zeros(D)
    if kind == 'steep':
        c = 1.0 + i / D

        def fn(x):
            x2 = x * x
            return float(np.cumsum(-c * (x2 * x2))[-1]), -4.0 * c * (x2 * x)
        return fn, 1.0 + 0.5 * np.cos(i)
    if kind == 'steep2':
        c = 1.0 + i / D

        def fn(x):
            r = np.sqrt(np.sqrt(np.sqrt(np.sqrt(np.abs(x)))))
            return float(np.cumsum(-c * (x * x / r))[-1]), -1.9375 * c * (x / r)
        return fn, 1.0 + 0.5 * np.cos(i)
    if kind in WAVY:
        a, b = WAVY[kind]

        def fn(x):
            return float(np.cumsum(0.5 * x * x + a * np.sin(b * x))[-1]), x + (a * b) * np.cos(b * x)
        return fn, np.zeros(D)
    raise ValueError(kind)


# 'wavy' kinds: (a, b) of sum_i 0.5 x_i^2 + a sin(b x_i), summed in index order like the device does; start 0
WAVY = {'wavy': (5.0, 7.0), 'wavy2': (0.5, 3.0)}
