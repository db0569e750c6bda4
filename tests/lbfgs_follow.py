"""TEST INFRASTRUCTURE - the L-BFGS oracle replayed along a recorded trace.

A free-running comparison of two L-BFGS runs stops being a step-level check once rounding has been amplified (two float64
oracle runs on the chained Rosenbrock objective whose starts differ by 1e-15 are 1e-7 apart after 40-70 closures and O(1) apart
later), long before a history of 100 evicts its first pair.  ``FollowOracle`` removes the accumulation: it is the oracle of
oracle/lbfgs_np.py, but every closure is evaluated at the RECORDED trial point, and every line search and outer step continues
from the recorded accepted point.  What it reports per closure is the distance between the point it proposed and the recorded
one - one round's direction and line-search arithmetic on the recorded run's own iterates.  A run whose history holds another
set of pairs than the oracle's (stale pair, mis-ordered ring) proposes another direction at the first such round.

Shared by tests/test_lbfgs_follow_cpu.py (which pins the method: what it measures on a clean run and on mutants) and
tests/test_gpu_lbfgs_history.py (which judges the device with it).
"""
import numpy as np

from oracle import lbfgs_np as ln

SEGMENTS = [(0, 10), (10, 13)]                 # + (13, D): the gtol segments of the KAT runs
TOL = 1e-5                                     # see tests/test_lbfgs_follow_cpu.py for the numbers on both sides of it

# chained Rosenbrock, (D, history): every run accepts more than 100 pairs (the insertion slot passes 99) ...
ROSEN_CASES = [(49, 7), (49, 40), (49, 100), (86, 7), (86, 40), (86, 100)]
# ... and these accept 100 + history or more: hist_head itself passes 99 and starts again at 0
HEAD_WRAP = {(49, 7), (86, 7), (86, 40), (86, 100)}


class TraceExhausted(RuntimeError):
    pass


class FollowOracle(ln.LbfgsOracle):
    """rows: [n, D + 1] recorded (x_trial, loss) of every closure call.  After the run: ``dev[i]`` is the deviation of the
    proposal from row i relative to max(1, |row|inf), ``trace[i]`` the (recorded point, oracle loss there)."""

    def __init__(self, rows, evalfn, **kw):
        rows = np.asarray(rows)
        super().__init__(rows[0, :-1], evalfn, **kw)
        self.rows = rows[:, :-1].astype(self.x.dtype)
        self.dev = []
        self._proposed = []            # (closure index, proposed point) of the running line search
        self._resume = None            # recorded point the next search / step continues from

    def _eval(self, x):
        i = len(self.trace)
        if i >= len(self.rows):
            raise TraceExhausted('the recorded trace ends after %d closures' % len(self.rows))
        row = self.rows[i]
        self.dev.append(float(np.abs(x - row).max() / max(1.0, np.abs(row).max())))
        self._proposed.append((i, x))
        return super()._eval(row)

    def _continue(self):
        if self._resume is not None:
            self.x = self._resume
            self._resume = None

    def _strong_wolfe(self, t, d, f, g, gtd, **kw):
        self._continue()
        self._proposed = []
        x = self.x
        out = super()._strong_wolfe(t, d, f, g, gtd, **kw)
        hit = [i for i, p in self._proposed if np.array_equal(p, x + out[2] * d)]
        assert hit, 'the accepted step is none of the proposals of its line search'
        self._resume = self.rows[hit[-1]].copy()
        return out

    def step(self):
        self._continue()
        out = super().step()
        self._continue()
        return out


def replay(rows, D, history, dtype=np.float64):
    """Replays ``rows`` with the clean oracle.  Returns the FollowOracle (``exhausted`` set when the oracle wanted more closures
    than were recorded)."""
    fn, _ = ln.kat_objective('rosen', D)
    fo = FollowOracle(rows, fn, history=history, dtype=dtype)
    fo.exhausted = False
    try:
        ln.run_fitting(fo, segments=SEGMENTS + [(13, D)])
    except TraceExhausted:
        fo.exhausted = True
    return fo


def check_replay(fo, rows, D, history):
    """The whole-run conditions shared by the CPU and the GPU test; returns the worst deviation."""
    assert not fo.exhausted and len(fo.trace) == len(rows), (D, history, len(fo.trace), len(rows), fo.exhausted)
    assert fo.n_pairs >= 101, (D, history, fo.n_pairs)
    if (D, history) in HEAD_WRAP:
        assert fo.n_pairs >= 100 + history, (D, history, fo.n_pairs)
    return max(fo.dev)
