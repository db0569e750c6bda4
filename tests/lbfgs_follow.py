"""TEST INFRASTRUCTURE - the L-BFGS oracle replayed along a recorded trace.

A free-running comparison of two L-BFGS runs stops being a step-level check once rounding has been amplified (two float64
oracle runs on the chained Rosenbrock objective whose starts differ by 1e-15 are 1e-7 apart after 40-70 closures and O(1) apart
later), long before a history of 100 evicts its first pair.  ``FollowOracle`` removes the accumulation: it is the oracle of
oracle/lbfgs_np.py, but every closure is evaluated at the RECORDED trial point, and every line search and outer step continues
from the recorded accepted point.  What it reports per closure is the distance between the point it proposed and the recorded
one - one round's direction and line-search arithmetic on the recorded run's own iterates.  A run whose history holds another
set of pairs than the oracle's (stale pair, mis-ordered ring) proposes another direction at the first such round.

Shared by tests/test_lbfgs_follow_cpu.py (which pins the method: what it measures on a clean run and on mutants) and
tests/test_gpu_lbfgs_history.py (which judges the device with it); with the objective and options of a case of
tests/lbfgs_branch_cases.py also by tests/test_lbfgs_branch_cases_cpu.py and tests/test_gpu_lbfgs_branches.py, which compare
the branch sequence of the replay (LbfgsOracle.branches) as well.  Limit of the method: inside ONE line search the oracle keeps
its own step lengths, so a search of many interior cubic extrapolations amplifies rounding closure by closure (27 x per
closure on -sum |x|^1.5: such a run is no case).
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
        ok = np.isfinite(row)
        if ok.all():
            self.dev.append(float(np.abs(x - row).max() / max(1.0, np.abs(row).max())))
        else:       # a non-finite recorded point: the proposal has to be non-finite in the same places (NaN for NaN, inf for inf)
            same = np.array_equal(x[~ok], row[~ok], equal_nan=True)
            self.dev.append(float(np.abs(x[ok] - row[ok]).max(initial=0.0) / max(1.0, np.abs(row[ok]).max(initial=0.0))) if same
                            else float('inf'))
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
        nb = len(self.branches)
        out = super()._strong_wolfe(t, d, f, g, gtd, **kw)
        hit = [i for i, p in self._proposed if np.array_equal(p, x + out[2] * d, equal_nan=True)]
        tags = [tag for _, tag in self.branches[nb:]]
        from_zero = 'max_ls' in tags or ('extrapolate' not in tags and ('bracket_fail_it0' in tags or 'bracket_gtd_pos' in tags))
        if not hit and out[2] == 0 and from_zero:      # a bracket [0, t] whose low end is still the point the search started from
            self._resume = x.copy()
            return out
        assert hit, 'the accepted step is none of the proposals of its line search'
        self._resume = self.rows[hit[-1]].copy()
        return out

    def step(self):
        self._continue()
        out = super().step()
        self._continue()
        return out


def replay(rows, D, history=100, dtype=np.float64, kind='rosen', case=None, cls=FollowOracle):
    """Replays ``rows`` with the clean oracle on objective ``kind``.  case: an entry of tests/lbfgs_branch_cases.py, whose
    optimiser and run_fitting options then apply (else the production ones at ``history``); cls: the oracle to replay with
    (FollowOracle or a mutant of it).  Returns the oracle (``exhausted`` set when it wanted more closures than were recorded;
    ``final`` = what run_fitting returned, None then)."""
    fn, _ = ln.kat_objective(kind, D)
    okw, fkw = dict(history=history), dict(segments=SEGMENTS + [(13, D)])
    if case is not None:
        from tests import lbfgs_branch_cases as bc
        okw, fkw = bc.oracle_opts(case)
    fo = cls(rows, fn, dtype=dtype, **okw)
    fo.exhausted = False
    fo.final = None
    try:
        fo.final, _ = ln.run_fitting(fo, **fkw)
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
