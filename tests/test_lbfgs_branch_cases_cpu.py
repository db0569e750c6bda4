"""CPU: the case set of tests/lbfgs_branch_cases.py itself, before tests/test_gpu_lbfgs_branches.py judges the device with it.

(a) the branch sequences recorded in tests/golden/lbfgs_kat_branches.npz reach, between them, every tag of
    oracle/lbfgs_np.py:TAGS but UNREACHED;
(b) the clean oracle replaying the reference's own trace (tests/lbfgs_follow.py) proposes the reference's points: both
    sides are float64, the deviation is held to 1e-8 (measured worst 1.5e-9, gmof49_lr16_s1; 4e-12 or less elsewhere);
(c) wrong oracles - one wrong decision each, the slips a rewrite of the device's line search is most likely to make -
    replaying the same traces are caught by at least one case: a deviation above lbfgs_follow.TOL or another closure count.
    Caught by (deviation, or the closure count parted): insuf never set - gmof49_s2, steep49 (0.79); clamp always to
    min + eps - steep2_49 (0.89); swap condition reversed - gmof49_lr16_s1, wavy49_lr8_s0; one cubic formula -
    gmof49_lr16_s1, wavy49_lr8_s0 (0.7); max_ls bracket [t_prev, t] - steep49, steep2_49 (0.011); extrapolation bounds
    (t, 10 t) - gmof49_s2 (0.0096), wavy2_49_s1 (0.0019), steep49; ys threshold 0 - quad49_tight; no tolerance_grad test
    behind a search - rosen49_tg1e3, wavy49_tg30.  A swap that does not copy the gradient is no mutant at all: see
    test_the_swap_s_gradient_copy_is_never_read.
"""
import math

import numpy as np
import pytest

from oracle import lbfgs_np as ln
from tests import lbfgs_branch_cases as bc
from tests import lbfgs_follow as lf

GOLD = bc.load_golden()
# No case found for it (searched: the seven objectives at D = 49 and 86, 10 seeds x 5 start scales, lr 2^-5 .. 64, max_iter
# 1 .. 60, tolerance_change up to 1): a bisection needs d2_square < 0, and the only unbounded interpolation is the zoom's.
# 'zoom_reordered' (low / high re-ordered after the high end was replaced) is reached by the quartic at max_iter >= 59 only,
# in a zoom whose bracket is 1e-15 of its position: the reference and the oracle part there.  Both stay unreached.
UNREACHED = {'cubic_bisect_unbounded_x1_gt_x2', 'zoom_reordered'}


@pytest.fixture(scope='module')
def clean():
    with np.errstate(all='ignore'):
        return {c['name']: lf.replay(GOLD[c['name'] + '_trace'], c['D'], kind=c['kind'], case=c) for c in bc.CASES}


def test_the_cases_reach_every_branch():
    seen = set()
    for c in bc.CASES:
        tags = {t for _, t in bc.tags_of(GOLD, c['name'])}
        assert tags <= set(ln.TAGS), tags - set(ln.TAGS)
        seen |= tags
    assert set(ln.TAGS) - seen == UNREACHED, (sorted(set(ln.TAGS) - seen), sorted(UNREACHED))


def test_cubic_interpolate_reports_its_branches():
    """the module-level function through its hook - the one place where the bisection with x1 > x2 is taken at all"""
    def tags(*a, **kw):
        out = []
        return ln.cubic_interpolate(*a, tag=out.append, **kw), out
    assert tags(0.0, 0.0, 1.0, 1.0, 2.0 / 3.0, 1.0, bounds=(0.2, 0.6)) == (pytest.approx(0.4), ['cubic_bisect_bounds'])
    assert tags(0.0, 0.0, 1.0, 1.0, 2.0 / 3.0, 1.0) == (pytest.approx(0.5), ['cubic_bisect_unbounded'])
    assert tags(1.0, 2.0 / 3.0, 1.0, 0.0, 0.0, 1.0) == (pytest.approx(0.5), ['cubic_bisect_unbounded_x1_gt_x2'])
    assert tags(0.0, 0.25, -1.0, 1.0, 0.25, 1.0) == (pytest.approx(0.5), ['cubic_x1_le_x2'])
    assert tags(1.0, 0.25, 1.0, 0.0, 0.25, -1.0) == (pytest.approx(0.5), ['cubic_x1_gt_x2'])
    assert tags(0.0, 0.25, -1.0, 1.0, 0.25, 1.0, bounds=(0.6, 0.9)) == (0.6, ['cubic_x1_le_x2', 'cubic_clamp_lo'])
    assert tags(0.0, 0.25, -1.0, 1.0, 0.25, 1.0, bounds=(0.1, 0.4)) == (0.4, ['cubic_x1_le_x2', 'cubic_clamp_hi'])
    assert ln.cubic_interpolate(0.0, 0.25, -1.0, 1.0, 0.25, 1.0) == pytest.approx(0.5)          # without a hook


def test_exits_behind_a_first_trial_point_are_all_there():
    """the five stop tests of step() firing right behind a line search that ended at its first trial point: the device's
    lb_fast_accept has to refuse each"""
    seen = {t for c in bc.CASES for _, t in bc.tags_of(GOLD, c['name'])}
    assert {'exit_max_iter_first', 'exit_max_eval_first', 'exit_tol_grad_first', 'exit_step_small_first',
            'exit_loss_change_first'} <= seen


@pytest.mark.parametrize('case', bc.CASES, ids=lambda c: c['name'])
def test_clean_replay_of_the_reference_trace(case, clean):
    name = case['name']
    fo, rows = clean[name], GOLD[name + '_trace']
    assert len(rows) == int(GOLD[name + '_n']) <= bc.MAX_CLOSURES
    assert not fo.exhausted and len(fo.trace) == len(rows)
    assert fo.branches == bc.tags_of(GOLD, name)
    assert np.array_equal(GOLD[name + '_x0'], rows[0][:-1])
    print('%s: %d closures, worst deviation %.2g' % (name, len(rows), max(fo.dev)))
    assert max(fo.dev) <= 1e-8, (name, max(fo.dev))
    final = float(GOLD[name + '_final'])
    assert (fo.final is None and math.isnan(final)) or fo.final == pytest.approx(final, rel=1e-12, abs=1e-12)


# ---------------------------------------------------------------------------------------------------- wrong oracles
class InsufNeverSet(lf.FollowOracle):
    def _zoom_trial(self, t, br, insuf):
        t, _ = super()._zoom_trial(t, br, insuf)
        return t, False


class ClampAlwaysToMin(lf.FollowOracle):
    def _zoom_trial(self, t, br, insuf):
        t0 = t
        t, insuf = super()._zoom_trial(t, br, insuf)
        if t != t0:                                        # clamped
            t = min(br) + 0.1 * (max(br) - min(br))
        return t, insuf


class SwapWithoutGradient(lf.FollowOracle):
    def _zoom_swap(self, gtd_new, br, bf, bg, bgtd, low, high):
        if gtd_new * (br[high] - br[low]) >= 0:
            br[high] = br[low]; bf[high] = bf[low]; bgtd[high] = bgtd[low]


class SwapSignReversed(lf.FollowOracle):
    def _zoom_swap(self, gtd_new, br, bf, bg, bgtd, low, high):
        if gtd_new * (br[low] - br[high]) >= 0:
            br[high] = br[low]; bf[high] = bf[low]; bg[high] = bg[low]; bgtd[high] = bgtd[low]


class CubicOneFormula(lf.FollowOracle):
    """the x1 > x2 branch of the cubic computed with the x1 <= x2 formula"""

    def _cubic(self, x1, f1, g1, x2, f2, g2, bounds=None):
        lo, hi = bounds if bounds is not None else ((x1, x2) if x1 <= x2 else (x2, x1))
        d1 = g1 + g2 - 3 * (f1 - f2) / (x1 - x2)
        d2s = d1 * d1 - g1 * g2
        if d2s >= 0:
            d2 = math.sqrt(d2s)
            return min(max(x2 - (x2 - x1) * ((g2 + d2 - d1) / (g2 - g1 + 2 * d2)), lo), hi)
        return (lo + hi) / 2.0


class MaxLsBracketFromLastTrial(lf.FollowOracle):
    def _max_ls_bracket_start(self, t_prev):
        return t_prev


class ExtrapolationFromT(lf.FollowOracle):
    def _extrapolation_bounds(self, t, t_prev):
        return t, t * 10


class YsThresholdZero(lf.FollowOracle):
    YS_MIN = 0.0


class NoGradientTestAfterSearch(lf.FollowOracle):
    def _grad_small_after_search(self, g):
        return False


MUTANTS = [InsufNeverSet, ClampAlwaysToMin, SwapSignReversed, CubicOneFormula, MaxLsBracketFromLastTrial, ExtrapolationFromT,
           YsThresholdZero, NoGradientTestAfterSearch]


def caught(mutant, case):
    """(caught, what) of one mutant replaying one case's reference trace"""
    rows = GOLD[case['name'] + '_trace']
    with np.errstate(all='ignore'):
        try:
            fo = lf.replay(rows, case['D'], kind=case['kind'], case=case, cls=mutant)
        except (AssertionError, ZeroDivisionError, IndexError) as e:         # the mutant left the recorded run altogether:
            return False, 'raised ' + type(e).__name__                          # reported, but no catch - the GPU test sees deviations and counts only
    if fo.exhausted or len(fo.trace) != len(rows):
        return True, ('wants more than the %d closures' % len(rows)) if fo.exhausted else 'closures %d / %d' % (len(fo.trace), len(rows))
    return max(fo.dev) > lf.TOL, 'deviation %.2g' % max(fo.dev)


@pytest.mark.parametrize('mutant', MUTANTS, ids=lambda m: m.__name__)
def test_a_wrong_line_search_is_caught(mutant):
    hits = []
    for case in bc.CASES:
        got, what = caught(mutant, case)
        if got:
            hits.append('%s (%s)' % (case['name'], what))
        elif what.startswith('raised'):
            print('%s on %s: %s' % (mutant.__name__, case['name'], what))
    print('%s: caught by %s' % (mutant.__name__, ', '.join(hits) or 'NO CASE'))
    assert hits, mutant.__name__


def test_the_swap_s_gradient_copy_is_never_read(clean):
    """`bracket_g[high_pos] = bracket_g[low_pos]` of the swap (lbfgs_ls.py:150) is dead: the search reads bracket_g at
    low_pos only (:166), an end changes from high to low only at :141, and :139 has by then overwritten its gradient with
    the new trial point's.  So a swap that forgets the copy is the same function and no run can tell it apart - held here on
    the cases that swap, so that nobody looks for the case that catches it (the device copies the vector all the same)."""
    swaps = [c for c in bc.CASES if 'zoom_swap' in {t for _, t in bc.tags_of(GOLD, c['name'])}]
    assert len(swaps) >= 2
    for case in swaps:
        with np.errstate(all='ignore'):
            fo = lf.replay(GOLD[case['name'] + '_trace'], case['D'], kind=case['kind'], case=case, cls=SwapWithoutGradient)
        assert fo.dev == clean[case['name']].dev and not fo.exhausted
