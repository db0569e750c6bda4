"""TEST INFRASTRUCTURE - the known-answer runs that walk every line-search branch of the L-BFGS (oracle/lbfgs_np.py:TAGS).

One entry per run: the objective (oracle/lbfgs_np.py:kat_objective, the device's kat_eval), the optimiser options of
mvfit_lbfgs_opts and the start.  ``start`` says how oracle/make_golden.py made x0 - (seed, sc): the objective's own start
+ sc * default_rng(seed).normal(D); None: the objective's own start; 'huge': see NONFINITE - the tests never regenerate it:
they read x0 from tests/golden/lbfgs_kat_branches.npz, like the reference's trace from that start.

lr and the four tolerances reach the device through float32 fields: F32 rounds them once, here, and every side (the
reference when the golden is made, the oracle, the device) gets the rounded value.

Shared by oracle/make_golden.py (goldens), tests/test_lbfgs_oracle.py, tests/test_lbfgs_branch_cases_cpu.py and
tests/test_gpu_lbfgs_branches.py.
"""
import os

import numpy as np

DEFAULTS = dict(lr=1.0, max_iter=30, history=100, tolerance_grad=1e-5, tolerance_change=1e-9, maxiters=30, ftol=1e-9, gtol=1e-9)
F32 = ('lr', 'tolerance_grad', 'tolerance_change', 'ftol', 'gtol')
MAX_CLOSURES = 160
KIND = dict(quad=0, rosen=1, gmof=2, linear=3, wavy=4, wavy2=5, steep=6, steep2=7)        # include/mvfit.h:mvfit_lbfgs_kat
NONFINITE = 'quad49_inf'      # x0 = start + 1e155 cos(i): the loss overflows to inf, the gradient does not


def _case(name, kind, D, start=None, **opts):
    assert not set(opts) - set(DEFAULTS), opts
    c = dict(DEFAULTS, **opts)
    for k in F32:
        c[k] = float(np.float32(c[k]))
    c.update(name=name, kind=kind, D=D, start=start)
    return c


CASES = [
    # ---- zoom phase: insufficient progress, swap, x1 > x2 ----
    _case('gmof49_lr16', 'gmof', 49, lr=16),                                  # insuf set
    _case('gmof49_s2', 'gmof', 49, (2, 2.0)),                                 # insuf = 1 clamp to min; bracket failure at it = 1; max_eval behind a first trial
    _case('gmof49_lr16_s1', 'gmof', 49, (1, 0.5), lr=16),                     # swap; cubic with x1 > x2
    _case('wavy49_lr8_s0', 'wavy', 49, (0, 0.5), lr=8),                       # insuf, swap, x1 > x2 on another objective
    _case('wavy49_lr32_mi1_s0', 'wavy', 49, (0, 0.5), lr=32, max_iter=1),     # zoom ended by max_iter; max_iter behind a first trial
    _case('wavy49_mi1_s6', 'wavy', 49, (6, 2.0), max_iter=1),                 # zoom skipped
    _case('wavy2_49_s1', 'wavy2', 49, (1, 4.0)),                              # bracket failure at it >= 2
    _case('quad86_s0', 'quad', 86, (0, 2.0)),                                 # Wolfe after two extrapolations
    _case('steep49', 'steep', 49, max_iter=48, maxiters=1),                   # max_ls; clamp to max and to min with insuf = 0; unbounded bisection; empty-history rejection
    _case('steep2_49', 'steep2', 49, maxiters=1),                             # max_ls, then clamp to max on the bracket [0, t]
    # ---- exits ----
    _case('quad49_tg1e3', 'quad', 49, tolerance_grad=1e3),
    _case('rosen49_tg1e3', 'rosen', 49, tolerance_grad=1e3),
    _case('wavy49_tg30', 'wavy', 49, tolerance_grad=30.0),                    # tolerance_grad behind a zoom
    _case('gmof49_gtol', 'gmof', 49, gtol=0.1),                               # run_fitting's gtol test
    _case('quad49_tc01', 'quad', 49, tolerance_change=0.1),                   # step-size test behind a first trial
    _case('wavy2_49_tc01_s3', 'wavy2', 49, (3, 0.5), tolerance_change=0.1),   # loss-change test behind a first trial
    _case('wavy2_49_lr4_tc001_s3', 'wavy2', 49, (3, 0.25), lr=4, tolerance_change=0.01),   # loss-change test behind a zoom
    _case('quad49_tight', 'quad', 49, tolerance_grad=1e-9, tolerance_change=1e-12),   # pairs rejected with 0 < y.s <= 1e-10
    _case('gmof49_mi4', 'gmof', 49, max_iter=4),                              # max_eval
    _case('wavy49_maxiters2', 'wavy', 49, maxiters=2),                        # run_fitting runs out of outer iterations
    _case('wavy2_86_h3', 'wavy2', 86, history=3),                             # eviction
    _case('quad96', 'quad', 96),                                              # D = the row stride LB_D
    _case(NONFINITE, 'quad', 49, 'huge'),                                     # non-finite loss at the opening closure; NaN direction from the 4th closure on: max_ls, zoom and exits on NaNs
]
assert len({c['name'] for c in CASES}) == len(CASES)

SEGMENTS = lambda D: [(0, 10), (10, 13), (13, D)]                           # the gtol segments of every KAT run


def oracle_opts(c):
    """keyword arguments of LbfgsOracle / of run_fitting"""
    return (dict(lr=c['lr'], max_iter=c['max_iter'], history=c['history'], tol_grad=c['tolerance_grad'],
                 tol_change=c['tolerance_change']),
            dict(maxiters=c['maxiters'], ftol=c['ftol'], gtol=c['gtol'], segments=SEGMENTS(c['D'])))


def device_opts(c):
    """keyword arguments of engine.lbfgs_kat"""
    return {k: c[k] for k in DEFAULTS}


def make_x0(c):
    """How oracle/make_golden.py makes the start of a case (the tests read the stored one)."""
    from oracle import lbfgs_np as ln
    _, x0 = ln.kat_objective(c['kind'], c['D'])
    if c['start'] == 'huge':
        return x0 + 1e155 * np.cos(np.arange(c['D'], dtype=np.float64))
    if c['start'] is not None:
        seed, sc = c['start']
        return x0 + sc * np.random.default_rng(seed).normal(size=c['D'])
    return x0


def load_golden():
    from tests.helpers import GOLD
    return dict(np.load(os.path.join(GOLD, 'lbfgs_kat_branches.npz')))


def tags_of(gold, name):
    """The recorded branch sequence of a case: [(closure index, tag)]"""
    return list(zip(gold[name + '_tag_at'].tolist(), gold[name + '_tags'].tolist()))
