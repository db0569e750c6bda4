"""The fit's planning (csrc/fit_plan.cpp) on the CPU: which phases a fit runs, each phase's driver, sub-batch size, form of the
vertex passes, work queue, launch cap and launches with their decoder-helper sets - built for the host (tests/
fit_plan_host_shim.cpp, ROCm's clang++) and pinned row by row.  The expected rows were worked out by hand from the rules
(DESIGN §4.4 has them as one table; they are the rules mvfit_fit followed when it still decided in line), not from this code.
Unless a row says otherwise: 256 compute units, 216 vertex tiles (SMPL), split-fp16 basis, sparse skinning, automatic options.
With 256 CUs the resident pass fits as form 1 (216 workgroups) beside <= 36 optimiser workgroups, as form 3 (108) beside <= 144.

Not reachable, so not pinned: 'N ring rows > 128' (a sub-batch beside the resident pass is sized from 128 or 96), and the
asynchronous drivers without the split-fp16 basis (every path into them asks for it: such a model fits in chained rounds)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from mvsmplfitting_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASYNC, ASYNC_SDF, SPARSE, GRAPH, EAGER = range(5)
NO_PAUSE = _lib.MAX_STAGES + 1
CAP = 1000
E_ARG = -1
FIELDS = ['B', 'n_cu', 'ntiles', 'half_basis', 'sparse_skinning', 'nv_even', 'helper_memory', 'profile', 'resident_auto_off',
          'debug_nopass', 'round_mode', 'resident_pass', 'sdf_two_phase', 'sdf_service', 'vposer_helpers', 'vposer_sets',
          'work_queue', 'flags', 'sdf_stages', 'num_stages', 'reuse_outer', 'cap']
DEFAULTS = dict(B=1, n_cu=256, ntiles=216, half_basis=1, sparse_skinning=1, nv_even=1, helper_memory=0, profile=0,
                resident_auto_off=0, debug_nopass=0, round_mode=0, resident_pass=-1, sdf_two_phase=1, sdf_service=1,
                vposer_helpers=1, vposer_sets=0, work_queue=1, flags=0, sdf_stages=0, num_stages=4, reuse_outer=0, cap=CAP)
VP = dict(helper_memory=1, flags=_lib.F_VPOSER)          # a model with the decoder, fitted with the VPoser prior
SDF = dict(sdf_stages=0b1100)                            # coll_loss_weight [0, 0, c, c]


@pytest.fixture(scope='module')
def shim():
    so = os.path.join(tempfile.mkdtemp(), 'libfit_plan_host.so')
    subprocess.run(['/opt/rocm/llvm/bin/clang++', '-O2', '-std=c++17', '-shared', '-fPIC', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'fit_plan_host_shim.cpp'),
                    os.path.join(ROOT, 'mvsmplfitting_amd', 'csrc', 'fit_plan.cpp'), '-o', so], check=True)
    lib = C.CDLL(so)
    lib.fit_plan_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_char_p, C.c_int]
    lib.fit_plan_nsets.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.fit_plan_constants.argtypes = [C.c_void_p]
    lib.fit_plan_pass_launch.argtypes = [C.c_int] * 5 + [C.c_void_p]
    lib.fit_plan_pass_launch.restype = None
    return lib


def inputs(**kw):
    assert not set(kw) - set(FIELDS), kw
    v = dict(DEFAULTS, **kw)
    return np.array([v[f] for f in FIELDS], np.int32)


def plan(lib, **kw):
    """{'rc', 'err', 'init', 'phases': [{'driver', 'pause', 'per', 'form', 'res_grid', 'refill', 'cap', 'launches': [(b_lo, b_hi,
    n_target, nsets)]}]}"""
    a = inputs(**kw)
    out = np.zeros(256, np.int32)
    err = C.create_string_buffer(256)
    n = lib.fit_plan_run(a.ctypes.data, out.ctypes.data, out.size, err, 256)
    assert 3 <= n <= out.size
    w = [int(x) for x in out[:n]]
    p = dict(rc=w[0], err=err.value.decode(), init=w[1], phases=[])
    i = 3
    for _ in range(w[2]):
        ph = dict(zip(['driver', 'pause', 'per', 'form', 'res_grid', 'refill', 'cap'], w[i:i + 7]))
        nl = w[i + 7]
        ph['launches'] = [tuple(w[i + 8 + 4 * k:i + 12 + 4 * k]) for k in range(nl)]
        i += 8 + 4 * nl
        p['phases'].append(ph)
    assert i == n
    return p


def one(lib, **kw):
    """the only phase of a fit that has one"""
    p = plan(lib, **kw)
    assert p['rc'] == 0 and len(p['phases']) == 1, p
    return p['phases'][0]


def rows(ph):
    return [(lo, hi) for lo, hi, _, _ in ph['launches']]


def sets(ph):
    return [s for _, _, _, s in ph['launches']]


def check_async(ph, per, form, res_grid, refill, launches, nsets=None, cap=CAP, driver=ASYNC, pause=NO_PAUSE):
    got = (ph['driver'], ph['pause'], ph['per'], ph['form'], ph['res_grid'], ph['refill'], ph['cap'], rows(ph))
    assert got == (driver, pause, per, form, res_grid, int(refill), cap, launches), got
    assert sets(ph) == (nsets if nsets is not None else [0] * len(launches))
    if not refill:          # a launch without a queue waits for its own problems (one with a queue for the whole batch)
        assert all(target == hi - lo for lo, hi, target, _ in ph['launches'])


def test_constants(shim):
    out = np.zeros(10, np.int32)
    shim.fit_plan_constants(out.ctypes.data)
    assert list(out) == [160, 128, 512, 8, 160, 96, 24, 16, 8, _lib.MAX_STAGES]


# ---- pinned rows: no prior ----
@pytest.mark.parametrize('B, per, form, res_grid', [(1, 32, 1, 216), (32, 32, 1, 216), (33, 64, 1, 216), (96, 96, 3, 108),
                                                     (128, 128, 3, 108)])
def test_async_one_launch(shim, B, per, form, res_grid):
    p = plan(shim, B=B)
    assert p['rc'] == 0 and p['init'] == 0 and len(p['phases']) == 1
    check_async(p['phases'][0], per, form, res_grid, False, [(0, B)])
    assert p['phases'][0]['launches'][0][2] == B


@pytest.mark.parametrize('B, mult', [(129, 3), (160, 3), (161, 3), (165, 3), (300, 4), (512, 5)])
def test_async_work_queue(shim, B, mult):
    """more problems than rows beside the resident pass: ONE launch of 128 rows that waits for all B problems; its cap is a
    row's, over the problems it takes (the per-problem cap is not enforced on this path)"""
    ph = one(shim, B=B)
    check_async(ph, 128, 3, 108, True, [(0, 128)], cap=mult * CAP)
    assert ph['launches'][0][2] == B


def test_async_work_queue_cap_saturates(shim):
    assert one(shim, B=300, cap=1 << 29)['cap'] == 1 << 30


def test_async_work_queue_off(shim):
    ph = one(shim, B=300, work_queue=0)
    check_async(ph, 128, 3, 108, False, [(0, 128), (128, 256), (256, 300)])
    assert [t for _, _, t, _ in ph['launches']] == [128, 128, 44]


# ---- pinned rows: VPoser helpers ----
@pytest.mark.parametrize('B, per, form, res_grid, launches, nsets', [
    (1, 32, 1, 216, [(0, 1)], [1]),
    (32, 32, 3, 108, [(0, 32)], [8]),              # the automatic choice drops 16 sets to 8, so the resident pass fits
    (33, 64, 3, 108, [(0, 33)], [8]),
    (96, 96, 0, 0, [(0, 96)], [8]),                # 160 workgroups leave no room for the resident pass
    (128, 64, 3, 108, [(0, 64), (64, 128)], [8, 8]),
    (129, 96, 0, 0, [(0, 96), (96, 129)], [8, 8]),
    (300, 96, 0, 0, [(0, 96), (96, 192), (192, 288), (288, 300)], [8, 8, 8, 12]),
])
def test_async_with_helpers(shim, B, per, form, res_grid, launches, nsets):
    p = plan(shim, B=B, **VP)
    assert p['init'] == 0
    check_async(one(shim, B=B, **VP), per, form, res_grid, False, launches, nsets)


def test_helper_set_knob(shim):
    assert sets(one(shim, B=32, vposer_sets=4, **VP)) == [4] and one(shim, B=32, vposer_sets=4, **VP)['form'] == 3
    # 16 asked for: no automatic drop, 160 workgroups, per-round passes
    ph = one(shim, B=32, vposer_sets=16, **VP)
    assert sets(ph) == [16] and (ph['form'], ph['res_grid']) == (0, 0)
    # the knob cannot push problems past a set's 24 slots, nor past 8 sets above 32 problems
    assert sets(one(shim, B=96, vposer_sets=1, **VP)) == [4] and one(shim, B=96, vposer_sets=1, **VP)['form'] == 3
    assert sets(one(shim, B=96, vposer_sets=16, **VP)) == [8]
    # never more sets than problems
    assert sets(one(shim, B=5, **VP)) == [5]


def test_helpers_off(shim):
    """vposer_helpers = 0, or a VPoser flag without helper memory, or helper memory without the flag: the plan of a fit without"""
    for kw in (dict(VP, vposer_helpers=0), dict(flags=_lib.F_VPOSER), dict(helper_memory=1)):
        check_async(one(shim, B=300, **kw), 128, 3, 108, True, [(0, 128)], cap=4 * CAP)
        check_async(one(shim, B=32, **kw), 32, 1, 216, False, [(0, 32)])


def test_plan_nsets_of_the_closure_route(shim):
    """closure_via_helpers: the automatic count without passes beside it, whatever vposer_sets says"""
    a = inputs(B=160, vposer_sets=3, **VP)
    want = {1: 1, 5: 5, 24: 16, 32: 16, 33: 8, 96: 8, 160: 8}
    assert {n: shim.fit_plan_nsets(a.ctypes.data, n, 0, 0) for n in want} == want
    assert shim.fit_plan_nsets(a.ctypes.data, 32, 0, 1) == 8 and shim.fit_plan_nsets(a.ctypes.data, 32, 16, 1) == 16


# ---- the form of the passes ----
def test_forced_resident_pass(shim):
    check_async(one(shim, B=32, resident_pass=0), 32, 0, 0, False, [(0, 32)])
    check_async(one(shim, B=300, resident_pass=0), 160, 0, 0, False, [(0, 160), (160, 300)])
    check_async(one(shim, B=128, resident_pass=1), 128, 1, 216, False, [(0, 128)])          # forced although it does not fit
    check_async(one(shim, B=32, resident_pass=2), 32, 3, 108, False, [(0, 32)])             # (form 2 maps to 3)
    check_async(one(shim, B=32, resident_pass=3), 32, 3, 108, False, [(0, 32)])
    check_async(one(shim, B=300, resident_pass=1), 128, 1, 216, True, [(0, 128)], cap=4 * CAP)
    # a forced form still needs the tables the resident pass reads
    check_async(one(shim, B=32, resident_pass=1, sparse_skinning=0), 32, 0, 0, False, [(0, 32)])


@pytest.mark.parametrize('off', [dict(sparse_skinning=0), dict(nv_even=0), dict(resident_auto_off=1), dict(debug_nopass=1)])
def test_per_round_passes(shim, off):
    """dense skinning rows, an odd vertex count, a ctx whose resident pass timed out, the no-pass hook: per-round launches, and
    sub-batches sized from 160"""
    check_async(one(shim, B=32, **off), 32, 0, 0, False, [(0, 32)])
    check_async(one(shim, B=160, **off), 160, 0, 0, False, [(0, 160)])
    check_async(one(shim, B=165, **off), 96, 0, 0, False, [(0, 96), (96, 165)])
    check_async(one(shim, B=300, **off), 160, 0, 0, False, [(0, 160), (160, 300)])
    # with helpers the sub-batch stays sized from 96
    check_async(one(shim, B=100, **dict(VP, **off)), 64, 0, 0, False, [(0, 64), (64, 100)], [8, 8])


def test_resident_auto_off_keeps_16_sets(shim):
    """nothing to make room for: the automatic set count is not halved"""
    check_async(one(shim, B=32, resident_auto_off=1, **VP), 32, 0, 0, False, [(0, 32)], [16])


def test_exact_fp32_runs_chained(shim):
    p = plan(shim, B=32, half_basis=0)
    assert p['init'] == 1 and [ph['driver'] for ph in p['phases']] == [GRAPH] and p['phases'][0]['cap'] == CAP
    p = plan(shim, B=32, half_basis=0, **SDF)
    assert p['init'] == 1 and [ph['driver'] for ph in p['phases']] == [GRAPH]


def test_other_device_sizes(shim):
    # 304 CUs: form 1 beside up to 84 workgroups
    check_async(one(shim, B=64, n_cu=304), 64, 1, 216, False, [(0, 64)])
    # 230 CUs: the queue's 128 rows + 108 resident workgroups exceed the 226 the form was chosen for (96 rows): kept as it is
    check_async(one(shim, B=129, n_cu=230), 128, 3, 108, True, [(0, 128)], cap=3 * CAP)
    # 64 CUs: nothing fits
    check_async(one(shim, B=32, n_cu=64), 32, 0, 0, False, [(0, 32)])


# ---- modes ----
def test_round_mode_1(shim):
    for kw in ({}, SDF, VP):
        p = plan(shim, B=32, round_mode=1, **kw)
        assert p['rc'] == 0 and p['init'] == 1 and [ph['driver'] for ph in p['phases']] == [GRAPH]
        assert p['phases'][0]['cap'] == CAP and p['phases'][0]['launches'] == []
    p = plan(shim, B=32, round_mode=1, profile=1)
    assert p['init'] == 1 and [ph['driver'] for ph in p['phases']] == [EAGER] and p['phases'][0]['cap'] == CAP


def test_profile_keeps_the_asynchronous_fit(shim):
    check_async(one(shim, B=32, profile=1), 32, 1, 216, False, [(0, 32)])


def test_reuse_outer_has_no_queue(shim):
    check_async(one(shim, B=300, reuse_outer=1, flags=_lib.F_REUSE_OUTER_VALUE), 128, 3, 108, False,
                [(0, 128), (128, 256), (256, 300)])


@pytest.mark.parametrize('B, launches, nsets', [(165, [(0, 165)], [0]), (1, [(0, 1)], [0])])
def test_sparse_verts(shim, B, launches, nsets):
    for kw in ({}, dict(half_basis=0), dict(round_mode=1), dict(profile=1)):
        p = plan(shim, B=B, flags=_lib.F_SPARSE_VERTS, **kw)
        ph = p['phases'][0]
        assert p['init'] == 0 and len(p['phases']) == 1
        assert (ph['driver'], ph['pause'], ph['per'], ph['cap'], rows(ph), sets(ph)) == (SPARSE, NO_PAUSE, B, CAP, launches, nsets)
        assert [t for _, _, t, _ in ph['launches']] == [B]


@pytest.mark.parametrize('B, per, launches, nsets', [
    (32, 32, [(0, 32)], [16]),                     # no passes beside it: 16 sets
    (33, 33, [(0, 33)], [8]),
    (160, 160, [(0, 160)], [8]),
    (165, 83, [(0, 83), (83, 165)], [8, 8]),       # all workgroups resident: at most 160 problems per launch (not whole chunks)
    (400, 134, [(0, 134), (134, 268), (268, 400)], [8, 8, 8]),
])
def test_sparse_verts_with_helpers(shim, B, per, launches, nsets):
    ph = one(shim, B=B, helper_memory=1, flags=_lib.F_SPARSE_VERTS | _lib.F_VPOSER)
    assert (ph['driver'], ph['per'], ph['cap'], rows(ph), sets(ph)) == (SPARSE, per, CAP, launches, nsets)
    assert plan(shim, B=B, helper_memory=1, flags=_lib.F_SPARSE_VERTS | _lib.F_VPOSER)['init'] == 0


def test_sparse_verts_helpers_off(shim):
    ph = one(shim, B=400, helper_memory=1, vposer_helpers=0, flags=_lib.F_SPARSE_VERTS | _lib.F_VPOSER)
    assert (ph['driver'], rows(ph), sets(ph)) == (SPARSE, [(0, 400)], [0])


# ---- fits with the SDF term ----
def test_sdf_two_phase_with_service(shim):
    """stages 0-1 asynchronously up to the pause in front of stage 2, then service rounds (per-round passes: sized from 160)"""
    p = plan(shim, B=32, **SDF)
    assert p['rc'] == 0 and p['init'] == 0 and len(p['phases']) == 2
    check_async(p['phases'][0], 32, 1, 216, False, [(0, 32)], pause=2)
    check_async(p['phases'][1], 32, 0, 0, False, [(0, 32)], driver=ASYNC_SDF)
    # SPARSE_VERTS is ignored while the term is active
    assert plan(shim, B=32, flags=_lib.F_SPARSE_VERTS, **SDF) == dict(p)
    # dense skinning (the model of the GPU tests of this path), B = 165
    p = plan(shim, B=165, sparse_skinning=0, **SDF)
    check_async(p['phases'][0], 96, 0, 0, False, [(0, 96), (96, 165)], pause=2)
    check_async(p['phases'][1], 96, 0, 0, False, [(0, 96), (96, 165)], driver=ASYNC_SDF)


def test_sdf_service_tail_sub_batches(shim):
    """every non-final sub-batch of a service tail hands launch_sdf_term b_hi < B: B > 160, B > 96 with helpers"""
    check_async(plan(shim, B=165, **SDF)['phases'][1], 96, 0, 0, False, [(0, 96), (96, 165)], driver=ASYNC_SDF)
    check_async(plan(shim, B=160, **SDF)['phases'][1], 160, 0, 0, False, [(0, 160)], driver=ASYNC_SDF)
    check_async(plan(shim, B=100, **dict(VP, **SDF))['phases'][1], 64, 0, 0, False, [(0, 64), (64, 100)], [8, 8], driver=ASYNC_SDF)
    check_async(plan(shim, B=96, **dict(VP, **SDF))['phases'][1], 96, 0, 0, False, [(0, 96)], [8], driver=ASYNC_SDF)


def test_sdf_lead_phase_keeps_the_work_queue(shim):
    """Two-phase fit, B = 165, sparse skinning, no helpers: the lead phase plans refill together with a pause_stage - one launch
    of 128 rows whose target is the whole batch.  A row whose problem pauses at the stage boundary takes the next problem from
    the queue like one whose problem finished (fit_persistent_kernel: `done || paused`), so problems 128..164 run their lead
    stages on rows that became free (on the GPU: tests/test_gpu_sdf_batches.py, work_queue 1 against 0)."""
    p = plan(shim, B=165, **SDF)
    assert p['rc'] == 0 and p['init'] == 0 and len(p['phases']) == 2
    check_async(p['phases'][0], 128, 3, 108, True, [(0, 128)], cap=3 * CAP, pause=2)
    assert p['phases'][0]['launches'][0][2] == 165
    check_async(p['phases'][1], 96, 0, 0, False, [(0, 96), (96, 165)], driver=ASYNC_SDF)


def test_sdf_service_off(shim):
    p = plan(shim, B=32, sdf_service=0, **SDF)
    assert p['init'] == 0 and [ph['driver'] for ph in p['phases']] == [ASYNC, GRAPH]
    check_async(p['phases'][0], 32, 1, 216, False, [(0, 32)], pause=2)
    assert p['phases'][1]['cap'] == CAP and p['phases'][1]['pause'] == NO_PAUSE
    p = plan(shim, B=165, sdf_service=0, sparse_skinning=0, **SDF)
    check_async(p['phases'][0], 96, 0, 0, False, [(0, 96), (96, 165)], pause=2)
    assert p['phases'][1]['driver'] == GRAPH


def test_sdf_two_phase_off(shim):
    """chained rounds in every stage; the service goes with it"""
    p = plan(shim, B=32, sdf_two_phase=0, **SDF)
    assert p['init'] == 1 and [ph['driver'] for ph in p['phases']] == [GRAPH]


def test_sdf_profiled_and_reuse_outer_keep_chained_tails(shim):
    p = plan(shim, B=32, profile=1, **SDF)
    assert p['init'] == 0 and [ph['driver'] for ph in p['phases']] == [ASYNC, EAGER] and p['phases'][0]['pause'] == 2
    p = plan(shim, B=165, reuse_outer=1, flags=_lib.F_REUSE_OUTER_VALUE, **SDF)
    assert p['init'] == 0 and [ph['driver'] for ph in p['phases']] == [ASYNC, GRAPH]
    check_async(p['phases'][0], 96, 3, 108, False, [(0, 96), (96, 165)], pause=2)          # (no queue with reuse_outer)


def test_sdf_in_the_first_stage_has_no_lead_phase(shim):
    for mask in (0b1111, 0b0001, 0b0101):
        check_async(one(shim, B=32, sdf_stages=mask), 32, 0, 0, False, [(0, 32)], driver=ASYNC_SDF)
        assert plan(shim, B=32, sdf_stages=mask)['init'] == 0
        p = plan(shim, B=32, sdf_stages=mask, sdf_service=0)
        assert p['init'] == 1 and [ph['driver'] for ph in p['phases']] == [GRAPH]
        p = plan(shim, B=32, sdf_stages=mask, profile=1)
        assert p['init'] == 1 and [ph['driver'] for ph in p['phases']] == [EAGER]


def test_sdf_pause_stage_is_the_first_stage_with_the_term(shim):
    assert plan(shim, B=32, sdf_stages=0b1000)['phases'][0]['pause'] == 3
    assert plan(shim, B=32, sdf_stages=0b1010)['phases'][0]['pause'] == 1
    assert plan(shim, B=32, sdf_stages=0b10, num_stages=2)['phases'][0]['pause'] == 1
    # stages past num_stages do not count
    check_async(one(shim, B=32, sdf_stages=0, num_stages=2), 32, 1, 216, False, [(0, 32)])


# ---- errors ----
def test_too_many_resident_workgroups(shim):
    for kw in (dict(ntiles=520, resident_pass=1), dict(ntiles=520, n_cu=1000), dict(ntiles=1026, resident_pass=3)):
        p = plan(shim, B=1, **kw)
        n = 520 if kw['ntiles'] == 520 else 513
        assert p['rc'] == E_ARG and p['err'] == 'resident vertex pass: %d workgroups > 512 back-pressure words' % n
    assert plan(shim, B=1, ntiles=1024, resident_pass=3)['rc'] == 0
    # the service tail of an SDF fit has per-round passes: only the lead phase can fail
    assert plan(shim, B=1, ntiles=520, resident_pass=1, sdf_stages=0b1111)['rc'] == 0
    assert plan(shim, B=1, ntiles=520, resident_pass=1, **SDF)['rc'] == E_ARG


# ---- properties ----
def test_properties_of_every_batch_size(shim):
    n_cu = 256
    for helpers in (0, 1):
        for wq in (0, 1):
            for B in range(1, 700):
                ph = one(shim, B=B, work_queue=wq, **(VP if helpers else {}))
                where = (B, helpers, wq, ph)
                assert ph['driver'] == ASYNC and ph['per'] % 32 == 0, where
                assert ph['cap'] >= CAP and (ph['cap'] == CAP or ph['refill']), where
                assert ph['form'] == 0 or ph['per'] <= 128, where
                assert ph['res_grid'] == {0: 0, 1: 216, 3: 108}[ph['form']], where
                for lo, hi, target, nsets in ph['launches']:
                    assert 0 < hi - lo <= ph['per'], where
                    assert (hi - lo) + 8 * nsets + ph['res_grid'] <= n_cu - 4, where          # all workgroups resident
                    assert (0 < nsets and hi - lo <= 24 * nsets) if helpers else nsets == 0, where   # a set has 24 slots
                    assert target == (B if ph['refill'] else hi - lo), where
                if ph['refill']:
                    assert wq and not helpers and B > 128 and rows(ph) == [(0, 128)], where
                else:
                    r = rows(ph)
                    assert r[0][0] == 0 and r[-1][1] == B and all(a[1] == b[0] for a, b in zip(r, r[1:])), where


# ---- which instantiation of the single-launch kernel a launch runs (fit_plan.h: PersistentVariant) ----
PLAIN, LEAN, REUSE, REUSE_LEAN, HELPERS, HELPERS_REUSE, QUEUE, QUEUE_LEAN, SDF_SERVICE, SDF_HELPERS = range(10)
# (sdf_service, queue, helpers, reuse_outer, lean) -> variant: the service first, then the queue, then the helpers; reuse_outer
# and lean count only where the row above has an instantiation for them.  All 32 rows, written out.
VARIANTS = {
    (0, 0, 0, 0, 0): PLAIN,         (0, 0, 0, 0, 1): LEAN,
    (0, 0, 0, 1, 0): REUSE,         (0, 0, 0, 1, 1): REUSE_LEAN,
    (0, 0, 1, 0, 0): HELPERS,       (0, 0, 1, 0, 1): HELPERS,
    (0, 0, 1, 1, 0): HELPERS_REUSE, (0, 0, 1, 1, 1): HELPERS_REUSE,
    (0, 1, 0, 0, 0): QUEUE,         (0, 1, 0, 0, 1): QUEUE_LEAN,
    (0, 1, 0, 1, 0): QUEUE,         (0, 1, 0, 1, 1): QUEUE_LEAN,
    (0, 1, 1, 0, 0): QUEUE,         (0, 1, 1, 0, 1): QUEUE_LEAN,
    (0, 1, 1, 1, 0): QUEUE,         (0, 1, 1, 1, 1): QUEUE_LEAN,
    (1, 0, 0, 0, 0): SDF_SERVICE,   (1, 0, 0, 0, 1): SDF_SERVICE,
    (1, 0, 0, 1, 0): SDF_SERVICE,   (1, 0, 0, 1, 1): SDF_SERVICE,
    (1, 0, 1, 0, 0): SDF_HELPERS,   (1, 0, 1, 0, 1): SDF_HELPERS,
    (1, 0, 1, 1, 0): SDF_HELPERS,   (1, 0, 1, 1, 1): SDF_HELPERS,
    (1, 1, 0, 0, 0): SDF_SERVICE,   (1, 1, 0, 0, 1): SDF_SERVICE,
    (1, 1, 0, 1, 0): SDF_SERVICE,   (1, 1, 0, 1, 1): SDF_SERVICE,
    (1, 1, 1, 0, 0): SDF_HELPERS,   (1, 1, 1, 0, 1): SDF_HELPERS,
    (1, 1, 1, 1, 0): SDF_HELPERS,   (1, 1, 1, 1, 1): SDF_HELPERS,
}


@pytest.mark.parametrize('case', sorted(VARIANTS), ids=lambda c: ''.join(map(str, c)))
def test_persistent_variant(shim, case):
    assert shim.fit_plan_persistent_variant(*case) == VARIANTS[case]


def test_persistent_variant_count(shim):
    assert len(VARIANTS) == 32
    assert shim.fit_plan_persistent_variant_count() == 10 == len(set(VARIANTS.values()))


# ---- which kernel a per-round vertex pass runs (fit_plan.h: plan_pass_launch) ----
EXACT, SPLIT, LOOP, PIPE = range(4)
# (split-fp16 basis, sparse skinning rows, even vertex count) -> (kernel, workgroups per tile) for chunks 1, 2, 5 (rows) x
# pass_kernel 0, 1, 2 (columns).  All 72 cells, written out; the SPARSE_W instantiation is the model's sparse_skinning everywhere
# but in the lock-step loop, which has none, and in the pipeline, which has no other.
PASS_TABLE = {
    (0, 0, 0): [[(EXACT, 1)] * 3, [(EXACT, 2)] * 3, [(EXACT, 5)] * 3],
    (0, 0, 1): [[(EXACT, 1)] * 3, [(EXACT, 2)] * 3, [(EXACT, 5)] * 3],
    (0, 1, 0): [[(EXACT, 1)] * 3, [(EXACT, 2)] * 3, [(EXACT, 5)] * 3],
    (0, 1, 1): [[(EXACT, 1)] * 3, [(EXACT, 2)] * 3, [(EXACT, 5)] * 3],
    (1, 0, 0): [[(SPLIT, 1)] * 3, [(LOOP, 1), (SPLIT, 2), (LOOP, 1)], [(LOOP, 1), (SPLIT, 5), (LOOP, 1)]],
    (1, 0, 1): [[(SPLIT, 1)] * 3, [(LOOP, 1), (SPLIT, 2), (LOOP, 1)], [(LOOP, 1), (SPLIT, 5), (LOOP, 1)]],
    (1, 1, 0): [[(SPLIT, 1)] * 3, [(SPLIT, 2), (SPLIT, 2), (SPLIT, 2)], [(SPLIT, 5), (SPLIT, 5), (SPLIT, 5)]],
    (1, 1, 1): [[(SPLIT, 1)] * 3, [(PIPE, 1), (SPLIT, 2), (PIPE, 1)], [(PIPE, 1), (SPLIT, 5), (PIPE, 1)]],
}
PASS_CELLS = [(key, ci, pk) for key in sorted(PASS_TABLE) for ci in range(3) for pk in range(3)]


@pytest.mark.parametrize('key, ci, pk', PASS_CELLS, ids=lambda v: ''.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_pass_launch(shim, key, ci, pk):
    split, sparse, even = key
    chunks = (1, 2, 5)[ci]
    out = np.zeros(3, np.int32)
    shim.fit_plan_pass_launch(split, sparse, even, chunks, pk, out.ctypes.data)
    kernel, grid_y = PASS_TABLE[key][ci][pk]
    want_sparse = {LOOP: 0, PIPE: 1}.get(kernel, sparse)
    assert tuple(out) == (kernel, want_sparse, grid_y)


def test_pass_launch_table_is_whole(shim):
    assert len(PASS_CELLS) == 72 and shim.fit_plan_pass_kernel_count() == 4
    # pass_kernel 2 is pass_kernel 0 in every cell
    assert all(row[0] == row[2] for rows_ in PASS_TABLE.values() for row in rows_)


def test_pass_plan_helper_reads_the_same_table():
    """tests/pass_plan.py (the ids of the GPU matrix) against the table above"""
    from tests import pass_plan
    for key, ci, pk in PASS_CELLS:
        kernel, grid_y = PASS_TABLE[key][ci][pk]
        got = pass_plan.pass_launch(*key, (1, 2, 5)[ci], pk)
        assert (got[0], got[2]) == (kernel, grid_y)
    assert pass_plan.kernel_name(SPLIT, 1) == 'lbs_vertex_pass_split_kernel<true>'
    assert pass_plan.kernel_name(PIPE, 1) == 'lbs_vertex_pass_pipe_kernel'
    assert pass_plan.short_name(1, 1, 1, 129, 0) == 'pipe' and pass_plan.short_name(1, 0, 0, 97, 0) == 'loop_dense'
    assert pass_plan.short_name(1, 1, 0, 65, 0) == 'split_sparse' and pass_plan.short_name(0, 0, 0, 65, 0) == 'exact_dense'
