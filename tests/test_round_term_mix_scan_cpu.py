"""The scan share of the term mix in the plan of a round's term (csrc/round_term.cpp) on the CPU: the step list of every mix
with a scan share, the pass-through rule with the scan among the vertex terms, the plan's bytes - the key of the captured round
graph - and that a mix without the share is the plan it was.  Built for the host from tests/round_term_mix_scan_host_shim.cpp,
the sibling of round_term_scan_host_shim.cpp that also fills the mix's four scan inputs and writes out the new step fields
(behind the old ones).  Expected values are written out from the rules: silhouette evaluation, target kernel,
scan evaluation with the MIX's scan scalars, cotangent mix, one pull-back, scene term, record merge."""
import ctypes as C
import itertools
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import test_round_term_cpu as base
from tests import test_round_term_scan_cpu as sbase
from tests.test_round_term_cpu import (ALWAYS, MASKS, MIX, MIX_ALL, MIX_COTANGENT, MIX_RECORD, MIX_SCENE, MIX_W, MIXED, OCC, PULLBACK, ROWS,
                                       SIL_OUT, TARGETS)
from tests.test_round_term_scan_cpu import SCAN_EVAL

ROOT = base.ROOT
MIX_SCAN_FIELDS = [('mix.scan', 'F'), ('mix.scan_w_s2m', 'F'), ('mix.scan_w_m2s', 'F'), ('mix.scan_sigma', 'F')]
FIELDS = sbase.FIELDS + MIX_SCAN_FIELDS
KIND = dict(FIELDS)
SLOT_FLAGS = sbase.SLOT_FLAGS
# what a scan share adds to a mix's consumed inputs: the set's baked values, the MIX's scalars, the scan term's round buffers
SCAN_SET = ['scan.ws', 'scan.N', 'scan.Pmax', 'scan.nf', 'scan.ns', 'scan.faces', 'scan.g_verts', 'scan.loss']
MIX_SCAN_W = ['mix.scan_w_s2m', 'mix.scan_w_m2s', 'mix.scan_sigma']
SCAN_SHARE = SCAN_SET + MIX_SCAN_W + ['mix.scan']


def _base():
    """test_round_term_scan_cpu's base state (a scan set present, its term off, the term's own scalars set) and the mix's four
    scan inputs at distinct values with the share 0"""
    v = sbase._base()
    for i, (name, _kind) in enumerate(MIX_SCAN_FIELDS):
        v[name] = 40.5 + 0.125 * i
    v['mix.scan'] = 0.0
    return v


def _mix(sc, sil, vt, scan, **kw):
    return dict(_base(), **dict({'mix.on': 1, 'mix.scene': sc, 'mix.silhouette': sil, 'mix.vertex_targets': vt, 'mix.scan': scan,
                                 'obst.on': 1}, **kw))


def _flat(v):
    assert set(v) == set(KIND), set(v) ^ set(KIND)
    return np.array([v[name] for name, _ in FIELDS], np.float64)


@pytest.fixture(scope='module')
def shim():
    so = os.path.join(tempfile.mkdtemp(), 'libround_term_mix_scan_host.so')
    subprocess.run(['/opt/rocm/llvm/bin/clang++', '-O2', '-std=c++17', '-shared', '-fPIC', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'round_term_mix_scan_host_shim.cpp'),
                    os.path.join(ROOT, 'mvsmplfitting_amd', 'csrc', 'round_term.cpp'), '-o', so], check=True)
    lib = C.CDLL(so)
    lib.round_term_slot.argtypes = [C.c_void_p]
    lib.round_term_name.argtypes = [C.c_int]
    lib.round_term_name.restype = C.c_char_p
    lib.round_term_plan.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    assert lib.round_term_num_inputs() == len(FIELDS)
    return lib


def plan(lib, v, live=1):
    """test_round_term_cpu.plan over this file's fields"""
    a = _flat(v)
    out = np.zeros(256, np.float64)
    key = np.full(lib.round_term_key_bytes(), 0xa5, np.uint8)
    n = lib.round_term_plan(a.ctypes.data, live, out.ctypes.data, out.size, key.ctypes.data)
    assert 7 <= n <= out.size
    w = [float(x) for x in out[:n]]
    p = dict(kind=int(w[0]), B=int(w[1]), Bpad=int(w[2]), nv=int(w[3]), sums=(int(w[4]), int(w[5])), steps=[])
    i = 7
    for _ in range(int(w[6])):
        m = int(w[i + 1])
        p['steps'].append((int(w[i]), w[i + 2:i + 2 + m]))
        i += 2 + m
    assert i == n
    return p, key.tobytes()


def _changed(v, name):
    """one input at another value (a share stays > 0 where it was, and leaves exactly 1)"""
    w = dict(v)
    w[name] = {'P': v[name] + 8, 'I': v[name] + 1, 'F': v[name] * 1.5 + 0.25, 'B': 1 - v[name]}[KIND[name]]
    return w


# ---- the expected steps, from the rules ----
def scan_eval(v):
    """the set's baked values, the mix's scalars (not the scan term's own), the scan term's round buffers"""
    return (SCAN_EVAL, [v['scan.ws'], v['scan.faces'], v['scan.N'], v['scan.Pmax'], v['scan.nf'], v['scan.ns'], v['mix.scan_w_s2m'],
                        v['mix.scan_w_m2s'], v['mix.scan_sigma'], v['scan.loss'], v['scan.g_verts']])


def cotangent(v, sil, vt, scan, parts_sums):
    old = base.cotangent(v, sil, vt, parts_sums)[1]
    return (MIX_COTANGENT, old + ([v['mix.scan'], v['scan.g_verts'], v['scan.loss']] if scan else [0.0, 0, 0]))


def record(v, sil, vt, scan):
    old = base.record(v, sil, vt)[1]
    return (MIX_RECORD, old + ([v['mix.scan'], v['scan.loss']] if scan else [0.0, 0]))


def expected(v, passes=None):
    """the mix's steps for the shares in v; passes: the term ('scan') whose own buffers go to the pull-back"""
    sc, sil, vt, scan = (v[k] > 0 for k in ('mix.scene', 'mix.silhouette', 'mix.vertex_targets', 'mix.scan'))
    steps = []
    if sil:
        steps.append(base.sil_eval(v, 'mix'))
    if vt:
        steps.append(base.vt_eval(v))
    if scan:
        steps.append(scan_eval(v))
    rec = v['mix.rec_verts'] if sc else v['sdf_adj']
    if passes:
        steps.append(base.pullback(v[passes + '.g_verts'], v[passes + '.loss'], v['mix.part'], rec))
    else:
        steps.append(cotangent(v, sil, vt, scan, not sc))
        steps.append(base.mixed_pull(v, rec))
    if sc:
        steps.append(base.scene(v, v['mix.rec_scene']))
        steps.append(record(v, sil, vt, scan))
    return steps


def consumed(v, passes=False):
    sc, sil, vt = (v[k] > 0 for k in ('mix.scene', 'mix.silhouette', 'mix.vertex_targets'))
    live = ALWAYS + MIX_ALL + SCAN_SHARE + ([] if passes else MIXED)
    if sc:
        live += MIX_SCENE
    if sil:
        live += MASKS + MIX_W + SIL_OUT + (OCC if v['sil.occ_on'] else [])
    if vt:
        live += TARGETS
    return set(live)


# every subset of shares with at least two > 0 and the scan among them (share values other than 1)
SUBSETS = [s for s in itertools.product((0, 1), repeat=3) if any(s)]
SHARE = (0.5, 0.75, 2.0)


def _subset_state(s):
    return _mix(*(SHARE[i] * s[i] for i in range(3)), 1.5, **{'sil.occ_on': 1})


def test_there_are_seven_subsets_and_seven_steps_at_most(shim):
    assert len(SUBSETS) == 7
    assert shim.round_term_max_steps() == 7
    p, _ = plan(shim, _subset_state((1, 1, 1)))
    assert len(p['steps']) == 7
    assert [k for k, _ in p['steps']] == [base.SIL_EVAL, base.VT_EVAL, SCAN_EVAL, MIX_COTANGENT, PULLBACK, base.SCENE_STEP, MIX_RECORD]


@pytest.mark.parametrize('subset', SUBSETS)
def test_step_list(shim, subset):
    v = _subset_state(subset)
    p, _key = plan(shim, v)
    want = expected(v)
    assert (p['kind'], p['B'], p['Bpad'], p['nv']) == (MIX, v['B'], v['Bpad'], v['nv'])
    assert [k for k, _ in p['steps']] == [k for k, _ in want]
    for i, ((_, got), (_, w)) in enumerate(zip(p['steps'], want)):
        assert got == [float(x) for x in w], (i, got, w)
    assert p['sums'] == (v['mix.sums'], 4)


@pytest.mark.parametrize('subset', SUBSETS)
def test_the_key_changes_with_what_a_live_step_consumes_and_with_nothing_else(shim, subset):
    v = _subset_state(subset)
    live = consumed(v)
    assert live <= set(KIND)
    _, key = plan(shim, v)
    for field, _kind in FIELDS:
        if field in SLOT_FLAGS:
            continue
        _, other = plan(shim, _changed(v, field))
        assert (other != key) == (field in live), (field, 'consumed' if field in live else 'not consumed')
    # the scan term's own scalars and partials are not the mix's
    for field in ['scan.w_s2m', 'scan.w_m2s', 'scan.sigma', 'scan.part']:
        assert field not in live


def test_scan_alone_among_the_vertex_terms_with_share_one_passes_through(shim):
    """scene + scan with scan == 1: no cotangent step, the scan term's own buffers go to the pull-back"""
    v = _mix(0.5, 0.0, 0.0, 1.0)
    p, key = plan(shim, v)
    want = expected(v, passes='scan')
    assert [k for k, _ in want] == [SCAN_EVAL, PULLBACK, base.SCENE_STEP, MIX_RECORD]
    assert p['steps'] == [(k, [float(x) for x in vals]) for k, vals in want]
    live = consumed(v, passes=True)
    for field, _kind in FIELDS:
        if field not in SLOT_FLAGS:
            assert (plan(shim, _changed(v, field))[1] != key) == (field in live), field
    # its neighbour mixes
    v2 = _mix(0.5, 0.0, 0.0, 2.0)
    assert plan(shim, v2)[0]['steps'] == [(k, [float(x) for x in vals]) for k, vals in expected(v2)]
    assert MIX_COTANGENT in [k for k, _ in plan(shim, v2)[0]['steps']]


@pytest.mark.parametrize('shares', [(0.5, 1.0, 0.0, 1.5), (0.5, 0.0, 1.0, 1.5), (0.0, 1.0, 0.0, 1.0), (0.0, 0.0, 1.0, 1.0)])
def test_a_share_of_one_beside_a_live_scan_share_does_not_pass_through(shim, shares):
    """the old pass-through cases (one of silhouette / vertex targets with share 1) hold only while the scan share is 0"""
    v = _mix(*shares)
    p, _ = plan(shim, v)
    assert p['steps'] == [(k, [float(x) for x in vals]) for k, vals in expected(v)]
    assert MIX_COTANGENT in [k for k, _ in p['steps']]


@pytest.mark.parametrize('name', [n for n in ROWS if n.startswith('mix')])
def test_without_a_scan_share_a_mix_plan_is_the_one_it_was(shim, name):
    """steps and sums of test_round_term_cpu.ROWS, the new step fields zero, and no scan input - the set's, the term's or the
    mix's scalars - reaches the bytes"""
    row, kind, steps, sums, _ = ROWS[name]
    v = dict(_base(), **row)
    assert v['mix.scan'] == 0.0
    p, key = plan(shim, v)
    assert p['kind'] == kind and p['sums'] == sums
    extra = {MIX_COTANGENT: 3, MIX_RECORD: 2}
    got = []
    for k, vals in p['steps']:
        n = extra.get(k, 0)
        if n:
            assert vals[-n:] == [0.0] * n, (k, vals)
            vals = vals[:-n]
        got.append((k, vals))
    assert got == [(k, [float(x) for x in vals]) for k, vals in steps]
    for field, _kind in sbase.SCAN_FIELDS + MIX_SCAN_FIELDS:
        if field not in ('scan.term', 'mix.scan'):
            assert plan(shim, _changed(v, field))[1] == key, field
    assert plan(shim, dict(v, **{'mix.scan': 1.5}))[1] != key


@pytest.mark.parametrize('name', [n for n in ROWS if not n.startswith('mix')])
def test_the_mix_scan_inputs_reach_no_other_slot(shim, name):
    row, kind, steps, sums, _ = ROWS[name]
    v = dict(_base(), **row)
    p, key = plan(shim, v)
    assert p['kind'] == kind and p['sums'] == sums
    assert [(k, vals) for k, vals in p['steps']] == [(k, [float(x) for x in vals]) for k, vals in steps]
    for field, _kind in MIX_SCAN_FIELDS:
        assert plan(shim, dict(v, **{field: 3.25}))[1] == key, field


def test_the_bytes_are_a_function_of_the_inputs(shim):
    keys = {}
    for _ in range(2):
        for s in SUBSETS:
            keys.setdefault(s, []).append(plan(shim, _subset_state(s))[1])
    for s, (a, b) in keys.items():
        assert a == b, s
    assert len(set(k[0] for k in keys.values())) == len(SUBSETS)


def test_a_round_without_the_term_has_the_empty_plan(shim):
    p, key = plan(shim, _subset_state((1, 1, 1)), live=0)
    assert p['steps'] == [] and key == bytes(len(key))
