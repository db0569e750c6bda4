"""The landmark term in the plan of a round's term (csrc/round_term.cpp) on the CPU: its place among the holders of the term
slot, its two launches with every pointer and scalar they take, the plan's bytes - the key of the captured round graph - and
that the lm block reaches no older slot's plan.  Built for the host from tests/round_term_landmark_host_shim.cpp, the sibling of
the scan shim that also fills the lm block.  Expected values are written out from the rules: the landmark row is
the vertex-target row with the landmark kernel in place of the target kernel."""
import ctypes as C
import itertools
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import test_round_term_cpu as base
from tests import test_round_term_scan_cpu as scan
from tests.test_round_term_cpu import MIX, PULLBACK, ROWS, SCENE, SDF, SILHOUETTE, VERTEX_TARGET
from tests.test_round_term_scan_cpu import SCAN, SCAN_EVAL

ROOT = base.ROOT
LANDMARK = 6                            # TERM_LANDMARK, appended after TERM_SCAN
LM_EVAL = 9                             # STEP_LM_EVAL, appended after STEP_SCAN_EVAL
NAMES = scan.NAMES + ['landmark']

LM_FIELDS = [('lm.on', 'B'), ('lm.term', 'B'), ('lm.tab', 'P'), ('lm.tgt', 'P'), ('lm.L', 'I'), ('lm.nt', 'I'), ('lm.has3d', 'B'),
             ('lm.rho', 'F'), ('lm.w3d', 'F'), ('lm.rho3d', 'F'), ('lm.g_verts', 'P'), ('lm.loss', 'P'), ('lm.part', 'P')]
FIELDS = scan.FIELDS + LM_FIELDS
KIND = dict(FIELDS)
SLOT_FLAGS = scan.SLOT_FLAGS + ['lm.term']
# what the landmark row's two launches consume: table and targets with their sizes, the scalars, the round buffers, the record slot
LM_LIVE = ['lm.tab', 'lm.tgt', 'lm.L', 'lm.nt', 'lm.has3d', 'lm.rho', 'lm.w3d', 'lm.rho3d', 'lm.g_verts', 'lm.loss', 'lm.part', 'sdf_adj']


def _base():
    """the scan test's base state and, behind it, a table with targets present and the term off: distinct fake addresses and
    scalars that are exact in float32"""
    v = scan._base()
    for i, (name, kind) in enumerate(LM_FIELDS):
        v[name] = {'P': 0xb00000 + 0x1000 * i, 'I': 401 + i, 'F': 30.5 + 0.125 * i, 'B': 0}[kind]
    v['lm.on'] = 1
    return v


def _zero_lm(v):
    return dict(v, **{name: 0 for name, _ in LM_FIELDS})


def _flat(v):
    assert set(v) == set(KIND), set(v) ^ set(KIND)
    return np.array([v[name] for name, _ in FIELDS], np.float64)


@pytest.fixture(scope='module')
def shim():
    so = os.path.join(tempfile.mkdtemp(), 'libround_term_landmark_host.so')
    subprocess.run(['/opt/rocm/llvm/bin/clang++', '-O2', '-std=c++17', '-shared', '-fPIC', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'round_term_landmark_host_shim.cpp'),
                    os.path.join(ROOT, 'mvsmplfitting_amd', 'csrc', 'round_term.cpp'), '-o', so], check=True)
    lib = C.CDLL(so)
    lib.round_term_slot.argtypes = [C.c_void_p]
    lib.round_term_name.argtypes = [C.c_int]
    lib.round_term_name.restype = C.c_char_p
    lib.round_term_plan.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    assert lib.round_term_num_inputs() == len(FIELDS) <= 128
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
    w = dict(v)
    w[name] = {'P': v[name] + 8, 'I': v[name] + 1, 'F': v[name] * 1.5 + 0.25, 'B': 1 - v[name]}[KIND[name]]
    return w


def _lm_state():
    # (occluders set, a target set and a scan set present: none is the landmark term's)
    return dict(_base(), **{'lm.term': 1, 'sil.occ_on': 1})


def test_the_existing_numbers_have_not_moved():
    assert (SDF, SCENE, SILHOUETTE, VERTEX_TARGET, MIX, SCAN) == (0, 1, 2, 3, 4, 5)
    assert (base.SIL_EVAL, base.VT_EVAL, base.MIX_COTANGENT, PULLBACK, base.SCENE_STEP, base.MIX_RECORD, base.SDF_STEP,
            SCAN_EVAL) == tuple(range(1, 9))


def test_the_plan_keeps_its_size(shim):
    """the step union is no larger with the landmark step in it: 6 ints, the sums' address and 7 steps of a kind word (padded)
    and the mixed cotangent's 96 bytes, as before the landmark step"""
    assert shim.round_term_key_bytes() == 4 * 6 + 8 + 7 * (8 + 96)


def test_term_slot_precedence(shim):
    """mix, vertex-target, silhouette, scan, landmark, scene, else sdf - over all 128 combinations of the occupancy facts; the
    setters allow the landmark term only alone"""
    for combo in itertools.product((0, 1), repeat=7):
        obst, silt, vt, mix, faces, sc, lm = combo
        v = dict(_base(), **{'obst.on': obst, 'silt.on': silt, 'vt.term': vt, 'mix.on': mix, 'sdf_num_faces': 100 * faces,
                             'scan.term': sc, 'lm.term': lm})
        want = (MIX if mix else VERTEX_TARGET if vt else SILHOUETTE if silt else SCAN if sc else LANDMARK if lm else
                SCENE if obst else SDF)
        got = shim.round_term_slot(_flat(v).ctypes.data)
        assert got == want, combo
        assert shim.round_term_name(got).decode() == NAMES[want]
    v = _base()
    assert shim.round_term_slot(_flat(dict(v, **{'lm.term': 1})).ctypes.data) == LANDMARK
    assert shim.round_term_slot(_flat(v).ctypes.data) == SDF            # table and targets alone hold nothing


def test_step_list(shim):
    v = _lm_state()
    p, _key = plan(shim, v)
    assert (p['kind'], p['B'], p['Bpad'], p['nv']) == (LANDMARK, v['B'], v['Bpad'], v['nv'])
    want = [(LM_EVAL, [v['lm.tab'], v['lm.tgt'], v['lm.L'], v['lm.nt'], v['lm.has3d'], v['lm.rho'], v['lm.w3d'], v['lm.rho3d'],
                       v['lm.loss'], v['lm.g_verts']]),
            (PULLBACK, [v['lm.g_verts'], v['lm.loss'], v['lm.part'], v['sdf_adj']])]
    assert [k for k, _ in p['steps']] == [LM_EVAL, PULLBACK]
    for i, ((_, got), (_, w)) in enumerate(zip(p['steps'], want)):
        assert got == [float(x) for x in w], (i, got, w)
    assert p['sums'] == (v['lm.loss'], 4)                               # L_j itself, one float per problem


def test_the_key_changes_with_what_a_live_step_consumes_and_with_nothing_else(shim):
    v = _lm_state()
    live = set(base.ALWAYS + LM_LIVE)
    assert live <= set(KIND)
    _, key = plan(shim, v)
    for field, _kind in FIELDS:
        if field in SLOT_FLAGS:
            continue
        _, other = plan(shim, _changed(v, field))
        assert (other != key) == (field in live), (field, 'consumed' if field in live else 'not consumed')


OLDER = dict({name: row[0] for name, row in ROWS.items()}, scan={'scan.term': 1, 'sil.occ_on': 1})


@pytest.mark.parametrize('name', list(OLDER))
def test_the_lm_block_reaches_no_older_slot(shim, name):
    """every older slot's plan - steps, sums and bytes - is what it is with the lm block all zeros, whatever the block holds (a
    table and targets present, the term's buffers allocated)"""
    v = dict(_base(), **OLDER[name])
    p, key = plan(shim, v)
    p0, key0 = plan(shim, _zero_lm(v))
    assert key == key0 and p == p0
    if name in ROWS:
        _, kind, steps, sums, _ = ROWS[name]
        assert p['kind'] == kind and p['sums'] == sums
        assert [(k, vals) for k, vals in p['steps']] == [(k, [float(x) for x in vals]) for k, vals in steps]
    else:
        assert p['kind'] == SCAN and [k for k, _ in p['steps']] == [SCAN_EVAL, PULLBACK]
    for field, _kind in LM_FIELDS:
        if field != 'lm.term':
            assert plan(shim, _changed(v, field))[1] == key, field


def test_the_bytes_are_a_function_of_the_inputs(shim):
    v = _lm_state()
    a = plan(shim, v)[1]
    plan(shim, dict(_base(), **ROWS['mix (+,+,+)'][0]))                 # (another plan in between: another stack history)
    assert plan(shim, v)[1] == a
    assert a not in [plan(shim, dict(_base(), **row))[1] for row in OLDER.values()]


def test_a_round_without_the_term_has_the_empty_plan(shim):
    p, key = plan(shim, _lm_state(), live=0)
    assert p['steps'] == [] and key == bytes(len(key))
