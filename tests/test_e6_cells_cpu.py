"""E6's lane cells (csrc/model_prep.cpp: HostModel::e6_cells, ModelLds::e6_cells) on the CPU.

E6 of the closure's adjoint (csrc/closure_device.h) sums g_A_j = sum_s W[s][j] [g_x v_posed^T | g_x] with sixteen lanes per
joint, lane g adding the vertices s = g, g + 16, ...  The cells list, per (joint, lane), the non-zero weights only - each as
4 s + t, the word of selw that holds it - in ascending s, padded to E6_NZ with E6_INVALID; the flag is 0 when a cell is longer
or the model's skinning is dense.  Here the shipped builder (tests/e6_cells_host_shim.cpp) against a NumPy restatement, the
flag at the length E6_NZ and one past it, and both summation orders restated in float32: the twelve row totals of every joint
must be the same words."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

from mvsmplfitting_amd import _lib, synthetic as syn
from tests import helpers
from tests.test_model_prep_cpu import model_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES = 16


@pytest.fixture(scope='module')
def shim():
    so = os.path.join(tempfile.mkdtemp(), 'libe6_cells_host.so')
    subprocess.run(['/opt/rocm/llvm/bin/clang++', '-O2', '-std=c++17', '-shared', '-fPIC', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'e6_cells_host_shim.cpp'),
                    os.path.join(ROOT, 'mvsmplfitting_amd', 'csrc', 'model_prep.cpp'), '-o', so], check=True)
    lib = C.CDLL(so)
    lib.e6_run.restype = C.c_void_p
    lib.e6_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_char_p, C.c_int]
    lib.e6_free.argtypes = [C.c_void_p]
    lib.e6_get.argtypes = [C.c_void_p] + [C.c_void_p] * 5
    lib.e6_sizes.argtypes = [C.c_void_p]
    return lib


@pytest.fixture(scope='module')
def sizes(shim):
    v = np.zeros(6, np.int32)
    shim.e6_sizes(v.ctypes.data_as(C.c_void_p))
    return dict(zip(('NJ', 'LANES', 'E6_NZ', 'E6_INVALID', 'NS_STRIDE', 'NS_MAX'), (int(x) for x in v)))


def cells_of(shim, sizes, model, dense_skinning=0):
    """the builder's tables for a model: dict(cells [NJ][16][E6_NZ], wT, selw, selj, ns, flag, sel_sparse)"""
    m, keep = model_struct(model)
    rc, err = C.c_int(0), C.create_string_buffer(512)
    h = shim.e6_run(C.byref(m), _lib.CONTRACTION_SPLIT_FP16, dense_skinning, C.byref(rc), err, 512)
    try:
        assert rc.value == 0, err.value
        NJ, NZ = sizes['NJ'], sizes['E6_NZ']
        cells = np.zeros((NJ, LANES, NZ), np.uint16)
        wT = np.zeros((NJ, sizes['NS_STRIDE']), np.float32)
        selw, selj = np.zeros((sizes['NS_MAX'], 4), np.float32), np.zeros(sizes['NS_MAX'], np.uint32)
        info = np.zeros(4, np.int32)
        shim.e6_get(h, *(a.ctypes.data_as(C.c_void_p) for a in (cells, wT, selw, selj, info)))
        assert info[3] == cells.size
        return dict(cells=cells, wT=wT, selw=selw, selj=selj, ns=int(info[0]), flag=int(info[1]), sel_sparse=int(info[2]))
    finally:
        shim.e6_free(h)


def selected(model):
    """the objective's vertices in the builder's order: the non-zero columns of the keypoint selection, ascending"""
    nv = model['v_template'].shape[0]
    hit = np.zeros(nv, bool)
    reg = model.get('kp_regressor')
    n_rows = 14 if reg is not None else 24
    for src in model['joint_map']:
        if src >= n_rows:
            hit[model['face_vertex_ids'][src - n_rows]] = True
        elif reg is not None:
            hit |= reg[src] != 0
    return np.nonzero(hit)[0]


def cell_model(n_entries):
    """the top4 body with the weights of its selected vertices replaced: vertex s = g + 16 k hangs on the joints 1 + 2 k and
    2 + 2 k (every cell of those joints has one entry), and the first n_entries vertices of lane 0 also on joint 0 - one cell
    of exactly n_entries entries, at most three non-zeros per vertex"""
    model = dict(_model('top4'))
    W = model['lbs_weights'].copy()
    sel = selected(model)
    assert len(sel) > 16 * (n_entries - 1)
    for s, v in enumerate(sel):
        k = s // 16
        W[v] = 0
        W[v, 1 + 2 * k], W[v, 2 + 2 * k] = 0.5, 0.5
        if s % 16 == 0 and k < n_entries:
            W[v, 0], W[v, 2 + 2 * k] = 0.25, 0.25
    model['lbs_weights'] = W
    return model


@functools.lru_cache(maxsize=None)
def _model(name):
    return {'top4': lambda: syn.make_body_model(0, skin_topk=4), 'dense': lambda: syn.make_body_model(0),
            'smpl': lambda: syn.make_body_model(0, model_type='smpl'),
            'smpl4': lambda: syn.make_body_model(0, skin_topk=4, model_type='smpl'), 'lsp': lambda: helpers.body_model(0, 4)}[name]()


def numpy_cells(t, sizes):
    """the restatement: per (joint, lane) the words 4 s + t of the non-zero wT[j][s], s = g, g + 16, ..., ascending"""
    NJ = sizes['NJ']
    lists = [[[] for _ in range(LANES)] for _ in range(NJ)]
    for j in range(NJ):
        for s in range(t['ns']):
            if t['wT'][j, s] != 0:
                slot = [q for q in range(4) if (int(t['selj'][s]) >> (8 * q)) & 0xff == j and t['selw'][s, q] != 0]
                assert len(slot) == 1 and t['selw'][s, slot[0]].tobytes() == t['wT'][j, s].tobytes()
                lists[j][s % LANES].append(4 * s + slot[0])
    return lists


@pytest.mark.parametrize('name,ns', [('top4', 88), ('lsp', 69), ('smpl4', 5)])
def test_cells_list_exactly_the_non_zero_weights(shim, sizes, name, ns):
    t = cells_of(shim, sizes, _model(name))
    assert t['ns'] == ns and t['sel_sparse'] == 1
    lists = numpy_cells(t, sizes)
    longest = max(len(c) for row in lists for c in row)
    hist = np.bincount([len(c) for row in lists for c in row], minlength=sizes['E6_NZ'] + 1)
    print('%s: ns %d, non-zeros %d of %d, longest cell %d, cells with 0/1/2/... entries %s'
          % (name, ns, sum(len(c) for row in lists for c in row), sizes['NJ'] * ns, longest, hist.tolist()))
    assert longest <= sizes['E6_NZ'] and t['flag'] == 1
    for j in range(sizes['NJ']):
        for g in range(LANES):
            want = lists[j][g] + [sizes['E6_INVALID']] * (sizes['E6_NZ'] - len(lists[j][g]))
            assert t['cells'][j, g].tolist() == want, (j, g)
            assert sorted(lists[j][g]) == lists[j][g]


@pytest.mark.parametrize('name,ns', [('dense', 88), ('smpl', 5)])
def test_dense_skinning_keeps_the_dense_rows(shim, sizes, name, ns):
    t = cells_of(shim, sizes, _model(name))
    assert t['ns'] == ns and t['sel_sparse'] == 0 and t['flag'] == 0
    assert (t['cells'] == sizes['E6_INVALID']).all()


def test_flag_at_the_padded_length_and_one_past_it(shim, sizes):
    NZ = sizes['E6_NZ']
    full = cells_of(shim, sizes, cell_model(NZ))
    lists = numpy_cells(full, sizes)
    assert max(len(c) for row in lists for c in row) == NZ == len(lists[0][0])
    assert full['sel_sparse'] == 1 and full['flag'] == 1
    assert full['cells'][0, 0].tolist() == lists[0][0] and full['cells'][0, 0].tolist() == [4 * 16 * k for k in range(NZ)]
    over = cells_of(shim, sizes, cell_model(NZ + 1))
    lists = numpy_cells(over, sizes)
    assert max(len(c) for row in lists for c in row) == NZ + 1 == len(lists[0][0])
    assert over['sel_sparse'] == 1 and over['flag'] == 0


def _fma(a, b, c):
    """float32 fma stand-in: the product of two float32 is exact in float64; the sum is rounded there and again to float32.
    What the comparison rests on holds for it as for the instruction: a zero product leaves a finite non-zero or +0 sum as it was."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _row_totals(t, gx, vp, use_cells, sizes):
    """E6's twelve row totals per joint, float32, in the kernel's order: per lane the entries in ascending s, then the butterfly
    of row16_sum (xor 1, xor 2, half mirror, mirror)"""
    NJ, ns = sizes['NJ'], t['ns']
    acc = np.zeros((NJ, LANES, 12), np.float32)
    flat_w = t['selw'].ravel()
    for j in range(NJ):
        for g in range(LANES):
            if use_cells:
                ent = [(np.float32(0) if e & sizes['E6_INVALID'] else flat_w[e & (sizes['E6_INVALID'] - 1)],
                        (e & (sizes['E6_INVALID'] - 1)) >> 2) for e in t['cells'][j, g].tolist()]
            else:
                ent = [(t['wT'][j, s], s) for s in range(g, ns, LANES)]
            a = acc[j, g]
            for w, s in ent:
                gw = (w * gx[s]).astype(np.float32)                     # rounded products
                for r in range(3):
                    a[3 * r:3 * r + 3] = _fma(np.repeat(gw[r], 3), vp[s], a[3 * r:3 * r + 3])
                a[9:12] = _fma(np.repeat(np.float32(w), 3), gx[s], a[9:12])
    lane = np.arange(LANES)
    for perm in (lane ^ 1, lane ^ 2, lane ^ 7, lane ^ 15):
        acc = acc + acc[:, perm]
    return acc


@pytest.mark.parametrize('name', ['top4', 'lsp', 'smpl4', 'full'])
def test_both_summation_orders_give_the_same_words(shim, sizes, name):
    t = cells_of(shim, sizes, cell_model(sizes['E6_NZ']) if name == 'full' else _model(name))
    assert t['flag'] == 1
    rng = np.random.default_rng(11)
    ns = t['ns']
    for trial in range(3):
        gx = rng.normal(0, 1, (ns, 3)).astype(np.float32)
        vp = rng.normal(0, 0.5, (ns, 3)).astype(np.float32)
        if trial >= 1:                                                   # zeros of both signs and denormal-sized g_x
            gx[rng.random((ns, 3)) < 0.3] = 0
            gx[rng.random((ns, 3)) < 0.1] = np.float32(-0.0)
            tiny = rng.random((ns, 3)) < 0.3
            gx[tiny] = (gx[tiny] * np.float32(1e-38)).astype(np.float32)
        if trial == 2:
            gx = (gx * np.float32(1e-36)).astype(np.float32)             # every sum of the phase is denormal-sized
        with np.errstate(under='ignore'):
            dense = _row_totals(t, gx, vp, False, sizes)
            cells = _row_totals(t, gx, vp, True, sizes)
        assert np.isfinite(dense).all()
        differing = int((dense.view(np.uint32) != cells.view(np.uint32)).sum())
        print('%s trial %d: %d of %d words differ, %d totals non-zero' % (name, trial, differing, dense.size, int((dense != 0).sum())))
        assert differing == 0
