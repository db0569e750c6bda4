"""Model preparation (csrc/model_prep.cpp) on the CPU: every table mvfit_create_ex uploads, built by the shipped builder for
the host (tests/model_prep_host_shim.cpp, with ROCm's clang++: GCC before 12 has no x86 _Float16) and checked against a NumPy
restatement bit for bit, the schedules and selection lists as properties, and every argument check with its code and
message.  The C ABI path of the same checks: test_gpu_smpl_joints.py::test_joint_map_range_is_checked_in_both_modes."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

from mvsmplfitting_amd import _lib, synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NJ, NKP, KROWS, KGROUPS, TILE_V = 24, 17, 224, 28, 32
NS_MAX, NS_STRIDE, NC_MAX, KNNZ_MAX, KP_NZ, VS_NZ, VPS_SLICES = 96, 112, 288, 160, 12, 2, 8
E_ARG, E_UNSUPPORTED = -1, -4
EXACT, SPLIT, HALF = _lib.CONTRACTION_EXACT_FP32, _lib.CONTRACTION_SPLIT_FP16, _lib.CONTRACTION_HALF_BASIS


@pytest.fixture(scope='module')
def shim():
    so = os.path.join(tempfile.mkdtemp(), 'libmodel_prep_host.so')
    subprocess.run(['/opt/rocm/llvm/bin/clang++', '-O2', '-std=c++17', '-shared', '-fPIC', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'model_prep_host_shim.cpp'),
                    os.path.join(ROOT, 'mvsmplfitting_amd', 'csrc', 'model_prep.cpp'), '-o', so], check=True)
    lib = C.CDLL(so)
    lib.prep_run.restype = C.c_void_p
    lib.prep_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_char_p, C.c_int]
    lib.prep_free.argtypes = [C.c_void_p]
    lib.prep_get.restype = C.c_long
    lib.prep_get.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]
    return lib


class Prepared:
    def __init__(self, lib, h):
        self.lib, self.h = lib, h

    def __call__(self, name, dtype=np.float32, shape=None):
        n = self.lib.prep_get(self.h, name.encode(), None)
        assert n >= 0, name
        a = np.zeros(n // np.dtype(dtype).itemsize, dtype)
        self.lib.prep_get(self.h, name.encode(), a.ctypes.data_as(C.c_void_p))
        return a.reshape(shape) if shape is not None else a

    def i(self, name, shape=None):
        return self(name, np.int32, shape)

    def scalar(self, name, dtype=np.int32):
        return self(name, dtype)[0]


def model_struct(model, vposer=None, gmm=None, **override):
    """mvfit_model over the arrays (kept alive by the returned pair); override replaces arrays (None: a NULL pointer)"""
    keep = []

    def fp(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a, np.float32)
        keep.append(a)
        return a.ctypes.data_as(C.POINTER(C.c_float))

    def ip(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a, np.int32)
        keep.append(a)
        return a.ctypes.data_as(C.POINTER(C.c_int32))
    arr = dict(model, **override)
    m = _lib.Model()
    m.num_verts = arr['v_template'].shape[0]
    m.num_faces = arr['faces'].shape[0] if arr.get('faces') is not None else 0
    for k in ('v_template', 'shapedirs', 'posedirs', 'J_regressor', 'lbs_weights', 'kp_regressor'):
        setattr(m, k, fp(arr.get(k)))
    for k in ('parents', 'face_vertex_ids', 'joint_map', 'faces'):
        setattr(m, k, ip(arr.get(k)))
    if vposer is not None:
        for k in ('fc1_w', 'fc1_b', 'fc2_w', 'fc2_b', 'out_w', 'out_b'):
            setattr(m, 'vp_' + k, fp(vposer.get(k)))
    if gmm is not None:
        m.gmm_M = gmm[0].shape[0]
        m.gmm_means, m.gmm_precisions, m.gmm_nll_weights = fp(gmm[0]), fp(gmm[1]), fp(gmm[2])
    return m, keep


def prepare(lib, model, contraction=SPLIT, dense_skinning=0, vposer=None, gmm=None, **override):
    m, keep = model_struct(model, vposer, gmm, **override)
    rc, err = C.c_int(0), C.create_string_buffer(512)
    h = lib.prep_run(C.byref(m), contraction, dense_skinning, C.byref(rc), err, 512)
    return rc.value, err.value.decode(), h


@pytest.fixture
def prepared(shim):
    made = []

    def run(*a, **kw):
        rc, err, h = prepare(shim, *a, **kw)
        made.append(h)
        assert rc == 0, err
        return Prepared(shim, h)
    yield run
    for h in made:
        shim.prep_free(h)


@functools.lru_cache(maxsize=None)
def _model(name):
    return {'dense': lambda: syn.make_body_model(0), 'top4': lambda: syn.make_body_model(0, skin_topk=4),
            'smpl': lambda: syn.make_body_model(0, model_type='smpl')}[name]()


@functools.lru_cache(maxsize=1)
def _vposer():
    return syn.make_vposer_decoder()


@functools.lru_cache(maxsize=1)
def _gmm():
    return syn.gmm_constants(syn.make_gmm())


@functools.lru_cache(maxsize=None)
def _basis(name):
    """[KROWS][nv_pad][3]: rows 0..206 posedirs, 207..216 shapedirs (beta index), zero rows and vertices past the model"""
    mdl = _model(name)
    nv = mdl['v_template'].shape[0]
    nv_pad = -(-nv // TILE_V) * TILE_V
    b = np.zeros((KROWS, nv_pad, 3), np.float32)
    b[:207, :nv] = mdl['posedirs'].reshape(207, nv, 3)
    b[207:217, :nv] = mdl['shapedirs'].transpose(2, 0, 1)
    return b


def _selection(mdl):
    """dense 17 x nv keypoint selection (float64 like the builder's) and the skeleton joint of each keypoint (-1: a row)"""
    nv = mdl['v_template'].shape[0]
    reg = mdl.get('kp_regressor')
    n_rows = 14 if reg is not None else NJ
    ksel, joint = np.zeros((NKP, nv)), np.full(NKP, -1)
    for k, src in enumerate(mdl['joint_map']):
        if src < n_rows:
            if reg is None:
                joint[k] = src
            else:
                ksel[k] = reg[src]
        else:
            ksel[k, mdl['face_vertex_ids'][src - n_rows]] = 1.0
    return ksel, joint


def _bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


CASES = [('dense', SPLIT, 0, True), ('dense', EXACT, 0, False), ('dense', HALF, 1, False), ('top4', SPLIT, 0, True),
         ('top4', EXACT, 1, True), ('top4', HALF, 0, False), ('smpl', SPLIT, 1, False), ('smpl', HALF, 0, True)]


@pytest.mark.parametrize('name,contraction,dense,extras', CASES, ids=['%s-c%d-d%d-%s' % (c[0], c[1], c[2], 'vg' if c[3] else 'plain')
                                                                    for c in CASES])
def test_tables_equal_the_numpy_restatement(prepared, name, contraction, dense, extras):
    mdl = _model(name)
    P = prepared(mdl, contraction, dense, vposer=_vposer() if extras else None, gmm=_gmm() if extras else None)
    nv = mdl['v_template'].shape[0]
    nt = -(-nv // TILE_V)
    nv_pad = nt * TILE_V
    assert (P.scalar('nv'), P.scalar('ntiles'), P.scalar('nv_pad')) == (nv, nt, nv_pad)
    basis = _basis(name)
    # bs4 [ntiles][3][KGROUPS][64][4]: row 2 (4 g + q) + (l >> 5), vertex 32 T + (l & 31)
    T, k, g, l, q = np.ix_(np.arange(nt), np.arange(3), np.arange(KGROUPS), np.arange(64), np.arange(4))
    bs4 = basis[2 * (4 * g + q) + (l >> 5), TILE_V * T + (l & 31), k]
    assert _bits_equal(P('bs4', shape=bs4.shape), bs4)
    # split fp16 basis [ntiles][3][14][hi, lo][64][8]: row 16 G + 8 (l >> 5) + t
    assert P.scalar('half_basis') == int(contraction == HALF)
    scale = P.scalar('bs_scale', np.float32)
    if contraction == EXACT:
        assert P('bs_h2', np.float16).size == 0 and scale == 1.0
    else:
        mx = np.abs(bs4).max()
        assert np.frexp(scale)[0] == 0.5 and 2.0 ** 13 <= mx * scale < 2.0 ** 14
        T, k, G, l, t = np.ix_(np.arange(nt), np.arange(3), np.arange(KROWS // 16), np.arange(64), np.arange(8))
        x = basis[16 * G + 8 * (l >> 5) + t, TILE_V * T + (l & 31), k] * scale
        hi = x.astype(np.float16)
        lo = (x - hi.astype(np.float32)).astype(np.float16)
        assert _bits_equal(P('bs_h2', np.float16, (nt, 3, KROWS // 16, 2, 64, 8)), np.stack([hi, lo], axis=3))
    assert _bits_equal(P('bs_vm', shape=(nv, 3, KROWS)), np.ascontiguousarray(basis[:, :nv].transpose(1, 2, 0)))
    # rest pose and skinning
    W = mdl['lbs_weights']
    vt = np.zeros((3, nv_pad), np.float32)
    vt[:, :nv] = mdl['v_template'].T
    assert _bits_equal(P('vt_planes', shape=(3, nv_pad)), vt)
    Wp = np.zeros((nv_pad, NJ), np.float32)
    Wp[:nv] = W
    assert _bits_equal(P('wt_tiles', shape=(nt, NJ, TILE_V)), np.ascontiguousarray(Wp.reshape(nt, TILE_V, NJ).transpose(0, 2, 1)))
    assert _bits_equal(P('w_vm', shape=(nv, NJ)), W)
    if dense or ((W != 0).sum(1) > 4).any():
        assert P('wsp_w').size == 0 and P.i('wsp_j').size == 0
    else:
        sw, sj = np.zeros((nv_pad, 4), np.float32), np.zeros((nv_pad, 4), np.int32)
        for v in range(nv):
            js = np.nonzero(W[v])[0]                       # ascending joints
            sw[v, :len(js)], sj[v, :len(js)] = W[v, js], js
        assert _bits_equal(P('wsp_w', shape=(nv_pad, 4)), sw) and _bits_equal(P.i('wsp_j', (nv_pad, 4)), sj)
    # selected vertices: non-zero columns of the 17 x nv selection
    ksel, kjoint = _selection(mdl)
    sel = np.nonzero((ksel != 0).any(0))[0].astype(np.int32)
    ns = len(sel)
    nc, nc_pad = 3 * ns, (3 * ns + 3) // 4 * 4
    assert (P.scalar('ns'), P.scalar('nc'), P.scalar('nc_pad')) == (ns, nc, nc_pad)
    assert (P.scalar('lds.ns'), P.scalar('lds.nc'), P.scalar('lds.nc_pad')) == (ns, nc, nc_pad)
    assert _bits_equal(P.i('sel_v'), sel)
    lsel = np.zeros(NS_MAX, np.int32)
    lsel[:ns] = sel
    assert _bits_equal(P.i('lds.sel_v'), lsel)
    vt_sub = np.zeros(NC_MAX, np.float32)
    vt_sub[:nc] = mdl['v_template'][sel].ravel()
    assert _bits_equal(P('lds.vt_sub'), vt_sub)
    pd = np.zeros((KROWS, nc_pad), np.float32)
    pd[:, :nc] = basis[:, sel].reshape(KROWS, nc)
    assert _bits_equal(P('pd_sub', shape=(KROWS, nc_pad)), pd)
    assert _bits_equal(P('pd_subT', shape=(nc_pad, KROWS)), np.ascontiguousarray(pd.T))
    wT = np.zeros((NJ, NS_STRIDE), np.float32)
    wT[:, :ns] = W[sel].T
    assert _bits_equal(P('lds.wT', shape=(NJ, NS_STRIDE)), wT)
    selw, selj = np.zeros((NS_MAX, 4), np.float32), np.zeros(NS_MAX, np.uint32)
    for s, v in enumerate(sel):
        js = np.nonzero(W[v])[0][:4]
        selw[s, :len(js)] = W[v, js]
        selj[s] = sum(int(j) << (8 * t) for t, j in enumerate(js))
    assert _bits_equal(P('lds.selw', shape=(NS_MAX, 4)), selw)
    assert _bits_equal(P('lds.selj', np.uint32), selj)
    assert P.scalar('lds.sel_sparse') == int(((W[sel] != 0).sum(1) <= 4).all())
    # keypoint sources (5 bits each, 31 = a selection row) and the selection CSRs / padded lists
    kj = np.full(3, 0x3fffffff, np.uint32)                   # six slots per word, all 31 (the last word has five keypoints)
    for k in np.nonzero(kjoint >= 0)[0]:
        kj[k // 6] = (kj[k // 6] & ~np.uint32(31 << (5 * (k % 6)))) | np.uint32(kjoint[k] << (5 * (k % 6)))
    assert _bits_equal(P('lds.kp_joint', np.uint32), kj) and P.scalar('lds.n_skel') == (kjoint >= 0).sum()
    dense_sel = ksel[:, sel].astype(np.float32)              # [17][ns]
    kp_start, kp_s, kp_w = P.i('lds.kp_start'), P.i('lds.kp_s'), P('lds.kp_w')
    vs_start, vs_k, vs_w = P.i('lds.vs_start'), P.i('lds.vs_k'), P('lds.vs_w')
    nnz = int((dense_sel != 0).sum())
    assert kp_start[NKP] == nnz and (vs_start[ns:] == nnz).all()
    ks, ss = np.nonzero(dense_sel)                           # keypoint-major, ascending s
    assert _bits_equal(kp_start, np.searchsorted(ks, np.arange(NKP + 1)).astype(np.int32))
    assert _bits_equal(kp_s[:nnz], ss.astype(np.int32)) and _bits_equal(kp_w[:nnz], dense_sel[ks, ss])
    ss2, ks2 = np.nonzero(dense_sel.T)                       # vertex-major, ascending k
    assert _bits_equal(vs_start[:ns + 1], np.searchsorted(ss2, np.arange(ns + 1)).astype(np.int32))
    assert _bits_equal(vs_k[:nnz], ks2.astype(np.int32)) and _bits_equal(vs_w[:nnz], dense_sel.T[ss2, ks2])
    kpp_s, kpp_w = P.i('lds.kpp_s', (NKP, KP_NZ)), P('lds.kpp_w', shape=(NKP, KP_NZ))
    vsp_k, vsp_w = P.i('lds.vsp_k', (NS_MAX, VS_NZ)), P('lds.vsp_w', shape=(NS_MAX, VS_NZ))
    padded = int(np.diff(kp_start).max() <= KP_NZ and np.diff(vs_start).max() <= VS_NZ)
    assert P.scalar('lds.padded') == padded
    # property: each form reproduces the dense selection
    for rebuild in ('kp', 'vs', 'kpp', 'vsp'):
        R = np.zeros((NKP, ns), np.float32)
        for k in range(NKP):
            if rebuild == 'kp':
                R[k, kp_s[kp_start[k]:kp_start[k + 1]]] = kp_w[kp_start[k]:kp_start[k + 1]]
            elif rebuild == 'kpp' and padded:
                np.add.at(R[k], kpp_s[k], kpp_w[k])
        for s in range(ns):
            if rebuild == 'vs':
                R[vs_k[vs_start[s]:vs_start[s + 1]], s] = vs_w[vs_start[s]:vs_start[s + 1]]
            elif rebuild == 'vsp' and padded:
                np.add.at(R[:, s], vsp_k[s], vsp_w[s])
        if rebuild in ('kp', 'vs') or padded:
            assert _bits_equal(R, dense_sel), rebuild
    # tile lists: ascending s within each tile; together they partition the selection
    tstart, tlocal, tslot = P.i('tile_sel_start'), P.i('tile_sel_local'), P.i('tile_sel_slot')
    order = np.argsort(sel // TILE_V, kind='stable')
    assert _bits_equal(tstart, np.searchsorted(sel[order] // TILE_V, np.arange(nt + 1)).astype(np.int32))
    assert _bits_equal(tslot, order.astype(np.int32)) and _bits_equal(tlocal, sel[order] % TILE_V)
    assert sorted(tslot) == list(range(ns))
    for T in range(nt):
        assert (sel[tslot[tstart[T]:tstart[T + 1]]] // TILE_V == T).all()
    # joints as an affine function of beta: sequential float64 sums over the regressor's non-zeros
    J = mdl['J_regressor']
    J_t, J_S = np.zeros(NJ * 3, np.float32), np.zeros((NJ * 3, 11), np.float32)
    for j in range(NJ):
        vs = np.nonzero(J[j])[0]
        w = J[j, vs].astype(np.float64)
        for a in range(3):
            J_t[3 * j + a] = np.cumsum(w * mdl['v_template'][vs, a].astype(np.float64))[-1]
            J_S[3 * j + a, :10] = np.cumsum(w[:, None] * mdl['shapedirs'][vs, a].astype(np.float64), axis=0)[-1]
    assert _bits_equal(P('lds.J_t'), J_t) and _bits_equal(P('lds.J_S', shape=(NJ * 3, 11)), J_S)
    # VPoser decoder
    assert P.scalar('has_vposer', np.uint8) == int(extras)
    if extras:
        vp = _vposer()
        w1, w2, w3 = vp['fc1_w'], vp['fc2_w'], vp['out_w']
        for nm, want in (('vp_w1', w1), ('vp_b1', vp['fc1_b']), ('vp_w2', w2), ('vp_b2', vp['fc2_b']), ('vp_w3', w3),
                         ('vp_b3', vp['out_b']), ('vp_w1T', w1.T), ('vp_w2T', w2.T), ('vp_w3T', np.pad(w3.T, ((0, 0), (0, 6))))):
            assert _bits_equal(P(nm, shape=want.shape), np.ascontiguousarray(want)), nm
        h, j, tid, q = np.ix_(np.arange(VPS_SLICES), np.arange(16), np.arange(512), np.arange(4))
        tw2 = w2[64 * h + 8 * (tid >> 6) + (j >> 1), 8 * (tid & 63) + 4 * (j & 1) + q]
        assert _bits_equal(P('vp_tw2', shape=tw2.shape), tw2)
        h, j, tid, q = np.ix_(np.arange(VPS_SLICES), np.arange(6), np.arange(512), np.arange(4))
        o = (tid & 63) + 64 * (j >> 1)
        tw3 = np.where(o < 138, np.pad(w3, ((0, 54), (0, 0)))[o, 64 * h + 8 * (tid >> 6) + 4 * (j & 1) + q], np.float32(0))
        assert _bits_equal(P('vp_tw3', shape=tw3.shape), tw3)
    else:
        assert all(P(nm).size == 0 for nm in ('vp_w1', 'vp_w2T', 'vp_tw2', 'vp_tw3'))
    # max-mixture prior
    if extras:
        means, prec, nllw = _gmm()
        M = means.shape[0]
        assert P.scalar('gmm_M') == M
        pad = np.zeros((M, 69, 72), np.float32)
        pad[:, :, :69] = prec
        padT = np.zeros((M, 69, 72), np.float32)
        padT[:, :, :69] = prec.transpose(0, 2, 1)
        assert _bits_equal(P('gmm_means', shape=means.shape), means)
        assert _bits_equal(P('gmm_prec', shape=pad.shape), pad) and _bits_equal(P('gmm_precT', shape=padT.shape), padT)
        # logf: correctly rounded on these weights (the float64 log rounded once)
        assert _bits_equal(P('gmm_lognw'), np.log(nllw.astype(np.float64)).astype(np.float32))
    else:
        assert P.scalar('gmm_M') == 0 and P('gmm_means').size == 0
    # faces and the vertex -> face CSR (ascending face id per vertex)
    faces = mdl['faces'].astype(np.int32)
    assert P.scalar('num_faces') == len(faces) and _bits_equal(P.i('faces', faces.shape), faces)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(faces.ravel(), minlength=nv))]).astype(np.int32)
    assert _bits_equal(P.i('vf_ptr'), ptr)
    assert _bits_equal(P.i('vf_idx'), (np.argsort(faces.ravel(), kind='stable') // 3).astype(np.int32))


def _depths(parents):
    d = np.zeros(NJ, int)
    for j in range(1, NJ):
        d[j] = d[parents[j]] + 1
    return d


TREES = {'smpl': syn.SMPL_PARENTS, 'chain': np.arange(NJ) - 1, 'star': np.r_[-1, np.zeros(NJ - 1)],
         'binary': np.r_[-1, (np.arange(1, NJ) - 1) // 2], 'broom': np.r_[-1, np.arange(0, 11), np.full(12, 11)]}


@pytest.mark.parametrize('tree', sorted(TREES))
def test_chain_schedules(prepared, tree):
    parents = np.asarray(TREES[tree], np.int32)
    P = prepared(_model('top4'), EXACT, 0, parents=parents)
    depth = _depths(parents)
    children = [[j for j in range(1, NJ) if parents[j] == p] for p in range(NJ)]
    assert _bits_equal(P.i('lds.parents'), parents) and P.scalar('lds.nlevels') == depth.max() + 1
    level_joints = np.argsort(depth, kind='stable').astype(np.int32)
    starts = np.searchsorted(depth[level_joints], np.arange(NJ + 1)).astype(np.int32)
    assert _bits_equal(P.i('lds.level_joints'), level_joints) and _bits_equal(P.i('lds.level_start'), starts)
    assert _bits_equal(P.i('lds.child_list'), np.asarray(sum(children, []) + [0], np.int32))      # 23 edges in 24 slots
    assert _bits_equal(P.i('lds.child_start'), np.cumsum([0] + [len(c) for c in children]).astype(np.int32))
    # forward: every non-root joint once, in a pass after its parent's
    fwd, n_fwd = P.i('lds.fwd_tab', (NJ, 5)), P.scalar('lds.n_fwd')
    assert (fwd[n_fwd:] == -1).all()
    seen = {0: -1}
    for ps in range(n_fwd):
        for e in fwd[ps][fwd[ps] >= 0]:
            j, p = int(e) & 0xff, int(e) >> 8
            assert p == parents[j] and j not in seen and seen[p] < ps
            seen[j] = ps
    assert sorted(seen) == list(range(NJ))
    # adjoint: every parent -> child edge once; <= 3 children per entry, a parent at most once per pass, deepest first
    bwd, n_bwd = P.i('lds.bwd_tab', (NJ, 5)), P.scalar('lds.n_bwd')
    assert (bwd[n_bwd:] == -1).all()
    edges, last_depth = [], np.inf
    for ps in range(n_bwd):
        ents = bwd[ps][bwd[ps] != -1]
        assert len(ents) > 0
        ps_parents = [int(e) & 0x1f for e in ents]
        assert len(set(ps_parents)) == len(ps_parents)
        for e in ents:
            e = int(e) & 0xffffffff
            p = e & 0x1f
            ch = [c for c in ((e >> 8) & 0xff, (e >> 16) & 0xff, (e >> 24) & 0xff) if c != 31]
            assert 1 <= len(ch) <= 3 and bool(e & 0x80) == any(q == p for q, _ in edges)
            assert depth[p] <= last_depth
            last_depth = depth[p]
            edges += [(p, c) for c in ch]
    assert sorted(edges) == sorted((int(parents[j]), j) for j in range(1, NJ))
    # pointer jumping: 2^s-th ancestors, the fewest steps that cover the longest path
    anc, n_jump = P.i('lds.anc_tab', (5, NJ)), P.scalar('lds.n_jump')
    for s in range(5):
        for j in range(NJ):
            a = j
            for _ in range(2 ** s):
                a = parents[a] if a >= 0 else -1
            assert anc[s, j] == a
    L = depth.max() + 1
    assert 2 ** n_jump >= L and (n_jump == 0 or 2 ** (n_jump - 1) < L)


def _err(shim, *a, **kw):
    rc, err, h = prepare(shim, *a, **kw)
    shim.prep_free(h)
    return rc, err


def test_argument_checks_keep_their_codes_and_messages(shim):
    base, smpl = _model('top4'), _model('smpl')
    p = base['parents'].copy()
    p[0] = 0
    assert _err(shim, base, parents=p) == (E_ARG, 'parents[0] must be -1')
    p = base['parents'].copy()
    p[5] = 7
    assert _err(shim, base, parents=p) == (E_ARG, 'parents must be topologically ordered')
    jm = base['joint_map'].copy()
    jm[3] = 19
    assert _err(shim, base, joint_map=jm) == (E_ARG, 'joint_map entry 19 out of range (0..18)')
    jm = smpl['joint_map'].copy()
    jm[2] = 29
    assert _err(shim, smpl, joint_map=jm) == (E_ARG, 'joint_map entry 29 out of range (0..28)')
    jm[2] = -1
    assert _err(shim, smpl, joint_map=jm) == (E_ARG, 'joint_map entry -1 out of range (0..28)')
    fv = base['face_vertex_ids'].copy()
    fv[1] = base['v_template'].shape[0]
    assert _err(shim, base, face_vertex_ids=fv) == (E_ARG, 'face vertex id out of range')
    assert _err(shim, smpl, joint_map=np.arange(NKP) % NJ) == (
        E_UNSUPPORTED, 'the keypoints read no vertex (joint_map names no face vertex)')
    kr = np.zeros_like(base['kp_regressor'])
    kr[:, :120] = 0.1
    assert _err(shim, base, kp_regressor=kr) == (E_UNSUPPORTED, 'keypoint regressor touches 125 vertices (max 96)')
    kr = np.zeros_like(base['kp_regressor'])
    for r in range(14):
        kr[r, 6 * r:6 * r + 14] = 0.1
    assert _err(shim, base, kp_regressor=kr) == (E_UNSUPPORTED, 'keypoint selection has more than 160 non-zeros')
    vp = dict(_vposer(), fc2_b=None)
    assert _err(shim, base, vposer=vp) == (E_ARG, 'incomplete vposer weights')
    assert _err(shim, base, gmm=syn.gmm_constants(syn.make_gmm(num_gaussians=9))) == (E_ARG, 'gmm: M <= 8 and all arrays required')
    means, prec, nllw = _gmm()
    assert _err(shim, base, gmm=(means, None, nllw)) == (E_ARG, 'gmm: M <= 8 and all arrays required')
    # first failing check wins: topological order is checked after the selection
    jm = base['joint_map'].copy()
    jm[0] = 40
    p = base['parents'].copy()
    p[5] = 7
    assert _err(shim, base, joint_map=jm, parents=p)[1] == 'joint_map entry 40 out of range (0..18)'
    # the chain-pass limits (24 forward / adjoint passes, 32 levels) cannot be reached with 24 joints: the extreme trees
    # of test_chain_schedules (a 24-joint chain, a star) pass them


def test_invalid_faces_are_dropped_silently(prepared):
    base = _model('top4')
    f = base['faces'].copy()
    f[10, 1] = base['v_template'].shape[0]
    for P in (prepared(base, faces=f), prepared(base, faces=None)):
        assert P.scalar('num_faces') == 0 and P.i('faces').size == 0 and P.i('vf_ptr').size == 0
