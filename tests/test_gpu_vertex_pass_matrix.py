"""GPU: every kernel launch_vertex_pass can choose (fit_plan.cpp: plan_pass_launch), at the batch sizes where each one's chunk
mechanism first matters, on SMPL's 6890 vertices and on reduced models (tests/small_models.py) of 672, 673 and 674 vertices:
21 full tiles; an odd count whose last tile holds one vertex; a last tile of one vertex pair.

One pool of 129 parameter rows; a run takes its first B.  B = 33 / 65: a ragged chunk of one problem; 97: the third and fourth
chunk of the lock-step loop (single-buffered operands requested one chunk ahead, tau alternating by iteration parity); 129:
five chunks, the pipeline's second use of both operand buffers and a last chunk of one problem.  pass_kernel 1 runs one
workgroup per (tile, chunk) at the same sizes.  The ids carry the kernels of a cell as plan_pass_launch names them (through
the host build of the plan, tests/pass_plan.py): <single chunk>+<more chunks>.

Asserted: every vertex and keypoint of every problem against the float64 oracle (2e-6, the project's bound for the full-width
pass, tests/test_gpu_closure.py; half_basis 1e-7 < worst < 1e-4); row b the same bits at every B and pass_kernel, and with
dense_skinning on a <= 4-weights model; nothing written outside the B rows; the closure (the side outputs the step kernel
reads) against the oracle, every problem.  The row kernels' odd-length tails are at the end.

Worst |error| against the float64 oracle measured on an MI355X, over all B and every pass_kernel (the figures of pass_kernel
0, 1 and 2 are the same, as the bits are), vertices / keypoints:
  model        split_fp16            exact_fp32            half_basis
  full_dense   5.85e-07 / 5.36e-07   6.39e-07 / 4.17e-07   3.86e-05 / 1.85e-05
  full_top4    5.83e-07 / 4.18e-07   6.41e-07 / 3.72e-07   3.90e-05 / 1.87e-05     (dense_skinning: as split_fp16)
  top4_672     4.84e-07 / 4.18e-07   5.57e-07 / 3.72e-07   3.67e-05 / 1.87e-05
  top4_673     4.84e-07 / 4.18e-07   5.57e-07 / 3.72e-07   3.67e-05 / 1.87e-05     (dense_skinning: as split_fp16)
  top4_674     4.84e-07 / 4.18e-07   5.57e-07 / 3.72e-07   3.67e-05 / 1.87e-05
  dense_673    5.60e-07 / 5.36e-07   5.83e-07 / 4.17e-07   3.55e-05 / 1.85e-05
The keypoints stay inside the vertices' 2e-6, so that is their bound too.  Closures (B = 97 / 65): loss within 1.0e-7 relative,
gradient within 2.2e-7 of its largest entry."""
import functools

import numpy as np
import pytest
import torch

from mvsmplfitting_amd import _lib
from mvsmplfitting_amd import synthetic as syn
from oracle import closure_np as cn
from tests import pass_plan
from tests import term_mix_oracle as tm
from tests import vjp_helpers as vh
from tests.gpu_helpers import make_engine
from tests.helpers import body_model, oracle_for, stage_weights
from tests.small_models import sub_model
from tests.test_gpu_closure import GRAD_RTOL, LOSS_RTOL, VERT_ATOL
from tests.vertex_target_oracle import vertex_target_loss

pytestmark = pytest.mark.gpu

NPOOL = 129
BS = (1, 31, 32, 33, 64, 65, 97, 129)
VERT_BOUND = 2e-6                       # tests/test_gpu_closure.py: test_half_width_basis_operands' bound for the full-width pass
HALF_LO, HALF_HI = 1e-7, 1e-4           # the same test: really the half-width path, inside its relaxed tolerance
MODELS = {                              # name: (skin_topk, vertices or None for all 6890)
    'full_dense': (None, None), 'full_top4': (4, None), 'top4_672': (4, 672), 'top4_673': (4, 673), 'top4_674': (4, 674),
    'dense_673': (None, 673),
}
CONTRACTIONS = ('split_fp16', 'exact_fp32', 'half_basis')
# (model, contraction, dense_skinning)
ENGINES = [(m, c, 0) for m in MODELS for c in CONTRACTIONS] + [('full_top4', 'split_fp16', 1), ('top4_673', 'split_fp16', 1)]


def _nv(mname):
    return MODELS[mname][1] or 6890


def _facts(ekey):
    """(split-fp16 basis, sparse skinning rows, even vertex count) of an engine, as mvfit_create_ex derives them"""
    mname, contraction, dense = ekey
    return contraction != 'exact_fp32', MODELS[mname][0] == 4 and not dense, _nv(mname) % 2 == 0


def _kernels(ekey, pk):
    f = _facts(ekey)
    return pass_plan.short_name(*f, 32, pk), pass_plan.short_name(*f, NPOOL, pk)


def _id(ekey, pk):
    one, many = _kernels(ekey, pk)
    return '%s-%s%s-pk%d-%s+%s' % (ekey[0], ekey[1], '-dense_skinning' if ekey[2] else '', pk, one, many)


@functools.lru_cache(maxsize=None)
def model_of(mname):
    topk, nv = MODELS[mname]
    full = body_model(0, topk)
    return full if nv is None else sub_model(full, nv)


@functools.lru_cache(maxsize=None)
def pool():
    rng = np.random.default_rng(7)
    x = np.zeros((NPOOL, 118), np.float32)
    x[:, 10:82] = rng.normal(0, 0.3, (NPOOL, 72))
    x[:, 0:10] = rng.normal(0, 1.5, (NPOOL, 10))
    x[:, 82:85] = rng.normal(0, 0.5, (NPOOL, 3))
    x[:, 85] = 1.0 + rng.normal(0, 0.05, NPOOL)
    return x


@functools.lru_cache(maxsize=None)
def oracle_rows(mname):
    """float64 oracle vertices [129, nv, 3] and keypoints [129, 17, 3] of the pool, once per model"""
    orc = oracle_for(model_of(mname), None, None)
    x = pool()
    out = [orc.body(dict(cn.unpack(x[b, :86].astype(np.float64), False), use_vposer=False), want_cache=False) for b in range(NPOOL)]
    v = np.stack([o['vertices'] for o in out])
    j = np.stack([o['joints'] for o in out])
    v.setflags(write=False)
    j.setflags(write=False)
    return v, j


@pytest.fixture(scope='module')
def engines():
    made = {}

    def get(ekey):
        if ekey not in made:
            mname, contraction, dense = ekey
            made[ekey] = make_engine(model_of(mname), contraction=contraction, dense_skinning=dense)
        return made[ekey]
    yield get
    for e in made.values():
        e.close()


def _placeholder(eng, B):
    eng.set_problems(syn.make_camera_ring(1), np.zeros((B, 1, 17, 2), np.float32), np.zeros((B, 1, 17), np.float32))


def _run(eng, B, pk):
    eng.set_options(pass_kernel=pk)
    _placeholder(eng, B)
    v, j = eng.vertices(pool()[:B])
    return v.cpu().numpy(), j.cpu().numpy()


@pytest.fixture(scope='module')
def reference(engines):
    """the B = 129, pass_kernel 0 run of an engine (vertices, keypoints), once"""
    done = {}

    def get(ekey):
        if ekey not in done:
            done[ekey] = _run(engines(ekey), NPOOL, 0)
        return done[ekey]
    return get


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


CELLS = [(e, pk) for e in ENGINES for pk in (0, 1)] + [(('full_top4', 'split_fp16', 0), 2), (('full_dense', 'split_fp16', 0), 2)]


@pytest.mark.parametrize('ekey, pk', CELLS, ids=[_id(e, pk) for e, pk in CELLS])
def test_every_problem_against_the_oracle_and_the_same_bits_at_every_batch_size(engines, reference, ekey, pk):
    mname, contraction, _ = ekey
    eng = engines(ekey)
    v64, j64 = oracle_rows(mname)
    v_ref, j_ref = reference(ekey)
    f = _facts(ekey)
    worst_v = worst_j = 0.0
    for B in BS:
        # the id names this cell's kernels
        assert pass_plan.short_name(*f, B, pk) == _kernels(ekey, pk)[B > 32]
        v, j = _run(eng, B, pk)
        assert v.shape == (B, _nv(mname), 3) and np.isfinite(v).all() and np.isfinite(j).all()
        ev = np.abs(v.astype(np.float64) - v64[:B]).reshape(B, -1).max(axis=1)
        ej = np.abs(j.astype(np.float64) - j64[:B]).reshape(B, -1).max(axis=1)
        worst_v, worst_j = max(worst_v, ev.max()), max(worst_j, ej.max())
        if contraction != 'half_basis':
            assert ev.max() < VERT_BOUND, (B, int(ev.argmax()), ev.max())
            assert ej.max() < VERT_BOUND, (B, int(ej.argmax()), ej.max())
        # nothing a problem gets depends on B, on its position or on the kernel
        nbad = np.count_nonzero((_bits(v) != _bits(v_ref[:B])).reshape(B, -1).any(axis=1))
        assert nbad == 0, ('vertices of %d problems differ from the B = 129, pass_kernel 0 run' % nbad, B)
        assert np.array_equal(_bits(j), _bits(j_ref[:B])), B
    print('%s: worst |error| vertices %.3g keypoints %.3g' % (_id(ekey, pk), worst_v, worst_j))
    if contraction == 'half_basis':
        assert HALF_LO < worst_v < HALF_HI, worst_v
        assert worst_j < HALF_HI, worst_j


def test_pass_kernel_2_is_pass_kernel_0():
    for e in ENGINES:
        for B in (32, 33, NPOOL):
            assert pass_plan.pass_launch(*_facts(e), (B + 31) // 32, 2) == pass_plan.pass_launch(*_facts(e), (B + 31) // 32, 0)


@pytest.mark.parametrize('mname', ['full_top4', 'top4_673'])
def test_dense_skinning_gives_the_4_pair_blends_bits(reference, mname):
    """the same non-zero products in the same order: the dense 24-column blend on a <= 4-weights model"""
    v0, j0 = reference((mname, 'split_fp16', 0))
    v1, j1 = reference((mname, 'split_fp16', 1))
    assert _facts((mname, 'split_fp16', 0))[1] and not _facts((mname, 'split_fp16', 1))[1]
    assert np.array_equal(_bits(v0), _bits(v1)) and np.array_equal(_bits(j0), _bits(j1))


GUARD = 64
NAN_PATTERN = 0x7fc5a5a5                # a quiet NaN with a payload no computation produces


@pytest.mark.parametrize('B', [1, 33])
@pytest.mark.parametrize('contraction', ['split_fp16', 'exact_fp32'])
@pytest.mark.parametrize('mname', ['top4_673', 'dense_673', 'top4_674'])
def test_nothing_outside_the_rows_is_written(engines, mname, contraction, B):
    eng = engines((mname, contraction, 0))
    nv = _nv(mname)
    n = B * nv * 3
    x = eng._dev(pool()[:B])
    for pk in (0, 1):
        eng.set_options(pass_kernel=pk)
        _placeholder(eng, B)
        raw = torch.full((n + GUARD,), NAN_PATTERN, dtype=torch.int32, device=eng.device)
        buf = raw.view(torch.float32)
        assert buf.data_ptr() % 8 == 0
        eng._check(eng._lib.mvfit_vertices(eng._ctx, x.data_ptr(), 0, buf.data_ptr(), None))
        eng.sync()
        out = raw.cpu().numpy()
        assert np.all(out[n:] == NAN_PATTERN), (pk, np.flatnonzero(out[n:] != NAN_PATTERN)[:8])
        rows = out[:n].view(np.float32)
        assert np.isfinite(rows).all(), (pk, np.flatnonzero(~np.isfinite(rows))[:8])
        assert np.array_equal(out[:n].view(np.uint32), _bits(_run(eng, B, pk)[0]).reshape(-1))


# ---- the side outputs the step kernel reads: the closure against the oracle, every problem ----
CLOSURE_CELLS = [(('full_dense', 'split_fp16', 0), 97, 0), (('full_top4', 'split_fp16', 0), 97, 1),
                 (('top4_673', 'split_fp16', 0), 65, 0), (('dense_673', 'exact_fp32', 0), 65, 0)]


@pytest.mark.parametrize('ekey, B, pk', CLOSURE_CELLS,
                         ids=['%s-%s-B%d-pk%d-%s' % (e[0], e[1], B, pk, pass_plan.short_name(*_facts(e), B, pk)) for e, B, pk in CLOSURE_CELLS])
def test_closure_against_the_oracle(engines, ekey, B, pk):
    mname = ekey[0]
    eng = engines(ekey)
    orc = oracle_for(model_of(mname), None, None)
    V = 2
    cams = syn.make_camera_ring(V)
    rng = np.random.default_rng(19)
    gt = rng.uniform(300, 1700, (B, V, 17, 2)).astype(np.float32)
    conf = rng.uniform(0.3, 1.0, (B, V, 17)).astype(np.float32)
    x = pool()[:B]
    wts0 = stage_weights(2)
    wts = dict(wts0, flags=0)
    eng.set_options(pass_kernel=pk)
    eng.set_problems(cams, gt, conf)
    out = eng.closure(x, wts, want_verts=True)
    loss = out['loss'].cpu().numpy().astype(np.float64)
    grad = out['grad'].cpu().numpy().astype(np.float64)
    verts = out['verts'].cpu().numpy().astype(np.float64)
    ls = eng.closure(x, dict(wts, flags=_lib.F_SPARSE_VERTS))['loss'].cpu().numpy().astype(np.float64)
    v64, _ = oracle_rows(mname)
    worst = [0.0, 0.0]
    for b in range(B):
        L, g, o = orc.closure(x[b, :86].astype(np.float64), cams, gt[b], conf[b], wts0)
        worst = [max(worst[0], abs(loss[b] - L) / abs(L)), max(worst[1], np.abs(grad[b, :86] - g).max() / np.abs(g).max())]
        assert abs(loss[b] - L) <= LOSS_RTOL * abs(L), b
        assert np.abs(grad[b, :86] - g).max() <= GRAD_RTOL * np.abs(g).max(), b
        assert np.all(grad[b, 86:] == 0.0)
        assert np.abs(verts[b] - v64[b]).max() < VERT_ATOL, b
    print('closure %s B %d pk %d: worst loss rel %.3g, grad / max %.3g' % (ekey[0], B, pk, worst[0], worst[1]))
    # full-vertex mode (the loss from the pass's side outputs) and objective-vertices-only mode agree
    assert np.all(np.abs(ls - loss) <= 2e-6 * np.abs(loss))


# ---- the odd-length tails of the row kernels: n = 3 * 673 = 2019 floats per problem, B = 3 ----
NV_ODD = 673


@pytest.fixture(scope='module')
def odd_engine(engines):
    eng = engines(('top4_673', 'split_fp16', 0))
    _placeholder(eng, 3)
    return eng


def _offset(t):
    """a copy of t whose first element is at 4 mod 8 bytes"""
    flat = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    flat[1:] = t.reshape(-1)
    off = flat[1:].view(t.shape)
    assert off.data_ptr() % 8 == 4 and off.is_contiguous()
    return off


def test_term_mix_cotangent_odd_row_length(odd_engine):
    """what tests/test_gpu_term_mix.py::test_the_cotangent_kernel_against_the_oracle asserts at 6890, at an odd row length; then
    with every source and the destination at 4 mod 8"""
    eng = odd_engine
    _placeholder(eng, 3)
    rng = np.random.default_rng(29)
    gs = eng._dev(rng.standard_normal((3, NV_ODD, 3)).astype(np.float32))
    gv = eng._dev(rng.standard_normal((3, NV_ODD, 3)).astype(np.float32))
    Ls = eng._dev(rng.uniform(0.5, 50.0, 3).astype(np.float32))
    Lv = eng._dev(rng.uniform(0.5, 50.0, 3).astype(np.float32))
    for lam_s, lam_v in ((2.0, 0.25), (0.3, 0.0), (0.0, 1.7), (1.0, 1.0)):
        nan_g, nan_L = torch.full_like(gs, float('nan')), torch.full_like(Ls, float('nan'))
        a_g, a_L = (gs, Ls) if lam_s else (nan_g, nan_L)
        t_g, t_L = (gv, Lv) if lam_v else (nan_g, nan_L)
        g_ref, L_ref = tm.mix_cotangent(lam_s, gs.cpu().numpy(), Ls.cpu().numpy(), lam_v, gv.cpu().numpy(), Lv.cpu().numpy())
        g, L = eng.term_mix_cotangent(lam_s, a_g, a_L, lam_v, t_g, t_L)
        assert np.isfinite(g.cpu().numpy()).all()
        assert np.array_equal(_bits(g.cpu().numpy()), _bits(g_ref)), (lam_s, lam_v)
        assert np.array_equal(_bits(L.cpu().numpy()), _bits(L_ref)), (lam_s, lam_v)
        # bases at 4 mod 8, the floats behind the destination's last row untouched
        raw = torch.full((3 * NV_ODD * 3 + 1 + GUARD,), NAN_PATTERN, dtype=torch.int32, device=eng.device)
        g_off = raw.view(torch.float32)[1:1 + 3 * NV_ODD * 3].view(3, NV_ODD, 3)
        assert g_off.data_ptr() % 8 == 4
        L_off = torch.empty(3, device=eng.device)
        a_off, t_off = _offset(a_g), _offset(t_g)
        eng._check(eng._lib.mvfit_term_mix_cotangent(eng._ctx, lam_s, a_off.data_ptr(), a_L.data_ptr(), lam_v,
                                                     t_off.data_ptr(), t_L.data_ptr(), g_off.data_ptr(), L_off.data_ptr()))
        eng.sync()
        assert np.array_equal(_bits(g_off.cpu().numpy()), _bits(g_ref)), (lam_s, lam_v)
        assert np.array_equal(_bits(L_off.cpu().numpy()), _bits(L_ref))
        out = raw.cpu().numpy()
        assert out[0] == NAN_PATTERN and np.all(out[1 + 3 * NV_ODD * 3:] == NAN_PATTERN)
    g, L = eng.term_mix_cotangent(0.5, gs, Ls, 0.0, None, None)                # a skipped component's buffers may be absent
    assert np.array_equal(g.cpu().numpy(), np.float32(0.5) * gs.cpu().numpy())


@pytest.mark.parametrize('K', [2, 4])
def test_vertex_target_loss_odd_row_length(odd_engine, K):
    """tests/test_gpu_vertex_target.py::test_the_op_against_the_oracle at n odd: the gradient bit for bit, the loss within one
    float32 ulp of the oracle's float64 value; row 1 has all weights zero, K = 4 has NaN-filled rows of weight 0"""
    eng = odd_engine
    _placeholder(eng, 3)
    rng = np.random.default_rng(31)
    verts = rng.normal(0, 0.5, (3, NV_ODD, 3)).astype(np.float32)
    T2 = (verts[:, None] + rng.normal(0, 0.02, (3, 2, NV_ODD, 3))).astype(np.float32)
    a2 = rng.uniform(0.5, 1.5, (3, 2)).astype(np.float32)
    a2[1] = 0.0
    a2[0, 0] = 0.0
    if K == 4:
        T = np.full((3, 4, NV_ODD, 3), np.nan, np.float32)
        T[:, 0], T[:, 2] = T2[:, 0], T2[:, 1]
        a = np.zeros((3, 4), np.float32)
        a[:, 0], a[:, 2] = a2[:, 0], a2[:, 1]
    else:
        T, a = T2, a2
    L_ref, g_ref = vertex_target_loss(verts, T, a)
    eng.set_vertex_targets(T, a)
    try:
        L, g = eng.vertex_target_loss(verts)
        L_only, none = eng.vertex_target_loss(verts, need_grad=False)
        # vertices and gradient at 4 mod 8, guard floats behind the gradient's last row
        v_off = _offset(eng._dev(verts))
        raw = torch.full((verts.size + 1 + GUARD,), NAN_PATTERN, dtype=torch.int32, device=eng.device)
        g_off = raw.view(torch.float32)[1:1 + verts.size].view(3, NV_ODD, 3)
        L_off = torch.empty(3, device=eng.device)
        eng._check(eng._lib.mvfit_vertex_target_loss(eng._ctx, v_off.data_ptr(), L_off.data_ptr(), g_off.data_ptr()))
        eng.sync()
    finally:
        eng.clear_vertex_targets()
    L, g = L.cpu().numpy(), g.cpu().numpy()
    assert none is None and np.array_equal(L_only.cpu().numpy(), L)
    assert np.isfinite(L).all() and np.isfinite(g).all()
    assert np.array_equal(_bits(g), _bits(g_ref))                                    # bit for bit
    ulp = np.spacing(np.abs(L_ref).astype(np.float32)).astype(np.float64)
    err = np.abs(L.astype(np.float64) - L_ref)
    print('K %d: L %s, worst error %.3g ulp' % (K, L_ref, (err / ulp).max()))
    assert L_ref[0] > 0 and L_ref[2] > 0
    assert (err <= ulp).all()
    assert L[1] == 0.0 and not g[1].any()
    assert np.array_equal(L_off.cpu().numpy(), L) and np.array_equal(_bits(g_off.cpu().numpy()), _bits(g))
    out = raw.cpu().numpy()
    assert out[0] == NAN_PATTERN and np.all(out[1 + verts.size:] == NAN_PATTERN)


@pytest.mark.parametrize('B', [1, 33])
@pytest.mark.parametrize('mname', ['top4_673', 'dense_673'])
def test_vertices_backward_odd_vertex_count(engines, mname, B):
    """tests/test_gpu_vertices_backward.py::test_vjp_against_oracle on the 673-vertex models (the last slice of the tile kernel
    holds one vertex), every problem"""
    model = model_of(mname)
    eng = engines((mname, 'split_fp16', 0))
    _placeholder(eng, B)
    xs = vh.random_points(500 + B, B, False)
    gv, gj = vh.cotangents(600 + B, B, NV_ODD)
    x = np.stack([vh.x_to118(p, False) for p in xs]).astype(np.float32)
    got = eng.vertices_backward(x, gv, gj, 0).cpu().numpy().astype(np.float64)
    orc = vh.VjpOracle(model, None)
    for b in range(B):
        ref = vh.g_to118(orc.vjp(xs[b], gv[b], gj[b], False), False)
        err = np.abs(got[b] - ref).max()
        assert err <= GRAD_RTOL * np.abs(ref).max(), (b, err, np.abs(ref).max())
    # a second call: the same bits
    again = eng.vertices_backward(x, gv, gj, 0).cpu().numpy().astype(np.float64)
    assert np.array_equal(got, again)

