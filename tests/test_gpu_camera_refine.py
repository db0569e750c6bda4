"""GPU: mvfit_camera_normal_eqs and mvfit_refine_cameras against their NumPy restatement (tests/camera_refine_oracle.py) - the
sums, the Levenberg-Marquardt runs decision for decision, the known answer -, independence of the other views, the skips and
bounds, the error codes.  No body model is involved: the joints are random points."""
import ctypes as C

import numpy as np
import pytest
import torch

from mvsmplfitting_amd import _lib
from mvsmplfitting_amd.engine import MvFit, MvFitError, pack_cameras, unpack_cameras
from tests import camera_refine_oracle as co
from tests.helpers import body_model
from tests.test_camera_refine_cpu import LM_CASES, LM_FTOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    with MvFit(body_model()) as e:
        yield e


def _set(eng, cams15, gt, w):
    eng.set_problems(unpack_cameras(cams15, np.float32), gt, w)


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a).view(np.uint64)


@pytest.fixture(scope='module')
def wide():
    """(31, 16): the maximum number of views and an odd point count; view 3 has every weight 0, view 7 lies behind."""
    joints, gt, w, true, start = co.make_case(31, 16, seed=5, noise=20.0)
    w[:, 3] = 0.0
    gt[:, 3] = np.nan
    start[7, 11] -= 10.0
    return joints, gt, w, true, start


def _check_normal_eqs(eng, joints, gt, w, cams, rho, dw):
    _set(eng, cams, gt, w)
    got = {k: v.cpu().numpy() for k, v in eng.camera_normal_eqs(joints, cams, rho=rho, data_weight=dw).items()}
    assert got['E'].dtype == np.float64 and got['H'].shape == (cams.shape[0], 9, 9) and got['count'].dtype == np.int32
    for v in range(cams.shape[0]):
        E, g, H, count = co.normal_eqs(joints, gt[:, v], w[:, v], cams[v], np.float32(rho), np.float32(dw))
        assert got['count'][v] == count
        if E == np.inf:
            assert got['E'][v] == np.inf
            continue
        for name, a, b in (('E', got['E'][v], E), ('g', got['g'][v], g), ('H', got['H'][v], H)):
            err, scale = np.abs(a - b).max(), np.abs(b).max()
            print('view %d %s: max |device - oracle| = %.3e, max |oracle| = %.3e' % (v, name, err, scale))
            assert err <= 1e-10 * scale
        assert np.array_equal(got['H'][v], got['H'][v].T)
    return got


@pytest.mark.parametrize('B,V', [(1, 1), (16, 3)])
def test_normal_eqs_against_oracle(eng, B, V):
    """(1, 1): 17 points, most lanes idle; (16, 3): 272 points, a second ragged pass of 16.  Both sides are float64 sums of at
    most 527 terms: rounding is about 1e-13 of the absolute sum, a wrong Jacobian entry is wrong by O(1); bound 1e-10 of the
    largest entry per view and array."""
    joints, gt, w, true, start = co.make_case(B, V, seed=4, noise=20.0)
    _check_normal_eqs(eng, joints, gt, w, start, 100.0, 1.0)


def test_normal_eqs_wide_with_an_empty_view_and_one_behind(eng, wide):
    joints, gt, w, true, start = wide
    got = _check_normal_eqs(eng, joints, gt, w, start, 70.0, 0.325)
    assert got['count'][3] == 0 and got['E'][3] == 0.0 and not got['g'][3].any() and not got['H'][3].any()
    assert got['E'][7] == np.inf and got['count'][7] > 0
    only_E = eng.camera_normal_eqs(joints, start, rho=70.0, data_weight=0.325, need_grad=False)
    assert 'g' not in only_E and np.array_equal(_bits(only_E['E']), _bits(got['E']))


def test_a_view_does_not_depend_on_the_others(eng, wide):
    """A view's E, g, H, cams_out and report carry the same bits when the call holds that view alone and among 16."""
    joints, gt, w, true, start = wide
    _set(eng, start, gt, w)
    all_ = eng.camera_normal_eqs(joints, start)
    cams_all, rep_all = eng.refine_cameras(joints, start, free='all')
    for v in (0, 7, 12):
        _set(eng, start[v:v + 1], gt[:, v:v + 1], w[:, v:v + 1])
        one = eng.camera_normal_eqs(joints, start[v:v + 1])
        for k in ('E', 'g', 'H'):
            assert np.array_equal(_bits(one[k][0]), _bits(all_[k][v])), (v, k)
        assert int(one['count'][0]) == int(all_['count'][v])
        cams_one, rep_one = eng.refine_cameras(joints, start[v:v + 1], free='all')
        assert np.array_equal(_bits(cams_one[0]), _bits(cams_all[v])) and np.array_equal(_bits(rep_one[0]), _bits(rep_all[v]))
    assert rep_all[7, 4] == 5 and rep_all[3, 4] == 4


@pytest.mark.parametrize('B,V,seed,noise', LM_CASES)
@pytest.mark.parametrize('free', ['extrinsics', 'all'])
def test_refine_against_oracle_lm(eng, B, V, seed, noise, free):
    """Noisy cases whose accept / reject decisions are all clear (tests/test_camera_refine_cpu.py checks that none is closer
    than 1e-6 relative): it, acc and status equal the oracle's; E1 and the camera within 100 times the oracle's own spread
    between ascending and descending summation of the points on the same case (the device sums in a third order; 100 covers
    that a spread of two orders underestimates the rounding of either), with a floor of 1e-12 of the array's largest entry."""
    joints, gt, w, true, start = co.make_case(B, V, seed, noise=noise)
    _set(eng, start, gt, w)
    cams, rep = eng.refine_cameras(joints, start, free=free, ftol=LM_FTOL)
    cams, rep = cams.cpu().numpy(), rep.cpu().numpy()
    for v in range(V):
        a, ra = co.lm(joints, gt[:, v], w[:, v], start[v], free_mask=co.FREE[free], ftol=LM_FTOL)
        b, rb = co.lm(joints, gt[:, v], w[:, v], start[v], free_mask=co.FREE[free], ftol=LM_FTOL, reverse=True)
        assert (rep[v, 2], rep[v, 3], rep[v, 4], rep[v, 5]) == (ra[2], ra[3], ra[4], ra[5]), (v, rep[v], ra)
        assert rep[v, 0] == pytest.approx(ra[0], rel=1e-10)
        for name, got, fw, rv in (('E1', rep[v, 1:2], ra[1:2], rb[1:2]), ('R', cams[v, :9], a[:9], b[:9]),
                                  ('t', cams[v, 9:12], a[9:12], b[9:12]), ('f, c', cams[v, 12:], a[12:], b[12:])):
            spread, err, scale = np.abs(fw - rv).max(), np.abs(got - fw).max(), np.abs(fw).max()
            print('view %d %s: oracle spread %.3e, |device - oracle| %.3e, scale %.3e' % (v, name, spread, err, scale))
            assert err <= max(100.0 * spread, 1e-12 * scale)
        assert rep[v, 1] < rep[v, 0] and rep[v, 7] == 0.0


@pytest.mark.parametrize('free', ['extrinsics', 'extrinsics+focal', 'all'])
def test_known_answer(eng, free):
    """Exact float32 pixels, a start 2.5 degrees and 7 cm off: the rotation angle and |t - t_true| end within 10 times the
    oracle's own recovery error on the same inputs."""
    joints, gt, w, true, start = co.make_case(16, 3, seed=1)
    _set(eng, start, gt, w)
    cams, rep = eng.refine_cameras(joints, start, free=free)
    cams, rep = cams.cpu().numpy(), rep.cpu().numpy()
    for v in range(3):
        a, ra = co.lm(joints, gt[:, v], w[:, v], start[v], free_mask=co.FREE[free])
        ang_o, dt_o = co.rot_angle(a[:9], true[v, :9]), np.linalg.norm(a[9:12] - true[v, 9:12])
        ang_d, dt_d = co.rot_angle(cams[v, :9], true[v, :9]), np.linalg.norm(cams[v, 9:12] - true[v, 9:12])
        print('view %d free %s: angle device %.3e oracle %.3e rad, |t - t_true| device %.3e oracle %.3e m, it %d / %d'
              % (v, free, ang_d, ang_o, dt_d, dt_o, rep[v, 2], ra[2]))
        assert ang_d <= 10 * ang_o and dt_d <= 10 * dt_o
        assert rep[v, 4] in (0, 2) and rep[v, 1] < 1e-4 < rep[v, 0]
        R = cams[v, :9].reshape(3, 3)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14


def test_skips_and_bounds(eng):
    joints, gt, w, true, start = co.make_case(16, 3, seed=1)
    few = w[:, 2].copy()
    few.reshape(-1)[20:] = 0.0                                           # view 2: 20 points or fewer
    w[:, 2] = few
    _set(eng, start, gt, w)
    cams, rep = eng.refine_cameras(joints, start, fixed_views=(0,), min_points=34)
    assert rep[0, 4] == 3 and rep[1, 4] in (0, 2) and rep[2, 4] == 4
    assert rep[0, 2] == 0 and rep[0, 0] == rep[0, 1] and rep[2, 5] == float((w[:, 2] != 0).sum())
    for v in (0, 2):
        assert np.array_equal(_bits(cams[v]), start[v].view(np.uint64))
    assert not np.array_equal(_bits(cams[1]), start[1].view(np.uint64))
    c1, r1 = eng.refine_cameras(joints, start, max_iter=1, min_points=1)
    assert (r1[:, 4] == 1).all() and (r1[:, 2] == 1).all() and (r1[:, 3] == 1).all() and (r1[:, 1] < r1[:, 0]).all()
    # in place
    buf = torch.as_tensor(start, device=eng.device).clone()
    o = _lib.CameraRefineOpts(C.sizeof(_lib.CameraRefineOpts), 3, 1, 20, 34, 100.0, 1.0, 1e-3, 1e-12)
    rep2 = torch.empty(3, 8, dtype=torch.float64, device=eng.device)
    j = torch.as_tensor(joints, device=eng.device).contiguous()
    assert eng._lib.mvfit_refine_cameras(eng._ctx, j.data_ptr(), buf.data_ptr(), C.byref(o), buf.data_ptr(), rep2.data_ptr()) == 0
    assert np.array_equal(_bits(buf), _bits(cams)) and np.array_equal(_bits(rep2), _bits(rep))
    # the tuple form and the array form are one rig
    tup = unpack_cameras(start)
    assert np.array_equal(pack_cameras(tup).view(np.uint64), start.view(np.uint64))
    c3, r3 = eng.refine_cameras(joints, tup, fixed_views=(0,))
    assert np.array_equal(_bits(c3), _bits(cams))
    with pytest.raises(MvFitError):
        eng.refine_cameras(joints, start, free='everything')


def test_error_codes(eng):
    joints, gt, w, true, start = co.make_case(4, 2, seed=2)
    lib = eng._lib
    j = torch.as_tensor(joints, device=eng.device).contiguous()
    cm = torch.as_tensor(start, device=eng.device).contiguous()
    out, rep = torch.empty_like(cm), torch.empty(2, 8, dtype=torch.float64, device=eng.device)
    E = torch.empty(2, dtype=torch.float64, device=eng.device)

    def opts(**kw):
        v = dict(size=C.sizeof(_lib.CameraRefineOpts), free_mask=3, fixed_views=0, max_iter=20, min_points=34, rho=100.0,
                 data_weight=1.0, lambda0=1e-3, ftol=1e-12)
        v.update(kw)
        return _lib.CameraRefineOpts(*[v[f[0]] for f in _lib.CameraRefineOpts._fields_])

    def refine(ctx, jp, ci, o, co_, rp):
        return lib.mvfit_refine_cameras(ctx, jp, ci, C.byref(o) if o is not None else None, co_, rp)

    with MvFit(body_model()) as fresh:                                   # before mvfit_set_problems
        assert refine(fresh._ctx, j.data_ptr(), cm.data_ptr(), opts(), out.data_ptr(), rep.data_ptr()) == -3
        assert b'mvfit_set_problems' in lib.mvfit_last_error(fresh._ctx)
        assert lib.mvfit_camera_normal_eqs(fresh._ctx, j.data_ptr(), cm.data_ptr(), 100.0, 1.0, E.data_ptr(), None, None, None) == -3
        assert b'mvfit_set_problems' in lib.mvfit_last_error(fresh._ctx)
    _set(eng, start, gt, w)
    ptrs = dict(joints=j.data_ptr(), cams_in=cm.data_ptr(), opts=opts(), cams_out=out.data_ptr(), report=rep.data_ptr())
    for name in ptrs:
        a = dict(ptrs, **{name: None})
        assert refine(eng._ctx, a['joints'], a['cams_in'], a['opts'], a['cams_out'], a['report']) == -1
        assert name.encode() in lib.mvfit_last_error(eng._ctx)
    bad = dict(size=[8], free_mask=[0, 16], max_iter=[0, 65], min_points=[0], rho=[0.0, float('nan'), float('inf')],
               data_weight=[-1.0, float('nan')], lambda0=[0.0, float('inf'), float('nan')], ftol=[-1e-3, float('nan')])
    for field, values in bad.items():
        for x in values:
            assert refine(eng._ctx, j.data_ptr(), cm.data_ptr(), opts(**{field: x}), out.data_ptr(), rep.data_ptr()) == -1, (field, x)
            assert field.encode() in lib.mvfit_last_error(eng._ctx), (field, lib.mvfit_last_error(eng._ctx))
    for name, args in (('joints', (None, cm.data_ptr(), 100.0, 1.0, E.data_ptr())), ('cams', (j.data_ptr(), None, 100.0, 1.0, E.data_ptr())),
                       ('E', (j.data_ptr(), cm.data_ptr(), 100.0, 1.0, None)), ('rho', (j.data_ptr(), cm.data_ptr(), -1.0, 1.0, E.data_ptr())),
                       ('data_weight', (j.data_ptr(), cm.data_ptr(), 100.0, float('nan'), E.data_ptr()))):
        assert lib.mvfit_camera_normal_eqs(eng._ctx, *args, None, None, None) == -1
        assert name.encode() in lib.mvfit_last_error(eng._ctx)
    # the ops still work after the refusals, and the limits themselves are accepted
    assert refine(eng._ctx, j.data_ptr(), cm.data_ptr(), opts(max_iter=64, free_mask=15, ftol=0.0), out.data_ptr(), rep.data_ptr()) == 0
    assert lib.mvfit_camera_normal_eqs(eng._ctx, j.data_ptr(), cm.data_ptr(), 100.0, 0.0, E.data_ptr(), None, None, None) == 0
    eng.sync()
    assert (E.cpu().numpy() == 0.0).all() and np.isfinite(out.cpu().numpy()).all()
