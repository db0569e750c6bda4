"""GPU: mvfit_associate_views against its NumPy restatement (tests/associate_oracle.py) - the cost matrix bit for bit,
labels and cluster counts equal -, independence of the batch and of the frame groups, the decisive scene, error codes."""
import ctypes as C

import numpy as np
import pytest
import torch

from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import MvFit
from tests import associate_oracle as ao
from tests.helpers import body_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    with MvFit(body_model()) as e:
        yield e


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _device(eng, kp, count, K, E, **kw):
    labels, num, cost = eng.associate_views(kp, count, K, E, return_cost=True, **kw)
    return cost.cpu().numpy(), labels.cpu().numpy(), num.cpu().numpy()


def _crowd(F, V, N, seed):
    """Random detections around the camera ring: N persons per frame, every view sees a random subset in a random order
    with 25 px noise (so true pairs are loose and false pairs not far), plus slots of random pixels; random counts."""
    rng = np.random.default_rng(seed)
    K, E = ao.camera_matrices(syn.make_camera_ring(V))
    kp = np.zeros((F, V, N, 17, 3), np.float32)
    count = rng.integers(N // 2, N + 1, (F, V)).astype(np.int32)
    count[0, 0] = N                                                        # a full view and an empty one are always there
    count[F - 1, V - 1] = 0
    for f in range(F):
        pts = rng.uniform(-1.5, 1.5, (N, 1, 3)) * [1.0, 0.3, 1.0] + (rng.random((N, 17, 3)) - 0.5) * [0.7, 1.7, 0.4]
        uv = ao.project(pts, K, E)                                         # [V, N, 17, 2]
        for v in range(V):
            who = rng.permutation(N)
            for k in range(N):
                xy = uv[v, who[k]] + rng.normal(0, 25.0, (17, 2)) if rng.random() < 0.8 else rng.uniform(0, 1500, (17, 2))
                cf = rng.uniform(0.1, 1.0, (17, 1)) * (rng.random((17, 1)) < 0.85)
                kp[f, v, k] = np.concatenate([xy, cf], 1)
    return kp, count, K, E


@pytest.fixture(scope='module')
def crowd80():
    kp, count, K, E = _crowd(3, 5, 16, seed=80)
    return dict(kp=kp, count=count, K=K, E=E, want=ao.associate(kp, count, K, E, max_cost=1.0, min_joints=6, min_views=2))


def _check(got, want):
    cost, labels, num = got
    assert np.array_equal(_bits(cost), _bits(want[0]))
    assert np.array_equal(labels, want[1]) and labels.dtype == np.int32
    assert np.array_equal(num, want[2])


def test_cost_bits_small_with_every_branch(eng):
    """F = 2, V = 3, Nmax = 3 (D = 9: less than a tile), a view without detections, uneven counts, joints without
    confidence, a pair with fewer than min_joints common joints, and two views with one rotation that see a joint at the
    same pixel: the parallel-ray branch."""
    rng = np.random.default_rng(9)
    K = np.tile(np.array([[1200.0, 0, 960.0], [0, 1200.0, 540.0], [0, 0, 1]]), (3, 1, 1))
    K[2, 0, 0] = K[2, 1, 1] = 1500.0
    E = np.tile(np.eye(4), (3, 1, 1))
    E[0, :3, 3], E[1, :3, 3] = [0.0, 0.0, 4.0], [0.5, 0.1, 4.0]            # views 0 and 1: the same rotation
    R2 = syn.look_at_rotation([3.0, 0.5, 2.0])
    E[2, :3, :3], E[2, :3, 3] = R2, -R2 @ np.array([3.0, 0.5, 2.0])
    count = np.array([[3, 0, 2], [1, 3, 3]], np.int32)
    pts = (rng.random((2, 3, 17, 3)) - 0.5) * [2.0, 1.7, 1.0]
    kp = np.zeros((2, 3, 3, 17, 3), np.float32)
    for f in range(2):
        uv = ao.project(pts[f], K, E)
        for v in range(3):
            for k, p in enumerate(rng.permutation(3)):
                cf = rng.uniform(0.2, 1.0, 17) * (rng.random(17) < 0.8)
                kp[f, v, k] = np.concatenate([uv[v, p] + rng.normal(0, 3.0, (17, 2)), cf[:, None]], 1)
    kp[0, 1] = rng.uniform(0, 1000, (3, 17, 3))                            # slots at or above their count: never read
    kp[1, 0, 1:] = np.nan
    kp[0, 2, 1, 5:, 2] = 0.0                                               # five joints only: below min_joints = 6 with anyone
    kp[1, 1, 2, 0] = kp[1, 0, 0, 0] = [700.0, 300.0, 0.9]                  # one pixel, parallel rays
    want = ao.associate(kp, count, K, E, max_cost=0.3, min_joints=6, min_views=2)
    _, d, _ = ao.rays(kp[1], K, E)
    assert np.array_equal(d[0, 0, 0], d[1, 2, 0])                          # the branch is taken: the cross product is 0
    cost = want[0]
    assert np.all(np.isinf(cost[0][7])) and np.isfinite(cost[0][0, 6]) and np.isfinite(cost[1][0, 5])
    got = _device(eng, kp, count, K, E, max_cost=0.3, min_joints=6, min_views=2)
    _check(got, want)
    c = got[0]
    view = np.repeat(np.arange(3), 3)
    for f in range(2):
        valid = (np.arange(3)[None] < count[f][:, None]).reshape(-1)
        off = ~(valid[:, None] & valid[None, :] & (view[:, None] != view[None, :]))
        assert np.all(_bits(c[f][off]) == 0x7ff0000000000000)              # diagonal, same view, empty slots: +inf exactly
        assert np.array_equal(_bits(c[f]), _bits(c[f].T))
    assert np.all(got[1][0, 1] == -1) and np.all(got[1][1, 0, 1:] == -1)


def test_many_merges_over_several_tiles(eng, crowd80):
    """D = 80 (5 x 5 tiles of 16), max_cost = 1.0: dozens of merges and cannot-link refusals per frame."""
    want = crowd80['want']
    merged = [(want[1][f] >= 0).sum() - want[2][f] for f in range(3)]
    print('merges that ended in a kept cluster per frame:', merged, 'clusters:', want[2].tolist())
    assert min(merged) >= 24
    got = _device(eng, crowd80['kp'], crowd80['count'], crowd80['K'], crowd80['E'], max_cost=1.0)
    _check(got, want)
    for f in range(3):                                                     # a cluster never holds two detections of a view
        for c in range(got[2][f]):
            assert ((got[1][f] == c).sum(1) <= 1).all()


def test_capacity(eng):
    """V = 16, Nmax = 16: D = 256, one detection per thread of the clustering workgroup, 136 cost tiles."""
    kp, count, K, E = _crowd(1, 16, 16, seed=256)
    count[0, :15] = 16
    want = ao.associate(kp, count, K, E, max_cost=1.0, min_joints=6, min_views=3)
    assert (want[1] >= 0).sum() >= 100
    _check(_device(eng, kp, count, K, E, max_cost=1.0, min_joints=6, min_views=3), want)


def test_a_frame_does_not_depend_on_the_batch_or_the_frame_groups(eng, crowd80):
    kp, count, K, E, want = (crowd80[k] for k in ('kp', 'count', 'K', 'E', 'want'))
    one = tuple(w[2:3] for w in want)
    _check(_device(eng, kp[2:3], count[2:3], K, E, max_cost=1.0), one)
    # frames of one group: D * (17 * 32 + D * 8) bytes each under 256 MB less the 512-byte head (include/mvfit.h)
    D = 80
    group = ((256 << 20) - 512) // (D * (17 * 32 + D * 8))
    F = group + 4
    order = np.concatenate([np.arange(F - 1) % 3, [2]])                    # frame 2 of the case is the last of the call
    labels, num, cost = eng.associate_views(kp[order], count[order], K, E, max_cost=1.0, return_cost=True)
    assert np.array_equal(_bits(cost[-1:].cpu().numpy()), _bits(one[0]))
    assert np.array_equal(_bits(cost[group - 1:group + 2].cpu().numpy()), _bits(want[0][order[group - 1:group + 2]]))
    assert np.array_equal(labels.cpu().numpy(), want[1][order]) and np.array_equal(num.cpu().numpy(), want[2][order])
    # without the cost matrix, and a smaller call after a larger one
    labels, num = eng.associate_views(kp[::-1].copy(), count[::-1].copy(), K, E, max_cost=1.0)
    assert np.array_equal(labels.cpu().numpy(), want[1][::-1]) and np.array_equal(num.cpu().numpy(), want[2][::-1])


def test_the_decisive_scene_is_recovered(eng):
    s = ao.decisive_scene(syn.make_camera_ring(4))
    labels, num = eng.associate_views(s['kp'], s['count'], s['K'], s['E'])
    assert int(num[0]) == 3 and ao.same_partition(labels.cpu().numpy(), s['truth'])
    _check(_device(eng, s['kp'], s['count'], s['K'], s['E']), ao.associate(s['kp'], s['count'], s['K'], s['E']))


def test_argument_errors(eng):
    F, V, N = 1, 3, 2
    dev = eng.device
    kp = torch.zeros(F, 16, 16, 17, 3, device=dev)
    cnt = torch.zeros(F, 16, dtype=torch.int32, device=dev)
    K = torch.eye(3, dtype=torch.float64, device=dev).repeat(16, 1, 1)
    E = torch.eye(4, dtype=torch.float64, device=dev).repeat(16, 1, 1)
    lab = torch.zeros(F, 16, 16, dtype=torch.int32, device=dev)
    num = torch.zeros(F, dtype=torch.int32, device=dev)

    def call(F=F, V=V, N=N, kp=kp, cnt=cnt, K=K, E=E, max_cost=0.05, min_joints=6, min_views=2, lab=lab, num=num):
        p = lambda t: None if t is None else t.data_ptr()
        return eng._lib.mvfit_associate_views(eng._ctx, F, V, N, p(kp), p(cnt), p(K), p(E), C.c_double(max_cost), min_joints,
                                              min_views, None, p(lab), p(num))
    assert call() == 0 and call(num=None) == 0 and call(max_cost=0.0) == 0 and call(V=16, N=16, min_views=16, min_joints=17) == 0
    bad = [dict(F=0), dict(V=1), dict(V=17), dict(N=0), dict(N=17), dict(min_joints=0), dict(min_joints=18), dict(min_views=1),
           dict(min_views=4), dict(max_cost=-0.01), dict(max_cost=float('inf')), dict(max_cost=float('nan')), dict(kp=None),
           dict(cnt=None), dict(K=None), dict(E=None), dict(lab=None)]
    for kw in bad:
        assert call(**kw) == -1, kw                                        # MVFIT_E_ARG
    eng.sync()
    with pytest.raises(Exception, match='min_joints'):
        eng.associate_views(kp[:, :3, :2], cnt[:, :3], K[:3], E[:3], min_joints=0)
