"""CPU: the NumPy restatement of the camera refinement (tests/camera_refine_oracle.py) checked against itself - the gradient
against central differences, H against its definition, the known answer on exact data, the skip statuses, points without
weight - and the condition under which its Levenberg-Marquardt decisions may be compared with the device's; the camera file
writer's round trip."""
import os

import numpy as np
import pytest

from mvsmplfitting_amd import io_formats
from tests import camera_refine_oracle as co

DEMO_CAMS = os.path.join(os.path.dirname(__file__), 'golden', 'demo_data', '3DOH50K_Parameters.txt')

# (B, V, seed, noise px): the cases tests/test_gpu_camera_refine.py compares oracle.lm with the device on, at LM_FTOL.  With the
# default ftol = 1e-12 a run ends on decreases of 1e-13 of E, comparisons that rounding decides; at 1e-4 it ends on the first
# decrease below 1e-4 E, and the seeds are the first for which that decrease, like every other, is above 1e-6 E.
LM_CASES = [(16, 3, 10, 30.0), (31, 4, 10, 30.0), (5, 2, 10, 8.0)]
LM_FTOL = 1e-4


@pytest.fixture(scope='module')
def case16():
    """The set-up of the prototype: 16 frames at f = 1500, a camera 3.5 m away, 10 % zero weights, exact float32 pixels."""
    return co.make_case(16, 2, seed=1)


def test_gradient_against_central_differences(case16):
    """g against central differences of E along each of the 9 parameters, 1e-7 relative to the largest entry of its group's
    scale (rotation, translation, focal length, centre have very different magnitudes: each entry against itself)."""
    joints, gt, w, true, start = case16
    cam = start[0]
    E, g, H, count = co.normal_eqs(joints, gt[:, 0], w[:, 0], cam)
    assert count == int((w[:, 0] != 0).sum()) and np.isfinite(E)
    for i in range(9):
        h = 1e-6 if i < 6 else 1e-4
        d = np.zeros(9)
        d[i] = h
        Ep = co.normal_eqs(joints, gt[:, 0], w[:, 0], co.step(cam, d), need_grad=False)[0]
        Em = co.normal_eqs(joints, gt[:, 0], w[:, 0], co.step(cam, -d), need_grad=False)[0]
        fd = (Ep - Em) / (2 * h)
        print('param %d: g = %.12e, central difference = %.12e, relative %.2e' % (i, g[i], fd, abs(fd - g[i]) / abs(g[i])))
        assert abs(fd - g[i]) <= 1e-7 * abs(g[i])


def test_H_is_symmetric_and_the_JtJ_sum(case16):
    joints, gt, w, true, start = case16
    cam = start[1]
    E, g, H, _ = co.normal_eqs(joints, gt[:, 1], w[:, 1], cam, rho=80.0, data_weight=0.7)
    assert np.array_equal(H, H.T)
    assert np.all(np.linalg.eigvalsh(H) > -1e-9 * np.abs(H).max())
    # the definition, point by point
    Hd, gd, Ed = np.zeros((9, 9)), np.zeros(9), 0.0
    X = joints.astype(np.float64).reshape(-1, 3)
    ww, gg = w[:, 1].astype(np.float64).reshape(-1), gt[:, 1].astype(np.float64).reshape(-1, 2)
    rho2 = 80.0 ** 2
    for i in range(X.shape[0]):
        if ww[i] == 0:
            continue
        p, Ju, Jv = co.jacobian(cam, X[i:i + 1])
        uv = cam[12] * p[0, :2] / p[0, 2] + cam[13:15]
        k = 0.7 ** 2 * ww[i] ** 2
        for r, Jrow in ((gg[i, 0] - uv[0], Ju[0]), (gg[i, 1] - uv[1], Jv[0])):
            s = rho2 ** 2 / (r * r + rho2) ** 2
            Ed += k * rho2 * r * r / (r * r + rho2)
            gd -= 2 * k * s * r * Jrow
            Hd += 2 * k * s * np.outer(Jrow, Jrow)
    assert abs(E - Ed) <= 1e-12 * Ed
    assert np.abs(g - gd).max() <= 1e-12 * np.abs(gd).max()
    assert np.abs(H - Hd).max() <= 1e-12 * np.abs(Hd).max()


def test_jacobian_rows_against_differences_of_the_projection(case16):
    joints, gt, w, true, start = case16
    cam, X = true[0], joints.astype(np.float64).reshape(-1, 3)[:5]
    p, Ju, Jv = co.jacobian(cam, X)

    def proj(c_):
        q = X @ c_[:9].reshape(3, 3).T + c_[9:12]
        return c_[12] * q[:, :2] / q[:, 2:3] + c_[13:15]
    for i in range(9):
        d = np.zeros(9)
        d[i] = 1e-6
        fd = (proj(co.step(cam, d)) - proj(co.step(cam, -d))) / 2e-6
        assert np.abs(fd[:, 0] - Ju[:, i]).max() <= 1e-6 * max(1.0, np.abs(Ju[:, i]).max())
        assert np.abs(fd[:, 1] - Jv[:, i]).max() <= 1e-6 * max(1.0, np.abs(Jv[:, i]).max())


@pytest.mark.parametrize('free', ['extrinsics', 'all'])
def test_known_answer_on_exact_data(case16, free):
    """A start 2.5 degrees and 7 cm off returns to the truth on exact float32 pixels within a few iterations."""
    joints, gt, w, true, start = case16
    for v in range(2):
        cam, rep = co.lm(joints, gt[:, v], w[:, v], start[v], free_mask=co.FREE[free], max_iter=20)
        ang, dt = co.rot_angle(cam[:9], true[v, :9]), np.linalg.norm(cam[9:12] - true[v, 9:12])
        print('view %d free %s: E0 %.3e E1 %.3e it %d acc %d status %d, angle %.2e rad, |dt| %.2e m'
              % (v, free, rep[0], rep[1], rep[2], rep[3], rep[4], ang, dt))
        assert rep[4] in (0, 2) and rep[2] <= 12
        assert rep[1] < 1e-4 < rep[0]
        # float32 pixels at ~1000 px carry 6e-5 px of rounding: 1e-7 rad and 1e-6 m are well above what it leaves
        assert ang < 1e-6 and dt < (1e-5 if free == 'extrinsics' else 1e-3)
        assert abs(cam[12] - 1500.0) < (1e-12 if free == 'extrinsics' else 0.5)


def test_forward_and_reverse_summation_agree(case16):
    joints, gt, w, true, start = case16
    a, ra = co.lm(joints, gt[:, 0], w[:, 0], start[0])
    b, rb = co.lm(joints, gt[:, 0], w[:, 0], start[0], reverse=True)
    print('forward / reverse: max |dR| %.2e' % np.abs(a[:9] - b[:9]).max())
    assert np.abs(a[:9] - b[:9]).max() < 1e-12


def test_skip_statuses(case16):
    joints, gt, w, true, start = case16
    cam, rep = co.lm(joints, gt[:, 0], w[:, 0], start[0], fixed=True)
    assert rep[4] == 3 and np.array_equal(cam, start[0]) and rep[0] == rep[1] and rep[2] == 0
    few = w[:, 0].copy()
    few.reshape(-1)[20:] = 0
    cam, rep = co.lm(joints, gt[:, 0], few, start[0], min_points=34)
    assert rep[4] == 4 and np.array_equal(cam, start[0]) and rep[5] == int((few != 0).sum()) < 34
    back = start[0].copy()
    back[11] -= 10.0                                                     # the bodies at pz < 0
    cam, rep = co.lm(joints, gt[:, 0], w[:, 0], back)
    assert rep[4] == 5 and np.array_equal(cam, back) and rep[0] == np.inf
    E, g, H, count = co.normal_eqs(joints, gt[:, 0], w[:, 0], back)
    assert E == np.inf and count > 0
    cam, rep = co.lm(joints, gt[:, 0], w[:, 0], start[0], max_iter=1)
    assert rep[4] == 1 and rep[2] == 1


def test_a_point_without_weight_changes_nothing(case16):
    joints, gt, w, true, start = case16
    g2 = gt[:, 0].copy()
    g2[w[:, 0] == 0] = np.nan
    j2 = joints.copy()
    j2[w[:, 0] == 0] = np.nan
    assert (w[:, 0] == 0).sum() > 10
    a = co.normal_eqs(joints, gt[:, 0], w[:, 0], start[0])
    b = co.normal_eqs(j2, g2, w[:, 0], start[0])
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]
    ca, ra = co.lm(joints, gt[:, 0], w[:, 0], start[0])
    cb, rb = co.lm(j2, g2, w[:, 0], start[0])
    assert np.array_equal(ca, cb) and np.array_equal(ra, rb)


@pytest.mark.parametrize('B,V,seed,noise', LM_CASES)
def test_lm_cases_have_no_close_decision(B, V, seed, noise):
    """The cases whose iteration counts the GPU test compares: no E' < E comparison of theirs is closer than 1e-6 relative,
    forward or reverse, so a last-bit difference of the sums cannot flip one."""
    joints, gt, w, true, start = co.make_case(B, V, seed, noise=noise)
    for v in range(V):
        for free in (3, 15):
            for rev in (False, True):
                dec = []
                cam, rep = co.lm(joints, gt[:, v], w[:, v], start[v], free_mask=free, reverse=rev, decisions=dec,
                                 ftol=LM_FTOL)
                m = co.decision_margin(dec)
                assert m > 1e-6, (v, free, rev, m, rep)
                assert rep[1] < rep[0]


def test_save_camera_para_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    ex = rng.normal(size=(5, 4, 4)) * 10 ** rng.uniform(-6, 3, (5, 4, 4))
    ex[:, 3] = [0, 0, 0, 1]
    K = rng.normal(size=(5, 3, 3)) * 1000
    p = str(tmp_path / 'cams.txt')
    io_formats.save_camera_para(p, ex, K)
    ex2, K2 = io_formats.load_camera_para(p)
    assert np.array_equal(ex2.view(np.uint64), ex.view(np.uint64)) and np.array_equal(K2.view(np.uint64), K.view(np.uint64))


def test_save_camera_para_reproduces_the_demo_file(tmp_path):
    ex, K = io_formats.load_camera_para(DEMO_CAMS)
    p = str(tmp_path / 'cams.txt')
    io_formats.save_camera_para(p, ex, K)
    ex2, K2 = io_formats.load_camera_para(p)
    assert np.array_equal(ex2, ex) and np.array_equal(K2, K)
    with open(p) as a, open(DEMO_CAMS) as b:
        assert a.read().split() == b.read().split()
        a.seek(0), b.seek(0)
        assert [len(l.split()) for l in a] == [len(l.split()) for l in b][:sum(1 for _ in open(p))]
