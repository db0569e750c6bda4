"""CPU: joint_refine.refine_joint with a scan share, against a small engine defined here: the quadratic engine of
tests/test_joint_refine_cpu.py with a fourth part, L_scan,j = ||V_j - P_j||^2 against a "scan set" P that the engine owns like
its masks.  The joint energy is computed directly; the scan part is a problem's own and needs no correction in E."""
import numpy as np
import pytest
import torch

from mvsmplfitting_amd.joint_refine import check_shares, refine_joint
from tests.test_joint_refine_cpu import FRM, GROUP, MIX, SEQ, SIZES, STAGE, QuadraticEngine, _joint_energy, _world

SHARES4 = dict(scene=0.5, silhouette=2.0, temporal=0.25, scan=1.5)
SCAN = dict(scan_w_s2m=1.0, scan_w_m2s=0.5, scan_sigma=0.05)
KW = dict(shares=SHARES4, scene_sizes=SIZES, seq_id=SEQ, frame_idx=FRM, grid_size=16, scale_factor=0.3, robustifier=0.01,
          w_in=1.0, w_out=0.5, sigma=3.0, max_iter=9, **SCAN)


class ScanQuadraticEngine(QuadraticEngine):
    """QuadraticEngine whose mix takes a scan share: the four-keyword set_term_mix, four parts, term_mix_read(scan=True)."""

    def __init__(self, centres, masks, scans, moves=()):
        super().__init__(centres, masks, moves)
        self.P = None if scans is None else np.asarray(scans, np.float64)
        self.reads = []

    def set_term_mix(self, scene=0.0, silhouette=0.0, vertex_targets=0.0, w_in=1.0, w_out=1.0, sigma=0.0, scan=0.0, scan_w_s2m=1.0,
                     scan_w_m2s=0.0, scan_sigma=0.0):
        assert (scene == 0 or self.obst is not None) and (vertex_targets == 0 or self.targets is not None)
        assert scan == 0 or self.P is not None
        assert (w_in, w_out, sigma) == (1.0, 0.5, 3.0)
        assert (scan_w_s2m, scan_w_m2s, scan_sigma) == (1.0, 0.5, 0.05)
        self.mix = (scene, silhouette, vertex_targets, scan)

    def _anchors(self, j):
        out = super()._anchors(j)
        if self.mix[3] > 0:
            out.append((self.mix[3], self.P[j], 3))
        return out

    def closure(self, x, stage, want_grad=True):
        assert self.mix is not None and not want_grad
        u = np.asarray(torch.as_tensor(np.asarray(x))[:, :6].double())
        v = u @ MIX
        self.parts = np.zeros((self.B, 4))
        pen = np.zeros(self.B)
        for j in range(self.B):
            for lam, p, kind in self._anchors(j):
                d = ((v[j] - p) ** 2).sum()
                pen[j] += lam * d
                self.parts[j, kind] += lam * d / self.mix[kind]
        return dict(loss=torch.as_tensor(((u - self.c) ** 2).sum(1) + stage['coll_loss_weight'] ** 2 * pen))

    def term_mix_read(self, scan=False):
        assert self.mix is not None
        self.reads.append(scan)
        return torch.as_tensor(self.parts if scan else self.parts[:, :3])


def _scans(c, seed=7):
    return (c + 0.25 * np.random.default_rng(seed).normal(size=c.shape)) @ MIX


def _energy4(c, masks, scans, x, w, shares=SHARES4):
    """test_joint_refine_cpu._joint_energy and, per group, the scan distances added with their share: nothing else changes"""
    E, parts = _joint_energy(c, masks, x, w, shares)
    v = np.asarray(x, np.float64)[:, :6] @ MIX
    d = ((v - scans) ** 2).sum(1)
    p4 = np.zeros((3, 4))
    p4[:, :3] = parts
    for j in range(7):
        p4[GROUP[j], 3] += d[j]
    return E + w * w * shares['scan'] * p4[:, 3], p4


def test_shares_with_and_without_the_scan_key():
    assert check_shares(dict(scene=1, temporal=2)) == (1.0, 0.0, 2.0)                  # the 3-tuple it was
    assert check_shares(dict(scene=1, scan=2)) == (1.0, 0.0, 0.0, 2.0)
    assert check_shares(dict(scene=1, temporal=2, scan=0)) == (1.0, 0.0, 2.0, 0.0)
    with pytest.raises(ValueError, match='at least two shares'):
        check_shares(dict(scan=1))
    with pytest.raises(ValueError, match='at least two shares'):
        check_shares(dict(scene=1, scan=0.0))
    with pytest.raises(ValueError, match="unknown shares \\['scans'\\]"):
        check_shares(dict(scene=1, scans=1))
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='finite and >= 0'):
            check_shares(dict(scene=1, scan=bad))


def test_four_column_reports_and_the_joint_energy():
    c, masks, x0 = _world()
    scans = _scans(c)
    w = STAGE['coll_loss_weight']
    eng = ScanQuadraticEngine(c, masks, scans)
    x, rep = refine_joint(eng, torch.as_tensor(x0), STAGE, sweeps=3, **KW)
    E0, parts0 = _energy4(c, masks, scans, x0, w)
    assert rep['group'].tolist() == GROUP and rep['shares'] == SHARES4
    assert rep['parts0'].shape == (3, 4) and rep['parts_problem'].shape == (7, 4)
    assert np.allclose(rep['E0'], E0, rtol=1e-12, atol=0) and np.allclose(rep['parts0'], parts0, rtol=1e-12, atol=0)
    assert 1 <= len(rep['sweeps']) <= 3 and eng.n_fit == len(rep['sweeps'])
    prev = E0
    for sw in rep['sweeps']:
        Ek, pk = _energy4(c, masks, scans, sw['params'], w)
        assert sw['parts'].shape == (3, 4)
        assert np.allclose(sw['E'], Ek, rtol=1e-12, atol=0) and np.allclose(sw['parts'], pk, rtol=1e-12, atol=0)
        assert (sw['E'] <= prev).all() and (sw['E'][sw['accepted']] < prev[sw['accepted']]).all()
        prev = sw['E']
    assert rep['sweeps'][0]['accepted'].all()
    E, parts = _energy4(c, masks, scans, x.numpy(), w)
    got = np.array([rep['parts_problem'][np.array(GROUP) == g].sum(0) for g in range(3)])
    assert np.allclose(got, parts, rtol=1e-12, atol=0)
    assert (parts[:, 3] < parts0[:, 3]).all()                        # the bodies moved towards their scans
    loss = np.array([rep['loss'][np.array(GROUP) == g].sum() for g in range(3)])
    assert np.allclose(loss, E + 0.5 * w * w * SHARES4['temporal'] * parts[:, 2], rtol=1e-12, atol=0)
    assert eng.reads and all(eng.reads)                              # every read asked for the four parts
    # the mix off, targets and obstacles cleared; the scan set and the masks are the caller's
    assert eng.mix is None and eng.targets is None and eng.obst is None
    assert np.array_equal(eng.P, scans) and np.array_equal(eng.M, masks)


def test_scan_and_silhouette_alone_link_no_problems():
    c, masks, x0 = _world(5)
    scans = _scans(c, 8)
    w = STAGE['coll_loss_weight']
    eng = ScanQuadraticEngine(c, masks, scans)
    kw = dict(KW, shares=dict(silhouette=1.5, scan=0.5))
    for k in ('scene_sizes', 'seq_id', 'frame_idx'):
        kw.pop(k)
    x, rep = refine_joint(eng, torch.as_tensor(x0), STAGE, sweeps=1, **kw)
    assert rep['group'].tolist() == list(range(7)) and eng.n_obst == 0 and eng.n_targets == 0
    v = x0[:, :6] @ MIX
    E0 = ((x0[:, :6] - c) ** 2).sum(1) + w * w * (1.5 * ((v - masks) ** 2).sum(1) + 0.5 * ((v - scans) ** 2).sum(1))
    assert np.allclose(rep['E0'], E0, rtol=1e-12, atol=0)
    assert not rep['parts0'][:, 0].any() and not rep['parts0'][:, 2].any()
    assert np.allclose(rep['parts0'][:, 3], ((v - scans) ** 2).sum(1), rtol=1e-12, atol=0)


def test_without_a_scan_share_the_engine_is_called_as_before():
    """the three-keyword engine of tests/test_joint_refine_cpu.py accepts nothing else; a scan key of 0 is no scan share"""
    c, masks, x0 = _world()
    three = dict(scene=0.5, silhouette=2.0, temporal=0.25)
    kw = {k: v for k, v in KW.items() if k not in SCAN}
    a = QuadraticEngine(c, masks)
    xa, ra = refine_joint(a, torch.as_tensor(x0), STAGE, sweeps=2, **dict(kw, shares=three))
    b = QuadraticEngine(c, masks)
    xb, rb = refine_joint(b, torch.as_tensor(x0), STAGE, sweeps=2, **dict(kw, shares=dict(three, scan=0.0)))
    assert torch.equal(xa, xb) and ra['parts0'].shape == (3, 3) and rb['parts0'].shape == (3, 3)
    assert np.array_equal(ra['E0'], rb['E0'])


def test_the_engine_is_left_clean_when_the_fit_raises():
    c, masks, x0 = _world(3)
    scans = _scans(c)
    eng = ScanQuadraticEngine(c, masks, scans, moves=[lambda x: RuntimeError('boom')])
    with pytest.raises(RuntimeError, match='boom'):
        refine_joint(eng, x0, STAGE, **KW)
    assert eng.mix is None and eng.targets is None and eng.obst is None
    assert np.array_equal(eng.P, scans)                              # the scan set is the caller's
