"""CPU: the landmark term's NumPy oracle (tests/landmark_oracle.py) against torch.autograd of the same formula in float64 -
robust and plain penalties, with and without the 3-D part, a vertex shared by two landmarks, a vertex named twice inside one
landmark, and entries of confidence 0 that hold NaN."""
import numpy as np
import pytest
import torch

from mvsmplfitting_amd import synthetic as syn
from tests.landmark_oracle import landmark_loss

B, V, NV = 3, 4, 40


def _case(seed=0):
    rng = np.random.default_rng(seed)
    verts = rng.normal(0, 0.4, (B, NV, 3))
    ids = np.array([[0, -1, 7, 7], [NV - 1, 5, 0, 0], [5, 9, 11, 13], [9, 9, 0, 2], [21, 0, 0, 0]], np.int32)
    w = np.array([[1.0, 0.0, 0.0, 0.0], [0.5, 0.5, 0.0, 0.0], [0.1, 0.2, 0.3, 0.4], [0.75, 0.25, 0.0, 0.0],
                  [1.25, 0.0, 0.0, 0.0]])                    # row 3: vertex 9 twice; 5 and 9 shared; an id of -1 in a dead slot
    cams = syn.make_camera_ring(V)
    L = len(ids)
    p = np.einsum('lk,blkc->blc', w, verts[:, np.where(w != 0, ids, 0)])
    xy = syn.project_points(p, *cams) + rng.normal(0, 3.0, (B, V, L, 2))
    conf = rng.uniform(0.5, 1.0, (B, V, L))
    xyz = p + rng.normal(0, 0.02, p.shape)
    conf3 = rng.uniform(0.5, 1.0, (B, L))
    conf[1] = 0.0
    conf[0, 2, 3] = 0.0
    conf3[1] = 0.0
    conf3[2, 4] = 0.0
    xy[conf == 0] = np.nan
    xyz[conf3 == 0] = np.nan
    return verts, ids, w, cams, xy, conf, xyz, conf3


def _torch_loss(verts, ids, w, cams, xy, conf, xyz, conf3, rho, w3d, rho3d):
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    Vt = t(verts).requires_grad_(True)
    wt = t(w)
    live = wt != 0
    p = (wt[None, :, :, None] * Vt[:, torch.as_tensor(np.where(w != 0, ids, 0)).long()]).sum(dim=2)
    R, tt, f, c = (t(a) for a in cams)
    q = torch.einsum('vij,blj->bvli', R, p) + tt[None, :, None, :]
    u = f[None, :, None, None] * q[..., :2] / q[..., 2:3] + c[None, :, None, :]

    def g(r, s):
        return r * r if s == 0 else s * s * r * r / (r * r + s * s)
    cf = t(conf)
    r = u - torch.nan_to_num(t(xy))
    loss = (cf ** 2 * g(r, rho).sum(-1)).sum(dim=(1, 2))
    if xyz is not None:
        loss = loss + w3d * (t(conf3) ** 2 * g(p - torch.nan_to_num(t(xyz)), rho3d).sum(-1)).sum(dim=1)
    loss.sum().backward()
    assert live.any()
    return loss.detach().numpy(), Vt.grad.numpy()


@pytest.mark.parametrize('rho,with3d,rho3d', [(100.0, False, 0.0), (0.0, False, 0.0), (100.0, True, 0.05), (30.0, True, 0.0)])
def test_oracle_matches_autograd(rho, with3d, rho3d):
    verts, ids, w, cams, xy, conf, xyz, conf3 = _case()
    kw = dict(xyz=xyz, conf3=conf3) if with3d else {}
    L, g = landmark_loss(verts, ids, w, cams, xy, conf, rho=rho, w3d=2.5, rho3d=rho3d, **kw)
    L_t, g_t = _torch_loss(verts, ids, w, cams, xy, conf, xyz if with3d else None, conf3, rho, 2.5, rho3d)
    assert np.isfinite(L).all() and np.isfinite(g).all()
    assert np.allclose(L, L_t, rtol=1e-12, atol=0)
    assert np.abs(g - g_t).max() <= 1e-11 * np.abs(g_t).max()
    assert L[1] == 0.0 and not g[1].any()                    # all confidences zero
    used = np.unique(ids[w != 0])
    rest = np.setdiff1d(np.arange(NV), used)
    assert not g[:, rest].any() and g[0][used].any(axis=1).all()
    L_only, none = landmark_loss(verts, ids, w, cams, xy, conf, rho=rho, w3d=2.5, rho3d=rho3d, need_grad=False, **kw)
    assert none is None and np.array_equal(L_only, L)


def test_dead_entries_change_nothing():
    verts, ids, w, cams, xy, conf, xyz, conf3 = _case()
    ref = landmark_loss(verts, ids, w, cams, xy, conf, xyz, conf3, w3d=1.0, rho3d=0.05)
    ids2 = ids.copy()
    ids2[w == 0] = 123456
    xy2, xyz2 = xy.copy(), xyz.copy()
    xy2[conf == 0] = 7.0
    xyz2[conf3 == 0] = -3.0
    got = landmark_loss(verts, ids2, w, cams, xy2, conf, xyz2, conf3, w3d=1.0, rho3d=0.05)
    assert np.array_equal(ref[0], got[0]) and np.array_equal(ref[1], got[1])


def test_float32_evaluation_stays_float32_and_close():
    verts, ids, w, cams, xy, conf, xyz, conf3 = _case()
    L64, g64 = landmark_loss(verts, ids, w, cams, xy, conf, xyz, conf3, w3d=1.0, rho3d=0.05)
    L32, g32 = landmark_loss(verts.astype(np.float32), ids, w.astype(np.float32), tuple(np.float32(a) for a in cams),
                             xy.astype(np.float32), conf.astype(np.float32), xyz.astype(np.float32), conf3.astype(np.float32),
                             w3d=1.0, rho3d=0.05, dtype=np.float32)
    assert L32.dtype == np.float32 and g32.dtype == np.float32
    live = L64 > 0
    assert (np.abs(L32[live] - L64[live]) / L64[live]).max() < 1e-3
    assert np.abs(g32 - g64).max() / np.abs(g64).max() < 1e-3
