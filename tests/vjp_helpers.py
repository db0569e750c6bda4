"""Shared by the tests of mvfit_vertices_backward (tests/test_vertices_vjp_cpu.py, tests/test_gpu_vertices_backward.py) and
tools/make_golden_vjp.py: the configurations, the seeded points and cotangents, and the float64 hand-derived VJP.

The oracle VJP is the closure oracle's adjoint with every loss weight 0 (oracle/closure_np.py:ClosureOracle.closure):
the vertex cotangent enters as its g_verts_extra, the keypoint cotangent folded through the selection matrix Ksel
(keypoint k = Ksel[k] . vertices).  The skeleton keypoints of the 'smpl' kind (tests/smpl_oracle.py) are no rows of
Ksel: their cotangent seeds the chain's g_G_t (SmplVjpOracle).  Every keypoint is its source + transl: g_transl gets
the sum of the keypoint cotangent."""
from __future__ import annotations

import numpy as np

from mvsmplfitting_amd import synthetic as syn
from oracle import closure_np as cn
from tests.helpers import body_model
from tests.smpl_oracle import SmplClosureOracle

B_GOLD = 3
MODES = ('v', 'j', 'vj')                # cotangent on the vertices, on the joints, on both
CONFIGS = {
    'lsp_dense': dict(kind='smpllsp', skin_topk=None, vposer=False, seed=101),
    'lsp_top4': dict(kind='smpllsp', skin_topk=4, vposer=False, seed=102),
    'lsp_vposer': dict(kind='smpllsp', skin_topk=None, vposer=True, seed=103),
    'smpl': dict(kind='smpl', skin_topk=None, vposer=False, seed=104),
}
ZERO_WTS = dict(data_weight=0.0, body_pose_weight=0.0, shape_weight=0.0, bending_prior_weight=0.0, rho=100.0)


def model_for(cfg):
    if cfg['kind'] == 'smpl':
        return syn.make_body_model(0, skin_topk=cfg['skin_topk'], model_type='smpl')
    return body_model(0, cfg['skin_topk'])


def vposer_for(cfg):
    return syn.make_vposer_decoder() if cfg['vposer'] else None


def random_points(seed, B, use_vposer):
    """Compact parameters (oracle/closure_np.py:param_layout), float32-representable."""
    lay, D = cn.param_layout(use_vposer)
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 0.3, (B, D))
    x[:, lay['betas'][0]:lay['betas'][1]] = rng.normal(0.0, 1.0, (B, 10))
    x[:, lay['transl'][0]:lay['transl'][1]] = rng.normal(0.0, 0.5, (B, 3))
    x[:, lay['scale'][0]] = 1.0 + rng.normal(0.0, 0.1, B)
    if use_vposer:
        x[:, lay['pose_embedding'][0]:lay['pose_embedding'][1]] = rng.normal(0.0, 0.5, (B, 32))
    return x.astype(np.float32).astype(np.float64)


def cotangents(seed, B, nv, mode='vj'):
    """(g_verts[B,nv,3] | None, g_joints[B,17,3] | None), float32 values."""
    rng = np.random.default_rng(seed + 7919)
    gv = rng.standard_normal((B, nv, 3)).astype(np.float32)
    gj = rng.standard_normal((B, 17, 3)).astype(np.float32)
    return (gv if 'v' in mode else None), (gj if 'j' in mode else None)


def cotangent_checksum(gv, gj):
    s = 0.0
    for a in (gv, gj):
        if a is not None:
            s += float(np.abs(a.astype(np.float64)).sum())
    return s


def x_to118(xc, use_vposer):
    """compact point -> flat x[118] (include/mvfit.h; the embedding slots 0 without VPoser, body_pose 0 with)."""
    xc = np.asarray(xc, np.float64)
    out = np.zeros(118)
    out[0:13] = xc[0:13]
    if use_vposer:
        out[82:86] = xc[13:17]
        out[86:118] = xc[17:49]
    else:
        out[13:86] = xc[13:86]
    return out


def g_to118(g, use_vposer):
    """compact gradient -> the flat layout of mvfit_vertices_backward (unused slots 0)."""
    return x_to118(g, use_vposer)


class SmplVjpOracle(SmplClosureOracle):
    """tests/smpl_oracle.py with the keypoint cotangent as the seed of its skeleton rows."""
    seed = None

    def _g_kp(self, aux, cams, w_conf, wts, joints3d):
        return np.asarray(self.seed, self.dtype)


class VjpOracle:
    """float64 VJP of (vertices, joints) at one compact point."""

    def __init__(self, model, vposer=None):
        self.smpl = model.get('kp_regressor') is None
        self.o = SmplVjpOracle(model, np.float64, vposer=vposer) if self.smpl else \
            cn.ClosureOracle(model, np.float64, vposer=vposer)
        self.nv = model['v_template'].shape[0]
        self.cams = syn.make_camera_ring(1)

    def vjp(self, xc, gv=None, gj=None, use_vposer=False):
        """compact gradient of <gv, vertices> + <gj, joints>."""
        lay, _ = cn.param_layout(use_vposer)
        gv = np.zeros((self.nv, 3)) if gv is None else np.asarray(gv, np.float64)
        gj = np.zeros((17, 3)) if gj is None else np.asarray(gj, np.float64)
        extra = gv + self.o.Ksel.T @ gj
        if self.smpl:
            self.o.seed = np.where((self.o.kp_joint >= 0)[:, None], gj, 0.0)
        gt = np.zeros((1, 17, 2))
        conf = np.zeros((1, 17))
        _, g, _ = self.o.closure(xc, self.cams, gt, conf, ZERO_WTS, use_vposer=use_vposer, g_verts_extra=extra)
        # d keypoint / d transl = I (the keypoint is its source + transl, body_models_scale.py:393-403), where the fold
        # through Ksel gave the row sums of the regressor
        g = g.copy()
        g[lay['transl'][0]:lay['transl'][1]] += gj.sum(0) - (self.o.Ksel.T @ gj).sum(0)
        return g
