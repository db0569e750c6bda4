"""TESTS ONLY - float64 restatement of the closure for a model WITHOUT a keypoint regressor (model_type 'smpl',
pose_format 'coco17', include/mvfit.h): keypoint k is the posed skeleton joint joint_map[k] < 24 (the translation column
of the chained transform, reference code/smplx/lbs.py:370, + transl) or the face vertex joint_map[k] - 24.

Built on oracle/closure_np.py:ClosureOracle: its selection matrix keeps only the face-vertex rows (the skeleton rows are
empty), the forward then adds G_t to the skeleton rows, and the adjoint adds what the skeleton rows contribute - their
g_kp seeded into g_G_t and carried down the chain to pose, root scale and betas - to the base class's gradient (the
adjoint is linear in its seeds: the two parts add)."""
import numpy as np

from oracle import closure_np as cn

NJ = 24


class SmplClosureOracle(cn.ClosureOracle):
    def __init__(self, model: dict, dtype=np.float64, vposer=None, gmm=None):
        assert model.get('kp_regressor') is None, "the 'smpl' kind has no keypoint regressor"
        # (the base class is handed an empty regressor and the LSP map; its selection matrix is replaced below)
        super().__init__(dict(model, kp_regressor=np.zeros((14, model['v_template'].shape[0]), np.float32),
                              joint_map=np.arange(17)), dtype, vposer=vposer, gmm=gmm)
        jm = np.asarray(model['joint_map'], np.int64)
        assert jm.min() >= 0 and jm.max() < NJ + 5
        self.kp_joint = np.where(jm < NJ, jm, -1)
        sel = np.zeros((17, self.vt.shape[0]), dtype)
        for k, s in enumerate(jm):
            if s >= NJ:
                sel[k, self.face_ids[s - NJ]] = 1.0
        self.Ksel = sel

    def body(self, p: dict, want_cache=True):
        out = super().body(p, want_cache=True)
        Gt = out['_cache'][11]
        sk = self.kp_joint >= 0
        out['joints'] = out['joints'].copy()
        out['joints'][sk] += Gt[self.kp_joint[sk]]              # the row itself is empty: kp = transl so far
        if not want_cache:
            del out['_cache']
        return out

    def _backward(self, out, aux, cams, w_conf, wts, use_vposer, z, prior, fix_shape, g_verts_extra=None, joints3d=None):
        g = super()._backward(out, aux, cams, w_conf, wts, use_vposer, z, prior, fix_shape, g_verts_extra, joints3d)
        dt = self.dtype
        beta, theta, tau, s, J, R, rc, v_posed, Rm, tm, Gr, Gt, Tr, cache_vp = out['_cache']
        g_kp = self._g_kp(aux, cams, w_conf, wts, joints3d)
        # seeds: g_G_t[j] = sum of the g_kp of the keypoints that are joint j
        g_Gt = np.zeros((NJ, 3), dt)
        for k, j in enumerate(self.kp_joint):
            if j >= 0:
                g_Gt[j] += g_kp[k]
        g_Gr = np.zeros((NJ, 3, 3), dt)
        g_Rm = np.zeros_like(g_Gr)
        g_tm = np.zeros_like(g_Gt)
        for i in range(NJ - 1, 0, -1):                         # the chain adjoint of ClosureOracle._backward
            pa = self.par[i]
            g_Rm[i] = Gr[pa].T @ g_Gr[i]
            g_tm[i] = Gr[pa].T @ g_Gt[i]
            g_Gr[pa] += g_Gr[i] @ Rm[i].T + np.outer(g_Gt[i], tm[i])
            g_Gt[pa] += g_Gt[i]
        g_Rm[0], g_tm[0] = g_Gr[0], g_Gt[0]
        g_J = g_tm.copy()
        for i in range(1, NJ):
            g_J[self.par[i]] -= g_tm[i]
        g_s = (g_Rm[0] * R[0]).sum()
        g_R = g_Rm.copy()
        g_R[0] = s * g_Rm[0]
        g_beta = np.einsum('vkl,vk->l', self.S, (self.JR.T @ g_J))
        g_theta = np.stack([cn.rodrigues_bwd(g_R[i], theta[i], rc[i]) for i in range(NJ)]).reshape(72)
        extra = np.zeros_like(g)
        extra[0:10] = g_beta
        extra[10:13] = g_theta[:3]
        if use_vposer:
            extra[16] = g_s
            extra[17:] = cn.vposer_decode_bwd(g_theta[3:], self.vp, cache_vp)
        else:
            extra[13:82] = g_theta[3:]
            extra[85] = g_s
        return g + extra

    def _g_kp(self, aux, cams, w_conf, wts, joints3d):
        """d loss / d keypoint [17,3] (the first lines of ClosureOracle._backward)."""
        dt = self.dtype
        cam_R, cam_t, cam_f, cam_c = (np.asarray(a, dt) for a in cams)
        rho2 = dt(wts['rho']) ** 2
        dw2 = dt(wts['data_weight']) ** 2
        r, p = aux['r'], aux['p']
        w2 = (np.asarray(w_conf, dt) ** 2)[..., None]
        g_uv = -w2 * dw2 * 2.0 * r * rho2 * rho2 / (r * r + rho2) ** 2
        f = cam_f[:, None]
        pz = p[..., 2]
        g_p = np.stack([f * g_uv[..., 0] / pz, f * g_uv[..., 1] / pz,
                        -f * (g_uv[..., 0] * p[..., 0] + g_uv[..., 1] * p[..., 1]) / (pz * pz)], axis=-1)
        g_kp = np.einsum('vab,vka->kb', cam_R, g_p)
        if joints3d is not None:
            r3 = aux['r3']
            c2 = (np.asarray(joints3d[1], dt) ** 2)[:, None]
            g_kp = g_kp - c2 * dw2 * 2.0 * r3 * rho2 * rho2 / (r3 * r3 + rho2) ** 2
        return g_kp
