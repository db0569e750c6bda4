"""Host-side handle on libmvfit: one ``MvFit`` = one mvfit_ctx = one GPU + one stream.

PyTorch is used only as the device-memory container (tensors' ``data_ptr()`` cross the C ABI);
every number is produced by the HIP kernels in mvsmplfitting_amd/csrc.
"""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np
import torch

from . import _lib

D = _lib.D
D_MODEL = _lib.D_MODEL

# slices of the flat parameter vector (include/mvfit.h)
SL = dict(betas=(0, 10), global_orient=(10, 13), body_pose=(13, 82), transl=(82, 85),
          scale=(85, 86), pose_embedding=(86, 118))

# reference cfg_files/fit_smpl.yaml:40-68
YAML_POSE_W = (404.0, 404.0, 57.4, 4.78)
YAML_SHAPE_W = (100.0, 50.0, 10.0, 5.0)


class MvFitError(RuntimeError):
    pass


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# the reference's Renderer.colors in dictionary order (code/utils/utils.py:904-912): body k of a scene takes entry k mod 7
SCENE_PALETTE = ((.8, .1, .1), (.1, .1, .8), (.1, .8, .1), (.7, .7, .9), (.9, .9, .8), (.7, .75, .5), (.5, .7, .75))


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def stage_weights(image_height: float, flags: int = 0, rho: float = 100.0,
                  pose_w=YAML_POSE_W, shape_w=YAML_SHAPE_W, coll_w=None):
    """Per-stage weights exactly as non_linear_solver builds them (reference
    code/utils/non_linear_solver.py:109-124,148-150,177-180): data_weight = 500/H,
    bending = 3.17 * body_pose_weight - the product rounded to float32 like the reference's float32 weight tensor."""
    out = []
    for s in range(len(pose_w)):
        out.append(dict(data_weight=500.0 / image_height, body_pose_weight=pose_w[s],
                        shape_weight=shape_w[s], bending_prior_weight=float(np.float32(3.17) * np.float32(pose_w[s])),
                        coll_loss_weight=0.0 if coll_w is None else coll_w[s], rho=rho, flags=flags))
    return out


_SDF_WALK_WARNING = ('%s walked over every face (about ten times slower, same bits): the workspace of the face lists did not '
                     'fit in half of the free device memory (is the GPU shared?)')

# Options every new engine starts from (field names of include/mvfit.h:mvfit_options; empty = the library's defaults).  The
# reference-seam mirror (fitting.py) builds its engine internally, so callers that need another default for a whole process
# (tests, bench.py's named configs) set it here; per-engine values go to MvFit(..., options=...) / set_options().
DEFAULT_OPTIONS: dict = {}
CONTRACTIONS = dict(split_fp16=_lib.CONTRACTION_SPLIT_FP16, exact_fp32=_lib.CONTRACTION_EXACT_FP32,
                    half_basis=_lib.CONTRACTION_HALF_BASIS)


class MvFit:
    def __init__(self, model: dict, vposer: dict | None = None, gmm=None, device: int = 0, options: dict | None = None,
                 library: str | None = None):
        """model: dict from mvsmplfitting_amd.synthetic.make_body_model (or real SMPL arrays with the
        same keys); vposer: decoder weight dict; gmm: (means, precisions, nll_weights); options: mvfit_options fields
        (``contraction`` also by name: 'split_fp16' | 'exact_fp32' | 'half_basis'); library: another build of libmvfit."""
        if not torch.cuda.is_available():
            raise MvFitError('MvFit needs a HIP device (torch.cuda.is_available() is False); '
                             'there is no CPU fallback')
        self._lib = _lib.load(library)
        self.device = torch.device('cuda', device)
        self.dtype = torch.float32
        self.nv = int(model['v_template'].shape[0])
        keep = []

        def fp(a):
            a = _f32(a)
            keep.append(a)
            return a.ctypes.data_as(C.POINTER(C.c_float))

        def ip(a):
            a = _i32(a)
            keep.append(a)
            return a.ctypes.data_as(C.POINTER(C.c_int32))
        m = _lib.Model()
        m.num_verts = self.nv
        m.num_faces = int(model['faces'].shape[0]) if model.get('faces') is not None else 0
        m.v_template = fp(model['v_template'])
        m.shapedirs = fp(model['shapedirs'])
        m.posedirs = fp(model['posedirs'])
        m.J_regressor = fp(model['J_regressor'])
        m.parents = ip(model['parents'])
        m.lbs_weights = fp(model['lbs_weights'])
        # None: model_type 'smpl' - joint_map then indexes the posed skeleton joints + face vertices (include/mvfit.h)
        m.kp_regressor = fp(model['kp_regressor']) if model.get('kp_regressor') is not None else None
        m.face_vertex_ids = ip(model['face_vertex_ids'])
        m.joint_map = ip(model['joint_map'])
        m.faces = ip(model['faces']) if model.get('faces') is not None else None
        if vposer is not None:
            m.vp_fc1_w = fp(vposer['fc1_w']); m.vp_fc1_b = fp(vposer['fc1_b'])
            m.vp_fc2_w = fp(vposer['fc2_w']); m.vp_fc2_b = fp(vposer['fc2_b'])
            m.vp_out_w = fp(vposer['out_w']); m.vp_out_b = fp(vposer['out_b'])
        if gmm is not None:
            means, prec, nllw = gmm
            m.gmm_M = int(means.shape[0])
            m.gmm_means = fp(means); m.gmm_precisions = fp(prec); m.gmm_nll_weights = fp(nllw)
        self.has_vposer = vposer is not None
        self.has_gmm = gmm is not None
        self.faces = _i32(model['faces']) if model.get('faces') is not None else None     # (what the scene term voxelises)
        ctx = C.c_void_p()
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            o = self._options_struct(dict(DEFAULT_OPTIONS, **(options or {})))
            rc = self._lib.mvfit_create_ex(C.byref(ctx), device, C.c_void_p(stream), C.byref(m), C.byref(o))
        self._ctx = ctx
        self._check(rc)
        self.B = 0
        self.V = 0
        self._obstacles = False
        self._sil_term = False
        self._vt_term = False
        self._mix = None                         # the shares of set_term_mix while it is on
        self._scan_shape = None                  # (N, Pmax) of set_scans while a scan set is present
        self._scan_term = False
        self._lm_L = 0                           # landmarks of set_landmarks while a table is present
        self._lm_term = False

    # ------------------------------------------------------------------ options (include/mvfit.h:mvfit_options)
    def _options_struct(self, values: dict, base=None):
        o = _lib.Options()
        if base is None:
            self._lib.mvfit_options_default(C.byref(o))
        else:
            C.memmove(C.byref(o), C.byref(base), C.sizeof(o))
        names = {f[0] for f in _lib.Options._fields_} - {'struct_size'}
        for k, v in values.items():
            if k not in names:
                raise MvFitError('unknown option %r (mvfit_options has %s)' % (k, sorted(names)))
            if k == 'contraction' and isinstance(v, str):
                v = CONTRACTIONS[v]
            setattr(o, k, int(v))
        return o

    def options(self) -> dict:
        o = _lib.Options()
        self._check(self._lib.mvfit_get_options(self._ctx, C.byref(o)))
        return {f[0]: int(getattr(o, f[0])) for f in _lib.Options._fields_ if f[0] != 'struct_size'}

    def set_options(self, **values):
        """Change run-time selectors between calls (round_mode, resident_pass, sdf_two_phase, sdf_face_lists, vposer_helpers,
        vposer_sets, closure_vposer_helpers, pass_kernel, sdf_service, work_queue); returns the previous values of the ones
        changed."""
        cur = _lib.Options()
        self._check(self._lib.mvfit_get_options(self._ctx, C.byref(cur)))
        old = {k: int(getattr(cur, k)) for k in values}
        self._check(self._lib.mvfit_set_options(self._ctx, C.byref(self._options_struct(values, base=cur))))
        return old

    def sdf_info(self) -> dict:
        """Which path served the last sdf() call / the SDF term of the last fit: 'walk', 'face_lists', or
        'walk_workspace_did_not_fit' (include/mvfit.h:mvfit_sdf_info)."""
        a, b = C.c_int(), C.c_int()
        self._check(self._lib.mvfit_sdf_info(self._ctx, C.byref(a), C.byref(b)))
        names = ('walk', 'face_lists', 'walk_workspace_did_not_fit')
        return dict(op=names[a.value], term=names[b.value])

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc):
        if rc != 0:
            msg = self._lib.mvfit_last_error(self._ctx)
            raise MvFitError('libmvfit error %d: %s' % (rc, msg.decode() if msg else '?'))

    def close(self):
        if getattr(self, '_ctx', None):
            self._lib.mvfit_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _dev(self, a, shape=None):
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(_f32(a))
        t = t.to(device=self.device, dtype=torch.float32).contiguous()
        if shape is not None:
            assert tuple(t.shape) == tuple(shape), (tuple(t.shape), shape)
        return t

    @staticmethod
    def _weights(w: dict) -> _lib.Weights:
        return _lib.Weights(w['data_weight'], w['body_pose_weight'], w['shape_weight'],
                            w['bending_prior_weight'], w.get('coll_loss_weight', 0.0),
                            w.get('rho', 100.0), int(w.get('flags', 0)))

    def sync(self):
        self._check(self._lib.mvfit_sync(self._ctx))

    # ------------------------------------------------------------------ inputs
    def set_problems(self, cams, gt_xy, w_conf):
        """cams = (R[V,3,3] | [B,V,3,3], t, f, c); gt_xy[B,V,17,2]; w_conf[B,V,17]."""
        cam_R, cam_t, cam_f, cam_c = cams
        gt = self._dev(gt_xy)
        B, V = int(gt.shape[0]), int(gt.shape[1])
        wc = self._dev(w_conf, (B, V, 17))
        if B != self.B or V != self.V:           # hook buffers were sized for the old batch (the C side drops them too)
            if getattr(self, '_trace', None) is not None:
                self.fit_trace(0)
            if getattr(self, '_capture', None) is not None:
                self.capture_pass(None)
        batched = 1 if np.ndim(cam_R) == 4 else 0
        R, t, f, c = self._dev(cam_R), self._dev(cam_t), self._dev(cam_f), self._dev(cam_c)
        self._check(self._lib.mvfit_set_problems(
            self._ctx, B, V, batched, R.data_ptr(), t.data_ptr(), f.data_ptr(), c.data_ptr(),
            gt.data_ptr(), wc.data_ptr()))
        if B != self.B or V != self.V:
            self._obstacles = False              # (the C side drops them with the batch they were frozen for)
            self._sil_term = False               # (and switches the silhouette term off)
            self._vt_term = False                # (and clears the vertex targets with their term)
            self._mix = None                     # (and switches the term mix off)
            self._scan_term = False              # (and the scan term; the scan set stays)
            self._lm_term = False                # (and the landmark targets with their term; the table stays)
        self.B, self.V = B, V

    def set_joints3d(self, gt3d, conf3d):
        """use_3d targets: gt3d[B,17,3], conf3d[B,17] (reference non_linear_solver.py:86-99)."""
        g = self._dev(gt3d, (self.B, 17, 3))
        c = self._dev(conf3d, (self.B, 17))
        self._check(self._lib.mvfit_set_joints3d(self._ctx, g.data_ptr(), c.data_ptr()))

    # ------------------------------------------------------------------ compute
    def closure(self, params, weights: dict, want_grad=True, want_verts=False, want_joints=False):
        """One closure evaluation of all B problems.  params [B,118] (tensor or array).
        Returns dict(loss[B], grad[B,118]?, verts[B,Nv,3]?, joints[B,17,3]?) of CUDA tensors."""
        x = self._dev(params, (self.B, D))
        out = dict(loss=torch.empty(self.B, device=self.device, dtype=torch.float32))
        grad = torch.empty(self.B, D, device=self.device) if want_grad else None
        verts = torch.empty(self.B, self.nv, 3, device=self.device) if want_verts else None
        joints = torch.empty(self.B, 17, 3, device=self.device) if want_joints else None
        w = self._weights(weights)
        self._check(self._lib.mvfit_closure(
            self._ctx, C.byref(w), x.data_ptr(), out['loss'].data_ptr(),
            grad.data_ptr() if want_grad else None, verts.data_ptr() if want_verts else None,
            joints.data_ptr() if want_joints else None))
        if want_grad:
            out['grad'] = grad
        if want_verts:
            out['verts'] = verts
        if want_joints:
            out['joints'] = joints
        return out

    def vertices(self, params, flags=0):
        x = self._dev(params, (self.B, D))
        verts = torch.empty(self.B, self.nv, 3, device=self.device)
        joints = torch.empty(self.B, 17, 3, device=self.device)
        self._check(self._lib.mvfit_vertices(self._ctx, x.data_ptr(), flags, verts.data_ptr(),
                                             joints.data_ptr()))
        return verts, joints

    def vertices_backward(self, params, grad_verts=None, grad_joints=None, flags=0):
        """Vector-Jacobian product of vertices(params, flags) (include/mvfit.h:mvfit_vertices_backward): the cotangents
        grad_verts[B,Nv,3] / grad_joints[B,17,3] (None = zero) -> grad[B,118] (CUDA tensor)."""
        x = self._dev(params, (self.B, D))
        gv = None if grad_verts is None else self._dev(grad_verts, (self.B, self.nv, 3))
        gj = None if grad_joints is None else self._dev(grad_joints, (self.B, 17, 3))
        out = torch.empty(self.B, D, device=self.device)
        self._check(self._lib.mvfit_vertices_backward(self._ctx, x.data_ptr(), int(flags),
                                                      None if gv is None else gv.data_ptr(),
                                                      None if gj is None else gj.data_ptr(), out.data_ptr()))
        return out

    def full_pose(self, params, flags=0):
        """ModelOutput.full_pose [B,72] = global_orient | body_pose (decoded from the embedding with F_VPOSER):
        include/mvfit.h:mvfit_full_pose."""
        x = self._dev(params, (self.B, D))
        out = torch.empty(self.B, 72, device=self.device)
        self._check(self._lib.mvfit_full_pose(self._ctx, x.data_ptr(), int(flags), out.data_ptr()))
        return out

    def fit(self, params, stages, lr=1.0, max_iter=30, history=100, tolerance_grad=1e-5,
            tolerance_change=1e-9, maxiters=30, ftol=1e-9, gtol=1e-9, max_rounds=0):
        """Device-resident staged fit.  params [B,118] -> (params_out tensor, stats dict)."""
        x = self._dev(params, (self.B, D)).clone()
        arr = (_lib.Weights * len(stages))(*[self._weights(s) for s in stages])
        o = _lib.LbfgsOpts(lr, max_iter, history, tolerance_grad, tolerance_change, maxiters, ftol,
                           gtol, len(stages), max_rounds)
        final = torch.empty(self.B, device=self.device)
        ncl = torch.empty(self.B, device=self.device, dtype=torch.int32)
        nit = torch.empty(self.B, device=self.device, dtype=torch.int32)
        rc = self._lib.mvfit_fit(self._ctx, arr, C.byref(o), x.data_ptr(), final.data_ptr(),
                                 ncl.data_ptr(), nit.data_ptr())
        self._check(rc)
        st4 = (C.c_uint32 * 4)()
        self._check(self._lib.mvfit_fit_stats(self._ctx, st4))
        stats = dict(final_loss=final, n_closure=ncl, n_iter=nit,
                     passes=dict(run=int(st4[0]), skipped=int(st4[1]), missed=int(st4[2]), timed_out=int(st4[3])))
        if stats['passes']['missed'] or stats['passes']['timed_out']:
            # never silent: "every closure round got its full vertex pass" does not hold for this fit (the fitted parameters
            # do not depend on the passes - they consume what the optimiser publishes - but the per-round vertices do)
            warnings.warn('vertex passes degraded in this fit: %d lost their operands before reading them, %d gave up waiting '
                          'for them (is the GPU shared, or were the pass workgroups not all resident?)'
                          % (stats['passes']['missed'], stats['passes']['timed_out']), RuntimeWarning)
        if any(float(dict(s).get('coll_loss_weight', 0.0)) > 0.0 for s in stages) and \
                self.sdf_info()['term'] == 'walk_workspace_did_not_fit':
            warnings.warn(_SDF_WALK_WARNING % 'the SDF term of this fit', RuntimeWarning)
        if any(int(dict(s).get('flags', 0)) & _lib.F_VPOSER for s in stages):
            # decoder helpers (vposer_service.h): an answer that timed out makes that problem decode in its own workgroup
            # from then on - another summation order, i.e. last-bit differences from run to run.  Never silent.
            dec = self.decoder_stats()
            stats['decoder'] = dec
            if dec['answers_timed_out'] or dec['helpers_gave_up']:
                warnings.warn('VPoser decoder helpers degraded in this fit (%d answers timed out, %d helpers gave up): the '
                              'affected problems decoded locally (results differ in the last bits; is the GPU shared?)'
                              % (dec['answers_timed_out'], dec['helpers_gave_up']), RuntimeWarning)
        return x, stats

    def decoder_stats(self):
        """Counters of the VPoser decoder helpers of the last fit (include/mvfit.h:mvfit_decoder_stats): launches that
        carried helpers, answers that timed out, helpers that gave up (both expected 0).  Waits for the fit."""
        st3 = (C.c_uint32 * 3)()
        self._check(self._lib.mvfit_decoder_stats(self._ctx, st3))
        return dict(launches=int(st3[0]), answers_timed_out=int(st3[1]), helpers_gave_up=int(st3[2]))

    def fit_trace(self, max_closures=0):
        """Record (x_trial[118], loss) of the first ``max_closures`` closure calls of every problem during the next
        fits (include/mvfit.h:mvfit_fit_trace); returns the [B, max_closures, 119] tensor (NaN where nothing was
        written).  ``max_closures=0`` switches tracing off."""
        if max_closures <= 0:
            self._check(self._lib.mvfit_fit_trace(self._ctx, None, 0))
            self._trace = None
            return None
        self._trace = torch.full((self.B, int(max_closures), D + 1), float('nan'), device=self.device)
        self._check(self._lib.mvfit_fit_trace(self._ctx, self._trace.data_ptr(), int(max_closures)))
        return self._trace

    def capture_pass(self, round_index=None):
        """Test hook (include/mvfit.h:mvfit_debug_capture_pass): the vertex pass of closure round ``round_index`` of
        the next asynchronous fits writes into the returned [B, Nv, 3] tensor.  None switches it off."""
        if round_index is None:
            self._check(self._lib.mvfit_debug_capture_pass(self._ctx, -1, None))
            self._capture = None
            return None
        self._capture = torch.full((self.B, self.nv, 3), float('nan'), device=self.device)
        self._check(self._lib.mvfit_debug_capture_pass(self._ctx, int(round_index), self._capture.data_ptr()))
        return self._capture

    def sdf(self, faces, vertices, grid_size=32):
        """phi[B,G,G,G] of the SDF voxelisation op (include/mvfit.h:mvfit_sdf).  faces: int tensor whose
        size(0) is taken as the number of triangles, like the reference binding does."""
        f = faces if isinstance(faces, torch.Tensor) else torch.as_tensor(np.asarray(faces))
        f = f.to(device=self.device, dtype=torch.int32).contiguous()
        v = self._dev(vertices)
        if v.dim() != 3 or v.shape[2] != 3:
            raise MvFitError('vertices must be [B, Nv, 3]')
        phi = torch.zeros(v.shape[0], grid_size, grid_size, grid_size, device=self.device)
        self._check(self._lib.mvfit_sdf(self._ctx, f.data_ptr(), int(f.shape[0]), v.data_ptr(), int(v.shape[0]),
                                        int(v.shape[1]), int(grid_size), phi.data_ptr()))
        if self.sdf_info()['op'] == 'walk_workspace_did_not_fit':
            warnings.warn(_SDF_WALK_WARNING % 'this mvfit_sdf call', RuntimeWarning)
        return phi

    def scene_sdf_loss(self, vertices, faces, scene_sizes=None, grid_size=32, scale_factor=0.2, robustifier=None,
                       need_grad=True, return_phi=False):
        """The scene collision loss between bodies (include/mvfit.h:mvfit_scene_sdf_loss; the reference's SDFLoss.forward).
        vertices[N,Nv,3] with the translation added; faces[F,3]; scene_sizes: bodies per scene, in order (None: all N bodies
        are one scene).  Returns (loss[S], g_vertices[N,Nv,3] or None, phi[N,G,G,G] or None): g_vertices is
        d loss[scene of the body] / d vertices."""
        f = faces if isinstance(faces, torch.Tensor) else torch.as_tensor(np.asarray(faces).astype(np.int64))
        f = f.to(device=self.device, dtype=torch.int32).contiguous()
        v = self._dev(vertices)
        if v.dim() != 3 or v.shape[2] != 3:
            raise MvFitError('vertices must be [N, Nv, 3]')
        if f.dim() != 2 or f.shape[1] != 3:
            raise MvFitError('faces must be [F, 3]')
        N = int(v.shape[0])
        sizes = [N] if scene_sizes is None else [int(n) for n in scene_sizes]
        if sum(sizes) != N:
            raise MvFitError('scene_sizes %r do not add up to the %d bodies' % (sizes, N))
        first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        G = int(grid_size)
        loss = torch.zeros(len(sizes), device=self.device)
        g = torch.zeros_like(v) if need_grad else None
        phi = torch.zeros(N, G, G, G, device=self.device) if return_phi else None
        self._check(self._lib.mvfit_scene_sdf_loss(
            self._ctx, v.data_ptr(), int(v.shape[1]), f.data_ptr(), int(f.shape[0]), first.ctypes.data_as(_lib._ip), len(sizes), G,
            float(scale_factor), float(robustifier) if robustifier else 0.0, loss.data_ptr(),
            g.data_ptr() if need_grad else None, phi.data_ptr() if return_phi else None))
        return loss, g, phi

    def set_scene_obstacles(self, vertices, scene_sizes, grid_size=32, scale_factor=0.2, robustifier=None):
        """Freeze the other bodies of every scene as obstacles of the fit (include/mvfit.h:mvfit_set_scene_obstacles).
        vertices[B,Nv,3] (world) of the B problems of set_problems; scene_sizes: problems per scene, in order (they add up to
        B).  While set, a stage with coll_loss_weight w > 0 adds (w * S_j)^2 to problem j in closure() and fit(), S_j = the
        samples of j's vertices in the frozen fields of the other bodies of its scene (the model's own faces)."""
        v = self._dev(vertices)
        if v.dim() != 3 or v.shape[0] != self.B or v.shape[1] != self.nv or v.shape[2] != 3:
            raise MvFitError('vertices must be [B, %d, 3] with B = %d' % (self.nv, self.B))
        first = np.concatenate([[0], np.cumsum([int(n) for n in scene_sizes])]).astype(np.int32)
        self._check(self._lib.mvfit_set_scene_obstacles(
            self._ctx, v.data_ptr(), first.ctypes.data_as(_lib._ip), len(first) - 1, int(grid_size), float(scale_factor),
            float(robustifier) if robustifier else 0.0))
        self._obstacles = True
        self._obstacle_grid = int(grid_size)

    def scene_obstacles(self):
        """Diagnostics: (phi [B,G,G,G], boxes [B,4] = centre and scale) of the frozen obstacles."""
        box = torch.empty(self.B, 4, device=self.device)
        self._check(self._lib.mvfit_scene_obstacles_read(self._ctx, None, box.data_ptr()))
        G = self._obstacle_grid
        phi = torch.empty(self.B, G, G, G, device=self.device)
        self._check(self._lib.mvfit_scene_obstacles_read(self._ctx, phi.data_ptr(), None))
        return phi, box

    def clear_scene_obstacles(self):
        """Remove the obstacles of set_scene_obstacles."""
        self._check(self._lib.mvfit_set_scene_obstacles(self._ctx, None, None, 0, 0, 0.0, 0.0))
        self._obstacles = False
        if self._mix and self._mix[0] > 0:
            self._mix = None                     # (no obstacles, no mix that uses them)

    # ------------------------------------------------------------------ silhouette term (include/mvfit.h:mvfit_set_silhouettes)
    def set_silhouettes(self, masks, image_body, cams, contour_stride=1):
        """Prepare a mask set (include/mvfit.h:mvfit_set_silhouettes): masks uint8 [M,H,W] (tensor or array, non-zero = on),
        image_body[M] = the body every image shows, cams = (R[M,3,3], t[M,3], f[M], c[M,2]) per image.  Distance fields and
        contour lists stay in the engine until clear_silhouettes() or the next set."""
        if isinstance(masks, torch.Tensor):
            m = masks.to(device=self.device, dtype=torch.uint8).contiguous()
        else:
            m = torch.from_numpy(np.ascontiguousarray(np.asarray(masks), dtype=np.uint8)).to(self.device)
        if m.dim() != 3:
            raise MvFitError('masks must be [M, H, W], got %r' % (tuple(m.shape),))
        M, H, W = (int(n) for n in m.shape)
        body = _i32(np.asarray(image_body).reshape(-1))
        R, t, f, c = (_f32(a) for a in cams)
        if body.size != M or R.shape != (M, 3, 3) or t.shape != (M, 3) or f.reshape(-1).shape != (M,) or c.shape != (M, 2):
            raise MvFitError('image_body and cams need one entry per image (%d)' % M)
        if M == 0:
            return self.clear_silhouettes()
        fp = C.POINTER(C.c_float)
        rc = self._lib.mvfit_set_silhouettes(
            self._ctx, M, H, W, m.data_ptr(), body.ctypes.data_as(_lib._ip), R.ctypes.data_as(fp), t.ctypes.data_as(fp),
            f.ctypes.data_as(fp), c.ctypes.data_as(fp), int(contour_stride))
        if rc:
            self._sil_term = False               # (a set that fails, or does not fit an enabled term, switches the term off)
        self._check(rc)
        self._sil_shape = (M, H, W)

    def clear_silhouettes(self):
        """Remove the mask set of set_silhouettes."""
        self._check(self._lib.mvfit_set_silhouettes(self._ctx, 0, 0, 0, None, None, None, None, None, None, 1))
        self._sil_term = False                   # (no masks, no term: the C side switches it off)
        if self._mix and self._mix[1] > 0:
            self._mix = None

    def set_silhouette_term(self, w_in=1.0, w_out=1.0, sigma=0.0):
        """Make the silhouette loss of the current mask set a term of closure() and fit() (include/mvfit.h:
        mvfit_set_silhouette_term): a stage with coll_loss_weight w > 0 adds w^2 * L_j to problem j, L_j = silhouette_loss of
        the trial point's vertices (image_body = the problem index), with its gradient through the model.  fit() runs such
        stages as chained rounds.  Needs set_problems and set_silhouettes; excludes set_sdf's term and scene obstacles."""
        self._check(self._lib.mvfit_set_silhouette_term(self._ctx, 1, float(w_in), float(w_out), float(sigma)))
        self._sil_term = True

    def clear_silhouette_term(self):
        """Switch the term of set_silhouette_term off (the mask set stays)."""
        self._check(self._lib.mvfit_set_silhouette_term(self._ctx, 0, 0.0, 0.0, 0.0))
        self._sil_term = False

    def silhouettes(self):
        """Diagnostics: (field [M,H,W] float32, contour_first [M+1] int32, contour_xy [C,2] int32) of the mask set."""
        n = C.c_int32(0)
        self._check(self._lib.mvfit_silhouettes_read(self._ctx, None, None, None, C.byref(n)))
        M, H, W = self._sil_shape
        field = torch.empty(M, H, W, device=self.device)
        first = torch.empty(M + 1, dtype=torch.int32, device=self.device)
        xy = torch.empty(int(n.value), 2, dtype=torch.int32, device=self.device)
        self._check(self._lib.mvfit_silhouettes_read(self._ctx, field.data_ptr(), first.data_ptr(),
                                                     xy.data_ptr() if n.value else None, C.byref(n)))
        return field, first, xy

    def silhouette_loss(self, vertices, w_in=1.0, w_out=1.0, sigma=0.0, need_grad=True, return_winner=False):
        """The silhouette loss of the mask set at vertices[N,Nv,3], translation included (include/mvfit.h:
        mvfit_silhouette_loss): w_in weighs the body-inside-mask term, w_out the mask-covered-by-body term, sigma > 0 makes
        both robust.  Returns (loss[N], g_vertices[N,Nv,3] or None) and, with return_winner, the int32 [C] nearest projected
        vertex of every kept contour point (-1: none)."""
        v = self._dev(vertices)
        if v.dim() != 3 or v.shape[1] != self.nv or v.shape[2] != 3:
            raise MvFitError('vertices must be [N, %d, 3], got %r' % (self.nv, tuple(v.shape)))
        N = int(v.shape[0])
        loss = torch.empty(N, device=self.device)
        g = torch.empty_like(v) if need_grad else None
        win = None
        if return_winner:
            n = C.c_int32(0)
            self._check(self._lib.mvfit_silhouettes_read(self._ctx, None, None, None, C.byref(n)))
            win = torch.empty(max(int(n.value), 1), dtype=torch.int32, device=self.device)
        self._check(self._lib.mvfit_silhouette_loss(self._ctx, v.data_ptr(), N, float(w_in), float(w_out), float(sigma),
                                                    loss.data_ptr(), g.data_ptr() if need_grad else None,
                                                    win.data_ptr() if return_winner else None))
        if return_winner:
            return loss, g, win[:int(n.value)]
        return loss, g

    # -------------------------------------------- occlusion between bodies (include/mvfit.h:mvfit_set_silhouette_occluders)
    def set_silhouette_occluders(self, vertices, body_scene, margin=0.02):
        """Freeze the other bodies of every scene as occluder depth maps per mask image (include/mvfit.h:
        mvfit_set_silhouette_occluders): vertices [N,Nv,3], body_scene [N] int (bodies with the same value >= 0 occlude one
        another in each other's images; < 0: no occluders), margin in the cameras' depth unit.  While they are set,
        silhouette_loss, closure and fit ignore what the maps hide.  They go with the mask set: every set_silhouettes or
        clear_silhouettes removes them."""
        v = self._dev(vertices)
        if v.dim() != 3 or v.shape[1] != self.nv or v.shape[2] != 3:
            raise MvFitError('vertices must be [N, %d, 3], got %r' % (self.nv, tuple(v.shape)))
        scene = _i32(np.asarray(body_scene).reshape(-1))
        if scene.size != int(v.shape[0]):
            raise MvFitError('body_scene needs one entry per body (%d), got %d' % (int(v.shape[0]), scene.size))
        self._check(self._lib.mvfit_set_silhouette_occluders(self._ctx, v.data_ptr(), int(v.shape[0]),
                                                             scene.ctypes.data_as(_lib._ip), float(margin)))

    def clear_silhouette_occluders(self):
        """Remove the occluders of set_silhouette_occluders (the mask set stays)."""
        self._check(self._lib.mvfit_set_silhouette_occluders(self._ctx, None, 0, None, 0.0))

    def silhouette_occluders(self):
        """Diagnostics: (z_occ [M,H,W] float32, z_own [M,H,W] float32, point_flag [C] uint8) of the frozen occluders; +inf
        where nothing covers the pixel sample."""
        n = C.c_int32(0)
        self._check(self._lib.mvfit_silhouettes_read(self._ctx, None, None, None, C.byref(n)))
        M, H, W = self._sil_shape
        z_occ = torch.empty(M, H, W, device=self.device)
        z_own = torch.empty(M, H, W, device=self.device)
        flag = torch.empty(max(int(n.value), 1), dtype=torch.uint8, device=self.device)
        self._check(self._lib.mvfit_silhouette_occluders_read(self._ctx, z_occ.data_ptr(), z_own.data_ptr(), flag.data_ptr()))
        return z_occ, z_own, flag[:int(n.value)]

    def silhouette_hidden(self, vertices):
        """uint8 [M,Nv]: 1 where vertex j of the image's body, at vertices [N,Nv,3], is valid and hidden by the image's
        occluders (include/mvfit.h:mvfit_silhouette_hidden); zeros without occluders."""
        v = self._dev(vertices)
        if v.dim() != 3 or v.shape[1] != self.nv or v.shape[2] != 3:
            raise MvFitError('vertices must be [N, %d, 3], got %r' % (self.nv, tuple(v.shape)))
        hidden = torch.empty(self._sil_shape[0], self.nv, dtype=torch.uint8, device=self.device)
        self._check(self._lib.mvfit_silhouette_hidden(self._ctx, v.data_ptr(), int(v.shape[0]), hidden.data_ptr()))
        return hidden

    # ------------------------------------------------------------------ scan loss (include/mvfit.h:mvfit_set_scans)
    def set_scans(self, points, count=None, weights=None):
        """Keep a scan set (include/mvfit.h:mvfit_set_scans): points [N,Pmax,3] world points (tensor or array; copied), count[N]
        = how many of a body's rows are points (None: all Pmax), weights [N,Pmax] finite and >= 0 (None: 1).  A row at or
        beyond count[n], or with weight 0, takes no part and may hold anything.  The set stays in the engine until
        clear_scans() or the next set; a second set of the same (N, Pmax) keeps the library's buffers."""
        p = self._dev(points)
        if p.dim() != 3 or p.shape[2] != 3:
            raise MvFitError('points must be [N, Pmax, 3], got %r' % (tuple(p.shape),))
        N, Pmax = int(p.shape[0]), int(p.shape[1])
        if N == 0:
            return self.clear_scans()
        cnt = np.full(N, Pmax, np.int32) if count is None else _i32(np.asarray(count).reshape(-1))
        if cnt.size != N:
            raise MvFitError('count needs one entry per body (%d), got %d' % (N, cnt.size))
        w = None
        if weights is not None:
            w = weights.detach().cpu().numpy() if isinstance(weights, torch.Tensor) else weights
            w = _f32(np.asarray(w))
            if w.shape != (N, Pmax):
                raise MvFitError('weights must be [%d, %d], got %r' % (N, Pmax, tuple(w.shape)))
        rc = self._lib.mvfit_set_scans(self._ctx, N, Pmax, p.data_ptr(), cnt.ctypes.data_as(_lib._ip),
                                       w.ctypes.data_as(_lib._fp) if w is not None else None)
        if rc and self._scan_term and (N != self.B or rc != -1):
            self._scan_term = False              # (a set that fails, or does not fit an enabled term, switches the term off)
        if rc and self._mix_scan() and (N != self.B or rc != -1):
            self._mix = None                     # (and a mix that gives the scan a share)
        self._check(rc)
        self._scan_shape = (N, Pmax)

    def clear_scans(self):
        """Remove the scan set of set_scans."""
        self._check(self._lib.mvfit_set_scans(self._ctx, 0, 0, None, None, None))
        self._scan_shape = None
        self._scan_term = False                  # (no scans, no term: the C side switches it off)
        if self._mix_scan():
            self._mix = None                     # (and no mix that uses them)

    def _mix_scan(self):
        return bool(self._mix) and len(self._mix) > 3 and self._mix[3] > 0

    def set_scan_term(self, w_s2m=1.0, w_m2s=0.0, sigma=0.0):
        """Make the scan loss of the current scan set a term of closure() and fit() (include/mvfit.h:mvfit_set_scan_term): a
        stage with coll_loss_weight w > 0 adds w^2 * L_j to problem j, L_j = scan_loss(w_s2m, w_m2s, sigma) of the trial
        point's vertices (scan body j is problem j), with its gradient through the model.  fit() runs such stages as chained
        rounds.  Needs set_problems and a scan set of B bodies; excludes set_sdf's term, scene obstacles, the silhouette and
        vertex-target terms and the term mix.  A second call with other scalars replaces them."""
        self._check(self._lib.mvfit_set_scan_term(self._ctx, 1, float(w_s2m), float(w_m2s), float(sigma)))
        self._scan_term = True

    def clear_scan_term(self):
        """Switch the term of set_scan_term off (the scan set stays)."""
        self._check(self._lib.mvfit_set_scan_term(self._ctx, 0, 0.0, 0.0, 0.0))
        self._scan_term = False

    def scan_loss(self, vertices, w_s2m=1.0, w_m2s=0.0, sigma=0.0, need_grad=True, return_nearest=False, search='auto'):
        """The scan loss of the scan set at vertices[N,Nv,3], translation included (include/mvfit.h:mvfit_scan_loss): w_s2m
        weighs the squared distance of every scan point to the nearest point of the body's surface, w_m2s that of every
        vertex to its nearest scan point; sigma > 0 (in the vertices' unit) makes both robust.  search: 'auto' or
        'exhaustive' (the same bits).  Returns (loss[N], g_vertices[N,Nv,3] or None) and, with return_nearest, the int32
        nearest_face [N,Pmax] and nearest_point [N,Nv] (-1: none, or a term with weight 0)."""
        if search not in ('auto', 'exhaustive'):
            raise MvFitError("search must be 'auto' or 'exhaustive', got %r" % (search,))
        v = self._dev(vertices)
        if v.dim() != 3 or v.shape[1] != self.nv or v.shape[2] != 3:
            raise MvFitError('vertices must be [N, %d, 3], got %r' % (self.nv, tuple(v.shape)))
        N = int(v.shape[0])
        loss = torch.empty(N, device=self.device)
        g = torch.empty_like(v) if need_grad else None
        nf = npt = None
        if return_nearest:
            shape = self._scan_shape or (N, 1)
            nf = torch.empty(N, shape[1], dtype=torch.int32, device=self.device)
            npt = torch.empty(N, self.nv, dtype=torch.int32, device=self.device)
        self._check(self._lib.mvfit_scan_loss(self._ctx, v.data_ptr(), N, float(w_s2m), float(w_m2s), float(sigma),
                                              1 if search == 'exhaustive' else 0, loss.data_ptr(),
                                              g.data_ptr() if need_grad else None,
                                              nf.data_ptr() if return_nearest else None,
                                              npt.data_ptr() if return_nearest else None))
        if return_nearest:
            return loss, g, nf, npt
        return loss, g

    # ------------------------------------------------------------------ surface landmarks (include/mvfit.h:mvfit_set_landmarks)
    def set_landmarks(self, vertex_ids, weights=None):
        """Keep the landmark table (include/mvfit.h:mvfit_set_landmarks): vertex_ids [L,4] int and weights [L,4], landmark l at
        sum_k weights[l,k] * V[vertex_ids[l,k]]; fewer than 4 columns are padded with dead slots (weight 0, never read).  A 1-D
        vertex_ids means one vertex per landmark with weight 1.  1 <= L <= 256.  The table is independent of the problems; a
        new table clears the targets and the term."""
        ids = np.asarray(vertex_ids.detach().cpu().numpy() if isinstance(vertex_ids, torch.Tensor) else vertex_ids)
        if ids.ndim == 1 and weights is None:
            ids = ids.reshape(-1, 1)
            w = np.ones(ids.shape, np.float32)
        else:
            if weights is None:
                raise MvFitError('set_landmarks: weights are needed with vertex_ids of %d dimensions' % ids.ndim)
            w = np.asarray(weights.detach().cpu().numpy() if isinstance(weights, torch.Tensor) else weights, np.float32)
        if ids.ndim != 2 or ids.shape != w.shape or not 1 <= ids.shape[1] <= 4:
            raise MvFitError('set_landmarks: vertex_ids and weights must both be [L, 1..4], got %r and %r' % (ids.shape, w.shape))
        L, k = ids.shape
        ids4 = np.zeros((L, 4), np.int32); ids4[:, :k] = ids
        w4 = np.zeros((L, 4), np.float32); w4[:, :k] = w
        if L == 0:
            raise MvFitError('set_landmarks: an empty table (clear_landmarks() removes one)')
        rc = self._lib.mvfit_set_landmarks(self._ctx, L, ids4.ctypes.data_as(_lib._ip), w4.ctypes.data_as(_lib._fp))
        if rc != -1:                             # (set, or a failed allocation: no targets and no term; an argument error keeps all)
            self._lm_term = False
            self._lm_L = L if rc == 0 else 0
        self._check(rc)

    def clear_landmarks(self):
        """Remove the table of set_landmarks, the targets and the term."""
        self._check(self._lib.mvfit_set_landmarks(self._ctx, 0, None, None))
        self._lm_L = 0
        self._lm_term = False

    def set_landmark_targets(self, xy, conf, xyz=None, conf3=None):
        """The targets of the current problems (include/mvfit.h:mvfit_set_landmark_targets): xy [B,V,L,2] pixels and conf
        [B,V,L] finite and >= 0; optionally, together, xyz [B,L,3] world positions and conf3 [B,L].  An entry of confidence 0 is
        never read and may hold NaN.  A second call at the same sizes keeps the library's buffers (and the captured round
        graph)."""
        if (xyz is None) != (conf3 is None):
            raise MvFitError('set_landmark_targets: xyz and conf3 come together')
        L = self._lm_L
        t = [self._dev(xy, (self.B, self.V, L, 2)), self._dev(conf, (self.B, self.V, L))]
        if xyz is not None:
            t += [self._dev(xyz, (self.B, L, 3)), self._dev(conf3, (self.B, L))]
        p = [x.data_ptr() for x in t] + [None, None]
        rc = self._lib.mvfit_set_landmark_targets(self._ctx, p[0], p[1], p[2], p[3])
        if rc not in (0, -1, -3):                # (a failed allocation: no targets and no term)
            self._lm_term = False
        self._check(rc)

    def clear_landmark_targets(self):
        """Remove the targets of set_landmark_targets (and switch their term off); the table stays."""
        self._check(self._lib.mvfit_set_landmark_targets(self._ctx, None, None, None, None))
        self._lm_term = False

    def landmark_loss(self, vertices, rho=100.0, w3d=0.0, rho3d=0.0, need_grad=True):
        """The landmark loss at vertices[B,Nv,3], translation included (include/mvfit.h:mvfit_landmark_loss): the robust
        (GMoF, rho in pixels; 0: plain squares) reprojection error of every landmark in every view, weighted by conf^2, plus
        w3d times the same on the 3-D targets (rho3d in the vertices' unit).  Returns (loss[B], g_vertices[B,Nv,3] or None)."""
        v = self._dev(vertices)
        if tuple(v.shape) != (self.B, self.nv, 3):
            raise MvFitError('vertices must be [%d, %d, 3], got %r' % (self.B, self.nv, tuple(v.shape)))
        loss = torch.empty(self.B, device=self.device)
        g = torch.empty_like(v) if need_grad else None
        self._check(self._lib.mvfit_landmark_loss(self._ctx, v.data_ptr(), float(rho), float(w3d), float(rho3d), loss.data_ptr(),
                                                  g.data_ptr() if need_grad else None))
        return loss, g

    def set_landmark_term(self, rho=100.0, w3d=0.0, rho3d=0.0):
        """Make the landmark loss of the current targets a term of closure() and fit() (include/mvfit.h:
        mvfit_set_landmark_term): a stage with coll_loss_weight w > 0 adds w^2 * L_j to problem j, L_j = landmark_loss(rho, w3d,
        rho3d) of the trial point's vertices, with its gradient through the model.  fit() runs such stages as chained rounds.
        Needs set_landmark_targets; excludes set_sdf's term, scene obstacles, the silhouette, vertex-target and scan terms and
        the term mix.  A second call with other scalars replaces them."""
        self._check(self._lib.mvfit_set_landmark_term(self._ctx, 1, float(rho), float(w3d), float(rho3d)))
        self._lm_term = True

    def clear_landmark_term(self):
        """Switch the term of set_landmark_term off (table and targets stay)."""
        self._check(self._lib.mvfit_set_landmark_term(self._ctx, 0, 0.0, 0.0, 0.0))
        self._lm_term = False

    def round_graph_info(self, drop=False):
        """dict(builds = round graphs captured on this engine so far, occluder_buffers = the device addresses of z_occ, z_own
        and point_flag, 0 before the first freeze) (include/mvfit.h:mvfit_round_graph_info).  drop=True drops the captured
        graph first: the next fit with chained rounds captures a fresh one."""
        out = (C.c_uint64 * 4)()
        self._check(self._lib.mvfit_round_graph_info(self._ctx, 1 if drop else 0, out))
        return dict(builds=int(out[0]), occluder_buffers=(int(out[1]), int(out[2]), int(out[3])))

    def set_vertex_targets(self, targets, weights):
        """Target vertex sets of the vertex-target term (include/mvfit.h:mvfit_set_vertex_targets): targets [B,K,Nv,3]
        (tensor or array; copied), weights [B,K] finite and >= 0, 1 <= K <= 4.  A row whose weight is 0 is never read and may
        hold anything.  A second call with the same K keeps the library's buffers (and the captured round graph)."""
        t = self._dev(targets)
        if t.dim() != 4 or t.shape[0] != self.B or t.shape[2] != self.nv or t.shape[3] != 3:
            raise MvFitError('targets must be [%d, K, %d, 3], got %r' % (self.B, self.nv, tuple(t.shape)))
        K = int(t.shape[1])
        w = weights.detach().cpu().numpy() if isinstance(weights, torch.Tensor) else weights
        w = np.ascontiguousarray(np.asarray(w, np.float32).reshape(self.B, K))
        rc = self._lib.mvfit_set_vertex_targets(self._ctx, K, t.data_ptr() if K else None, w.ctypes.data_as(C.POINTER(C.c_float)))
        if K == 0 or rc not in (0, -1):          # (cleared, or a failed allocation: no set and no term; an argument error keeps both)
            self._vt_term = False
        self._check(rc)

    def clear_vertex_targets(self):
        """Remove the targets of set_vertex_targets (and switch their term off)."""
        self._check(self._lib.mvfit_set_vertex_targets(self._ctx, 0, None, None))
        self._vt_term = False
        if self._mix and self._mix[2] > 0:
            self._mix = None                     # (no targets, no mix that uses them: the C side switches it off)

    def vertex_target_loss(self, vertices, need_grad=True):
        """The vertex-target loss at vertices[B,Nv,3] (include/mvfit.h:mvfit_vertex_target_loss): L_j = sum_k a_jk
        ||V_j - T_jk||^2 and its vertex gradient 2 sum_k a_jk (V_j - T_jk).  Returns (loss[B], g_vertices[B,Nv,3] or None)."""
        v = self._dev(vertices)
        if tuple(v.shape) != (self.B, self.nv, 3):
            raise MvFitError('vertices must be [%d, %d, 3], got %r' % (self.B, self.nv, tuple(v.shape)))
        loss = torch.empty(self.B, device=self.device)
        g = torch.empty_like(v) if need_grad else None
        self._check(self._lib.mvfit_vertex_target_loss(self._ctx, v.data_ptr(), loss.data_ptr(),
                                                       g.data_ptr() if need_grad else None))
        return loss, g

    def set_vertex_target_term(self):
        """Make the vertex-target loss of the current targets a term of closure() and fit() (include/mvfit.h:
        mvfit_set_vertex_target_term): a stage with coll_loss_weight w > 0 adds w^2 * L_j to problem j, with its gradient
        through the model.  fit() runs such stages as chained rounds.  Needs set_problems and set_vertex_targets; excludes
        set_sdf's term, scene obstacles and the silhouette term."""
        self._check(self._lib.mvfit_set_vertex_target_term(self._ctx, 1))
        self._vt_term = True

    def clear_vertex_target_term(self):
        """Switch the term of set_vertex_target_term off (the targets stay)."""
        self._check(self._lib.mvfit_set_vertex_target_term(self._ctx, 0))
        self._vt_term = False

    # ------------------------------------------------------------------ term mix (include/mvfit.h:mvfit_set_term_mix)
    def set_term_mix(self, scene=0.0, silhouette=0.0, vertex_targets=0.0, w_in=1.0, w_out=1.0, sigma=0.0, scan=0.0, scan_w_s2m=1.0,
                     scan_w_m2s=0.0, scan_sigma=0.0):
        """Make a weighted sum of the scene, silhouette, vertex-target and scan terms the term of closure() and fit()
        (include/mvfit.h:mvfit_set_term_mix): a stage with coll_loss_weight w > 0 adds w^2 * (scene * S_sc^2 + silhouette *
        L_sil + vertex_targets * L_vt + scan * L_scan) to every problem.  At least two shares > 0, each with its data set in
        place (set_scene_obstacles / set_silhouettes / set_vertex_targets / set_scans with B bodies); w_in, w_out, sigma are
        the silhouette term's scalars, scan_w_s2m, scan_w_m2s, scan_sigma the scan term's."""
        m = _lib.TermMix(C.sizeof(_lib.TermMix), float(scene), float(silhouette), float(w_in), float(w_out), float(sigma),
                         float(vertex_targets), float(scan), float(scan_w_s2m), float(scan_w_m2s), float(scan_sigma))
        rc = self._lib.mvfit_set_term_mix(self._ctx, C.byref(m))
        if rc not in (0, -1, -3):                # (a failed allocation leaves no mix; a refusal keeps the one in place)
            self._mix = None
        self._check(rc)
        self._mix = (float(scene), float(silhouette), float(vertex_targets)) + ((float(scan),) if float(scan) > 0 else ())

    def clear_term_mix(self):
        """Switch the mix of set_term_mix off (the data sets stay)."""
        self._check(self._lib.mvfit_set_term_mix(self._ctx, None))
        self._mix = None

    def term_mix_read(self, scan=False):
        """[B,3]: S_sc^2, L_sil, L_vt of the mix's last evaluation, unweighted (0 for a share of 0); scan=True: [B,4], with
        L_scan behind them (include/mvfit.h:mvfit_term_mix_read4)."""
        parts = torch.empty(self.B, 4 if scan else 3, device=self.device)
        read = self._lib.mvfit_term_mix_read4 if scan else self._lib.mvfit_term_mix_read
        self._check(read(self._ctx, parts.data_ptr()))
        return parts

    def term_mix_cotangent(self, silhouette, g_sil, L_sil, vertex_targets, g_vt, L_vt):
        """The mix's cotangent kernel on the caller's buffers (include/mvfit.h:mvfit_term_mix_cotangent): (g [B,Nv,3], L_v [B]).
        The buffers of a component with share 0 may be None."""
        ptr = lambda t: None if t is None else t.data_ptr()
        g = torch.empty(self.B, self.nv, 3, device=self.device)
        L = torch.empty(self.B, device=self.device)
        self._check(self._lib.mvfit_term_mix_cotangent(self._ctx, float(silhouette), ptr(g_sil), ptr(L_sil), float(vertex_targets),
                                                       ptr(g_vt), ptr(L_vt), g.data_ptr(), L.data_ptr()))
        return g, L

    def term_mix_cotangent3(self, silhouette, g_sil, L_sil, vertex_targets, g_vt, L_vt, scan, g_scan, L_scan):
        """term_mix_cotangent with the scan as third component (include/mvfit.h:mvfit_term_mix_cotangent3)."""
        ptr = lambda t: None if t is None else t.data_ptr()
        g = torch.empty(self.B, self.nv, 3, device=self.device)
        L = torch.empty(self.B, device=self.device)
        self._check(self._lib.mvfit_term_mix_cotangent3(self._ctx, float(silhouette), ptr(g_sil), ptr(L_sil), float(vertex_targets),
                                                        ptr(g_vt), ptr(L_vt), float(scan), ptr(g_scan), ptr(L_scan), g.data_ptr(),
                                                        L.data_ptr()))
        return g, L

    def term_mix_merge(self, scene, rec_scene, rec_verts):
        """The mix's record kernel on the caller's records [B, TERM_RECORD_FLOATS] (include/mvfit.h:mvfit_term_mix_merge)."""
        a, b = self._dev(rec_scene), self._dev(rec_verts)
        if tuple(a.shape) != (self.B, _lib.TERM_RECORD_FLOATS) or a.shape != b.shape:
            raise MvFitError('records must be [%d, %d]' % (self.B, _lib.TERM_RECORD_FLOATS))
        out = torch.empty_like(a)
        self._check(self._lib.mvfit_term_mix_merge(self._ctx, float(scene), a.data_ptr(), b.data_ptr(), out.data_ptr()))
        return out

    def set_sdf(self, faces, num_faces=1, grid_size=128):
        """Configure the interpenetration term (include/mvfit.h:mvfit_set_sdf).  ``faces`` [F,3]; ``num_faces``
        = how many leading triangles the op sees: 1 reproduces the reference's call site
        (faces.reshape(1,-1,3), fitting.py:367-368), None = all of them.  faces=None removes the term."""
        if faces is None:
            self._check(self._lib.mvfit_set_sdf(self._ctx, None, 0, 0))
            return
        f = faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else np.asarray(faces)
        f = np.ascontiguousarray(f.reshape(-1, 3), dtype=np.int32)
        n = f.shape[0] if num_faces is None else int(num_faces)
        if n < 1 or n > f.shape[0]:
            raise MvFitError(f'num_faces={n} outside [1, {f.shape[0]}]')
        self._check(self._lib.mvfit_set_sdf(self._ctx, f.ctypes.data, n, int(grid_size)))

    def triangulate(self, keypoints, intris, extris):
        """joints3d [B,17,3] float64 from keypoints [B,V,17,3] (u, v, confidence) and the float64 camera matrices
        intris [V,3,3], extris [V,4,4] (include/mvfit.h:mvfit_triangulate; reference recompute3D)."""
        kp = self._dev(keypoints)
        if kp.dim() != 4 or kp.shape[2] != 17 or kp.shape[3] != 3:
            raise MvFitError('keypoints must be [B, V, 17, 3]')
        B, V = int(kp.shape[0]), int(kp.shape[1])
        K = torch.as_tensor(np.asarray(intris, np.float64) if not isinstance(intris, torch.Tensor) else intris,
                            dtype=torch.float64, device=self.device).contiguous()
        E = torch.as_tensor(np.asarray(extris, np.float64) if not isinstance(extris, torch.Tensor) else extris,
                            dtype=torch.float64, device=self.device).contiguous()
        if tuple(K.shape) != (V, 3, 3) or tuple(E.shape) != (V, 4, 4):
            raise MvFitError('intris must be [V,3,3] and extris [V,4,4] with V = %d' % V)
        out = torch.empty(B, 17, 3, dtype=torch.float64, device=self.device)
        self._check(self._lib.mvfit_triangulate(self._ctx, B, V, kp.data_ptr(), K.data_ptr(), E.data_ptr(), out.data_ptr()))
        return out

    def associate_views(self, keypoints, count, intris, extris, max_cost=0.05, min_joints=6, min_views=2, return_cost=False):
        """Which detections of a frame's views show the same person (include/mvfit.h:mvfit_associate_views).
        keypoints [F,V,Nmax,17,3] (u, v, confidence) in each view's own order, count [F,V] detections per view, the float64
        camera matrices intris [V,3,3], extris [V,4,4].  max_cost: the largest mean distance between the rays of two
        detections of one person, in world units (metres); min_joints: joints both detections must carry; min_views:
        detections a person needs.  Returns (labels [F,V,Nmax] int32: cluster number or -1, num_clusters [F] int32) and,
        with return_cost, the cost matrix [F,D,D] float64, D = V * Nmax."""
        kp = self._dev(keypoints)
        if kp.dim() != 5 or kp.shape[3] != 17 or kp.shape[4] != 3:
            raise MvFitError('keypoints must be [F, V, Nmax, 17, 3]')
        F, V, N = int(kp.shape[0]), int(kp.shape[1]), int(kp.shape[2])
        cnt = count if isinstance(count, torch.Tensor) else torch.as_tensor(np.asarray(count))
        cnt = cnt.to(device=self.device, dtype=torch.int32).contiguous()
        if tuple(cnt.shape) != (F, V):
            raise MvFitError('count must be [F, V] = [%d, %d]' % (F, V))
        K, E = self._f64(intris, (V, 3, 3)), self._f64(extris, (V, 4, 4))
        labels = torch.empty(F, V, N, dtype=torch.int32, device=self.device)
        num = torch.empty(F, dtype=torch.int32, device=self.device)
        cost = torch.empty(F, V * N, V * N, dtype=torch.float64, device=self.device) if return_cost else None
        self._check(self._lib.mvfit_associate_views(
            self._ctx, F, V, N, kp.data_ptr(), cnt.data_ptr(), K.data_ptr(), E.data_ptr(), float(max_cost), int(min_joints),
            int(min_views), cost.data_ptr() if return_cost else None, labels.data_ptr(), num.data_ptr()))
        return (labels, num, cost) if return_cost else (labels, num)

    def _cams15(self, cams):
        if isinstance(cams, (tuple, list)) and len(cams) == 4:
            cams = pack_cameras(cams)
        return self._f64(cams, (self.V, 15))

    def camera_normal_eqs(self, joints, cams15, rho=100., data_weight=1., need_grad=True):
        """Energy of the keypoint data term per view as a function of the view's camera, with its gradient and Gauss-Newton
        matrix over the 9 camera parameters (include/mvfit.h:mvfit_camera_normal_eqs).  joints [B,17,3] (closure(...,
        want_joints=True)), cams15 [V,15] float64 (pack_cameras) or the (R, t, f, c) tuple; gt_xy and w_conf are those of
        set_problems.  Returns dict(E[V], count[V] int32, g[V,9]?, H[V,9,9]?) of CUDA tensors, float64."""
        j = self._dev(joints, (self.B, 17, 3))
        cm = self._cams15(cams15)
        V = self.V
        out = dict(E=torch.empty(V, dtype=torch.float64, device=self.device),
                   count=torch.empty(V, dtype=torch.int32, device=self.device))
        g = torch.empty(V, 9, dtype=torch.float64, device=self.device) if need_grad else None
        H = torch.empty(V, 9, 9, dtype=torch.float64, device=self.device) if need_grad else None
        self._check(self._lib.mvfit_camera_normal_eqs(
            self._ctx, j.data_ptr(), cm.data_ptr(), float(rho), float(data_weight), out['E'].data_ptr(),
            g.data_ptr() if need_grad else None, H.data_ptr() if need_grad else None, out['count'].data_ptr()))
        if need_grad:
            out['g'], out['H'] = g, H
        return out

    def refine_cameras(self, joints, cams, free='extrinsics', fixed_views=(), max_iter=20, min_points=34, rho=100.,
                       data_weight=1., lambda0=1e-3, ftol=1e-12):
        """Move the cameras against held bodies: Levenberg-Marquardt per view on the device (include/mvfit.h:
        mvfit_refine_cameras).  joints [B,17,3]; cams: the (R, t, f, c) tuple of set_problems or a [V,15] array; free:
        'extrinsics' | 'extrinsics+focal' | 'all' (or the free_mask itself); fixed_views: views returned as given.  Returns
        (cams15 [V,15] float64 tensor, report [V,8] float64 tensor: E0, E1, it, acc, status, count, lam, 0)."""
        j = self._dev(joints, (self.B, 17, 3))
        cm = self._cams15(cams)
        if isinstance(free, str) and free not in FREE_MASKS:
            raise MvFitError('free must be one of %s, got %r' % (sorted(FREE_MASKS), free))
        mask = FREE_MASKS[free] if isinstance(free, str) else free
        fixed = 0
        for v in fixed_views:
            if not 0 <= int(v) < self.V:
                raise MvFitError('fixed view %r outside [0, %d)' % (v, self.V))
            fixed |= 1 << int(v)
        o = _lib.CameraRefineOpts(C.sizeof(_lib.CameraRefineOpts), int(mask), fixed, int(max_iter), int(min_points), float(rho),
                                  float(data_weight), float(lambda0), float(ftol))
        out = torch.empty(self.V, 15, dtype=torch.float64, device=self.device)
        report = torch.empty(self.V, 8, dtype=torch.float64, device=self.device)
        self._check(self._lib.mvfit_refine_cameras(self._ctx, j.data_ptr(), cm.data_ptr(), C.byref(o), out.data_ptr(),
                                                   report.data_ptr()))
        return out, report

    def depth_guess(self, rest_joints, extri, intri, keypoints):
        """joints3d [B,17,3] float64 for frames seen by ONE camera (include/mvfit.h:mvfit_depth_guess; reference
        init_guess.py:54-74): rest_joints [17,3] float64, extri [4,4], intri [3,3] float64, keypoints [B,17,3]
        (u, v, confidence)."""
        kp = self._dev(keypoints)
        if kp.dim() != 3 or kp.shape[1] != 17 or kp.shape[2] != 3:
            raise MvFitError('keypoints must be [B, 17, 3]')
        f64 = lambda a, shape: self._f64(a, shape)
        R_, E_, K_ = f64(rest_joints, (17, 3)), f64(extri, (4, 4)), f64(intri, (3, 3))
        B = int(kp.shape[0])
        out = torch.empty(B, 17, 3, dtype=torch.float64, device=self.device)
        self._check(self._lib.mvfit_depth_guess(self._ctx, B, R_.data_ptr(), E_.data_ptr(), K_.data_ptr(), kp.data_ptr(),
                                                out.data_ptr()))
        return out

    def _f64(self, a, shape):
        t = torch.as_tensor(np.asarray(a, np.float64) if not isinstance(a, torch.Tensor) else a, dtype=torch.float64,
                            device=self.device).contiguous()
        if tuple(t.shape) != tuple(shape):
            raise MvFitError('expected shape %s, got %s' % (tuple(shape), tuple(t.shape)))
        return t

    def umeyama(self, src, dst, estimate_scale=True):
        """The reference's similarity alignment + cv2.Rodrigues (include/mvfit.h:mvfit_umeyama): src [npts,3],
        dst [B,npts,3] float64 -> dict(rot [B,3,3], rvec [B,3], trans [B,3], scale [B]) float64 tensors."""
        s_ = torch.as_tensor(np.asarray(src, np.float64) if not isinstance(src, torch.Tensor) else src,
                             dtype=torch.float64, device=self.device).contiguous()
        d_ = torch.as_tensor(np.asarray(dst, np.float64) if not isinstance(dst, torch.Tensor) else dst,
                             dtype=torch.float64, device=self.device).contiguous()
        if s_.dim() != 2 or d_.dim() != 3 or d_.shape[1:] != s_.shape or s_.shape[1] != 3:
            raise MvFitError('src must be [npts,3] and dst [B,npts,3]')
        B, npts = int(d_.shape[0]), int(s_.shape[0])
        out = dict(rot=torch.empty(B, 3, 3, dtype=torch.float64, device=self.device),
                   rvec=torch.empty(B, 3, dtype=torch.float64, device=self.device),
                   trans=torch.empty(B, 3, dtype=torch.float64, device=self.device),
                   scale=torch.empty(B, dtype=torch.float64, device=self.device))
        self._check(self._lib.mvfit_umeyama(self._ctx, B, npts, s_.data_ptr(), d_.data_ptr(), 1 if estimate_scale else 0,
                                            out['rot'].data_ptr(), out['rvec'].data_ptr(), out['trans'].data_ptr(),
                                            out['scale'].data_ptr()))
        return out

    def project(self, points):
        """uv [B, V, N, 2] = every view's pinhole projection of points [B, N, 3] with the cameras of set_problems
        (include/mvfit.h:mvfit_project_points; reference cam(verts), utils/utils.py:603-607)."""
        p = self._dev(points)
        if p.dim() != 3 or p.shape[0] != self.B or p.shape[2] != 3:
            raise MvFitError('points must be [B, N, 3] with B = %d' % self.B)
        uv = torch.empty(self.B, self.V, int(p.shape[1]), 2, device=self.device)
        self._check(self._lib.mvfit_project_points(self._ctx, p.data_ptr(), int(p.shape[1]), uv.data_ptr()))
        return uv

    def _render_inputs(self, vertices, points, images):
        """Argument checks shared by render_overlay and render_scene -> (v, p or None, img on the device, n, H, W)."""
        v = self._dev(vertices)
        if v.dim() != 3 or v.shape[0] != self.B or v.shape[1] != self.nv or v.shape[2] != 3:
            raise MvFitError('vertices must be [B, %d, 3] with B = %d' % (self.nv, self.B))
        p = None
        if points is not None:
            p = self._dev(points)
            if p.dim() != 3 or p.shape[0] != self.B or p.shape[2] != 3:
                raise MvFitError('points must be [B, P, 3] with B = %d' % self.B)
        if isinstance(images, torch.Tensor):
            img = images
        else:
            a = np.ascontiguousarray(images)
            img = torch.from_numpy(a if a.flags.writeable else a.copy())     # (e.g. np.asarray of a PIL image)
        if img.dtype != torch.uint8 or img.dim() != 4 or img.shape[3] != 3:
            raise MvFitError('images must be uint8 [n, H, W, 3]')
        img = img.to(self.device).contiguous()
        n, H, W = int(img.shape[0]), int(img.shape[1]), int(img.shape[2])
        return v, p, img, n, H, W

    def _render_out(self, images, img, out):
        if out is None:
            out = torch.empty_like(img)
        elif out is images:
            if img is not images:
                raise MvFitError('out=images renders in place: images must be a contiguous uint8 tensor on %s' % self.device)
            out = img
        elif (out.dtype != torch.uint8 or tuple(out.shape) != tuple(img.shape) or out.device != self.device
              or not out.is_contiguous()):
            raise MvFitError('out must be a contiguous uint8 device tensor of the images\' shape')
        return out

    def render_overlay(self, vertices, points, images, problems, views, face_id=False, out=None):
        """The body drawn over each view's image with the keypoints as red dots (include/mvfit.h:mvfit_render_overlay;
        reference save_images, utils/utils.py:574-597,659-712,977-1028).  vertices [B, Nv, 3] (e.g. ``vertices()``),
        points [B, P, 3] (P <= 64) or None, images uint8 [n, H, W, 3] RGB (torch tensor or NumPy array); image i is problem
        problems[i] seen by view views[i] of set_problems' cameras.  Returns a uint8 device tensor [n, H, W, 3] (``out``:
        a contiguous uint8 tensor of that shape on this engine's device to write into; ``out=images`` renders in place and
        needs ``images`` to be such a tensor) and, with face_id, also the int32 [n, H, W] visible face per pixel (-1: none)."""
        v, p, img, n, H, W = self._render_inputs(vertices, points, images)
        prob, view = _i32(np.asarray(problems).reshape(-1)), _i32(np.asarray(views).reshape(-1))
        if prob.size != n or view.size != n:
            raise MvFitError('problems and views need one entry per image (%d)' % n)
        out = self._render_out(images, img, out)
        fid = torch.empty(n, H, W, dtype=torch.int32, device=self.device) if face_id else None
        ip = C.POINTER(C.c_int32)
        self._check(self._lib.mvfit_render_overlay(
            self._ctx, v.data_ptr(), p.data_ptr() if p is not None else None, int(p.shape[1]) if p is not None else 0, n,
            prob.ctypes.data_as(ip), view.ctypes.data_as(ip), H, W, img.data_ptr(), out.data_ptr(),
            fid.data_ptr() if face_id else None))
        return (out, fid) if face_id else out

    def render_scene(self, vertices, points, images, bodies, views, colors=None, face_id=False, body_id=False, out=None):
        """Several bodies per image, depth-tested against one another (include/mvfit.h:mvfit_render_scene): image i shows the
        problems ``bodies[i]`` (a list per image; may be empty) seen by view ``views[i]``, each in its own opaque colour -
        ``colors``: None (slot k of an image takes entry k mod 7 of SCENE_PALETTE), one [3] RGB triple in [0, 1] per body in
        the nesting of ``bodies``, or a flat [n_bodies, 3] array.  vertices, points, images, ``out`` and the in-place rule as
        render_overlay.  Returns out, then with face_id the int32 [n, H, W] visible face within its body and with body_id
        the slot of the visible body (both -1 where nothing is drawn)."""
        v, p, img, n, H, W = self._render_inputs(vertices, points, images)
        bodies = [list(np.asarray(b, np.int64).reshape(-1)) for b in bodies]
        view = _i32(np.asarray(views).reshape(-1))
        if len(bodies) != n or view.size != n:
            raise MvFitError('bodies and views need one entry per image (%d)' % n)
        first = _i32(np.concatenate([[0], np.cumsum([len(b) for b in bodies])]))
        total = int(first[-1])
        prob = _i32([b for lst in bodies for b in lst] or [0])
        col = None
        if colors is not None:
            try:
                col = np.asarray(colors, np.float32)
            except ValueError:                              # ragged: the nesting of ``bodies``
                col = None
            if col is None or col.shape != (total, 3):
                try:
                    col = np.concatenate([np.asarray(c_, np.float32).reshape(-1, 3) for c_ in colors]
                                         + [np.zeros((0, 3), np.float32)])
                except (ValueError, TypeError):
                    raise MvFitError('colors must hold one RGB triple per body (%d)' % total)
            if col.ndim != 2 or col.shape != (total, 3):
                raise MvFitError('colors must hold one RGB triple per body (%d)' % total)
            col = np.ascontiguousarray(col if total else np.zeros((1, 3), np.float32), np.float32)
        out = self._render_out(images, img, out)
        fid = torch.empty(n, H, W, dtype=torch.int32, device=self.device) if face_id else None
        bid = torch.empty(n, H, W, dtype=torch.int32, device=self.device) if body_id else None
        ip = C.POINTER(C.c_int32)
        self._check(self._lib.mvfit_render_scene(
            self._ctx, v.data_ptr(), p.data_ptr() if p is not None else None, int(p.shape[1]) if p is not None else 0, n,
            first.ctypes.data_as(ip), prob.ctypes.data_as(ip), view.ctypes.data_as(ip),
            col.ctypes.data_as(C.POINTER(C.c_float)) if col is not None else None, H, W, img.data_ptr(), out.data_ptr(),
            fid.data_ptr() if face_id else None, bid.data_ptr() if body_id else None))
        res = (out,) + ((fid,) if face_id else ()) + ((bid,) if body_id else ())
        return res if len(res) > 1 else out

    def gather(self, rccl_comm, send, nranks):
        """All-gather of a contiguous device tensor over a raw RCCL communicator (include/mvfit.h:mvfit_gather) - the
        entry point of hosts that own an ncclComm_t; the Python adapters use torch.distributed (sharding.py), which does
        not hand out its communicator.  rccl_comm: the ncclComm_t as an integer / c_void_p.  -> [nranks, *send.shape]."""
        s_ = send.contiguous()
        if not s_.is_cuda:
            raise MvFitError('send must be a device tensor')
        recv = torch.empty((int(nranks),) + tuple(s_.shape), dtype=s_.dtype, device=s_.device)
        self._check(self._lib.mvfit_gather(self._ctx, rccl_comm, s_.data_ptr(), recv.data_ptr(), s_.numel() * s_.element_size()))
        return recv

    def sdf_term_read(self):
        """(samples [B,Nv,4] = phi_v and its local-coordinate gradient, S [B]) of the last evaluated term.  The scene term
        (set_scene_obstacles) keeps no per-vertex samples: (None, S) while it is set; so does the silhouette term
        (set_silhouette_term), the vertex-target term (set_vertex_target_term), the scan term (set_scan_term) and the landmark term (set_landmark_term), whose S is
        the loss L_j itself, and the term mix (set_term_mix), whose S is the weighted sum of its parts."""
        smp = None if (self._obstacles or self._sil_term or self._vt_term or self._mix or self._scan_term or self._lm_term) else torch.empty(self.B, self.nv, 4, device=self.device)
        S = torch.empty(self.B, device=self.device)
        self._check(self._lib.mvfit_sdf_term_read(self._ctx, None if smp is None else smp.data_ptr(), S.data_ptr()))
        return smp, S

    # ------------------------------------------------------------------ profiling
    def profile(self, enable=True):
        self._check(self._lib.mvfit_profile(self._ctx, 1 if enable else 0))

    def profile_vertex_pass_ms(self, launches=64, as_in_async_fit=False):
        """Average duration (ms) of `launches` back-to-back vertex-pass launches inside one hipEvent pair;
        ``as_in_async_fit``: the launch flavour of the asynchronous fit (include/mvfit.h)."""
        a = C.c_double()
        self._check(self._lib.mvfit_profile_vertex_pass_ex(self._ctx, int(launches), 1 if as_in_async_fit else 0, C.byref(a)))
        return a.value

    def profile_resident_pass_ms(self, rounds=100):
        """Per-round time (ms) of the RESIDENT vertex pass alone: one launch serving ``rounds`` (<= 128) closure rounds whose
        operands the last asynchronous fit left in the ring, inside one hipEvent pair (include/mvfit.h, flavour 2)."""
        a = C.c_double()
        self._check(self._lib.mvfit_profile_vertex_pass_ex(self._ctx, int(rounds), 2, C.byref(a)))
        return a.value

    def pass_profile(self):
        """How the vertex passes of the last asynchronous fit ran (include/mvfit.h:mvfit_pass_profile)."""
        tpw, wgs, n = C.c_int(), C.c_int(), C.c_int()
        span, busy, slowest = C.c_double(), C.c_double(), C.c_double()
        self._check(self._lib.mvfit_pass_profile(self._ctx, C.byref(tpw), C.byref(wgs), C.byref(n), C.byref(span), C.byref(busy),
                                                 C.byref(slowest)))
        form = tpw.value               # 0 per-round launches; 1 one tile per workgroup; 3 two tiles, role-split (form 2 was dropped)
        kernel = {0: None, 1: 'lbs_vertex_pass_resident_kernel<1>', 3: 'lbs_vertex_pass_resident_roles_kernel'}[form]
        return dict(form=form, tiles_per_workgroup=2 if form == 3 else form, kernel=kernel, workgroups=wgs.value, rounds_stamped=n.value,
                    round_span_ms=span.value, workgroup_busy_ms=busy.value, slowest_workgroup_ms=slowest.value)

    def profile_read(self):
        a, b = C.c_double(), C.c_double()
        n1, n2 = C.c_int(), C.c_int()
        self._check(self._lib.mvfit_profile_read(self._ctx, C.byref(a), C.byref(n1), C.byref(b),
                                                 C.byref(n2)))
        return dict(vertex_pass_ms=a.value, vertex_pass_launches=n1.value,
                    step_ms=b.value, step_launches=n2.value)


# free_mask of mvfit_refine_cameras by name (bit 0: omega, 1: dt, 2: f, 3: c)
FREE_MASKS = {'extrinsics': 3, 'extrinsics+focal': 7, 'all': 15}


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def pack_cameras(cams):
    """The (R[V,3,3], t[V,3], f[V], c[V,2]) tuple of set_problems as [V,15] float64 rows R (9, row-major), t (3), f, cx, cy:
    the camera form of camera_normal_eqs / refine_cameras.  float32 values widen exactly."""
    R, t, f, c = (np.asarray(_host(a), np.float64) for a in cams)
    if R.ndim != 3:
        raise ValueError('pack_cameras takes one rig [V,3,3], not per-problem cameras')
    V = R.shape[0]
    return np.concatenate([R.reshape(V, 9), t.reshape(V, 3), f.reshape(V, 1), c.reshape(V, 2)], axis=1)


def unpack_cameras(cams15, dtype=np.float64):
    """The inverse of pack_cameras: [V,15] -> (R[V,3,3], t[V,3], f[V], c[V,2]) NumPy arrays of ``dtype``."""
    a = np.asarray(_host(cams15), np.float64)
    if a.ndim != 2 or a.shape[1] != 15:
        raise ValueError('cams15 must be [V, 15]')
    V = a.shape[0]
    return (a[:, :9].reshape(V, 3, 3).astype(dtype), a[:, 9:12].astype(dtype), a[:, 12].astype(dtype),
            a[:, 13:15].astype(dtype))


def pack_params(betas=None, global_orient=None, body_pose=None, transl=None, scale=None,
                pose_embedding=None, B=1):
    """Assemble [B,118] float32 from per-tensor arrays (missing ones: zeros, scale ones)."""
    x = np.zeros((B, D), np.float32)
    x[:, 85] = 1.0
    for name, val in (('betas', betas), ('global_orient', global_orient), ('body_pose', body_pose),
                      ('transl', transl), ('scale', scale), ('pose_embedding', pose_embedding)):
        if val is not None:
            a, b = SL[name]
            x[:, a:b] = np.asarray(val, np.float32).reshape(B, b - a)
    return x


def lbfgs_kat(kind: int, D_: int, segs, x0, max_trace=80, device=0, library=None, **opts):
    """Run the float64 device L-BFGS on an analytic objective (include/mvfit.h:mvfit_lbfgs_kat); library: another build
    of libmvfit."""
    lib = _lib.load(library)
    o = _lib.LbfgsOpts(opts.get('lr', 1.0), opts.get('max_iter', 30), opts.get('history', 100),
                       opts.get('tolerance_grad', 1e-5), opts.get('tolerance_change', 1e-9),
                       opts.get('maxiters', 30), opts.get('ftol', 1e-9), opts.get('gtol', 1e-9), 1, 0)
    x = np.ascontiguousarray(x0, np.float64).copy()
    trace = np.zeros((max_trace, D_ + 1), np.float64)
    sg = _i32(segs)
    n = C.c_int()
    fl = C.c_double()
    rc = lib.mvfit_lbfgs_kat(device, kind, D_, sg.ctypes.data_as(C.POINTER(C.c_int32)), len(sg) - 1,
                             C.byref(o), x.ctypes.data_as(C.POINTER(C.c_double)),
                             trace.ctypes.data_as(C.POINTER(C.c_double)), max_trace, C.byref(n),
                             C.byref(fl))
    if rc != 0:
        raise MvFitError('mvfit_lbfgs_kat failed: %d' % rc)
    return x, trace[:min(n.value, max_trace)], n.value, fl.value
