"""TEST INFRASTRUCTURE - writes tests/golden/*.npz by running the REFERENCE itself.

Run in the build container (needs the read-only reference tree):
    python -m oracle.make_golden
The GPU box never sees the reference, so these files are how reference behaviour
travels.  Inputs are regenerated from seeds by mvsmplfitting_amd.synthetic; only the
small per-problem arrays and the reference's outputs are stored.

Files
  lsp_regressor.npz       the shipped 14x6890 keypoint regressor as 81 triplets (data)
  closure_<case>.npz      x[B,D], cams, gt_xy, conf, weights -> reference loss / grad /
                          joints / vertices in float64 and float32
  lbfgs_kat.npz           reference LBFGS+run_fitting closure traces on analytic objectives
  lbfgs_kat_branches.npz  the same for the runs of tests/lbfgs_branch_cases.py, with the oracle's branch tags
  fit_<case>.npz          reference 4-stage fits (final params / loss / closure counts)
"""
from __future__ import annotations

import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from mvsmplfitting_amd import synthetic as syn          # noqa: E402
from oracle import closure_np as cn                      # noqa: E402
from oracle import lbfgs_np as ln                        # noqa: E402
from oracle import ref_import as ri                      # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')

# yaml stage weights (reference cfg_files/fit_smpl.yaml:40-68)
STAGE_POSE_W = [404.0, 404.0, 57.4, 4.78]
STAGE_SHAPE_W = [100.0, 50.0, 10.0, 5.0]
DATA_W = 500.0 / 1536.0


def stage_weights(stage: int, rho=100.0):
    wp = STAGE_POSE_W[stage]
    return dict(data_weight=DATA_W, body_pose_weight=wp, shape_weight=STAGE_SHAPE_W[stage],
                bending_prior_weight=3.17 * wp, rho=rho)


CASES = {
    # name: (use_vposer, prior, vposer kwargs, stage, V, param sigma, z sigma, skin_topk)
    'l2_s0_v8': dict(use_vposer=False, prior='l2', stage=0, V=8, sig=0.15),
    'l2_s3_v6': dict(use_vposer=False, prior='l2', stage=3, V=6, sig=0.4),
    'l2_top4_v8': dict(use_vposer=False, prior='l2', stage=2, V=8, sig=0.2, skin_topk=4),
    'gmm_s2_v8': dict(use_vposer=False, prior='gmm', stage=2, V=8, sig=0.15),
    'gmm_s3_v8': dict(use_vposer=False, prior='gmm', stage=3, V=8, sig=0.1),
    'vp_s0_v8': dict(use_vposer=True, prior='l2', stage=0, V=8, sig=0.15, zsig=1.0,
                     vp=dict(seed=11)),
    'vpwild_s2_v8': dict(use_vposer=True, prior='l2', stage=2, V=8, sig=0.1, zsig=1.0,
                         vp=dict(seed=12, gain=4.0, identity_bias=False)),
    'l2_fixshape_v8': dict(use_vposer=False, prior='l2', stage=1, V=8, sig=0.15, fix_shape=True),
    'l2_angle_drop_v8': dict(use_vposer=False, prior='l2', stage=0, V=8, sig=0.15, big_knee=True),
    'l2_3d_v8': dict(use_vposer=False, prior='l2', stage=1, V=8, sig=0.15, use_3d=True),
}
B_CASE = 4


def build_case(name, cfg, lsp):
    model = syn.make_body_model(0, skin_topk=cfg.get('skin_topk'), kp_regressor=lsp)
    cams = syn.make_camera_ring(cfg['V'])
    use_vp = cfg['use_vposer']
    vpw = syn.make_vposer_decoder(**cfg['vp']) if use_vp else None
    gmm = syn.make_gmm() if cfg['prior'] == 'gmm' else None
    orc = cn.ClosureOracle(model, np.float64, vposer=vpw,
                           gmm=None if gmm is None else syn.gmm_constants(gmm, np.float64))
    frames = syn.make_frames(B_CASE, seed0=2000 + sum(map(ord, name)))
    lay, D = cn.param_layout(use_vp)
    xs, gts, confs, j3s = [], [], [], []
    for b in range(B_CASE):
        p = {k: frames[k][b] for k in frames}
        p['use_vposer'] = False
        out = orc.body(p, want_cache=False)
        gt, cf = syn.make_observations(out['joints'][None], cams, seed=77 + b)
        gt, cf = gt[0], cf[0]
        if b == 1:
            cf[2] = 0.0            # a whole view with zero confidence (dropped view, main.py:49-57)
        rng = np.random.default_rng(9000 + b)
        x = rng.normal(0, cfg['sig'], D)
        x[lay['scale'][0]] = 1.0 + rng.normal(0, 0.1)
        x[lay['transl'][0]:lay['transl'][1]] = rng.normal(0, 0.05, 3)
        if use_vp:
            x[lay['pose_embedding'][0]:] = rng.normal(0, cfg['zsig'], 32)
        if cfg.get('big_knee') and b >= 2:
            a0 = lay['body_pose'][0]
            x[a0 + 9] = -6.0       # exp(2*6)*w_bend > 1e4  -> angle prior dropped (fitting.py:349)
        xs.append(x); gts.append(gt); confs.append(cf)
        if cfg.get('use_3d'):      # gt_joints3d [17,3] + joints3d_conf [17] (non_linear_solver.py:86-99)
            r3 = np.random.default_rng(700 + b)
            c3 = r3.uniform(0.2, 1.0, 17)
            c3[11] = c3[12] = 0.0                      # the hips are zeroed (non_linear_solver.py:92-94)
            j3s.append(np.concatenate([out['joints'] + r3.normal(0, 0.04, (17, 3)), c3[:, None]], 1))
    j3 = np.asarray(j3s) if j3s else None
    return model, cams, vpw, gmm, np.asarray(xs), np.asarray(gts), np.asarray(confs), j3


def gen_closure_goldens(lsp, only=None):
    for name, cfg in CASES.items():
        if only and name not in only:
            continue
        model, cams, vpw, gmm, xs, gts, confs, j3 = build_case(name, cfg, lsp)
        wts = stage_weights(cfg['stage'])
        res = {}
        for dtn in ('float64', 'float32'):
            L, G, Jn, Vt = [], [], [], []
            for b in range(B_CASE):
                rp = ri.RefProblem(model, cams, gts[b], confs[b], dtn, use_vposer=cfg['use_vposer'],
                                   vposer_weights=vpw, prior=cfg['prior'], gmm=gmm,
                                   fix_shape=cfg.get('fix_shape', False),
                                   joints3d=None if j3 is None else (j3[b][:, :3], j3[b][:, 3]))
                if cfg.get('fix_shape'):
                    rp.smpl.betas.requires_grad = False     # init_guess.py:205-210
                x = xs[b]
                if cfg.get('fix_shape'):
                    # betas are frozen: flat vector drops them, value stays in the model
                    with rp.torch.no_grad():
                        rp.smpl.betas.copy_(rp.torch.tensor(x[:10], dtype=rp.dt).view(1, 10))
                    loss, grad, verts, joints = rp.eval_closure(x[10:], wts)
                else:
                    loss, grad, verts, joints = rp.eval_closure(x, wts)
                L.append(loss); G.append(grad); Jn.append(joints); Vt.append(verts)
            res[dtn] = (np.asarray(L), np.asarray(G), np.asarray(Jn), np.asarray(Vt))
        out = dict(x=xs, gt_xy=gts, conf=confs,
                   cam_R=cams[0], cam_t=cams[1], cam_f=cams[2], cam_c=cams[3],
                   wts=np.array([wts['data_weight'], wts['body_pose_weight'], wts['shape_weight'],
                                 wts['bending_prior_weight'], wts['rho']]),
                   loss64=res['float64'][0], grad64=res['float64'][1], joints64=res['float64'][2],
                   verts64_as32=res['float64'][3][:2].astype(np.float32),
                   loss32=res['float32'][0], grad32=res['float32'][1],
                   joints32=res['float32'][2].astype(np.float32),
                   model_checksum=np.array(syn.model_checksum(model)))
        if j3 is not None:
            out['joints3d'] = j3.astype(np.float32)
        np.savez_compressed(os.path.join(GOLD, 'closure_%s.npz' % name), **out)
        e_l = np.abs(res['float32'][0] - res['float64'][0]) / np.abs(res['float64'][0])
        print('%-18s loss64 %s  fp32-vs-fp64 rel %.1e' % (name, res['float64'][0], e_l.max()))


def run_ref_lbfgs(fn, x0, segments, dtype_name='float64', maxiters=30, tolerances=None, lr=1.0, max_iter=30, history=100,
                  ftol=1e-9, gtol=1e-9):
    """tolerances = (tolerance_grad, tolerance_change): construct the reference's LBFGS class directly (the factory
    does not forward them, optim_factory.py:50-52) - and so with any lr / max_iter / history other than what gen_lbfgs_kat
    has always asked the factory for.  maxiters / ftol / gtol are run_fitting's."""
    import torch
    ref = ri.load()
    dt = torch.float64 if dtype_name == 'float64' else torch.float32
    ps = [torch.nn.Parameter(torch.tensor(x0[a:b], dtype=dt)) for a, b in segments]
    if tolerances is None and (lr, max_iter, history) == (1.0, 30, 100):
        opt, _ = ref.optim_factory.create_optimizer(ps, optim_type='lbfgsls', lr=1.0, maxiters=30)
    else:
        tg, tc = tolerances if tolerances is not None else (1e-5, 1e-9)
        opt = ref.lbfgs_ls.LBFGS(ps, lr=lr, max_iter=max_iter, tolerance_grad=tg, tolerance_change=tc, history_size=history,
                                 line_search_fn='strong_Wolfe')
    trace = []

    def closure(backward=True):
        x = torch.cat([p.detach() for p in ps]).numpy().astype(np.float64)
        f, g = fn(x)
        for p, (a, b) in zip(ps, segments):
            p.grad = torch.tensor(g[a:b], dtype=dt)
        trace.append(np.concatenate([x, [f]]))
        return torch.tensor(f, dtype=dt)
    mon = ref.fitting.FittingMonitor(maxiters=maxiters, ftol=ftol, gtol=gtol)
    with contextlib.redirect_stdout(io.StringIO()):
        final = mon.run_fitting(opt, closure, ps, None, use_vposer=False)
    xf = torch.cat([p.detach() for p in ps]).numpy().astype(np.float64)
    return final, np.asarray(trace), xf


GTD_CASES = [('quad', 49, 1e-3), ('quad', 86, 1e-4), ('gmof', 49, 1e-2), ('gmof', 86, 1e-3)]


def gen_lbfgs_kat():
    out = {}
    for kind in ('quad', 'rosen', 'gmof'):
        for D in (49, 86):
            fn, x0 = ln.kat_objective(kind, D)
            seg = [(0, 10), (10, 13), (13, D)]
            final, trace, xf = run_ref_lbfgs(fn, x0, seg)
            key = '%s_%d' % (kind, D)
            out[key + '_trace'] = trace[:80]
            out[key + '_n'] = np.array(len(trace))
            out[key + '_final'] = np.array(final)
            out[key + '_xf'] = xf
            print('kat', key, 'closures', len(trace), 'final', final)
    # forced `gtd > -tolerance_change` exits right after a direction computation (lbfgs_ls.py:379-380): tiny
    # tolerance_grad, large tolerance_change; run_fitting then keeps stepping on the gradient the last closure left
    for kind, D, tc in GTD_CASES:
        fn, x0 = ln.kat_objective(kind, D)
        seg = [(0, 10), (10, 13), (13, D)]
        final, trace, xf = run_ref_lbfgs(fn, x0, seg, tolerances=(1e-12, tc))
        key = '%s_%d_gtd' % (kind, D)
        out[key + '_trace'] = trace[:80]
        out[key + '_n'] = np.array(len(trace))
        out[key + '_final'] = np.array(final)
        out[key + '_xf'] = xf
        out[key + '_tc'] = np.array(tc)
        print('kat', key, 'tolerance_change', tc, 'closures', len(trace), 'final', final)
    np.savez_compressed(os.path.join(GOLD, 'lbfgs_kat.npz'), **out)
    gen_lbfgs_kat_branches()


def gen_lbfgs_kat_branches():
    """tests/golden/lbfgs_kat_branches.npz: per case of tests/lbfgs_branch_cases.py the start, the reference's whole trace,
    closure count, final loss (NaN where run_fitting returns None) and final point - and the branch tags of the oracle
    replaying that trace (tests/lbfgs_follow.py), which tests/test_lbfgs_oracle.py holds to the trace closure for closure."""
    import warnings
    from tests import lbfgs_branch_cases as bc
    from tests import lbfgs_follow as lf
    out = {}
    for c in bc.CASES:
        name, D = c['name'], c['D']
        fn, _ = ln.kat_objective(c['kind'], D)
        x0 = bc.make_x0(c)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)           # the non-finite case overflows on purpose
            final, trace, xf = run_ref_lbfgs(fn, x0, bc.SEGMENTS(D), maxiters=c['maxiters'],
                                             tolerances=(c['tolerance_grad'], c['tolerance_change']), lr=c['lr'],
                                             max_iter=c['max_iter'], history=c['history'], ftol=c['ftol'], gtol=c['gtol'])
            assert len(trace) <= bc.MAX_CLOSURES, (name, len(trace))
            fo = lf.replay(trace, D, kind=c['kind'], case=c)
        assert not fo.exhausted and len(fo.trace) == len(trace), (name, len(fo.trace), len(trace))
        out[name + '_x0'] = x0
        out[name + '_trace'] = trace
        out[name + '_n'] = np.array(len(trace))
        out[name + '_final'] = np.array(np.nan if final is None else final)
        out[name + '_xf'] = xf
        out[name + '_tag_at'] = np.array([i for i, _ in fo.branches], np.int32)
        out[name + '_tags'] = np.array([t for _, t in fo.branches])
        print('kat branches', name, 'closures', len(trace), 'final', final, 'replay deviation %.2g' % np.nanmax(fo.dev))
    np.savez_compressed(os.path.join(GOLD, 'lbfgs_kat_branches.npz'), **out)


def run_reference_fit(rp, x0, stages):
    """The stage loop of non_linear_solver.py:156-211 around the reference's own optimiser / closure / run_fitting;
    returns final loss, flat params, closures per stage and the (x_flat, loss) trace of every closure call."""
    rp.set_flat(x0)
    ncl, trace, final = [], [], None
    for wts in stages:
        rp.set_weights(wts)
        opt = rp.make_optimizer()
        inner = rp.make_closure(opt)
        cnt = [0]

        def closure(backward=True, inner=inner, cnt=cnt):
            x = rp.get_flat().astype(np.float64)
            val = inner(backward)
            cnt[0] += 1
            trace.append(np.concatenate([x, [float(val)]]))
            return val
        with contextlib.redirect_stdout(io.StringIO()):
            final = rp.monitor.run_fitting(opt, closure, rp.final_params(), rp.smpl, use_vposer=rp.use_vposer,
                                           pose_embedding=rp.pose_embedding, vposer=rp.vposer)
        ncl.append(cnt[0])
    return final, rp.get_flat().astype(np.float64), ncl, np.asarray(trace)


TRACE_LEN = 120


def gen_fit_goldens(lsp):
    """Full 4-stage fits by the reference (non_linear_solver.py:156-211 restated as a driver around the reference's
    own create_optimizer / create_fitting_closure / run_fitting), float64 and float32, with the (x, loss) of the first
    TRACE_LEN closure calls."""
    stages = [stage_weights(st) for st in range(4)]
    for name, use_vp in (('l2', False), ('vposer', True)):
        model = syn.make_body_model(0, kp_regressor=lsp)
        cams = syn.make_camera_ring(8)
        vpw = syn.make_vposer_decoder() if use_vp else None
        orc = cn.ClosureOracle(model, np.float64, vposer=vpw)
        frames = syn.make_frames(2, seed0=1000)
        lay, D = cn.param_layout(use_vp)
        res = dict(x0=[], xf=[], final=[], ncl=[], gt_xy=[], conf=[], trace64=[], xf32=[], final32=[], ncl32=[], trace32=[])
        for b in range(2):
            p = {k: frames[k][b] for k in frames}
            p['use_vposer'] = False
            out = orc.body(p, want_cache=False)
            gt, cf = syn.make_observations(out['joints'][None], cams, seed=500 + b)
            gt, cf = gt[0], cf[0]
            x0 = np.zeros(D)
            x0[lay['scale'][0]] = 1.0
            for dtn, sfx in (('float64', ''), ('float32', '32')):
                rp = ri.RefProblem(model, cams, gt, cf, dtn, use_vposer=use_vp, vposer_weights=vpw)
                final, xf, ncl, trace = run_reference_fit(rp, x0, stages)
                res['xf' + sfx].append(xf); res['final' + sfx].append(final); res['ncl' + sfx].append(ncl)
                res['trace64' if not sfx else 'trace32'].append(trace[:TRACE_LEN])
                print('fit', name, b, dtn, 'closures/stage', ncl, 'final', final)
            res['x0'].append(x0); res['gt_xy'].append(gt); res['conf'].append(cf)
        np.savez_compressed(os.path.join(GOLD, 'fit_%s.npz' % name),
                            **{k: np.asarray(v) for k, v in res.items()},
                            cam_R=cams[0], cam_t=cams[1], cam_f=cams[2], cam_c=cams[3])


def main():
    os.makedirs(GOLD, exist_ok=True)
    r, c, v = ri.real_lsp_regressor()
    np.savez_compressed(os.path.join(GOLD, 'lsp_regressor.npz'), rows=r, cols=c, vals=v)
    lsp = (r, c, v)
    what = sys.argv[1:] or ['closure', 'kat', 'fit']
    if 'closure' in what:
        gen_closure_goldens(lsp)
    if 'kat' in what:
        gen_lbfgs_kat()
    if 'fit' in what:
        gen_fit_goldens(lsp)


if __name__ == '__main__':
    main()
