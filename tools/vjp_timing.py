"""Developer tool: time mvfit_vertices_backward (MvFit.vertices_backward) at B = 1, 32, 128 beside the same VJP by a float32
eager-PyTorch SMPL autograd on the same GPU, and print the byte and matrix-rate floors of the call.

    python tools/vjp_timing.py [--reps 5] [--calls 50]

Model: the synthetic SMPL-shaped body, top-4 skinning, LSP keypoint regressor (the shapes of real SMPL).  Times are device
events around `calls` back-to-back calls after a warm-up, the median of `reps` windows.  The eager autograd runs the forward
too (it has to: the graph is built by it); the library's call recomputes what it needs from the parameters as well, so both
figures are "gradient from parameters and cotangents"."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from mvsmplfitting_amd import synthetic as syn  # noqa: E402
from mvsmplfitting_amd.engine import MvFit  # noqa: E402

HBM_BPS = 8.0e12          # MI355X_MICROARCH: HBM3E peak (6.3 TB/s achievable)
FP32_MATRIX = 157.3e12    # fp32 peak, matrix and vector alike (v_mfma_f32_32x32x2_f32 runs at the vector rate)
KROWS = 224


def eager_smpl(model, dev):
    """float32 SMPL.forward in eager PyTorch (lbs.py:135-222 + the keypoint selection, body_models_scale.py:393-403)."""
    t = lambda a, dt=torch.float32: torch.tensor(np.asarray(a), dtype=dt, device=dev)
    vt, S, PD, JR, W = t(model['v_template']), t(model['shapedirs']), t(model['posedirs']), t(model['J_regressor']), t(model['lbs_weights'])
    par = [int(p) for p in model['parents']]
    nv = vt.shape[0]
    sel = np.zeros((19, nv), np.float32)
    sel[:14] = model['kp_regressor']
    sel[14 + np.arange(5), model['face_vertex_ids']] = 1.0
    K = t(sel[np.asarray(model['joint_map'])])

    def rod(r):
        a = torch.linalg.norm(r + 1e-8, dim=-1, keepdim=True)
        k = r / a
        z = torch.zeros_like(k[..., 0])
        Km = torch.stack([z, -k[..., 2], k[..., 1], k[..., 2], z, -k[..., 0], -k[..., 1], k[..., 0], z], -1).view(*r.shape[:-1], 3, 3)
        s, c = torch.sin(a)[..., None], torch.cos(a)[..., None]
        return torch.eye(3, device=dev) + s * Km + (1 - c) * (Km @ Km)

    def fwd(x):
        B = x.shape[0]
        beta, theta, tau, s = x[:, 0:10], x[:, 10:82].view(B, 24, 3), x[:, 82:85], x[:, 85]
        vs = vt + torch.einsum('vkl,bl->bvk', S, beta)
        J = torch.einsum('jv,bvk->bjk', JR, vs)
        R = rod(theta)
        pf = (R[:, 1:] - torch.eye(3, device=dev)).reshape(B, 207)
        vp = vs + (pf @ PD).view(B, nv, 3)
        Rm = torch.cat([s[:, None, None, None] * R[:, :1], R[:, 1:]], 1)
        tm = torch.cat([J[:, :1], J[:, 1:] - J[:, par[1:]]], 1)
        Gr, Gt = [Rm[:, 0]], [tm[:, 0]]
        for i in range(1, 24):
            Gr.append(Gr[par[i]] @ Rm[:, i])
            Gt.append((Gr[par[i]] @ tm[:, i, :, None])[..., 0] + Gt[par[i]])
        Gr, Gt = torch.stack(Gr, 1), torch.stack(Gt, 1)
        At = Gt - (Gr @ J[..., None])[..., 0]
        T = torch.einsum('vj,bjac->bvac', W, Gr)
        xs = (T @ vp[..., None])[..., 0] + W @ At
        return xs + tau[:, None], torch.einsum('kv,bva->bka', K, xs) + tau[:, None]
    return fwd


def timed(fn, reps, calls):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / calls)
    return float(np.median(out)), float(min(out)), float(max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--calls', type=int, default=50)
    args = ap.parse_args()
    model = syn.make_body_model(0, skin_topk=4)
    eng = MvFit(model)
    dev = eng.device
    nv = eng.nv
    fwd = eager_smpl(model, dev)
    print('B     vjp us (median [min max])      fwd us   eager fwd+bwd us   floor: bytes us  fp32-matrix us   |lib - eager| / max')
    for B in (1, 32, 128):
        eng.set_problems(syn.make_camera_ring(1), np.zeros((B, 1, 17, 2), np.float32), np.zeros((B, 1, 17), np.float32))
        rng = np.random.default_rng(B)
        x = np.zeros((B, 118), np.float32)
        x[:, :85] = rng.normal(0, 0.3, (B, 85))
        x[:, 85] = 1.0
        xt = torch.tensor(x, device=dev)
        gv = torch.tensor(rng.standard_normal((B, nv, 3)), dtype=torch.float32, device=dev)
        gj = torch.tensor(rng.standard_normal((B, 17, 3)), dtype=torch.float32, device=dev)
        lib = timed(lambda: eng.vertices_backward(xt, gv, gj), args.reps, args.calls)
        vf = timed(lambda: eng.vertices(xt), args.reps, args.calls)

        def eager():
            xe = xt.detach().requires_grad_(True)
            v, j = fwd(xe)
            return torch.autograd.grad((v, j), xe, grad_outputs=(gv, gj))[0]
        eg = timed(eager, args.reps, max(5, args.calls // 5))
        g_lib = eng.vertices_backward(xt, gv, gj)[:, :86]
        g_eag = eager()[:, :86]
        err = float((g_lib - g_eag).abs().max() / g_eag.abs().max())
        chunks = (B + 31) // 32
        bytes_ = chunks * nv * 3 * KROWS * 4 + B * (nv * 3 + 17 * 3 + 118 * 2) * 4
        flops = chunks * 2 * (2 * 32 * nv * 3 * KROWS)
        print('%-5d %8.1f [%7.1f %7.1f]  %8.1f   %12.1f        %8.2f        %8.2f        %.1e'
              % (B, lib[0], lib[1], lib[2], vf[0], eg[0], bytes_ / HBM_BPS * 1e6, flops / FP32_MATRIX * 1e6, err), flush=True)
    eng.close()


if __name__ == '__main__':
    main()
