"""TEST INFRASTRUCTURE - writes tests/golden/vertices_vjp_ref.npz, the vector-Jacobian products of the REFERENCE's own
float64 body module (code/smplx/body_models_scale.py:327-412 by torch.autograd), the goldens of mvfit_vertices_backward:

    python tools/make_golden_vjp.py          (needs the reference tree, like tools/make_golden_smpl_coco17.py)

Configurations (tests/vjp_helpers.py:CONFIGS): 'smpllsp' with dense skinning, with top-4 skinning, with the synthetic
VPoser decoder (body pose = vposer.decode(pose_embedding), fitting.py:170-173), and 'smpl' / COCO-17.  Per configuration
B_GOLD seeded points and, per mode ('v' vertices only, 'j' joints only, 'vj' both), the seeded cotangents: the file keeps
the seeds and a checksum of the regenerated cotangents, not the cotangents themselves.

Keys per configuration c:  c/x [B, D] compact points (float32 values) | c/seed | c/checksum_<mode> |
                            c/grad64_<mode> [B, D] compact gradient (oracle/closure_np.py:param_layout)
and model_checksum_<c>."""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from mvsmplfitting_amd import synthetic as syn          # noqa: E402
from oracle import ref_import as ri                      # noqa: E402
from tests import vjp_helpers as vh                      # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')


def ref_problem(cfg, model, vpw):
    cams = syn.make_camera_ring(1)
    gt, conf = np.zeros((1, 17, 2)), np.zeros((1, 17))
    if cfg['kind'] == 'smpl':
        from make_golden_smpl_coco17 import smpl_problem
        return smpl_problem(model, cams, gt, conf, 'float64')
    return ri.RefProblem(model, cams, gt, conf, 'float64', use_vposer=cfg['vposer'], vposer_weights=vpw)


def ref_vjp(rp, use_vposer, xc, gv, gj):
    import torch
    rp.set_flat(xc)
    bp = rp.vposer.decode(rp.pose_embedding, output_type='aa').view(1, -1) if use_vposer else None
    out = rp.smpl(return_verts=True, body_pose=bp)
    outs, cots = [], []
    if gv is not None:
        outs.append(out.vertices); cots.append(torch.tensor(gv[None], dtype=torch.float64))
    if gj is not None:
        outs.append(out.joints); cots.append(torch.tensor(gj[None], dtype=torch.float64))
    ps = rp.final_params()
    gs = torch.autograd.grad(outs, ps, grad_outputs=cots, allow_unused=True)
    return np.concatenate([(g if g is not None else torch.zeros_like(p)).detach().numpy().reshape(-1) for g, p in zip(gs, ps)])


def main():
    out = {}
    for name, cfg in vh.CONFIGS.items():
        model, vpw = vh.model_for(cfg), vh.vposer_for(cfg)
        rp = ref_problem(cfg, model, vpw)
        xs = vh.random_points(cfg['seed'], vh.B_GOLD, cfg['vposer'])
        out[name + '/x'] = xs.astype(np.float32)
        out[name + '/seed'] = np.int64(cfg['seed'])
        out['model_checksum_' + name] = np.float64(syn.model_checksum(model))
        orc = vh.VjpOracle(model, vpw)
        for mode in vh.MODES:
            gv, gj = vh.cotangents(cfg['seed'], vh.B_GOLD, model['v_template'].shape[0], mode)
            out['%s/checksum_%s' % (name, mode)] = np.float64(vh.cotangent_checksum(gv, gj))
            G = []
            for b in range(vh.B_GOLD):
                g = ref_vjp(rp, cfg['vposer'], xs[b], None if gv is None else gv[b], None if gj is None else gj[b])
                go = orc.vjp(xs[b], None if gv is None else gv[b], None if gj is None else gj[b], cfg['vposer'])
                print('%-10s %-2s b=%d  max|g| %.3e  |ref - oracle| %.2e' % (name, mode, b, np.abs(g).max(), np.abs(g - go).max()),
                      flush=True)
                G.append(g)
            out['%s/grad64_%s' % (name, mode)] = np.asarray(G)
    path = os.path.join(GOLD, 'vertices_vjp_ref.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
