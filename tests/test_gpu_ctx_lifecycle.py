"""GPU: one ctx through the life of its buffers (csrc/dev_mem.h owns them, by lifetime).  One engine over the small synthetic
model (sparse skinning, so the asynchronous drivers run) is resized 40 -> 3 -> 40 problems - Bpad 64 -> 32 -> 64: the problem
buffers, the ring, the SDF term's work areas and box parts are freed and allocated again in both directions - then given the
same shapes again (every buffer is kept), with a scene loss and a scene rendering in between (the workspaces that grow on
their own).  Every staged fit (SDF term in the last stage, a short face list) must be the same bits as that fit on an engine
that has done nothing else; no pass is lost or times out; after close() a new engine works."""
import numpy as np
import pytest
import torch

from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import stage_weights
from tests.gpu_helpers import make_engine
from tests.helpers import body_model

pytestmark = pytest.mark.gpu

B_BIG, B_SMALL, V = 40, 3, 2


def _fit(eng, model, cams, gt, conf, set_sdf=True):
    eng.set_problems(cams, gt, conf)
    if set_sdf:
        eng.set_sdf(model['faces'], num_faces=32, grid_size=16)
    x0 = np.zeros((gt.shape[0], 118), np.float32)
    x0[:, 85] = 1.0
    xf, st = eng.fit(x0, stage_weights(1536.0, coll_w=[0.0, 0.0, 0.0, 20.0]))
    assert st['passes']['run'] > 0, st['passes']                       # the asynchronous drivers ran
    assert st['passes']['missed'] == 0 and st['passes']['timed_out'] == 0, st['passes']
    res = (xf.cpu().numpy(), st['final_loss'].cpu().numpy(), st['n_closure'].cpu().numpy())
    assert np.all(np.isfinite(res[1]))
    return res


def _same(got, want, what):
    for k, name in enumerate(('parameters', 'final losses', 'closure counts')):
        assert np.array_equal(got[k], want[k]), (what, name)


def test_one_ctx_resized_down_up_and_kept_fits_like_a_fresh_one():
    model = body_model(0, 4)
    cams = syn.make_camera_ring(V)
    fr = syn.make_frames(B_BIG, seed0=8100)
    xgt = np.zeros((B_BIG, 118), np.float32)
    for k, (a, b) in dict(betas=(0, 10), global_orient=(10, 13), body_pose=(13, 82), transl=(82, 85), scale=(85, 86)).items():
        xgt[:, a:b] = fr[k]
    want = {}
    with make_engine(model) as ref:                     # the observations, and the fresh engine's fit of the large batch
        ref.set_problems(cams, np.zeros((B_BIG, V, 17, 2), np.float32), np.ones((B_BIG, V, 17), np.float32))
        gt, conf = syn.make_observations(ref.vertices(xgt)[1].cpu().numpy(), cams, seed=8107)
    with make_engine(model) as ref:
        want[B_BIG] = _fit(ref, model, cams, gt, conf)
    with make_engine(model) as ref:
        want[B_SMALL] = _fit(ref, model, cams, gt[:B_SMALL], conf[:B_SMALL])

    eng = make_engine(model)
    _same(_fit(eng, model, cams, gt, conf), want[B_BIG], 'first fit')
    # the workspaces with a lifetime of their own: the scene loss (2 bodies, G = 16) and a scene rendering (one 240 x 320 image)
    verts, joints = eng.vertices(xgt)
    pair = verts[:2].clone()
    pair[1] += torch.tensor([0.13, 0.02, 0.07], device=pair.device)
    loss, g, _ = eng.scene_sdf_loss(pair, model['faces'], grid_size=16, robustifier=0.05)
    again, g2, _ = eng.scene_sdf_loss(pair, model['faces'], grid_size=16, robustifier=0.05)
    assert np.isfinite(float(loss[0])) and torch.equal(loss, again) and torch.equal(g, g2)
    img = torch.zeros(1, 240, 320, 3, dtype=torch.uint8)
    out = eng.render_scene(verts, joints, img, [[0, 1]], [0])
    assert tuple(out.shape) == (1, 240, 320, 3) and torch.equal(out, eng.render_scene(verts, joints, img, [[0, 1]], [0]))
    _same(_fit(eng, model, cams, gt[:B_SMALL], conf[:B_SMALL]), want[B_SMALL], 'resized down')
    _same(_fit(eng, model, cams, gt, conf), want[B_BIG], 'resized up')
    _same(_fit(eng, model, cams, gt, conf, set_sdf=False), want[B_BIG], 'same shapes again: buffers kept')
    eng.close()
    with make_engine(model) as eng2:
        _same(_fit(eng2, model, cams, gt[:B_SMALL], conf[:B_SMALL]), want[B_SMALL], 'new engine after close()')
