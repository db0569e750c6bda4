"""TESTS ONLY - the cases of tests/golden/scene_sdf_ref.npz (tools/make_golden_scene_sdf.py: the reference's own SDFLoss,
float32 + autograd) as dicts, shared by the CPU and GPU tests of the scene collision loss."""
import functools
import os

import numpy as np

from mvsmplfitting_amd import synthetic as syn
from tests.helpers import GOLD

LOSS_RTOL = 1e-5          # the project's loss bound
GRAD_TOL = 2e-4           # of max |g_ref| (tests/test_gpu_sdf_term.py)


@functools.lru_cache(maxsize=None)
def gold():
    return dict(np.load(os.path.join(GOLD, 'scene_sdf_ref.npz')))


@functools.lru_cache(maxsize=None)
def case(name, robust=False):
    """name in a, b, c, d; robust: case b's second setting (r = 0.05).  Arrays are shared: treat them as read-only."""
    g = gold()
    c = {k.split('/', 1)[1]: v for k, v in g.items() if k.startswith(name + '/')}
    if name == 'd':
        model = syn.make_body_model(0)
        assert abs(syn.model_checksum(model) - float(c['model_checksum'])) <= 1e-6 * abs(float(c['model_checksum']))
        c['vertices'] = (model['v_template'][None].astype(np.float32) * c['body_scale'][:, None, None]).astype(np.float32)
        c['faces'] = model['faces'].astype(np.int32)
    out = dict(vertices=c['vertices'], translation=c['translation'], faces=c['faces'], grid_size=int(c['grid_size']),
               scale_factor=float(c['scale_factor']), robustifier=None, phi=c.get('phi'), gap=c['gap'])
    sfx = ''
    if name == 'd' or (name == 'b' and robust):
        out['robustifier'] = float(c['robustifier'])
        sfx = '_r' if name == 'b' else ''
        if name == 'b':
            out['gap'] = c['gap_r']
    out['loss'] = float(c['loss' + sfx])
    out['g_translation'] = c['g_translation' + sfx]
    if name == 'd':
        out['row_step'] = int(c['row_step'])
        out['g_vertices_rows'] = c['g_vertices_rows']
        out['g_max'] = float(c['g_max'])
    else:
        out['g_vertices'] = c['g_vertices' + sfx]
        out['g_max'] = float(np.abs(out['g_vertices']).max())
    out['translated'] = (out['vertices'] + out['translation'][:, None]).astype(np.float32)
    return out


def check(c, loss, g_vertices, g_translation=None):
    """loss / gradients of a run against case c at the issue's bounds; prints each figure before it asserts."""
    gv = np.asarray(g_vertices, np.float64)
    if 'g_vertices_rows' in c:
        gv_ref, gv = c['g_vertices_rows'], gv[:, ::c['row_step']]
    else:
        gv_ref = c['g_vertices']
    gt = gv_sum = np.asarray(g_vertices, np.float64).sum(axis=1) if g_translation is None else np.asarray(g_translation, np.float64)
    e_l = abs(float(loss) - c['loss']) / abs(c['loss'])
    e_g = np.abs(gv - gv_ref).max() / c['g_max']
    e_t = np.abs(gt - c['g_translation']).max() / np.abs(c['g_translation']).max()
    print('loss %.7g ref %.7g rel %.2e | g_vertices err/max %.2e | g_translation err/max %.2e' % (loss, c['loss'], e_l, e_g, e_t))
    assert e_l <= LOSS_RTOL, (loss, c['loss'])
    assert e_g <= GRAD_TOL, e_g
    assert e_t <= GRAD_TOL, e_t
    del gv_sum


def check_gap(c):
    """The reference's own float32-vs-float64 gap on the case, stored by the generator, is below a quarter of each bound:
    a badly conditioned fixture fails here."""
    gap_loss, gap_g, gap_t = (float(x) for x in c['gap'])
    print('reference fp32-vs-fp64 gap: loss %.2e g_vertices %.2e g_translation %.2e' % (gap_loss, gap_g, gap_t))
    assert gap_loss < LOSS_RTOL / 4 and gap_g < GRAD_TOL / 4 and gap_t < GRAD_TOL / 4, c['gap']
