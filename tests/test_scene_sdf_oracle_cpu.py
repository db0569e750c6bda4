"""CPU: the NumPy restatement of the scene collision loss (tests/scene_sdf_oracle.py) against the reference's own SDFLoss -
recorded (tests/golden/scene_sdf_ref.npz, tools/make_golden_scene_sdf.py) and, where the reference tree and oracle/_ref are
present, live - and its sampler against torch.nn.functional.grid_sample."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_import as ri
from oracle import sdf_np
from oracle import sdf_ref
from tests import scene_sdf_cases as sc
from tests import scene_sdf_oracle as so


def _run(c, **kw):
    return so.scene_loss(c['vertices'], c['translation'], c['faces'], c['grid_size'], c['scale_factor'], c['robustifier'], **kw)


@pytest.mark.parametrize('name,robust', [('a', False), ('c', False), ('b', False), ('b', True), ('d', False)])
def test_restatement_matches_the_recorded_reference_on_the_goldens_fields(name, robust):
    c = sc.case(name, robust)
    sc.check_gap(c)
    r = _run(c, phi=c['phi'])
    sc.check(c, r['loss'], r['g_vertices'], r['g_translation'])
    if name == 'b':
        assert not np.any(r['g_vertices'][2]) and r['hits'][2] == 0, 'the far body takes and gives nothing'


@pytest.mark.parametrize('name', ['a', 'c'])
def test_restatement_with_the_numpy_voxelisation_reproduces_the_fields_bit_for_bit(name):
    c = sc.case(name)
    r = _run(c, sdf=sdf_np.sdf)
    assert r['phi'].dtype == np.float32 and np.array_equal(r['phi'], c['phi'])
    sc.check(c, r['loss'], r['g_vertices'], r['g_translation'])


def test_case_c_samples_cells_with_corners_outside_the_grid():
    c = sc.case('c')
    assert int(sc.gold()['c/border_samples']) >= 8
    v = c['translated']
    cen, s = so.boxes(v, c['scale_factor'])
    n = 0
    for i in range(3):
        for j in range(3):
            if i != j:
                x = so.local_coords(v[j], cen[i], s[i])
                p, _ = so.sample(c['phi'][i], x)
                i0 = np.floor(((x.astype(np.float64) + 1) * 16 - 1) / 2)
                n += int(np.count_nonzero((p != 0) & np.any((i0 < 0) | (i0 + 1 > 15), axis=1)))
    assert n == int(sc.gold()['c/border_samples'])


def test_sampler_matches_grid_sample_inside_in_the_border_band_and_outside():
    rng = np.random.default_rng(5)
    G = 7
    phi = rng.uniform(0.1, 1.0, (G, G, G))
    x = np.concatenate([rng.uniform(-0.8, 0.8, (40, 3)), rng.uniform(-1.0 - 1.0 / G, 1.0 + 1.0 / G, (80, 3)),
                        rng.uniform(-1.6, 1.6, (40, 3)), [[-1.0, 1.0, 0.0], [1.0 + 0.5 / G, 0.0, 0.0]]])
    band = np.any(np.abs(x) > 1 - 1.0 / G, axis=1) & np.all(np.abs(x) < 1 + 1.0 / G, axis=1)
    assert band.sum() >= 20 and np.any(np.abs(x) > 1 + 1.0 / G, axis=1).sum() >= 20
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    pt = torch.nn.functional.grid_sample(torch.tensor(phi)[None, None], xt.view(1, -1, 1, 1, 3), mode='bilinear',
                                         padding_mode='zeros', align_corners=False).view(-1)
    pt.sum().backward()
    p, dp = so.sample(phi, x)
    assert np.count_nonzero(p[band]) >= 20
    assert np.abs(p - pt.detach().numpy()).max() <= 1e-12
    assert np.abs(dp - xt.grad.numpy()).max() <= 1e-10


@pytest.mark.skipif(not (os.path.isfile(os.path.join(ri.REF_ROOT, 'sdf', 'sdf', 'sdf_loss.py')) and sdf_ref.available()),
                    reason='reference tree / oracle/_ref not present')
def test_restatement_matches_the_unmodified_reference_live_on_case_a():
    import importlib.util
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    try:
        import make_golden_scene_sdf as mk
    finally:
        sys.path.pop(0)
    del importlib
    c = sc.case('a')
    ref = mk.run_reference(mk.load_sdf_loss(), c['vertices'], c['translation'], c['faces'], c['grid_size'], c['scale_factor'],
                           None, torch.float32)
    assert np.array_equal(ref['phi'], c['phi']) and float(ref['loss']) == pytest.approx(c['loss'], rel=1e-7)
    r = _run(c, sdf=sdf_np.sdf)
    assert abs(r['loss'] - float(ref['loss'])) <= sc.LOSS_RTOL * float(ref['loss'])
    assert np.abs(r['g_vertices'] - ref['g_vertices']).max() <= sc.GRAD_TOL * np.abs(ref['g_vertices']).max()
    assert np.abs(r['g_translation'] - ref['g_translation']).max() <= sc.GRAD_TOL * np.abs(ref['g_translation']).max()
