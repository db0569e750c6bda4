"""tests/small_models.py:sub_model on the CPU: the reduced model keeps the full model's keypoints and kept vertices (float64
oracle, 1e-12), passes the shipped model preparation (tests/model_prep_host_shim.cpp) and comes out with the skinning form and
vertex-count parity the GPU tests choose it for.  672 = 21 full tiles of 32; 673 = odd, the last tile holds one vertex; 674 =
the last tile holds one vertex pair."""
import functools

import numpy as np
import pytest

from mvsmplfitting_amd import synthetic as syn
from oracle import closure_np as cn
from tests.helpers import body_model, oracle_for
from tests.small_models import kept_vertices, referenced_vertices, sub_model
from tests.smpl_oracle import SmplClosureOracle
from tests.test_model_prep_cpu import Prepared, prepare, shim  # noqa: F401  (the host build of model_prep.cpp)

SIZES = (672, 673, 674)


@functools.lru_cache(maxsize=None)
def full_model(model_type, topk):
    if model_type == 'smpllsp':
        return body_model(0, topk)
    return syn.make_body_model(0, skin_topk=topk, model_type='smpl')


def poses(n=3):
    rng = np.random.default_rng(11)
    x = np.zeros((n, 86))
    x[:, :10] = rng.normal(0, 1.5, (n, 10))
    x[:, 10:82] = rng.normal(0, 0.3, (n, 72))
    x[:, 82:85] = rng.normal(0, 0.5, (n, 3))
    x[:, 85] = 1.0 + rng.normal(0, 0.05, n)
    return x


def oracle(model, model_type):
    return oracle_for(model, None, None) if model_type == 'smpllsp' else SmplClosureOracle(model)


@functools.lru_cache(maxsize=None)
def full_bodies(model_type, topk):
    orc = oracle(full_model(model_type, topk), model_type)
    return [orc.body(dict(cn.unpack(x, False), use_vposer=False), want_cache=False) for x in poses()]


def test_referenced_set_of_the_test_model():
    m = body_model(0, 4)
    ref = referenced_vertices(m)
    assert ref.size == 632 and np.all(np.diff(ref) > 0)
    for nv in SIZES:
        idx = kept_vertices(m, nv)
        assert idx.size == nv and np.all(np.diff(idx) > 0) and np.isin(ref, idx).all()
        # the fill: the lowest-numbered vertices outside the referenced set
        rest = np.setdiff1d(np.arange(6890), ref)[:nv - ref.size]
        assert np.array_equal(np.setdiff1d(idx, ref), rest)
    with pytest.raises(ValueError):
        sub_model(m, 631)
    assert sub_model(m, 632)['v_template'].shape == (632, 3)
    with pytest.raises(ValueError):
        sub_model(m, 6891)


@pytest.mark.parametrize('nv', SIZES)
@pytest.mark.parametrize('topk', [None, 4], ids=['dense', 'top4'])
@pytest.mark.parametrize('model_type', ['smpllsp', 'smpl'])
def test_sub_model_keeps_keypoints_and_vertices(shim, model_type, topk, nv):  # noqa: F811
    full = full_model(model_type, topk)
    sub = sub_model(full, nv)
    idx = kept_vertices(full, nv)
    # shapes and the renumbering
    assert sub['v_template'].shape == (nv, 3) and sub['shapedirs'].shape == (nv, 3, 10) and sub['lbs_weights'].shape == (nv, 24)
    assert sub['posedirs'].shape == (207, 3 * nv) and sub['J_regressor'].shape == (24, nv)
    assert (sub['kp_regressor'] is None) == (model_type == 'smpl')
    assert np.array_equal(idx[sub['face_vertex_ids']], full['face_vertex_ids'])
    assert sub['faces'].min() >= 0 and sub['faces'].max() < nv and sub['faces'].shape[0] > 0
    kept_faces = full['faces'][np.isin(full['faces'], idx).all(axis=1)]
    assert np.array_equal(idx[sub['faces']], kept_faces)
    assert np.array_equal(sub['posedirs'].reshape(207, nv, 3), full['posedirs'].reshape(207, 6890, 3)[:, idx])
    # the float64 oracle: keypoints of the sub-model = the full model's, vertices = the full model's at the kept indices
    orc = oracle(sub, model_type)
    for x, ref in zip(poses(), full_bodies(model_type, topk)):
        o = orc.body(dict(cn.unpack(x, False), use_vposer=False), want_cache=False)
        assert np.abs(o['joints'] - ref['joints']).max() <= 1e-12
        assert np.abs(o['vertices'] - ref['vertices'][idx]).max() <= 1e-12
    # the shipped model preparation takes it
    rc, err, h = prepare(shim, sub)
    try:
        assert rc == 0, err
        P = Prepared(shim, h)
        assert P.scalar('nv') == nv and P.scalar('ntiles') == (nv + 31) // 32 and P.scalar('nv_pad') == (nv + 31) // 32 * 32
        sparse_skinning = P('wsp_w').size > 0
        assert sparse_skinning == (topk == 4)
        if sparse_skinning:
            assert P('wsp_w').size == P.scalar('nv_pad') * 4
        nv_even = (int(P.scalar('nv')) & 1) == 0
        assert nv_even == (nv != 673)
    finally:
        shim.prep_free(h)
    # dense_skinning = 1 drops the 4-pair table of a top-4 model
    if topk == 4:
        rc, err, h = prepare(shim, sub, dense_skinning=1)
        try:
            assert rc == 0 and Prepared(shim, h)('wsp_w').size == 0
        finally:
            shim.prep_free(h)
