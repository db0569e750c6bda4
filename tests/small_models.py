"""Reduced body models for tests (pure NumPy): sub_model keeps the vertices a model's keypoints and skeleton depend on and
fills up to a chosen vertex count, so kernels can be run at vertex counts other than SMPL's 6890 - odd counts, ragged last
tiles - with keypoints that are the full model's."""
import numpy as np


def referenced_vertices(model):
    """ascending indices of the vertices a row of J_regressor, a row of kp_regressor (when present) or face_vertex_ids refers to"""
    nv = model['v_template'].shape[0]
    used = np.zeros(nv, bool)
    used |= (np.asarray(model['J_regressor']) != 0).any(axis=0)
    if model.get('kp_regressor') is not None:
        used |= (np.asarray(model['kp_regressor']) != 0).any(axis=0)
    used[np.asarray(model['face_vertex_ids'])] = True
    return np.flatnonzero(used)


def kept_vertices(model, nv):
    """the vertices of sub_model(model, nv), ascending: the referenced ones, then the lowest-numbered others"""
    full = model['v_template'].shape[0]
    ref = referenced_vertices(model)
    if nv < ref.size:
        raise ValueError('sub_model: %d vertices asked for, %d are referenced by the regressors and face_vertex_ids' % (nv, ref.size))
    if nv > full:
        raise ValueError('sub_model: %d vertices asked for, the model has %d' % (nv, full))
    keep = np.zeros(full, bool)
    keep[ref] = True
    rest = np.flatnonzero(~keep)[:nv - ref.size]
    keep[rest] = True
    return np.flatnonzero(keep)


def sub_model(model, nv):
    """The model restricted to nv of its vertices (kept_vertices): every per-vertex array sliced, face_vertex_ids and faces
    renumbered, the faces with a dropped vertex removed.  Skeleton, keypoints and the kept vertices are the full model's."""
    full = model['v_template'].shape[0]
    idx = kept_vertices(model, nv)
    new_id = np.full(full, -1, np.int64)
    new_id[idx] = np.arange(nv)
    out = dict(model)
    out['v_template'] = np.ascontiguousarray(model['v_template'][idx])
    out['shapedirs'] = np.ascontiguousarray(model['shapedirs'][idx])
    out['lbs_weights'] = np.ascontiguousarray(model['lbs_weights'][idx])
    out['J_regressor'] = np.ascontiguousarray(model['J_regressor'][:, idx])
    if model.get('kp_regressor') is not None:
        out['kp_regressor'] = np.ascontiguousarray(model['kp_regressor'][:, idx])
    pd = np.asarray(model['posedirs'])
    out['posedirs'] = np.ascontiguousarray(pd.reshape(pd.shape[0], full, 3)[:, idx].reshape(pd.shape[0], nv * 3))
    out['face_vertex_ids'] = new_id[np.asarray(model['face_vertex_ids'])].astype(np.int32)
    if model.get('faces') is not None:
        f = new_id[np.asarray(model['faces'])]
        out['faces'] = np.ascontiguousarray(f[(f >= 0).all(axis=1)].astype(np.int32))
    return out
