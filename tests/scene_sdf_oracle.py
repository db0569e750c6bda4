"""TESTS ONLY - NumPy restatement of the scene collision loss (include/mvfit.h:mvfit_scene_sdf_loss; reference
sdf/sdf/sdf_loss.py:51-99 as it executes) with its analytic gradient, and a CPU stand-in engine built on it.

The fields come from a callable ``sdf(faces, local_vertices[P,Nv,3] float32, G) -> phi[P,G,G,G]`` (oracle.sdf_np.sdf for small
meshes) or from an array of stored fields.  Boxes and local coordinates are float32, the way the reference computes them;
the interpolation is float64.  Runs where the reference tree is absent."""
from __future__ import annotations

import numpy as np
import torch

F32 = np.float32


def boxes(v, scale_factor):
    """v[P,Nv,3] float32 -> centre[P,3], scale[P] float32: boxes.mean(dim=1) and (1 + scale_factor) * 0.5 * max extent with
    the Python-float factor rounded to float32 first (sdf_loss.py:69-70)."""
    v = np.asarray(v, F32)
    lo, hi = v.min(axis=1), v.max(axis=1)
    c = ((lo + hi).astype(F32) / F32(2)).astype(F32)
    s = (F32((1 + scale_factor) * 0.5) * (hi - lo).astype(F32).max(axis=-1)).astype(F32)
    return c, s


def local_coords(v, c, s):
    return ((np.asarray(v, F32) - c).astype(F32) / s).astype(F32)


def sample(phi, x):
    """grid_sample(phi[None, None], x) for phi[G,G,G] (z, y, x order) at x[n,3] in [-1, 1] coordinates: trilinear, zeros
    padding, align_corners=False.  Returns (value[n], d value / d x [n,3]) in float64."""
    phi = np.asarray(phi, np.float64)
    G = phi.shape[0]
    ix = ((np.asarray(x, np.float64) + 1.0) * G - 1.0) / 2.0
    f0 = np.floor(ix)
    t = ix - f0
    i0 = f0.astype(np.int64)
    val = np.zeros(len(ix))
    grad = np.zeros((len(ix), 3))
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                d = np.array([dx, dy, dz])
                idx = i0 + d
                ok = np.all((idx >= 0) & (idx < G), axis=1)
                ic = np.clip(idx, 0, G - 1)
                cv = np.where(ok, phi[ic[:, 2], ic[:, 1], ic[:, 0]], 0.0)
                w = np.where(d == 1, t, 1.0 - t)
                sg = np.where(d == 1, 1.0, -1.0)
                val += cv * w[:, 0] * w[:, 1] * w[:, 2]
                grad[:, 0] += cv * sg[0] * w[:, 1] * w[:, 2]
                grad[:, 1] += cv * sg[1] * w[:, 0] * w[:, 2]
                grad[:, 2] += cv * sg[2] * w[:, 0] * w[:, 1]
    return val, grad * (G / 2.0)


def scene_loss(vertices, translation, faces, grid_size=32, scale_factor=0.2, robustifier=None, sdf=None, phi=None):
    """One scene.  vertices[P,Nv,3], translation[P,3] (or None: already added).  Returns a dict: loss, g_vertices[P,Nv,3],
    g_translation[P,3], phi[P,G,G,G], centre, scale, hits (samples taken inside a field's reach, per source body)."""
    v = np.asarray(vertices, F32)
    if translation is not None:
        v = (v + np.asarray(translation, F32)[:, None]).astype(F32)
    P, nv = v.shape[:2]
    g = np.zeros((P, nv, 3))
    out = dict(loss=0.0, g_vertices=g, g_translation=np.zeros((P, 3)), phi=None, hits=np.zeros(P, np.int64))
    if P == 1:
        return out
    c, s = boxes(v, scale_factor)
    if phi is None:
        phi = sdf(faces, np.stack([local_coords(v[i], c[i], s[i]) for i in range(P)]), grid_size)
    phi = np.asarray(phi)
    assert phi.shape == (P, grid_size, grid_size, grid_size), phi.shape
    total = 0.0
    for i in range(P):
        for j in range(P):
            if j == i:
                continue
            p, dp = sample(phi[i], local_coords(v[j], c[i], s[i]))
            dp = dp / np.float64(s[i])
            out['hits'][i] += int(np.count_nonzero(p))
            if robustifier:
                q = p / robustifier
                fr = q * q
                dp = dp * (2.0 * q / robustifier / (fr + 1.0) ** 2)[:, None]
                p = fr / (fr + 1.0)
            total += p.sum()
            g[j] += dp
    out['loss'] = total / P ** 2
    g /= P ** 2
    out['g_translation'] = g.sum(axis=1)
    out.update(phi=phi, centre=c, scale=s)
    return out


class OracleEngine:
    """CPU stand-in for MvFit.scene_sdf_loss (the engine SceneSDFLoss drives), on the restatement."""

    def __init__(self, sdf=None):
        if sdf is None:
            from oracle import sdf_np
            sdf = sdf_np.sdf
        self.sdf = sdf
        self.device = torch.device('cpu')
        self.calls = []

    def scene_sdf_loss(self, vertices, faces, scene_sizes=None, grid_size=32, scale_factor=0.2, robustifier=None,
                       need_grad=True, return_phi=False):
        assert vertices.dtype == torch.float32 and vertices.dim() == 3
        v = vertices.detach().cpu().numpy()
        f = faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else np.asarray(faces)
        sizes = [v.shape[0]] if scene_sizes is None else list(scene_sizes)
        assert sum(sizes) == v.shape[0]
        self.calls.append(dict(sizes=tuple(sizes), grid_size=grid_size, scale_factor=scale_factor, robustifier=robustifier))
        loss, g, b0 = [], np.zeros(v.shape), 0
        for n in sizes:
            r = scene_loss(v[b0:b0 + n], None, f, grid_size, scale_factor, robustifier, sdf=self.sdf)
            loss.append(r['loss'])
            g[b0:b0 + n] = r['g_vertices']
            b0 += n
        return (torch.tensor(np.asarray(loss), dtype=torch.float32), torch.tensor(g, dtype=torch.float32) if need_grad else None,
                None)
