"""NumPy restatement of the vertex-target term's contract (include/mvfit.h: mvfit_vertex_target_loss).

A problem's vertices are n = 3 Nv flat floats.  For the k with a_k > 0, in ascending k:
  d_k[e] = V[e] - T_k[e]                                        one fp32 subtraction
  g[e]   = float32(2 * sum_k double(a_k) * double(d_k[e]))      the sum in float64 from 0.0
  L      = sum_e sum_k double(a_k) * double(d_k[e])^2           in float64 (math.fsum: the exactly rounded sum)
A row whose weight is 0 is never read."""
import math

import numpy as np


def vertex_target_loss(vertices, targets, weights):
    """vertices [B,Nv,3], targets [B,K,Nv,3], weights [B,K] -> (L [B] float64, g [B,Nv,3] float32)."""
    V = np.ascontiguousarray(vertices, np.float32)
    T = np.ascontiguousarray(targets, np.float32)
    a = np.asarray(weights, np.float32)
    B, K = a.shape
    assert T.shape == (B, K) + V.shape[1:] and V.shape[0] == B
    L = np.zeros(B, np.float64)
    g = np.zeros(V.shape, np.float32)
    for j in range(B):
        s = np.zeros(V[j].size, np.float64)
        terms = []
        for k in range(K):
            if not a[j, k] > 0:
                continue
            d = (V[j].reshape(-1) - T[j, k].reshape(-1)).astype(np.float32).astype(np.float64)
            ak = np.float64(a[j, k])
            s = s + ak * d
            terms.append(ak * (d * d))
        g[j] = (2.0 * s).astype(np.float32).reshape(V[j].shape)
        L[j] = math.fsum(np.concatenate(terms).tolist()) if terms else 0.0
    return L, g
