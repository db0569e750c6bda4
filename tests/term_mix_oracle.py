"""TESTS ONLY - NumPy restatement of the term mix's arithmetic (include/mvfit.h: mvfit_set_term_mix; csrc/term_mix.hip).
Every function states the rounding of each operation: float32 products and sums are formed on float32 arrays (NumPy rounds
each operation once), float64 ones on float64 arrays.  A product of two float32 values is exact in float64."""
import numpy as np

FLT_MIN = np.float64(1.17549435e-38)
f32, f64 = np.float32, np.float64


def mix_cotangent(lam_sil, g_sil, L_sil, lam_vt, g_vt, L_vt):
    """(g, L_v): per float g = fl32(lam_sil g_sil) + fl32(lam_vt g_vt), L_v = fp32(f64(lam_sil) L_sil + f64(lam_vt) L_vt); a
    component with share 0 is skipped - neither read nor added."""
    lam_sil, lam_vt = f32(lam_sil), f32(lam_vt)
    sil, vt = lam_sil > 0, lam_vt > 0
    assert sil or vt
    g, L = None, None
    if sil:
        g = lam_sil * np.asarray(g_sil, f32)
        L = f64(lam_sil) * np.asarray(L_sil, f32).astype(f64)
    if vt:
        gv = lam_vt * np.asarray(g_vt, f32)
        Lv = f64(lam_vt) * np.asarray(L_vt, f32).astype(f64)
        g = gv if g is None else g + gv
        L = Lv if L is None else L + Lv
    assert g.dtype == f32 and L.dtype == f64
    return g, L.astype(f32)


def mix_record(lam_sc, rec_scene, rec_verts):
    """The merged records [B,R] from the scene term's and the pull-back's (entry 0 = S, then the adjoint): in float64, every
    operation rounded on its own, Q = lam_sc (S_sc S_sc) + S_v S_v, S = fp32(sqrt(Q)), a[e] = fp32(((lam_sc S_sc) a_sc[e] +
    S_v a_v[e]) / sqrt(Q)); Q < FLT_MIN: zeros."""
    lam = f64(f32(lam_sc))
    a_sc, a_v = np.asarray(rec_scene, f32).astype(f64), np.asarray(rec_verts, f32).astype(f64)
    S_sc, S_v = a_sc[:, :1], a_v[:, :1]
    Q = lam * (S_sc * S_sc) + S_v * S_v
    root = np.sqrt(Q)
    with np.errstate(divide='ignore', invalid='ignore'):
        out = ((lam * S_sc) * a_sc + S_v * a_v) / root
    out[:, :1] = root
    out = np.where(Q < FLT_MIN, 0.0, out)
    return out.astype(f32)


def mix_parts_sum(shares, parts):
    """sums [B] = fp32((lam_sc p_sc + lam_sil p_sil) + lam_vt p_vt) in float64 from the unweighted parts [B,3] (float32)."""
    lam = np.asarray(shares, f32).astype(f64)
    p = np.asarray(parts, f32).astype(f64)
    return ((lam[0] * p[:, 0] + lam[1] * p[:, 1]) + lam[2] * p[:, 2]).astype(f32)


def scene_part(S_sc):
    """S_sc^2 as the mix reports it: the float64 square of the float32 S, rounded once."""
    s = np.asarray(S_sc, f32).astype(f64)
    return (s * s).astype(f32)
