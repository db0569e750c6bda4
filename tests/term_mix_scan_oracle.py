"""TESTS ONLY - NumPy restatement of the term mix's arithmetic with the scan as third vertex term (include/mvfit.h:
mvfit_set_term_mix; csrc/term_mix.hip).  The rounding of each operation is stated as in tests/term_mix_oracle.py, whose
functions it uses for what did not change (the record merge, the scene part): float32 products and sums are formed on float32
arrays (NumPy rounds each operation once), float64 ones on float64 arrays.  A product of two float32 values is exact in
float64."""
import numpy as np

from tests.term_mix_oracle import f32, f64, mix_record, scene_part  # noqa: F401  (unchanged parts, re-exported)


def mix_cotangent3(lam_sil, g_sil, L_sil, lam_vt, g_vt, L_vt, lam_scan, g_scan, L_scan):
    """(g, L_v): per float g = (fl32(lam_sil g_sil) + fl32(lam_vt g_vt)) + fl32(lam_scan g_scan) and L_v = fp32((f64(lam_sil)
    L_sil + f64(lam_vt) L_vt) + f64(lam_scan) L_scan): the live components in the order silhouette, vertex targets, scan; a
    component with share 0 is skipped - neither read nor added."""
    g, L = None, None
    for lam, gk, Lk in ((lam_sil, g_sil, L_sil), (lam_vt, g_vt, L_vt), (lam_scan, g_scan, L_scan)):
        lam = f32(lam)
        if not lam > 0:
            continue
        gp = lam * np.asarray(gk, f32)                                  # one rounded float32 product
        Lp = f64(lam) * np.asarray(Lk, f32).astype(f64)                 # exact in float64
        g = gp if g is None else g + gp                                 # one rounded float32 add
        L = Lp if L is None else L + Lp                                 # one rounded float64 add
    assert g is not None, 'one share must be > 0'
    assert g.dtype == f32 and L.dtype == f64
    return g, L.astype(f32)


def mix_parts_sum4(shares, parts):
    """sums [B] = fp32(((lam_sc p_sc + lam_sil p_sil) + lam_vt p_vt) + lam_scan p_scan) in float64 from the unweighted parts
    [B,4] (float32); the last add is made only with a scan share > 0."""
    lam = np.asarray(shares, f32).astype(f64)
    p = np.asarray(parts, f32).astype(f64)
    s = (lam[0] * p[:, 0] + lam[1] * p[:, 1]) + lam[2] * p[:, 2]
    if lam[3] > 0:
        s = s + lam[3] * p[:, 3]
    return s.astype(f32)
