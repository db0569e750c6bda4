// libmvfit: the C ABI (include/mvfit.h) of the scan loss - mvfit_set_scans / mvfit_scan_loss.  Argument checks only; the
// kernels and the workspace are scan_loss.hip's, behind launchers.h.
#include "mvfit_ctx.h"

extern "C" int mvfit_set_scans(mvfit_ctx* c, int num_bodies, int max_points, const float* points, const int32_t* count,
                               const float* weights) {
    if (!c) return MVFIT_E_ARG;
    HIP_OK(c, hipSetDevice(c->device));
    if (num_bodies == 0) {                       // clear: the workspace goes with the set
        HIP_OK(c, hipStreamSynchronize(c->stream));
        c->scan.on = false;
        c->scan.ws.reset();
        return MVFIT_OK;
    }
    if (!c->num_faces) return fail(c, MVFIT_E_STATE, "mvfit_set_scans: the model was created without (valid) faces");
    if (num_bodies < 0 || num_bodies > 65535 || max_points < 1 || (long long)num_bodies * max_points > (1ll << 28))
        return fail(c, MVFIT_E_ARG, "mvfit_set_scans: sizes out of range (num_bodies=%d in [0, 65535], max_points=%d >= 1, at most "
                    "2^28 points in all)", num_bodies, max_points);
    if (!points || !count) return fail(c, MVFIT_E_ARG, "mvfit_set_scans: null %s", !points ? "points" : "count");
    for (int n = 0; n < num_bodies; ++n) {
        if (count[n] < 0 || count[n] > max_points)
            return fail(c, MVFIT_E_ARG, "mvfit_set_scans: count[%d] = %d outside [0, %d]", n, count[n], max_points);
        if (!weights) continue;
        for (int i = 0; i < count[n]; ++i) {
            const float w = weights[(size_t)n * max_points + i];
            if (!std::isfinite(w) || w < 0.f)
                return fail(c, MVFIT_E_ARG, "mvfit_set_scans: weights[%d][%d] = %g must be finite and >= 0", n, i, (double)w);
        }
    }
    return scan_set(c->scan, c->nv, c->num_faces, num_bodies, max_points, points, count, weights, c->stream, c->err);
}

extern "C" int mvfit_scan_loss(mvfit_ctx* c, const float* vertices, int num_bodies, float w_s2m, float w_m2s, float sigma,
                               uint32_t search, float* loss, float* g_vertices, int32_t* nearest_face, int32_t* nearest_point) {
    if (!c) return MVFIT_E_ARG;
    if (!c->scan.on) return fail(c, MVFIT_E_STATE, "mvfit_scan_loss: no scan set is present (mvfit_set_scans)");
    if (!vertices || !loss) return fail(c, MVFIT_E_ARG, "mvfit_scan_loss: null %s", !vertices ? "vertices" : "loss");
    if (num_bodies != c->scan.N)
        return fail(c, MVFIT_E_ARG, "mvfit_scan_loss: num_bodies = %d, the scan set has %d", num_bodies, c->scan.N);
    if (!std::isfinite(w_s2m) || !std::isfinite(w_m2s) || !std::isfinite(sigma) || w_s2m < 0.f || w_m2s < 0.f || sigma < 0.f)
        return fail(c, MVFIT_E_ARG, "mvfit_scan_loss: w_s2m = %g, w_m2s = %g and sigma = %g must be finite and >= 0", (double)w_s2m,
                    (double)w_m2s, (double)sigma);
    if (search > 1u) return fail(c, MVFIT_E_ARG, "mvfit_scan_loss: search = %u, not 0 (auto) or 1 (exhaustive)", search);
    HIP_OK(c, hipSetDevice(c->device));
    // search = 0 selects the culled search: at the timed shape it is the faster one
    return scan_loss(c->scan, c->d_faces, vertices, w_s2m, w_m2s, sigma, search == 1u, loss, g_vertices, nearest_face, nearest_point,
                     c->stream, c->err);
}
