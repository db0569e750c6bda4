// libmvfit: the C ABI (include/mvfit.h) of the scan loss - mvfit_set_scans / mvfit_scan_loss - and of the scan term inside the
// fit - mvfit_set_scan_term.  Argument checks and state only; the kernels and the workspace are scan_loss.hip's, behind
// launchers.h, and the rounds launch the term (round_term.cpp plans the launches).
#include "mvfit_ctx.h"

extern "C" int mvfit_set_scans(mvfit_ctx* c, int num_bodies, int max_points, const float* points, const int32_t* count,
                               const float* weights) {
    if (!c) return MVFIT_E_ARG;
    HIP_OK(c, hipSetDevice(c->device));
    if (num_bodies == 0) {                       // clear: the workspace goes with the set
        HIP_OK(c, hipStreamSynchronize(c->stream));
        c->scan.on = false;
        c->scan.ws.reset();
        term_source_gone(c, SRC_SCANS);          // no scans: no term and no mix that uses them
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
    const int rc = scan_set(c->scan, c->nv, c->num_faces, num_bodies, max_points, points, count, weights, c->stream, c->err);
    // a set that replaces the one of an enabled term must fit the batch like the first (scan body n is problem n); a failed
    // or unfit set leaves no term behind.  A set of the same sizes keeps every address, and with it the captured round graph.
    // The same holds for a mix that gives the scan a share.
    const bool in_mix = c->mix.on && c->mix.scan > 0.f;
    if ((c->scant.on || in_mix) && (rc || num_bodies != c->B)) {
        term_source_gone(c, SRC_SCANS);
        if (!rc && in_mix)
            return fail(c, MVFIT_E_ARG, "mvfit_set_scans: the set holds %d bodies, the ctx of the enabled term mix %d problems (the mix is "
                        "switched off)", num_bodies, c->B);
        if (!rc)
            return fail(c, MVFIT_E_ARG, "mvfit_set_scans: the set holds %d bodies, the enabled scan term's ctx %d problems (the term is "
                        "switched off)", num_bodies, c->B);
    }
    return rc;
}

// the round buffers of the scan term (cotangent, loss, pull-back partials) for the current batch: allocated by the first
// enable - the term's own setter or the term mix - and kept while B stays
int mvfit::ensure_scan_round(mvfit_ctx* c) {
    if (c->scant.part) return MVFIT_OK;
    HIP_OK(c, hipStreamSynchronize(c->stream));
    free_scan_term(c);                                       // (what an earlier call that failed half-way left)
    float *g = nullptr, *l = nullptr;
    HIP_OK(c, c->scanterm_mem.alloc(&g, (size_t)c->B * c->nv * 3 * sizeof(float), true));
    HIP_OK(c, c->scanterm_mem.alloc(&l, (size_t)c->B * sizeof(float), true));
    c->scant.g_verts = g; c->scant.loss = l;
    HIP_OK(c, c->scanterm_mem.alloc(&c->scant.part, vjp_part_bytes(c->Bpad, c->nv)));    // last: a term with partials is complete
    return MVFIT_OK;
}

// The scan term inside mvfit_fit / mvfit_closure (include/mvfit.h): state only - the rounds launch it.
extern "C" int mvfit_set_scan_term(mvfit_ctx* c, int enable, float w_s2m, float w_m2s, float sigma) {
    if (!c) return MVFIT_E_ARG;
    HIP_OK(c, hipSetDevice(c->device));
    if (!enable) {                                           // off: the buffers stay for the next enable of this batch
        c->scant.on = false;
        return MVFIT_OK;
    }
    if (c->B == 0) return fail(c, MVFIT_E_STATE, "call mvfit_set_problems first");
    if (!c->scan.on) return fail(c, MVFIT_E_STATE, "mvfit_set_scan_term: no scan set is present (mvfit_set_scans)");
    if (c->mix.on) return fail(c, MVFIT_E_STATE, "mvfit_set_scan_term: the term mix uses the ctx's term slot: switch it off first");
    if (c->sdf_num_faces || c->obst.on || c->silt.on || c->vt.term || c->lm.term)
        return fail(c, MVFIT_E_STATE, "mvfit_set_scan_term: the %s term uses the ctx's term slot (one term per ctx): remove it first",
                    term_name(c));
    if (c->scan.N != c->B)
        return fail(c, MVFIT_E_ARG, "mvfit_set_scan_term: the scan set holds %d bodies, the ctx %d problems (scan body n is problem n)",
                    c->scan.N, c->B);
    if (!std::isfinite(w_s2m) || !std::isfinite(w_m2s) || !std::isfinite(sigma) || w_s2m < 0.f || w_m2s < 0.f || sigma < 0.f)
        return fail(c, MVFIT_E_ARG, "mvfit_set_scan_term: w_s2m = %g, w_m2s = %g and sigma = %g must be finite and >= 0", (double)w_s2m,
                    (double)w_m2s, (double)sigma);
    if (!(w_s2m > 0.f) && !(w_m2s > 0.f)) return fail(c, MVFIT_E_ARG, "mvfit_set_scan_term: w_s2m and w_m2s are both 0");
    // a failure below leaves the previous state: the flag and the scalars change last
    if (const int rc = ensure_scan_round(c)) return rc;
    if (const int rc = ensure_sdf_buffers(c)) return rc;     // the record slot (SdfAdj) per problem
    c->scant.w_s2m = w_s2m; c->scant.w_m2s = w_m2s; c->scant.sigma = sigma;
    c->scant.on = true;
    return MVFIT_OK;
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
