// libmvfit: the C ABI (include/mvfit.h) of the surface landmark term - mvfit_set_landmarks / mvfit_set_landmark_targets /
// mvfit_landmark_loss - and of the term inside the fit - mvfit_set_landmark_term.  Argument checks, the table's CSR and state
// only; the kernel is landmark.hip's, and the rounds launch the term (round_term.cpp plans the launches).
#include "mvfit_ctx.h"

// the table goes, and with it the targets and the term
static void clear_landmarks(mvfit_ctx* c) {
    free_landmark_targets(c);
    c->lmtab_mem.release();
    c->lm = LmState{};
}

extern "C" int mvfit_set_landmarks(mvfit_ctx* c, int L, const int32_t* vertex_ids, const float* weights) {
    if (!c) return MVFIT_E_ARG;
    HIP_OK(c, hipSetDevice(c->device));
    if (L == 0 || !vertex_ids || !weights) {
        HIP_OK(c, hipStreamSynchronize(c->stream));
        clear_landmarks(c);
        return MVFIT_OK;
    }
    if (L < 1 || L > MVFIT_LANDMARKS_MAX) return fail(c, MVFIT_E_ARG, "mvfit_set_landmarks: L = %d outside [1, %d]", L, MVFIT_LANDMARKS_MAX);
    for (int i = 0; i < L * LM_NNZ; ++i) {
        if (weights[i] == 0.f) continue;                     // a dead slot: its id is never read
        if (!std::isfinite(weights[i]))
            return fail(c, MVFIT_E_ARG, "mvfit_set_landmarks: weight %g of landmark %d, slot %d must be finite", (double)weights[i], i / LM_NNZ,
                        i % LM_NNZ);
        if (vertex_ids[i] < 0 || vertex_ids[i] >= c->nv)
            return fail(c, MVFIT_E_ARG, "mvfit_set_landmarks: vertex id %d of landmark %d, slot %d outside [0, %d)", (int)vertex_ids[i], i / LM_NNZ,
                        i % LM_NNZ, c->nv);
    }
    // the CSR of the touched vertices: (vertex, entry) pairs sorted - vertices ascending, a vertex's entries 4 l + k ascending
    std::vector<std::pair<int32_t, int32_t>> ent;
    for (int i = 0; i < L * LM_NNZ; ++i)
        if (weights[i] != 0.f) ent.emplace_back(vertex_ids[i], i);
    std::sort(ent.begin(), ent.end());
    const int nnz = (int)ent.size();
    std::vector<int32_t> tv, tptr;
    for (int e = 0; e < nnz; ++e)
        if (e == 0 || ent[e].first != ent[e - 1].first) { tv.push_back(ent[e].first); tptr.push_back(e); }
    tptr.push_back(nnz);
    const int nt = (int)tv.size();
    std::vector<int32_t> h(lm_table_words(L, nt, nnz));
    for (int i = 0; i < L * LM_NNZ; ++i) h[i] = weights[i] != 0.f ? vertex_ids[i] : 0;
    memcpy(h.data() + L * LM_NNZ, weights, (size_t)L * LM_NNZ * sizeof(float));
    int32_t* at = h.data() + 2 * L * LM_NNZ;
    if (nt) memcpy(at, tv.data(), (size_t)nt * 4);
    memcpy(at + nt, tptr.data(), (size_t)(nt + 1) * 4);
    for (int e = 0; e < nnz; ++e) at[nt + nt + 1 + e] = ent[e].second;
    HIP_OK(c, hipStreamSynchronize(c->stream));
    clear_landmarks(c);                                      // the targets belong to the table they were set for
    int32_t* d = nullptr;
    HIP_OK(c, c->lmtab_mem.alloc(&d, h.size() * 4));
    HIP_OK(c, hipMemcpy(d, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    LmState& S = c->lm;
    S.tab = d; S.L = L; S.nt = nt; S.nnz = nnz;
    S.table = true;
    return MVFIT_OK;
}

// conf[n] as the caller holds it (device or host) on the host, checked
static int check_conf(mvfit_ctx* c, const float* conf, size_t n, const char* what, std::vector<float>& h) {
    h.resize(n);
    HIP_OK(c, hipMemcpy(h.data(), conf, n * sizeof(float), hipMemcpyDefault));
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(h[i]) || h[i] < 0.f)
            return fail(c, MVFIT_E_ARG, "mvfit_set_landmark_targets: %s[%zu] = %g must be finite and >= 0", what, i, (double)h[i]);
    return MVFIT_OK;
}

extern "C" int mvfit_set_landmark_targets(mvfit_ctx* c, const float* xy, const float* conf, const float* xyz, const float* conf3) {
    if (!c) return MVFIT_E_ARG;
    HIP_OK(c, hipSetDevice(c->device));
    LmState& S = c->lm;
    if (!xy) {                                               // clear: the buffers stay for a next set of the same shape
        S.on = false;
        S.term = false;
        return MVFIT_OK;
    }
    if (!S.table) return fail(c, MVFIT_E_STATE, "mvfit_set_landmark_targets: no landmark table is present (mvfit_set_landmarks)");
    if (c->B == 0) return fail(c, MVFIT_E_STATE, "call mvfit_set_problems first");
    if (!conf) return fail(c, MVFIT_E_ARG, "mvfit_set_landmark_targets: null conf");
    if ((xyz != nullptr) != (conf3 != nullptr))
        return fail(c, MVFIT_E_ARG, "mvfit_set_landmark_targets: xyz and conf3 come together (null %s)", !xyz ? "xyz" : "conf3");
    const bool has3d = xyz != nullptr;
    const int B = c->B, V = c->V, L = S.L;
    const size_t ni = (size_t)B * V * L, nl = (size_t)B * L;
    HIP_OK(c, hipStreamSynchronize(c->stream));
    std::vector<float> h;
    if (const int rc = check_conf(c, conf, ni, "conf", h)) return rc;
    if (has3d)
        if (const int rc = check_conf(c, conf3, nl, "conf3", h)) return rc;
    if (!S.tgt || S.tgt_L != L || S.has3d != has3d) {
        const bool term = S.term;                            // (a failed allocation leaves no targets and no term behind)
        S.on = S.term = false;
        c->lmtgt_mem.release();
        S.tgt = nullptr; S.tgt_L = 0; S.has3d = false;
        HIP_OK(c, c->lmtgt_mem.alloc(&S.tgt, lm_target_words(B, V, L, has3d) * sizeof(float)));
        S.tgt_L = L; S.has3d = has3d;
        S.term = term;
    }
    float* d = S.tgt;
    HIP_OK(c, hipMemcpyAsync(d, xy, ni * 2 * sizeof(float), hipMemcpyDefault, c->stream));
    HIP_OK(c, hipMemcpyAsync(d + ni * 2, conf, ni * sizeof(float), hipMemcpyDefault, c->stream));
    if (has3d) {
        HIP_OK(c, hipMemcpyAsync(d + ni * 3, xyz, nl * 3 * sizeof(float), hipMemcpyDefault, c->stream));
        HIP_OK(c, hipMemcpyAsync(d + ni * 3 + nl * 3, conf3, nl * sizeof(float), hipMemcpyDefault, c->stream));
    }
    HIP_OK(c, hipStreamSynchronize(c->stream));              // the caller may free its buffers now
    S.on = true;
    return MVFIT_OK;
}

static int check_scalars(mvfit_ctx* c, const char* who, float rho, float w3d, float rho3d) {
    if (!std::isfinite(rho) || !std::isfinite(w3d) || !std::isfinite(rho3d) || rho < 0.f || w3d < 0.f || rho3d < 0.f)
        return fail(c, MVFIT_E_ARG, "%s: rho = %g, w3d = %g and rho3d = %g must be finite and >= 0", who, (double)rho, (double)w3d, (double)rho3d);
    return MVFIT_OK;
}

extern "C" int mvfit_landmark_loss(mvfit_ctx* c, const float* vertices, float rho, float w3d, float rho3d, float* loss, float* g_vertices) {
    if (!c) return MVFIT_E_ARG;
    const LmState& S = c->lm;
    if (!S.table) return fail(c, MVFIT_E_STATE, "mvfit_landmark_loss: no landmark table is present (mvfit_set_landmarks)");
    if (!S.on) return fail(c, MVFIT_E_STATE, "mvfit_landmark_loss: no targets are present (mvfit_set_landmark_targets)");
    if (!vertices || !loss) return fail(c, MVFIT_E_ARG, "mvfit_landmark_loss: null %s", !vertices ? "vertices" : "loss");
    if (const int rc = check_scalars(c, "mvfit_landmark_loss", rho, w3d, rho3d)) return rc;
    HIP_OK(c, hipSetDevice(c->device));
    const DevProblems& Q = c->Q;
    const hipError_t e = launch_landmarks(vertices, c->nv, c->B, S.tab, S.L, S.nt, S.tgt, S.has3d,
                                          LmCams{Q.V, Q.cam_batched, Q.cam_R, Q.cam_t, Q.cam_f, Q.cam_c}, rho, w3d, rho3d, nullptr, loss,
                                          g_vertices, c->stream);
    if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "landmark launch: %s", hipGetErrorString(e));
    return MVFIT_OK;
}

// the round buffers of the term (cotangent, loss, pull-back partials) for the current batch: allocated by the first enable and
// kept while B stays
static int ensure_lm_round(mvfit_ctx* c) {
    LmState& S = c->lm;
    if (S.part) return MVFIT_OK;
    HIP_OK(c, hipStreamSynchronize(c->stream));
    c->lmterm_mem.release();                                 // (what an earlier call that failed half-way left)
    S.g_verts = nullptr; S.loss = nullptr;
    HIP_OK(c, c->lmterm_mem.alloc(&S.g_verts, (size_t)c->B * c->nv * 3 * sizeof(float), true));
    HIP_OK(c, c->lmterm_mem.alloc(&S.loss, (size_t)c->B * sizeof(float), true));
    HIP_OK(c, c->lmterm_mem.alloc(&S.part, vjp_part_bytes(c->Bpad, c->nv)));      // last: a term with partials is complete
    return MVFIT_OK;
}

// The landmark term inside mvfit_fit / mvfit_closure (include/mvfit.h): state only - the rounds launch it.
extern "C" int mvfit_set_landmark_term(mvfit_ctx* c, int enable, float rho, float w3d, float rho3d) {
    if (!c) return MVFIT_E_ARG;
    HIP_OK(c, hipSetDevice(c->device));
    if (!enable) {                                           // off: the buffers stay for the next enable of this batch
        c->lm.term = false;
        return MVFIT_OK;
    }
    if (c->B == 0) return fail(c, MVFIT_E_STATE, "call mvfit_set_problems first");
    if (!c->lm.on) return fail(c, MVFIT_E_STATE, "mvfit_set_landmark_term: no targets are present (mvfit_set_landmark_targets)");
    if (c->mix.on) return fail(c, MVFIT_E_STATE, "mvfit_set_landmark_term: the term mix uses the ctx's term slot: switch it off first");
    if (c->sdf_num_faces || c->obst.on || c->silt.on || c->vt.term || c->scant.on)
        return fail(c, MVFIT_E_STATE, "mvfit_set_landmark_term: the %s term uses the ctx's term slot (one term per ctx): remove it first",
                    term_name(c));
    if (const int rc = check_scalars(c, "mvfit_set_landmark_term", rho, w3d, rho3d)) return rc;
    // a failure below leaves the previous state: the flag and the scalars change last
    if (const int rc = ensure_lm_round(c)) return rc;
    if (const int rc = ensure_sdf_buffers(c)) return rc;     // the record slot (SdfAdj) per problem
    c->lm.rho = rho; c->lm.w3d = w3d; c->lm.rho3d = rho3d;
    c->lm.term = true;
    return MVFIT_OK;
}
