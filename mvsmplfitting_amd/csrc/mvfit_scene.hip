// libmvfit: the C ABI (include/mvfit.h), part 3 of 3 - the entries that never run the optimiser: the stand-alone SDF op, the
// scene collision loss and its frozen obstacles, silhouettes, triangulation, association, initial guesses, projection and the
// two renderers.  Argument checks, workspace sizing and grouping; the kernels are behind launchers.h and silhouette.h.
#include "mvfit_ctx.h"

extern "C" int mvfit_sdf(mvfit_ctx* c, const int32_t* faces, int num_faces, const float* vertices, int B, int num_vertices,
                         int G, float* phi) {
    if (!c) return MVFIT_E_ARG;
    if (!faces || !vertices || !phi || num_faces < 0 || B <= 0 || num_vertices <= 0 || G < 2 || G > 1024)
        return fail(c, MVFIT_E_ARG, "mvfit_sdf: bad argument (num_faces=%d B=%d num_vertices=%d G=%d)", num_faces, B, num_vertices, G);
    HIP_OK(c, hipSetDevice(c->device));
    // long face lists: exact culling on face lists (sdf_term.hip), bit-identical to the walk; mvfit_options::sdf_face_lists = 0
    // keeps the walk
    c->sdf_op_path = 0;
    if (sdf_op_uses_lists(num_faces) && c->opt.sdf_face_lists) {
        if (c->sdf_op_B != B || c->sdf_op_F != num_faces) {       // a new shape: decide once (the decision, also a refusal, is kept)
            HIP_OK(c, hipStreamSynchronize(c->stream));
            c->sdf_op_ws.reset();
            size_t free_b = 0, total_b = 0;
            HIP_OK(c, hipMemGetInfo(&free_b, &total_b));
            if (sdf_op_ws_bytes(B, num_faces) < free_b / 2) {
                HIP_OK(c, c->sdf_op_ws.reserve(sdf_op_ws_bytes(B, num_faces)));
                HIP_OK(c, hipMemsetAsync(c->sdf_op_ws.as<unsigned char>() + sdf_cull_zero_offset(B, num_faces), 0, sdf_cull_zero_bytes(B),
                                         c->stream));
            }
            c->sdf_op_B = B; c->sdf_op_F = num_faces;
        }
        if (c->sdf_op_ws.get()) {
            hipError_t e = launch_sdf_voxelize_culled(faces, num_faces, vertices, B, num_vertices, G, phi, c->sdf_op_ws.get(), c->stream);
            if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "sdf launch: %s", hipGetErrorString(e));
            c->sdf_op_path = 1;
            return MVFIT_OK;
        }
        c->sdf_op_path = 2;                                       // the workspace did not fit: the walk
    }
    hipError_t e = launch_sdf_voxelize(faces, num_faces, vertices, B, num_vertices, G, phi, c->stream);
    if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "sdf launch: %s", hipGetErrorString(e));
    return MVFIT_OK;
}

// SDFLoss.forward for num_scenes scenes (scene_sdf.hip).  Groups of consecutive whole scenes whose fields and local vertices
// stay under the 256 MB cap the renderer uses (one scene's, when that alone needs more); inside a group the bodies are
// voxelised in runs whose face lists stay under 2 GB.
// scene_first[num_scenes + 1]: starts at 0, 1 .. MVFIT_SCENE_BODIES_MAX bodies per scene
static int check_scene_first(mvfit_ctx* c, const char* who, const int32_t* scene_first, int num_scenes) {
    if (scene_first[0] != 0) return fail(c, MVFIT_E_ARG, "%s: scene_first[0] = %d, not 0", who, scene_first[0]);
    for (int s = 0; s < num_scenes; ++s) {
        const long long cnt = (long long)scene_first[s + 1] - scene_first[s];
        if (cnt < 0) return fail(c, MVFIT_E_ARG, "%s: scene_first decreases at scene %d", who, s);
        if (cnt == 0) return fail(c, MVFIT_E_ARG, "%s: scene %d is empty", who, s);
        if (cnt > MVFIT_SCENE_BODIES_MAX)
            return fail(c, MVFIT_E_ARG, "%s: scene %d has %lld bodies (at most %d)", who, s, cnt, MVFIT_SCENE_BODIES_MAX);
    }
    return MVFIT_OK;
}

// keep_box / keep_tab (both or neither; then phi_out is set too): the freeze of mvfit_set_scene_obstacles - boxes and table
// rows go to the caller's buffers as well, the faces are the model's own (checked at mvfit_create) and the pair kernels do
// not run (no loss).  Boxes and fields are what the loss call computes: the same kernels on the same inputs.
static int scene_sdf_run(mvfit_ctx* c, const char* who, const float* vertices, int num_vertices, const int32_t* faces, int num_faces,
                         const int32_t* scene_first, int num_scenes, int grid_size, float scale_factor, float robustifier,
                         float* loss, float* g_vertices, float* phi_out, float4* keep_box, int32_t* keep_tab) {
    const bool freeze = keep_box != nullptr;
    if (!vertices || !faces || !scene_first || (!loss && !freeze))
        return fail(c, MVFIT_E_ARG, "%s: null %s", who, !vertices ? "vertices" : !faces ? "faces" : !scene_first ? "scene_first" : "loss");
    if (num_vertices <= 0 || num_faces <= 0 || num_scenes <= 0)
        return fail(c, MVFIT_E_ARG, "%s: bad argument (num_vertices=%d num_faces=%d num_scenes=%d)", who, num_vertices,
                    num_faces, num_scenes);
    if (grid_size < 2 || grid_size > 128) return fail(c, MVFIT_E_ARG, "%s: grid_size %d outside [2, 128]", who, grid_size);
    if (const int rc = check_scene_first(c, who, scene_first, num_scenes)) return rc;
    const int N = scene_first[num_scenes];
    HIP_OK(c, hipSetDevice(c->device));
    // the voxelisation reads vertices through the face indices: checked on the host, as mvfit_set_sdf does (this also
    // orders the call behind the earlier ones: the staging below is free again)
    HIP_OK(c, hipStreamSynchronize(c->stream));
    if (!freeze) {
        std::vector<int32_t> h((size_t)num_faces * 3);
        HIP_OK(c, hipMemcpy(h.data(), faces, h.size() * 4, hipMemcpyDefault));
        for (int32_t vi : h)
            if (vi < 0 || vi >= num_vertices)
                return fail(c, MVFIT_E_ARG, "%s: face vertex index %d outside [0, %d)", who, (int)vi, num_vertices);
    }
    const int G = grid_size, nblk = scene_sdf_blocks(num_vertices);
    const size_t nvox = (size_t)G * G * G, cap = (size_t)256 << 20;
    const bool lists = sdf_op_uses_lists(num_faces) && c->opt.sdf_face_lists;
    const size_t per_body = (phi_out ? 0 : nvox * 4) + (size_t)num_vertices * 12;
    std::vector<int> group_end;                  // scene index one past each group
    int nb_max = 0;
    for (int s0 = 0; s0 < num_scenes;) {
        int s1 = s0 + 1;
        while (s1 < num_scenes && (size_t)(scene_first[s1 + 1] - scene_first[s0]) * per_body <= cap &&
               scene_first[s1 + 1] - scene_first[s0] <= 4096)
            ++s1;
        group_end.push_back(s1);
        nb_max = std::max(nb_max, scene_first[s1] - scene_first[s0]);
        s0 = s1;
    }
    // bodies voxelised per run of the face-list kernels: as many as the group has while the lists stay under 2 GB (11.6 MB per
    // body at 13,776 faces; one run of 128 bodies takes half the time of six runs of 22 - every run ends in a tail of few busy
    // workgroups) and, when the workspace has to grow, under half of the free memory, as mvfit_sdf decides it
    int run = lists ? (int)std::min<size_t>((size_t)nb_max, std::max<size_t>(1, ((size_t)2 << 30) / sdf_op_ws_bytes(1, num_faces))) : 0;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_tab = 0, o_first = o_tab + al((size_t)N * 16), o_box = o_first + al((size_t)(num_scenes + 1) * 4);
    const size_t o_part = o_box + al((size_t)N * 16), o_local = o_part + al((size_t)nb_max * nblk * 4);
    const size_t o_phi = o_local + al((size_t)nb_max * num_vertices * 12), o_cull = o_phi + (phi_out ? 0 : al((size_t)nb_max * nvox * 4));
    size_t need = o_cull + (lists ? sdf_op_ws_bytes(run, num_faces) : 0);
    if (need > c->scn_ws.size()) {
        c->scn_ws.reset();
        size_t free_b = 0, total_b = 0;
        HIP_OK(c, hipMemGetInfo(&free_b, &total_b));
        while (run > 1 && need > free_b / 2) {
            run = (run + 1) / 2;
            need = o_cull + sdf_op_ws_bytes(run, num_faces);
        }
        HIP_OK(c, c->scn_ws.reserve(need));
    }
    const size_t tb = o_box;                     // tables: a row per body, then scene_first
    HIP_OK(c, c->h_scn_tab.reserve(tb));
    int32_t* h_tab = c->h_scn_tab.as<int32_t>();
    for (int s = 0; s < num_scenes; ++s)
        for (int b = scene_first[s]; b < scene_first[s + 1]; ++b) {
            int32_t* r = h_tab + (size_t)b * 4;
            r[0] = scene_first[s]; r[1] = scene_first[s + 1] - scene_first[s]; r[2] = 0; r[3] = 0;
        }
    memcpy(c->h_scn_tab.as<unsigned char>() + o_first, scene_first, (size_t)(num_scenes + 1) * 4);
    unsigned char* ws = c->scn_ws.as<unsigned char>();
    HIP_OK(c, hipMemcpyAsync(ws, h_tab, tb, hipMemcpyHostToDevice, c->stream));
    if (freeze) HIP_OK(c, hipMemcpyAsync(keep_tab, h_tab, (size_t)N * 16, hipMemcpyHostToDevice, c->stream));
    float4* box = freeze ? keep_box : reinterpret_cast<float4*>(ws + o_box);
    float* part = reinterpret_cast<float*>(ws + o_part);
    float* local = reinterpret_cast<float*>(ws + o_local);
    const float factor = (float)((1.0 + (double)scale_factor) * 0.5);
    c->sdf_op_path = lists ? 1 : 0;
    int s0 = 0;
    for (int s1 : group_end) {
        const int b0 = scene_first[s0], n = scene_first[s1] - b0;
        float* phi = phi_out ? phi_out + (size_t)b0 * nvox : reinterpret_cast<float*>(ws + o_phi);
        hipError_t e = launch_scene_boxes(vertices, num_vertices, b0, n, factor, box, local, c->stream);
        if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "%s: box launch: %s", who, hipGetErrorString(e));
        if (lists) {
            for (int r0 = 0; r0 < n; r0 += run) {
                const int rn = std::min(run, n - r0);
                // the lists' count area must be zero where this run's layout puts it
                HIP_OK(c, hipMemsetAsync(ws + o_cull + sdf_cull_zero_offset(rn, num_faces), 0, sdf_cull_zero_bytes(rn), c->stream));
                e = launch_sdf_voxelize_culled(faces, num_faces, local + (size_t)r0 * num_vertices * 3, rn, num_vertices, G,
                                               phi + (size_t)r0 * nvox, ws + o_cull, c->stream);
                if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "%s: sdf launch: %s", who, hipGetErrorString(e));
            }
        } else {
            e = launch_sdf_voxelize(faces, num_faces, local, n, num_vertices, G, phi, c->stream);
            if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "%s: sdf launch: %s", who, hipGetErrorString(e));
        }
        if (freeze) { s0 = s1; continue; }
        e = launch_scene_pairs(vertices, num_vertices, b0, n, s0, s1 - s0, ws + o_tab, reinterpret_cast<const int32_t*>(ws + o_first),
                               box, phi, G, robustifier, g_vertices, part, loss, c->stream);
        if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "%s: pair launch: %s", who, hipGetErrorString(e));
        s0 = s1;
    }
    return MVFIT_OK;
}

extern "C" int mvfit_scene_sdf_loss(mvfit_ctx* c, const float* vertices, int num_vertices, const int32_t* faces, int num_faces,
                                    const int32_t* scene_first, int num_scenes, int grid_size, float scale_factor,
                                    float robustifier, float* loss, float* g_vertices, float* phi_out) {
    if (!c) return MVFIT_E_ARG;
    return scene_sdf_run(c, "mvfit_scene_sdf_loss", vertices, num_vertices, faces, num_faces, scene_first, num_scenes, grid_size,
                         scale_factor, robustifier, loss, g_vertices, phi_out, nullptr, nullptr);
}

// Freeze the obstacles of the scene term at `vertices` (scene_sdf.hip: scene_entries_kernel reads them in every chained round).
extern "C" int mvfit_set_scene_obstacles(mvfit_ctx* c, const float* vertices, const int32_t* scene_first, int num_scenes,
                                         int grid_size, float scale_factor, float robustifier) {
    if (!c) return MVFIT_E_ARG;
    HIP_OK(c, hipSetDevice(c->device));
    if (!vertices) {                                         // remove: the buffers stay for the next freeze of this batch
        term_source_gone(c, SRC_OBSTACLES);                  // no obstacles: no scene term and no mix that uses them
        return MVFIT_OK;
    }
    if (c->B == 0) return fail(c, MVFIT_E_STATE, "call mvfit_set_problems first");
    if (!c->num_faces) return fail(c, MVFIT_E_STATE, "mvfit_set_scene_obstacles: the model was created without (valid) faces");
    if (c->sdf_num_faces)
        return fail(c, MVFIT_E_STATE, "mvfit_set_scene_obstacles: mvfit_set_sdf's term is the interpenetration term (one per ctx): remove it first");
    if (c->silt.on)
        return fail(c, MVFIT_E_STATE, "mvfit_set_scene_obstacles: the silhouette term uses the ctx's term slot: switch it off first");
    if (c->vt.term)
        return fail(c, MVFIT_E_STATE, "mvfit_set_scene_obstacles: the vertex-target term uses the ctx's term slot: switch it off first");
    if (c->scant.on)
        return fail(c, MVFIT_E_STATE, "mvfit_set_scene_obstacles: the scan term uses the ctx's term slot: switch it off first");
    if (c->lm.term)
        return fail(c, MVFIT_E_STATE, "mvfit_set_scene_obstacles: the landmark term uses the ctx's term slot: switch it off first");
    if (c->nv > 8192) return fail(c, MVFIT_E_UNSUPPORTED, "the scene term supports up to 8192 vertices (model has %d)", c->nv);
    if (!scene_first || num_scenes <= 0) return fail(c, MVFIT_E_ARG, "mvfit_set_scene_obstacles: bad argument (num_scenes=%d)", num_scenes);
    if (grid_size < 2 || grid_size > 128) return fail(c, MVFIT_E_ARG, "mvfit_set_scene_obstacles: grid_size %d outside [2, 128]", grid_size);
    int rc = check_scene_first(c, "mvfit_set_scene_obstacles", scene_first, num_scenes);
    if (rc) return rc;
    if (scene_first[num_scenes] != c->B)
        return fail(c, MVFIT_E_ARG, "mvfit_set_scene_obstacles: the scenes hold %d bodies, the ctx %d problems", scene_first[num_scenes], c->B);
    const size_t nvox = (size_t)grid_size * grid_size * grid_size;
    TermSuspend off(c, SRC_OBSTACLES);                       // a failed freeze leaves no term behind (and no mix that uses it)
    if (c->obst.grid != grid_size || !c->obst.phi) {
        HIP_OK(c, hipStreamSynchronize(c->stream));
        free_obstacles(c);
        HIP_OK(c, c->obst_mem.alloc(&c->obst.tab, (size_t)c->B * 16));
        HIP_OK(c, c->obst_mem.alloc(&c->obst.box, (size_t)c->B * sizeof(float4)));
        HIP_OK(c, c->obst_mem.alloc(&c->obst.phi, (size_t)c->B * nvox * 4));
        c->obst.grid = grid_size;
    }
    rc = ensure_sdf_buffers(c);
    if (rc) return rc;
    hipError_t e = launch_scene_null_boxes(c->pb.sdf_box, c->B, c->stream);
    if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "mvfit_set_scene_obstacles: box launch: %s", hipGetErrorString(e));
    rc = scene_sdf_run(c, "mvfit_set_scene_obstacles", vertices, c->nv, c->d_faces, c->num_faces, scene_first, num_scenes, grid_size,
                       scale_factor, robustifier, nullptr, nullptr, c->obst.phi, c->obst.box, c->obst.tab);
    if (rc) return rc;
    c->obst.rob = robustifier;
    off.restore();
    c->obst.on = true;
    return MVFIT_OK;
}

extern "C" int mvfit_scene_obstacles_read(mvfit_ctx* c, float* phi, float* boxes) {
    if (!c) return MVFIT_E_ARG;
    if (!c->obst.on) return fail(c, MVFIT_E_STATE, "mvfit_scene_obstacles_read: no obstacles are set");
    HIP_OK(c, hipSetDevice(c->device));
    const size_t nvox = (size_t)c->obst.grid * c->obst.grid * c->obst.grid;
    if (phi) HIP_OK(c, hipMemcpyAsync(phi, c->obst.phi, (size_t)c->B * nvox * 4, hipMemcpyDeviceToDevice, c->stream));
    if (boxes) HIP_OK(c, hipMemcpyAsync(boxes, c->obst.box, (size_t)c->B * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    return MVFIT_OK;
}

// The silhouette term (silhouette.hip): the mask set is prepared once, the loss calls sample it.
extern "C" int mvfit_set_silhouettes(mvfit_ctx* c, int num_images, int height, int width, const uint8_t* masks,
                                     const int32_t* image_body, const float* cam_R, const float* cam_t, const float* cam_f,
                                     const float* cam_c, int contour_stride) {
    if (!c) return MVFIT_E_ARG;
    c->sil.occ_on = false;                                   // the occluders belong to the mask set: every call clears them
    HIP_OK(c, hipSetDevice(c->device));
    if (num_images == 0) {                                   // clear: the work areas stay for a next set of the same size
        c->sil.on = false;
        term_source_gone(c, SRC_MASKS);                      // no masks: no term and no mix that uses them
        return MVFIT_OK;
    }
    if (num_images < 0 || num_images > 65535 || height < 2 || height > 8192 || width < 2 || width > 8192)
        return fail(c, MVFIT_E_ARG, "mvfit_set_silhouettes: sizes out of range (num_images=%d in [0, 65535], height=%d and "
                    "width=%d in [2, 8192])", num_images, height, width);
    if (contour_stride < 1) return fail(c, MVFIT_E_ARG, "mvfit_set_silhouettes: contour_stride %d < 1", contour_stride);
    if (!masks || !image_body || !cam_R || !cam_t || !cam_f || !cam_c)
        return fail(c, MVFIT_E_ARG, "mvfit_set_silhouettes: null %s", !masks ? "masks" : !image_body ? "image_body" : !cam_R ? "cam_R" :
                    !cam_t ? "cam_t" : !cam_f ? "cam_f" : "cam_c");
    const int rc = sil_set(c->sil, c->nv, num_images, height, width, masks, image_body, cam_R, cam_t, cam_f, cam_c, contour_stride,
                           c->stream, c->err);
    // a set that replaces the one of an enabled term must fit the batch like the first (the term's kernels index the
    // problems' buffers by image_body); a failed or unfit set leaves no term behind
    const bool in_mix = c->mix.on && c->mix.silhouette > 0.f;
    if ((c->silt.on || in_mix) && (rc || c->sil.body_min < 0 || c->sil.body_max >= c->B)) {
        term_source_gone(c, SRC_MASKS);
        if (!rc)
            return fail(c, MVFIT_E_ARG, "mvfit_set_silhouettes: image_body holds %d .. %d, outside the %d problems of the enabled "
                        "silhouette term (the term is switched off)", c->sil.body_min, c->sil.body_max, c->B);
    }
    return rc;
}

// the round buffers of the silhouette term (cotangent, loss, pull-back partials) for the current batch: allocated by the
// first caller - the term's own setter or the term mix - and kept while B stays
static int ensure_sil_round(mvfit_ctx* c) {
    if (c->silt.part) return MVFIT_OK;
    HIP_OK(c, hipStreamSynchronize(c->stream));
    c->silterm_mem.release();                                // (what an earlier call that failed half-way left)
    c->silt = SilTerm{};
    float *g = nullptr, *l = nullptr;
    HIP_OK(c, c->silterm_mem.alloc(&g, (size_t)c->B * c->nv * 3 * sizeof(float), true));
    HIP_OK(c, c->silterm_mem.alloc(&l, (size_t)c->B * sizeof(float), true));
    c->silt.g_verts = g; c->silt.loss = l;
    HIP_OK(c, c->silterm_mem.alloc(&c->silt.part, vjp_part_bytes(c->Bpad, c->nv)));      // last: a term with partials is complete
    return MVFIT_OK;
}

// the same for the vertex-target term
static int ensure_vt_round(mvfit_ctx* c) {
    VtxTargets& T = c->vt;
    if (T.part) return MVFIT_OK;
    HIP_OK(c, hipStreamSynchronize(c->stream));
    c->vtterm_mem.release();                                 // (what an earlier call that failed half-way left)
    T.g_verts = nullptr; T.loss = nullptr;
    HIP_OK(c, c->vtterm_mem.alloc(&T.g_verts, (size_t)c->B * c->nv * 3 * sizeof(float), true));
    HIP_OK(c, c->vtterm_mem.alloc(&T.loss, (size_t)c->B * sizeof(float), true));
    HIP_OK(c, c->vtterm_mem.alloc(&T.part, vjp_part_bytes(c->Bpad, c->nv)));      // last: a term with partials is complete
    return MVFIT_OK;
}

// The silhouette term inside mvfit_fit / mvfit_closure (include/mvfit.h): state only - the rounds launch it (round_term.cpp plans the launches).
extern "C" int mvfit_set_silhouette_term(mvfit_ctx* c, int enable, float w_in, float w_out, float sigma) {
    if (!c) return MVFIT_E_ARG;
    HIP_OK(c, hipSetDevice(c->device));
    if (!enable) {                                           // off: the buffers stay for the next enable of this batch
        c->silt.on = false;
        return MVFIT_OK;
    }
    if (c->B == 0) return fail(c, MVFIT_E_STATE, "call mvfit_set_problems first");
    if (!c->sil.on) return fail(c, MVFIT_E_STATE, "mvfit_set_silhouette_term: no mask set is present (mvfit_set_silhouettes)");
    if (c->mix.on) return fail(c, MVFIT_E_STATE, "mvfit_set_silhouette_term: the term mix uses the ctx's term slot: switch it off first");
    if (c->vt.term)
        return fail(c, MVFIT_E_STATE, "mvfit_set_silhouette_term: the vertex-target term uses the ctx's term slot: switch it off first");
    if (c->scant.on)
        return fail(c, MVFIT_E_STATE, "mvfit_set_silhouette_term: the scan term uses the ctx's term slot: switch it off first");
    if (c->lm.term)
        return fail(c, MVFIT_E_STATE, "mvfit_set_silhouette_term: the landmark term uses the ctx's term slot: switch it off first");
    if (c->sdf_num_faces || c->obst.on)
        return fail(c, MVFIT_E_STATE, "mvfit_set_silhouette_term: %s the ctx's term slot (one term per ctx): remove %s first",
                    c->obst.on ? "scene obstacles use" : "mvfit_set_sdf's term uses", c->obst.on ? "them" : "it");
    if (!std::isfinite(w_in) || !std::isfinite(w_out) || !std::isfinite(sigma) || w_in < 0.f || w_out < 0.f)
        return fail(c, MVFIT_E_ARG, "mvfit_set_silhouette_term: w_in = %g and w_out = %g must be finite and >= 0, sigma = %g finite",
                    (double)w_in, (double)w_out, (double)sigma);
    if (c->sil.body_min < 0 || c->sil.body_max >= c->B)
        return fail(c, MVFIT_E_ARG, "mvfit_set_silhouette_term: image_body holds %d .. %d, outside [0, %d)", c->sil.body_min,
                    c->sil.body_max, c->B);
    if (const int rc = ensure_sil_round(c)) return rc;
    if (const int rc = ensure_sdf_buffers(c)) return rc;     // the record slot (SdfAdj) per problem
    c->silt.w_in = w_in; c->silt.w_out = w_out; c->silt.sigma = sigma;
    c->silt.on = true;
    return MVFIT_OK;
}

extern "C" int mvfit_silhouettes_read(mvfit_ctx* c, float* field, int32_t* contour_first, int32_t* contour_xy, int32_t* num_points) {
    if (!c) return MVFIT_E_ARG;
    if (!c->sil.on) return fail(c, MVFIT_E_STATE, "mvfit_silhouettes_read: no mask set is present");
    HIP_OK(c, hipSetDevice(c->device));
    if (num_points) *num_points = c->sil.C;
    return sil_read(c->sil, field, contour_first, contour_xy, c->stream, c->err);
}

extern "C" int mvfit_silhouette_loss(mvfit_ctx* c, const float* vertices, int num_bodies, float w_in, float w_out, float sigma,
                                     float* loss, float* g_vertices, int32_t* winner) {
    if (!c) return MVFIT_E_ARG;
    if (!c->sil.on) return fail(c, MVFIT_E_STATE, "mvfit_silhouette_loss: no mask set is present (mvfit_set_silhouettes)");
    if (!vertices || !loss) return fail(c, MVFIT_E_ARG, "mvfit_silhouette_loss: null %s", !vertices ? "vertices" : "loss");
    if (num_bodies < 1 || num_bodies > 65535)
        return fail(c, MVFIT_E_ARG, "mvfit_silhouette_loss: num_bodies %d outside [1, 65535]", num_bodies);
    if (c->sil.body_min < 0 || c->sil.body_max >= num_bodies)
        return fail(c, MVFIT_E_ARG, "mvfit_silhouette_loss: image_body holds %d .. %d, outside [0, %d)", c->sil.body_min,
                    c->sil.body_max, num_bodies);
    HIP_OK(c, hipSetDevice(c->device));
    return sil_loss(c->sil, vertices, num_bodies, w_in, w_out, sigma, loss, g_vertices, winner, c->stream, c->err);
}

// Occlusion between the bodies of a scene (include/mvfit.h; silhouette_occlusion.hip): the other bodies frozen as depth maps per
// mask image.  State of the mask set: the evaluation entries and the rounds read it (silhouette.hip: sil_loss / sil_round).
extern "C" int mvfit_set_silhouette_occluders(mvfit_ctx* c, const float* vertices, int num_bodies, const int32_t* body_scene,
                                              float margin) {
    if (!c) return MVFIT_E_ARG;
    c->sil.occ_on = false;                                   // a failed freeze leaves none set
    if (num_bodies == 0 || !vertices) return MVFIT_OK;       // clear: the buffers stay for the next freeze
    if (!c->sil.on) return fail(c, MVFIT_E_STATE, "mvfit_set_silhouette_occluders: no mask set is present (mvfit_set_silhouettes)");
    if (!c->num_faces) return fail(c, MVFIT_E_STATE, "mvfit_set_silhouette_occluders: the model was created without (valid) faces");
    if (!body_scene) return fail(c, MVFIT_E_ARG, "mvfit_set_silhouette_occluders: null body_scene");
    if (num_bodies < 1 || num_bodies > 65535)
        return fail(c, MVFIT_E_ARG, "mvfit_set_silhouette_occluders: num_bodies %d outside [1, 65535]", num_bodies);
    if (c->sil.body_min < 0 || c->sil.body_max >= num_bodies)
        return fail(c, MVFIT_E_ARG, "mvfit_set_silhouette_occluders: image_body holds %d .. %d, outside [0, %d)", c->sil.body_min,
                    c->sil.body_max, num_bodies);
    if (!std::isfinite(margin) || margin < 0.f)
        return fail(c, MVFIT_E_ARG, "mvfit_set_silhouette_occluders: margin = %g must be finite and >= 0", (double)margin);
    HIP_OK(c, hipSetDevice(c->device));
    return sil_occ_set(c->sil, vertices, num_bodies, body_scene, margin, c->d_faces, c->num_faces, c->stream, c->err);
}

extern "C" int mvfit_silhouette_occluders_read(mvfit_ctx* c, float* z_occ, float* z_own, uint8_t* point_flag) {
    if (!c) return MVFIT_E_ARG;
    if (!c->sil.on || !c->sil.occ_on) return fail(c, MVFIT_E_STATE, "mvfit_silhouette_occluders_read: no occluders are set");
    HIP_OK(c, hipSetDevice(c->device));
    return sil_occ_read(c->sil, z_occ, z_own, point_flag, c->stream, c->err);
}

extern "C" int mvfit_silhouette_hidden(mvfit_ctx* c, const float* vertices, int num_bodies, uint8_t* hidden) {
    if (!c) return MVFIT_E_ARG;
    if (!c->sil.on) return fail(c, MVFIT_E_STATE, "mvfit_silhouette_hidden: no mask set is present (mvfit_set_silhouettes)");
    if (!vertices || !hidden) return fail(c, MVFIT_E_ARG, "mvfit_silhouette_hidden: null %s", !vertices ? "vertices" : "hidden");
    if (num_bodies < 1 || num_bodies > 65535)
        return fail(c, MVFIT_E_ARG, "mvfit_silhouette_hidden: num_bodies %d outside [1, 65535]", num_bodies);
    if (c->sil.body_min < 0 || c->sil.body_max >= num_bodies)
        return fail(c, MVFIT_E_ARG, "mvfit_silhouette_hidden: image_body holds %d .. %d, outside [0, %d)", c->sil.body_min,
                    c->sil.body_max, num_bodies);
    HIP_OK(c, hipSetDevice(c->device));
    return sil_occ_hidden(c->sil, vertices, hidden, c->stream, c->err);
}

// The vertex-target set (include/mvfit.h; vertex_target.hip).  The set's three buffers are re-made only when K changes (B
// cannot: free_problem_buffers drops them), so a re-freeze keeps their addresses.
extern "C" int mvfit_set_vertex_targets(mvfit_ctx* c, int K, const float* targets, const float* weights) {
    if (!c) return MVFIT_E_ARG;
    HIP_OK(c, hipSetDevice(c->device));
    if (K == 0 || !targets) {                                // clear: the buffers stay for a next set of the same shape
        c->vt.on = false;
        term_source_gone(c, SRC_TARGETS);                    // no targets: no term and no mix that uses them
        return MVFIT_OK;
    }
    if (c->B == 0) return fail(c, MVFIT_E_STATE, "call mvfit_set_problems first");
    if (K < 1 || K > MVFIT_VERTEX_TARGETS_MAX)
        return fail(c, MVFIT_E_ARG, "mvfit_set_vertex_targets: K = %d outside [1, %d]", K, MVFIT_VERTEX_TARGETS_MAX);
    if (!weights) return fail(c, MVFIT_E_ARG, "mvfit_set_vertex_targets: null weights");
    for (size_t i = 0; i < (size_t)c->B * K; ++i)
        if (!std::isfinite(weights[i]) || weights[i] < 0.f)
            return fail(c, MVFIT_E_ARG, "mvfit_set_vertex_targets: weight %g of problem %d, target %d must be finite and >= 0",
                        (double)weights[i], (int)(i / K), (int)(i % K));
    const size_t row = (size_t)c->nv * 3 * sizeof(float);
    VtxTargets& T = c->vt;
    if (!T.partial || T.K != K) {
        HIP_OK(c, hipStreamSynchronize(c->stream));
        TermSuspend off(c, SRC_TARGETS);                     // (a failed allocation leaves no set and no term behind)
        c->vtgt_mem.release();
        T.on = false;
        T.targets = nullptr; T.weights = nullptr; T.partial = nullptr; T.K = 0;
        HIP_OK(c, c->vtgt_mem.alloc(&T.targets, (size_t)c->B * K * row));
        HIP_OK(c, c->vtgt_mem.alloc(&T.weights, (size_t)c->B * K * sizeof(float)));
        HIP_OK(c, c->vtgt_mem.alloc(&T.partial, (size_t)c->B * vertex_target_blocks(c->nv) * sizeof(double), true));   // last: a set with partials is complete
        T.K = K;
        off.restore();
    }
    HIP_OK(c, hipMemcpyAsync(T.targets, targets, (size_t)c->B * K * row, hipMemcpyDefault, c->stream));
    HIP_OK(c, hipMemcpyAsync(T.weights, weights, (size_t)c->B * K * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_OK(c, hipStreamSynchronize(c->stream));              // the caller may free both now
    T.on = true;
    return MVFIT_OK;
}

extern "C" int mvfit_vertex_target_loss(mvfit_ctx* c, const float* vertices, float* loss, float* g_vertices) {
    if (!c) return MVFIT_E_ARG;
    if (!c->vt.on) return fail(c, MVFIT_E_STATE, "mvfit_vertex_target_loss: no target set is present (mvfit_set_vertex_targets)");
    if (!vertices || !loss) return fail(c, MVFIT_E_ARG, "mvfit_vertex_target_loss: null %s", !vertices ? "vertices" : "loss");
    HIP_OK(c, hipSetDevice(c->device));
    const VtxTargets& T = c->vt;
    const hipError_t e = launch_vertex_target(vertices, c->nv, c->B, T.K, T.targets, T.weights, nullptr, T.partial, loss, g_vertices, c->stream);
    if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "vertex-target launch: %s", hipGetErrorString(e));
    return MVFIT_OK;
}

// The vertex-target term inside mvfit_fit / mvfit_closure (include/mvfit.h): state only - the rounds launch it (round_term.cpp plans the launches).
extern "C" int mvfit_set_vertex_target_term(mvfit_ctx* c, int enable) {
    if (!c) return MVFIT_E_ARG;
    HIP_OK(c, hipSetDevice(c->device));
    if (!enable) {                                           // off: the buffers stay for the next enable of this batch
        c->vt.term = false;
        return MVFIT_OK;
    }
    if (c->B == 0) return fail(c, MVFIT_E_STATE, "call mvfit_set_problems first");
    if (!c->vt.on) return fail(c, MVFIT_E_STATE, "mvfit_set_vertex_target_term: no target set is present (mvfit_set_vertex_targets)");
    if (c->mix.on) return fail(c, MVFIT_E_STATE, "mvfit_set_vertex_target_term: the term mix uses the ctx's term slot: switch it off first");
    if (c->sdf_num_faces || c->obst.on || c->silt.on || c->scant.on || c->lm.term)
        return fail(c, MVFIT_E_STATE, "mvfit_set_vertex_target_term: the %s term uses the ctx's term slot (one term per ctx): remove it first",
                    term_name(c));
    if (const int rc = ensure_vt_round(c)) return rc;
    if (const int rc = ensure_sdf_buffers(c)) return rc;     // the record slot (SdfAdj) per problem
    c->vt.term = true;
    return MVFIT_OK;
}

// The weighted sum of the scene, silhouette, vertex-target and scan terms inside mvfit_fit / mvfit_closure (include/mvfit.h): state
// and buffers only - the rounds launch it (round_term.cpp plans the launches).
extern "C" int mvfit_set_term_mix(mvfit_ctx* c, const mvfit_term_mix* mix) {
    if (!c) return MVFIT_E_ARG;
    HIP_OK(c, hipSetDevice(c->device));
    if (!mix) {                                              // off: the buffers stay for the next enable of this batch
        c->mix.on = false;
        return MVFIT_OK;
    }
    // exactly the layout before the scan share (its fields read as 0) or exactly this one
    if (mix->size != MVFIT_TERM_MIX_SIZE_V1 && mix->size != sizeof(mvfit_term_mix))
        return fail(c, MVFIT_E_ARG, "mvfit_set_term_mix: size %u is neither %u nor %zu", mix->size, (unsigned)MVFIT_TERM_MIX_SIZE_V1, sizeof(mvfit_term_mix));
    const bool v1 = mix->size == MVFIT_TERM_MIX_SIZE_V1;
    const float lam[4] = {mix->scene, mix->silhouette, mix->vertex_targets, v1 ? 0.f : mix->scan};
    const float zw_s2m = v1 ? 0.f : mix->scan_w_s2m, zw_m2s = v1 ? 0.f : mix->scan_w_m2s, zsigma = v1 ? 0.f : mix->scan_sigma;
    int live = 0;
    for (float l : lam) {
        if (!std::isfinite(l) || l < 0.f)
            return fail(c, MVFIT_E_ARG, "mvfit_set_term_mix: the shares (%g, %g, %g, %g) must be finite and >= 0", (double)lam[0], (double)lam[1],
                        (double)lam[2], (double)lam[3]);
        live += l > 0.f;
    }
    if (live < 2)
        return fail(c, MVFIT_E_ARG, "mvfit_set_term_mix: at least two shares must be > 0 (a single term keeps its own setter)");
    if (lam[1] > 0.f && (!std::isfinite(mix->sil_w_in) || !std::isfinite(mix->sil_w_out) || !std::isfinite(mix->sil_sigma) ||
                         mix->sil_w_in < 0.f || mix->sil_w_out < 0.f))
        return fail(c, MVFIT_E_ARG, "mvfit_set_term_mix: sil_w_in = %g and sil_w_out = %g must be finite and >= 0, sil_sigma = %g finite",
                    (double)mix->sil_w_in, (double)mix->sil_w_out, (double)mix->sil_sigma);
    if (lam[3] > 0.f) {                                      // (as mvfit_set_scan_term checks them)
        if (!std::isfinite(zw_s2m) || !std::isfinite(zw_m2s) || !std::isfinite(zsigma) || zw_s2m < 0.f || zw_m2s < 0.f || zsigma < 0.f)
            return fail(c, MVFIT_E_ARG, "mvfit_set_term_mix: scan_w_s2m = %g, scan_w_m2s = %g and scan_sigma = %g must be finite and >= 0",
                        (double)zw_s2m, (double)zw_m2s, (double)zsigma);
        if (!(zw_s2m > 0.f) && !(zw_m2s > 0.f)) return fail(c, MVFIT_E_ARG, "mvfit_set_term_mix: scan_w_s2m and scan_w_m2s are both 0");
    }
    if (c->B == 0) return fail(c, MVFIT_E_STATE, "call mvfit_set_problems first");
    if (c->sdf_num_faces)
        return fail(c, MVFIT_E_STATE, "mvfit_set_term_mix: mvfit_set_sdf's term uses the ctx's term slot and is not part of the mix: remove it first");
    if (c->silt.on || c->vt.term || c->scant.on || c->lm.term)
        return fail(c, MVFIT_E_STATE, "mvfit_set_term_mix: the %s term is on through its own setter: switch it off first", term_name(c));
    if (lam[0] > 0.f && !c->obst.on) return fail(c, MVFIT_E_STATE, "mvfit_set_term_mix: scene > 0 needs obstacles (mvfit_set_scene_obstacles)");
    if (lam[1] > 0.f && !c->sil.on) return fail(c, MVFIT_E_STATE, "mvfit_set_term_mix: silhouette > 0 needs a mask set (mvfit_set_silhouettes)");
    if (lam[2] > 0.f && !c->vt.on) return fail(c, MVFIT_E_STATE, "mvfit_set_term_mix: vertex_targets > 0 needs a target set (mvfit_set_vertex_targets)");
    if (lam[1] > 0.f && (c->sil.body_min < 0 || c->sil.body_max >= c->B))
        return fail(c, MVFIT_E_ARG, "mvfit_set_term_mix: image_body holds %d .. %d, outside [0, %d)", c->sil.body_min, c->sil.body_max, c->B);
    if (lam[3] > 0.f && !c->scan.on) return fail(c, MVFIT_E_STATE, "mvfit_set_term_mix: scan > 0 needs a scan set (mvfit_set_scans)");
    if (lam[3] > 0.f && c->scan.N != c->B)
        return fail(c, MVFIT_E_ARG, "mvfit_set_term_mix: the scan set holds %d bodies, the ctx %d problems (scan body n is problem n)", c->scan.N, c->B);
    TermMix& X = c->mix;
    if (!X.sums) {
        HIP_OK(c, hipStreamSynchronize(c->stream));
        free_term_mix(c);                                    // (what an earlier call that failed half-way left)
        HIP_OK(c, c->mix_mem.alloc(&X.g_verts, (size_t)c->B * c->nv * 3 * sizeof(float), true));
        HIP_OK(c, c->mix_mem.alloc(&X.loss, (size_t)c->B * sizeof(float), true));
        HIP_OK(c, c->mix_mem.alloc(&X.part, vjp_part_bytes(c->Bpad, c->nv)));
        HIP_OK(c, c->mix_mem.alloc(&X.rec_scene, (size_t)c->B * sizeof(SdfAdj), true));
        HIP_OK(c, c->mix_mem.alloc(&X.rec_verts, (size_t)c->B * sizeof(SdfAdj), true));
        HIP_OK(c, c->mix_mem.alloc(&X.parts, (size_t)c->B * 4 * sizeof(float), true));
        HIP_OK(c, c->mix_mem.alloc(&X.sums, (size_t)c->B * sizeof(float), true));      // last: a mix with sums is complete
    }
    X.on = false;                                            // (a failed allocation below leaves no mix behind)
    if (lam[1] > 0.f) { if (const int rc = ensure_sil_round(c)) return rc; }
    if (lam[2] > 0.f) { if (const int rc = ensure_vt_round(c)) return rc; }
    if (lam[3] > 0.f) { if (const int rc = ensure_scan_round(c)) return rc; }
    if (const int rc = ensure_sdf_buffers(c)) return rc;     // the record slot (SdfAdj) per problem
    X.scene = lam[0]; X.silhouette = lam[1]; X.vertex_targets = lam[2]; X.scan = lam[3];
    X.w_in = mix->sil_w_in; X.w_out = mix->sil_w_out; X.sigma = mix->sil_sigma;
    X.scan_w_s2m = zw_s2m; X.scan_w_m2s = zw_m2s; X.scan_sigma = zsigma;
    X.on = true;
    return MVFIT_OK;
}

// the mix's two kernels on the caller's buffers (include/mvfit.h): what the tests hold against the NumPy restatement
extern "C" int mvfit_term_mix_cotangent(mvfit_ctx* c, float silhouette, const float* g_sil, const float* L_sil, float vertex_targets,
                                        const float* g_vt, const float* L_vt, float* g, float* L_v) {
    if (!c) return MVFIT_E_ARG;
    if (c->B == 0) return fail(c, MVFIT_E_STATE, "call mvfit_set_problems first");
    const bool sil = silhouette > 0.f, vt = vertex_targets > 0.f;
    if (!std::isfinite(silhouette) || !std::isfinite(vertex_targets) || silhouette < 0.f || vertex_targets < 0.f || (!sil && !vt))
        return fail(c, MVFIT_E_ARG, "mvfit_term_mix_cotangent: the shares (%g, %g) must be finite and >= 0, one of them > 0",
                    (double)silhouette, (double)vertex_targets);
    if (!g || !L_v || (sil && (!g_sil || !L_sil)) || (vt && (!g_vt || !L_vt)))
        return fail(c, MVFIT_E_ARG, "mvfit_term_mix_cotangent: null buffer of a live component or of the result");
    HIP_OK(c, hipSetDevice(c->device));
    const hipError_t e = launch_term_mix_cotangent(c->nv, c->B, silhouette, g_sil, L_sil, vertex_targets, g_vt, L_vt, 0.f, nullptr, nullptr,
                                                   nullptr, g, L_v, nullptr, nullptr, c->stream);
    if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "term-mix cotangent launch: %s", hipGetErrorString(e));
    return MVFIT_OK;
}

extern "C" int mvfit_term_mix_cotangent3(mvfit_ctx* c, float silhouette, const float* g_sil, const float* L_sil, float vertex_targets,
                                         const float* g_vt, const float* L_vt, float scan, const float* g_scan, const float* L_scan,
                                         float* g, float* L_v) {
    if (!c) return MVFIT_E_ARG;
    if (c->B == 0) return fail(c, MVFIT_E_STATE, "call mvfit_set_problems first");
    const bool sil = silhouette > 0.f, vt = vertex_targets > 0.f, sn = scan > 0.f;
    if (!std::isfinite(silhouette) || !std::isfinite(vertex_targets) || !std::isfinite(scan) || silhouette < 0.f || vertex_targets < 0.f ||
        scan < 0.f || (!sil && !vt && !sn))
        return fail(c, MVFIT_E_ARG, "mvfit_term_mix_cotangent3: the shares (%g, %g, %g) must be finite and >= 0, one of them > 0",
                    (double)silhouette, (double)vertex_targets, (double)scan);
    if (!g || !L_v || (sil && (!g_sil || !L_sil)) || (vt && (!g_vt || !L_vt)) || (sn && (!g_scan || !L_scan)))
        return fail(c, MVFIT_E_ARG, "mvfit_term_mix_cotangent3: null buffer of a live component or of the result");
    HIP_OK(c, hipSetDevice(c->device));
    const hipError_t e = launch_term_mix_cotangent(c->nv, c->B, silhouette, g_sil, L_sil, vertex_targets, g_vt, L_vt, scan, g_scan, L_scan,
                                                   nullptr, g, L_v, nullptr, nullptr, c->stream);
    if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "term-mix cotangent launch: %s", hipGetErrorString(e));
    return MVFIT_OK;
}

extern "C" int mvfit_term_mix_merge(mvfit_ctx* c, float scene, const float* rec_scene, const float* rec_verts, float* rec) {
    static_assert(sizeof(SdfAdj) == MVFIT_TERM_RECORD_FLOATS * sizeof(float), "include/mvfit.h states the record's size");
    if (!c) return MVFIT_E_ARG;
    if (c->B == 0) return fail(c, MVFIT_E_STATE, "call mvfit_set_problems first");
    if (!std::isfinite(scene) || !(scene > 0.f)) return fail(c, MVFIT_E_ARG, "mvfit_term_mix_merge: scene = %g must be finite and > 0", (double)scene);
    if (!rec_scene || !rec_verts || !rec) return fail(c, MVFIT_E_ARG, "mvfit_term_mix_merge: null record buffer");
    if ((reinterpret_cast<uintptr_t>(rec_scene) | reinterpret_cast<uintptr_t>(rec_verts) | reinterpret_cast<uintptr_t>(rec)) & 3)
        return fail(c, MVFIT_E_ARG, "mvfit_term_mix_merge: record buffers must be 4-byte aligned");
    HIP_OK(c, hipSetDevice(c->device));
    const hipError_t e = launch_term_mix_record(c->B, scene, reinterpret_cast<const SdfAdj*>(rec_scene), reinterpret_cast<const SdfAdj*>(rec_verts),
                                                0.f, nullptr, 0.f, nullptr, 0.f, nullptr, nullptr, reinterpret_cast<SdfAdj*>(rec), nullptr, nullptr,
                                                c->stream);
    if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "term-mix record launch: %s", hipGetErrorString(e));
    return MVFIT_OK;
}

extern "C" int mvfit_term_mix_read(mvfit_ctx* c, float* parts) {
    if (!c) return MVFIT_E_ARG;
    if (!parts) return fail(c, MVFIT_E_ARG, "mvfit_term_mix_read: null parts");
    if (!c->mix.on) return fail(c, MVFIT_E_STATE, "mvfit_term_mix_read: the term mix is off (mvfit_set_term_mix)");
    HIP_OK(c, hipSetDevice(c->device));
    // the first three of a problem's four parts
    HIP_OK(c, hipMemcpy2DAsync(parts, 3 * sizeof(float), c->mix.parts, 4 * sizeof(float), 3 * sizeof(float), (size_t)c->B, hipMemcpyDeviceToDevice,
                               c->stream));
    return MVFIT_OK;
}

extern "C" int mvfit_term_mix_read4(mvfit_ctx* c, float* parts) {
    if (!c) return MVFIT_E_ARG;
    if (!parts) return fail(c, MVFIT_E_ARG, "mvfit_term_mix_read4: null parts");
    if (!c->mix.on) return fail(c, MVFIT_E_STATE, "mvfit_term_mix_read4: the term mix is off (mvfit_set_term_mix)");
    HIP_OK(c, hipSetDevice(c->device));
    HIP_OK(c, hipMemcpyAsync(parts, c->mix.parts, (size_t)c->B * 4 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    return MVFIT_OK;
}

extern "C" int mvfit_triangulate(mvfit_ctx* c, int B, int V, const float* keypoints, const double* intris, const double* extris,
                                 double* joints3d) {
    if (!c) return MVFIT_E_ARG;
    if (B <= 0 || V <= 0 || !keypoints || !intris || !extris || !joints3d)
        return fail(c, MVFIT_E_ARG, "mvfit_triangulate: bad argument (B=%d V=%d)", B, V);
    HIP_OK(c, hipSetDevice(c->device));
    hipError_t e = launch_triangulate(keypoints, intris, extris, B, V, NKP, joints3d, c->stream);
    if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "triangulate launch: %s", hipGetErrorString(e));
    return MVFIT_OK;
}

// Cross-view association of a frame's detections (associate.hip).  Frames go through in groups whose rays and linkage
// matrices stay under the 256 MB cap of the renderer's and the scene op's workspaces; a frame's result does not depend on
// its group.
extern "C" int mvfit_associate_views(mvfit_ctx* c, int F, int V, int Nmax, const float* keypoints, const int32_t* count,
                                     const double* intris, const double* extris, double max_cost, int min_joints, int min_views,
                                     double* cost_out, int32_t* labels, int32_t* num_clusters) {
    if (!c) return MVFIT_E_ARG;
    if (!keypoints || !count || !intris || !extris || !labels)
        return fail(c, MVFIT_E_ARG, "mvfit_associate_views: null %s",
                    !keypoints ? "keypoints" : !count ? "count" : !intris ? "intris" : !extris ? "extris" : "labels");
    if (F <= 0 || V > MVFIT_MAX_VIEWS || Nmax < 1 || Nmax > MVFIT_ASSOC_MAX_DET || min_views < 2 || min_views > V)
        return fail(c, MVFIT_E_ARG, "mvfit_associate_views: bad argument (F=%d V=%d Nmax=%d min_views=%d): 2 <= min_views <= V <= %d, "
                    "1 <= Nmax <= %d", F, V, Nmax, min_views, MVFIT_MAX_VIEWS, MVFIT_ASSOC_MAX_DET);
    if (min_joints < 1 || min_joints > NKP)
        return fail(c, MVFIT_E_ARG, "mvfit_associate_views: min_joints %d outside [1, %d]", min_joints, NKP);
    if (!(max_cost >= 0.0) || std::isinf(max_cost))
        return fail(c, MVFIT_E_ARG, "mvfit_associate_views: max_cost %g is not a finite value >= 0", max_cost);
    if (max_cost == 0.0) max_cost = 0.0;                     // -0.0: the kernels compare bit patterns
    HIP_OK(c, hipSetDevice(c->device));
    const int D = V * Nmax;
    const size_t cap = (size_t)256 << 20, per = assoc_frame_bytes(D);
    const int group = (int)std::min<size_t>({(size_t)F, std::max<size_t>(1, (cap - assoc_head_bytes()) / per), (size_t)32768});
    const size_t need = assoc_head_bytes() + (size_t)group * per;
    if (need > c->assoc_ws.size()) HIP_OK(c, hipStreamSynchronize(c->stream));          // an earlier call may still run on the old one
    HIP_OK(c, c->assoc_ws.reserve(need));
    for (int f0 = 0; f0 < F; f0 += group) {
        const hipError_t e = launch_associate_group(keypoints, count, intris, extris, f0, std::min(group, F - f0), V, Nmax, max_cost,
                                                    min_joints, min_views, c->assoc_ws.get(), cost_out, labels, num_clusters, c->stream);
        if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "mvfit_associate_views: launch: %s", hipGetErrorString(e));
    }
    return MVFIT_OK;
}

// Camera refinement against held bodies (camera_refine.hip): one workgroup per view, no workspace, no host synchronisation.
extern "C" int mvfit_camera_normal_eqs(mvfit_ctx* c, const float* joints, const double* cams, float rho, float data_weight,
                                       double* E, double* g, double* H, int32_t* count) {
    if (!c) return MVFIT_E_ARG;
    if (c->B == 0) return fail(c, MVFIT_E_STATE, "call mvfit_set_problems first");
    if (!joints || !cams || !E)
        return fail(c, MVFIT_E_ARG, "mvfit_camera_normal_eqs: null %s", !joints ? "joints" : !cams ? "cams" : "E");
    if (!std::isfinite(rho) || !(rho > 0.f)) return fail(c, MVFIT_E_ARG, "mvfit_camera_normal_eqs: rho = %g must be finite and > 0", (double)rho);
    if (!std::isfinite(data_weight) || !(data_weight >= 0.f))
        return fail(c, MVFIT_E_ARG, "mvfit_camera_normal_eqs: data_weight = %g must be finite and >= 0", (double)data_weight);
    HIP_OK(c, hipSetDevice(c->device));
    const hipError_t e = launch_camera_normal_eqs(joints, c->pb.gt, c->pb.wc, c->B, c->V, cams, rho, data_weight, E, g, H, count, c->stream);
    if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "mvfit_camera_normal_eqs: launch: %s", hipGetErrorString(e));
    return MVFIT_OK;
}

extern "C" int mvfit_refine_cameras(mvfit_ctx* c, const float* joints, const double* cams_in, const mvfit_camera_refine_opts* o,
                                    double* cams_out, double* report) {
    if (!c) return MVFIT_E_ARG;
    if (c->B == 0) return fail(c, MVFIT_E_STATE, "call mvfit_set_problems first");
    if (!joints || !cams_in || !o || !cams_out || !report)
        return fail(c, MVFIT_E_ARG, "mvfit_refine_cameras: null %s",
                    !joints ? "joints" : !cams_in ? "cams_in" : !o ? "opts" : !cams_out ? "cams_out" : "report");
    if (o->size < sizeof(mvfit_camera_refine_opts))
        return fail(c, MVFIT_E_ARG, "mvfit_refine_cameras: size %u < %zu", o->size, sizeof(mvfit_camera_refine_opts));
    if (o->free_mask == 0u || o->free_mask > 15u) return fail(c, MVFIT_E_ARG, "mvfit_refine_cameras: free_mask %u outside [1, 15]", o->free_mask);
    if (o->max_iter < 1 || o->max_iter > 64) return fail(c, MVFIT_E_ARG, "mvfit_refine_cameras: max_iter %d outside [1, 64]", o->max_iter);
    if (o->min_points < 1) return fail(c, MVFIT_E_ARG, "mvfit_refine_cameras: min_points %d < 1", o->min_points);
    if (!std::isfinite(o->rho) || !(o->rho > 0.f)) return fail(c, MVFIT_E_ARG, "mvfit_refine_cameras: rho = %g must be finite and > 0", (double)o->rho);
    if (!std::isfinite(o->data_weight) || !(o->data_weight >= 0.f))
        return fail(c, MVFIT_E_ARG, "mvfit_refine_cameras: data_weight = %g must be finite and >= 0", (double)o->data_weight);
    if (!std::isfinite(o->lambda0) || !(o->lambda0 > 0.0)) return fail(c, MVFIT_E_ARG, "mvfit_refine_cameras: lambda0 = %g must be finite and > 0", o->lambda0);
    if (!(o->ftol >= 0.0)) return fail(c, MVFIT_E_ARG, "mvfit_refine_cameras: ftol = %g must be >= 0", o->ftol);
    HIP_OK(c, hipSetDevice(c->device));
    const hipError_t e = launch_camera_refine(joints, c->pb.gt, c->pb.wc, c->B, c->V, cams_in, o->free_mask, o->fixed_views, o->max_iter,
                                              o->min_points, o->rho, o->data_weight, o->lambda0, o->ftol, cams_out, report, c->stream);
    if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "mvfit_refine_cameras: launch: %s", hipGetErrorString(e));
    return MVFIT_OK;
}

extern "C" int mvfit_depth_guess(mvfit_ctx* c, int B, const double* rest_joints, const double* extri, const double* intri,
                                 const float* keypoints, double* joints3d) {
    if (!c) return MVFIT_E_ARG;
    if (B <= 0 || !rest_joints || !extri || !intri || !keypoints || !joints3d)
        return fail(c, MVFIT_E_ARG, "mvfit_depth_guess: bad argument (B=%d)", B);
    HIP_OK(c, hipSetDevice(c->device));
    hipError_t e = launch_depth_guess(rest_joints, extri, intri, keypoints, B, NKP, joints3d, c->stream);
    if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "depth guess launch: %s", hipGetErrorString(e));
    return MVFIT_OK;
}

extern "C" int mvfit_umeyama(mvfit_ctx* c, int B, int npts, const double* src, const double* dst, int estimate_scale,
                             double* rot, double* rvec, double* trans, double* scale) {
    if (!c) return MVFIT_E_ARG;
    if (B <= 0 || npts < 3 || !src || !dst || !rot || !rvec || !trans || !scale)
        return fail(c, MVFIT_E_ARG, "mvfit_umeyama: bad argument (B=%d npts=%d)", B, npts);
    HIP_OK(c, hipSetDevice(c->device));
    hipError_t e = launch_umeyama(src, dst, B, npts, estimate_scale, rot, rvec, trans, scale, c->stream);
    if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "umeyama launch: %s", hipGetErrorString(e));
    return MVFIT_OK;
}

extern "C" int mvfit_project_points(mvfit_ctx* c, const float* points, int num_points, float* uv) {
    if (!c) return MVFIT_E_ARG;
    if (!points || !uv || num_points <= 0) return fail(c, MVFIT_E_ARG, "mvfit_project_points: bad argument (num_points=%d)", num_points);
    if (c->B == 0) return fail(c, MVFIT_E_STATE, "call mvfit_set_problems first (the cameras come from there)");
    HIP_OK(c, hipSetDevice(c->device));
    hipError_t e = launch_project_points(c->Q, points, num_points, uv, c->stream);
    if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "projection launch: %s", hipGetErrorString(e));
    return MVFIT_OK;
}

// grows the renderer's workspace and normal buffer (kept in the ctx) to at least ws / nb bytes
static int render_reserve(mvfit_ctx* c, size_t ws, size_t nb) {
    if (ws > c->render_ws.size() || nb > c->render_nrm.size())
        HIP_OK(c, hipStreamSynchronize(c->stream));             // earlier calls may still read the old buffers
    HIP_OK(c, c->render_ws.reserve(ws));
    HIP_OK(c, c->render_nrm.reserve(nb));
    return MVFIT_OK;
}

extern "C" int mvfit_render_overlay(mvfit_ctx* c, const float* vertices, const float* points, int num_points, int num_images,
                                    const int32_t* image_problem, const int32_t* image_view, int height, int width,
                                    const uint8_t* images, uint8_t* out, int32_t* face_id) {
    if (!c) return MVFIT_E_ARG;
    if (!c->num_faces) return fail(c, MVFIT_E_STATE, "mvfit_render_overlay: the model was created without (valid) faces");
    if (c->B == 0) return fail(c, MVFIT_E_STATE, "call mvfit_set_problems first (the cameras come from there)");
    if (!vertices || !images || !out || !image_problem || !image_view || num_images < 1 || height < 1 || height > 8192 ||
        width < 1 || width > 8192 || num_points < 0 || num_points > 64)
        return fail(c, MVFIT_E_ARG, "mvfit_render_overlay: bad argument (num_images=%d height=%d width=%d num_points=%d)",
                    num_images, height, width, num_points);
    for (int i = 0; i < num_images; ++i)
        if (image_problem[i] < 0 || image_problem[i] >= c->B || image_view[i] < 0 || image_view[i] >= c->V)
            return fail(c, MVFIT_E_ARG, "mvfit_render_overlay: image %d names problem %d / view %d (B=%d V=%d)", i,
                        image_problem[i], image_view[i], c->B, c->V);
    HIP_OK(c, hipSetDevice(c->device));
    // images per group: at most RENDER_GROUP_MAX and a workspace of at most 256 MB - or one image's, when a single image
    // needs more (8 H W bytes of visibility, 512 MB at 8192 x 8192; images are not tiled)
    const size_t cap = (size_t)256 << 20;
    int G = std::min(num_images, RENDER_GROUP_MAX);
    while (G > 1 && render_ws_bytes(G, c->nv, c->num_faces, height, width) > cap) --G;
    const size_t ws = render_ws_bytes(G, c->nv, c->num_faces, height, width);
    const size_t nb = (size_t)c->B * c->nv * 3 * sizeof(double);
    if (int rc = render_reserve(c, ws, nb)) return rc;
    hipError_t e = launch_render_normals(vertices, c->B, c->nv, c->d_faces, c->d_vf_ptr, c->d_vf_idx, c->render_nrm.as<double>(), c->stream);
    const size_t px = (size_t)height * width;
    for (int i0 = 0; i0 < num_images && e == hipSuccess; i0 += G) {
        const int n = std::min(G, num_images - i0);
        e = launch_render_group(c->Q, image_problem + i0, image_view + i0, n, vertices, c->render_nrm.as<double>(), c->nv, c->d_faces,
                                c->num_faces, points, points ? num_points : 0, height, width, images + (size_t)i0 * px * 3,
                                out + (size_t)i0 * px * 3, face_id ? face_id + (size_t)i0 * px : nullptr, c->render_ws.get(),
                                c->stream);
    }
    if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "render launch: %s", hipGetErrorString(e));
    return MVFIT_OK;
}

// utils.py:904-912 Renderer.colors in dictionary order
static const float SCENE_PALETTE[7][3] = {{.8f, .1f, .1f}, {.1f, .1f, .8f}, {.1f, .8f, .1f}, {.7f, .7f, .9f},
                                          {.9f, .9f, .8f}, {.7f, .75f, .5f}, {.5f, .7f, .75f}};

extern "C" int mvfit_render_scene(mvfit_ctx* c, const float* vertices, const float* points, int num_points, int num_images,
                                  const int32_t* image_first, const int32_t* body_problem, const int32_t* image_view,
                                  const float* body_color, int height, int width, const uint8_t* images, uint8_t* out,
                                  int32_t* face_id, int32_t* body_id) {
    if (!c) return MVFIT_E_ARG;
    if (!c->num_faces) return fail(c, MVFIT_E_STATE, "mvfit_render_scene: the model was created without (valid) faces");
    if (c->B == 0) return fail(c, MVFIT_E_STATE, "call mvfit_set_problems first (the cameras come from there)");
    if (!vertices || !images || !out || !image_first || !image_view || num_images < 1 || height < 1 || height > 8192 ||
        width < 1 || width > 8192 || num_points < 0 || num_points > 64)
        return fail(c, MVFIT_E_ARG, "mvfit_render_scene: bad argument (num_images=%d height=%d width=%d num_points=%d)",
                    num_images, height, width, num_points);
    if (image_first[0] != 0) return fail(c, MVFIT_E_ARG, "mvfit_render_scene: image_first[0] = %d, not 0", image_first[0]);
    for (int i = 0; i < num_images; ++i) {
        const long long cnt = (long long)image_first[i + 1] - image_first[i];
        if (cnt < 0) return fail(c, MVFIT_E_ARG, "mvfit_render_scene: image_first decreases at image %d", i);
        if (cnt > SCENE_BODIES_MAX)
            return fail(c, MVFIT_E_ARG, "mvfit_render_scene: image %d lists %lld bodies (at most %d)", i, cnt, SCENE_BODIES_MAX);
        if (image_view[i] < 0 || image_view[i] >= c->V)
            return fail(c, MVFIT_E_ARG, "mvfit_render_scene: image %d names view %d (V=%d)", i, image_view[i], c->V);
    }
    const int total = image_first[num_images];
    if (total > 0 && !body_problem) return fail(c, MVFIT_E_ARG, "mvfit_render_scene: body_problem is NULL");
    for (int j = 0; j < total; ++j) {
        if (body_problem[j] < 0 || body_problem[j] >= c->B)
            return fail(c, MVFIT_E_ARG, "mvfit_render_scene: body %d names problem %d (B=%d)", j, body_problem[j], c->B);
        if (body_color)
            for (int k = 0; k < 3; ++k)
                if (!(body_color[j * 3 + k] >= 0.f && body_color[j * 3 + k] <= 1.f))        // NaN fails both
                    return fail(c, MVFIT_E_ARG, "mvfit_render_scene: colour of body %d outside [0, 1]", j);
    }
    HIP_OK(c, hipSetDevice(c->device));
    // the call's tables, built in a pinned staging slot so that the copy to the device does not block the host
    const size_t tab_words = (size_t)num_images * SCENE_IMAGE_WORDS + (size_t)total * SCENE_INST_WORDS;
    const size_t tb = tab_words * sizeof(int32_t);
    const int slot = c->scene_slot;
    c->scene_slot ^= 1;
    if (c->scene_copied[slot]) HIP_OK(c, hipEventSynchronize(c->scene_copied[slot]));
    else HIP_OK(c, hipEventCreateWithFlags(&c->scene_copied[slot], hipEventDisableTiming));
    HIP_OK(c, c->h_scene_tab[slot].reserve(tb));
    int32_t* ti = c->h_scene_tab[slot].as<int32_t>();
    int32_t* tj = ti + (size_t)num_images * SCENE_IMAGE_WORDS;
    for (int i = 0; i < num_images; ++i) {
        const int first = image_first[i], cnt = image_first[i + 1] - first;
        ti[i * 4 + 0] = first; ti[i * 4 + 1] = cnt; ti[i * 4 + 2] = image_view[i];
        ti[i * 4 + 3] = cnt ? body_problem[first] : 0;
        for (int k = 0; k < cnt; ++k) {
            int32_t* r = tj + (size_t)(first + k) * SCENE_INST_WORDS;
            r[0] = body_problem[first + k]; r[1] = i; r[2] = k;
            const float* col = body_color ? body_color + (size_t)(first + k) * 3 : SCENE_PALETTE[k % 7];
            memcpy(r + 3, col, 12);
        }
    }
    // groups of consecutive images: at most RENDER_GROUP_MAX images and a workspace of at most 256 MB counting instances -
    // or one image's, when that alone needs more
    const size_t cap = (size_t)256 << 20;
    std::vector<int> group_end;
    size_t ws = 0;
    for (int i0 = 0; i0 < num_images;) {
        int i1 = i0 + 1;
        while (i1 < num_images && i1 - i0 < RENDER_GROUP_MAX &&
               scene_ws_bytes(i1 + 1 - i0, image_first[i1 + 1] - image_first[i0], c->nv, c->num_faces, height, width) <= cap)
            ++i1;
        ws = std::max(ws, scene_ws_bytes(i1 - i0, image_first[i1] - image_first[i0], c->nv, c->num_faces, height, width));
        group_end.push_back(i1);
        i0 = i1;
    }
    const size_t nb = (size_t)c->B * c->nv * 3 * sizeof(double);
    if (int rc = render_reserve(c, ws, nb)) return rc;
    if (tb > c->scene_tab.size()) HIP_OK(c, hipStreamSynchronize(c->stream));
    HIP_OK(c, c->scene_tab.reserve(tb));
    HIP_OK(c, hipMemcpyAsync(c->scene_tab.get(), ti, tb, hipMemcpyHostToDevice, c->stream));
    HIP_OK(c, hipEventRecord(c->scene_copied[slot], c->stream));
    hipError_t e = launch_render_normals(vertices, c->B, c->nv, c->d_faces, c->d_vf_ptr, c->d_vf_idx, c->render_nrm.as<double>(), c->stream);
    const size_t px = (size_t)height * width;
    int i0 = 0;
    for (size_t g = 0; g < group_end.size() && e == hipSuccess; ++g) {
        const int i1 = group_end[g], j0 = image_first[i0], m = image_first[i1] - j0;
        e = launch_scene_group(c->Q, c->scene_tab.as<int32_t>(), num_images, i0, i1 - i0, j0, m, vertices, c->render_nrm.as<double>(), c->nv, c->d_faces,
                               c->num_faces, points, points ? num_points : 0, height, width, images + (size_t)i0 * px * 3,
                               out + (size_t)i0 * px * 3, face_id ? face_id + (size_t)i0 * px : nullptr,
                               body_id ? body_id + (size_t)i0 * px : nullptr, c->render_ws.get(), c->stream);
        i0 = i1;
    }
    if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "render launch: %s", hipGetErrorString(e));
    return MVFIT_OK;
}
