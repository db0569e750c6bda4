// libmvfit: the C ABI (include/mvfit.h), part 1 of 3 - context lifetime and options, the problems and their work buffers, the SDF
// term's buffers, vertices / vertices_backward / full_pose, the drop-in closure, the profile entries and mvfit_gather.
// mvfit_fit.hip runs the optimiser, mvfit_scene.hip holds the entries that never do; mvfit_ctx.h is what the three share.
// No kernel lives in these files: the optimiser kernels are in fit_kernels.hip (launchers: fit_kernels.h), every other in the
// file of its launcher (launchers.h).  The model's tables are built by model_prep.cpp and uploaded by mvfit_create_ex; every
// allocation of a ctx has an owner of dev_mem.h, which does all the freeing.
#include <dlfcn.h>

#include "model_prep.h"
#include "mvfit_ctx.h"

// one model table to the device (null for an empty one: a part the model does not have)
template <typename T>
static T* dev_upload(mvfit_ctx* c, const T* h, size_t n) {
    if (n == 0) return nullptr;
    T* d = nullptr;
    if (c->model_mem.alloc(&d, n * sizeof(T)) != hipSuccess) c->alloc_failed = true;      // (mvfit_create_ex checks after all uploads)
    else if (hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) c->upload_failed = true;
    return d;
}
template <typename T>
static T* dev_upload(mvfit_ctx* c, const std::vector<T>& h) { return dev_upload(c, h.data(), h.size()); }
template <typename D, typename T>
static const D* dev_upload_as(mvfit_ctx* c, const std::vector<T>& h) { return reinterpret_cast<const D*>(dev_upload(c, h)); }

// HostModel -> c->M and the renderer's faces; a failed allocation or copy is only recorded (mvfit_create_ex checks once)
static void upload_model(mvfit_ctx* c, const HostModel& h) {
    DevModel& M = c->M;
    c->nv = M.nv = h.nv;
    M.nv_pad = h.nv_pad;
    M.ntiles = h.ntiles;
    M.bs4 = dev_upload(c, h.bs4);
    M.bs_h2 = dev_upload_as<float4>(c, h.bs_h2);
    M.bs_scale = h.bs_scale;
    M.half_basis = h.half_basis;
    M.vt_planes = dev_upload(c, h.vt_planes);
    M.wt_tiles = dev_upload(c, h.wt_tiles);
    M.wsp_w = dev_upload_as<float4>(c, h.wsp_w);
    M.wsp_j = dev_upload_as<int4>(c, h.wsp_j);
    M.bs_vm = dev_upload(c, h.bs_vm);
    M.w_vm = dev_upload(c, h.w_vm);
    M.ns = h.ns; M.nc = h.nc; M.nc_pad = h.nc_pad;
    M.sel_v = dev_upload(c, h.sel_v);
    M.pd_sub = dev_upload(c, h.pd_sub);
    M.pd_subT = dev_upload(c, h.pd_subT);
    M.tile_sel_start = dev_upload(c, h.tile_sel_start);
    M.tile_sel_local = dev_upload(c, h.tile_sel_local);
    M.tile_sel_slot = dev_upload(c, h.tile_sel_slot);
    {   // the LDS image and, behind it in the same allocation, E6's lane cells (closure_device.h: prologue)
        std::vector<unsigned char> img(sizeof(ModelLds) + NJ * E6_ROW_BYTES, 0);
        ModelLds lds = h.lds;
        if (debug_hook("MVFIT_E6_DENSE") != 0) lds.e6_cells = 0;          // (hooks build only) E6 on the dense rows of wT
        if (debug_hook("MVFIT_BWD_STREAM_LATE") != 0) lds.stream_late |= 1;   // (hooks build only) E7's stream loads in-slot on every wave
        if (debug_hook("MVFIT_FWD_STREAM_LATE") != 0) lds.stream_late |= 2;   // (hooks build only) E2's forward stream likewise
        if (debug_hook("MVFIT_VIEW_SUMS_SERIAL") != 0) lds.stream_late |= 4;  // (hooks build only) E4's view sums as loops of conditional reads
        memcpy(img.data(), &lds, sizeof(ModelLds));
        memcpy(img.data() + sizeof(ModelLds), h.e6_cells.data(), std::min<size_t>(h.e6_cells.size() * 2, NJ * E6_ROW_BYTES));
        M.mlds = reinterpret_cast<const ModelLds*>(dev_upload(c, img));
    }
    M.vp_w1 = dev_upload(c, h.vp_w1); M.vp_b1 = dev_upload(c, h.vp_b1);
    M.vp_w2 = dev_upload(c, h.vp_w2); M.vp_b2 = dev_upload(c, h.vp_b2);
    M.vp_w3 = dev_upload(c, h.vp_w3); M.vp_b3 = dev_upload(c, h.vp_b3);
    M.vp_w1T = dev_upload(c, h.vp_w1T); M.vp_w2T = dev_upload(c, h.vp_w2T); M.vp_w3T = dev_upload(c, h.vp_w3T);
    M.vpt.tw2 = dev_upload_as<float4>(c, h.vp_tw2);
    M.vpt.tw3 = dev_upload_as<float4>(c, h.vp_tw3);
    M.vpt.w1T = M.vp_w1T; M.vpt.b1 = M.vp_b1; M.vpt.b2 = M.vp_b2;
    c->has_vposer = h.has_vposer;
    c->gmm_M = M.gmm_M = h.gmm_M;
    M.gmm_means = dev_upload(c, h.gmm_means);
    M.gmm_prec = dev_upload(c, h.gmm_prec);
    M.gmm_precT = dev_upload(c, h.gmm_precT);
    M.gmm_lognw = dev_upload(c, h.gmm_lognw);
    c->d_faces = dev_upload(c, h.faces);
    c->d_vf_ptr = dev_upload(c, h.vf_ptr);
    c->d_vf_idx = dev_upload(c, h.vf_idx);
    c->num_faces = h.num_faces;
}

void mvfit::drop_graph(mvfit_ctx* c) {
    if (c->round_graph) { hipGraphExecDestroy(c->round_graph); c->round_graph = nullptr; }
    c->graph_key.clear();
}

extern "C" const char* mvfit_last_error(const mvfit_ctx* ctx) { return ctx ? ctx->err.c_str() : "null ctx"; }

// what the fit's plan (fit_plan.h) depends on in this ctx; mvfit_fit adds the fit's own stages and options
FitPlanIn mvfit::plan_inputs(const mvfit_ctx* c) {
    FitPlanIn in;
    in.B = c->B; in.n_cu = c->n_cu; in.ntiles = c->M.ntiles;
    in.half_basis = c->M.bs_h2 != nullptr; in.sparse_skinning = c->M.wsp_w != nullptr; in.nv_even = (c->M.nv & 1) == 0;
    in.helper_memory = c->vps_mem != nullptr;
    in.profile = c->profile; in.resident_auto_off = c->resident_auto_off;
    in.debug_nopass = debug_hook("MVFIT_DEBUG_NOPASS") != 0;          // (hooks build only)
    in.round_mode = c->opt.round_mode; in.resident_pass = c->opt.resident_pass; in.sdf_two_phase = c->opt.sdf_two_phase;
    in.sdf_service = c->opt.sdf_service; in.vposer_helpers = c->opt.vposer_helpers; in.vposer_sets = c->opt.vposer_sets;
    in.work_queue = c->opt.work_queue;
    return in;
}

// what the plan of a round's term (round_term.h) depends on in this ctx
TermInputs mvfit::term_inputs(const mvfit_ctx* c) {
    TermInputs in;
    in.B = c->B; in.Bpad = c->Bpad; in.nv = c->nv;
    in.sdf_faces = c->sdf_faces.as<int32_t>(); in.sdf_num_faces = c->sdf_num_faces; in.sdf_grid = c->sdf_grid; in.sdf_cull = c->sdf_cull.get();
    in.sdf_box = c->pb.sdf_box; in.sdf_samp = c->pb.sdf_samp; in.sdf_entries = c->pb.sdf_entries; in.sdf_adj = c->pb.sdf_adj;
    const Obstacles& ob = c->obst;
    in.obst.on = ob.on; in.obst.tab = ob.tab; in.obst.box = ob.box; in.obst.phi = ob.phi; in.obst.grid = ob.grid; in.obst.rob = ob.rob;
    const SilState& S = c->sil;
    in.sil.on = S.on; in.sil.ws = S.ws.get(); in.sil.cs = S.cs.get();
    in.sil.M = S.M; in.sil.H = S.H; in.sil.W = S.W; in.sil.C = S.C; in.sil.nchunks = S.nchunks; in.sil.stride = S.stride;
    in.sil.occ = S.occ.get(); in.sil.occ_on = S.occ_on; in.sil.occ_margin = S.occ_margin;
    const SilTerm& st = c->silt;
    in.silt.on = st.on; in.silt.w_in = st.w_in; in.silt.w_out = st.w_out; in.silt.sigma = st.sigma;
    in.silt.g_verts = st.g_verts; in.silt.loss = st.loss; in.silt.part = st.part;
    const VtxTargets& T = c->vt;
    in.vt.on = T.on; in.vt.term = T.term; in.vt.K = T.K; in.vt.targets = T.targets; in.vt.weights = T.weights; in.vt.partial = T.partial;
    in.vt.g_verts = T.g_verts; in.vt.loss = T.loss; in.vt.part = T.part;
    const TermMix& X = c->mix;
    in.mix.on = X.on; in.mix.scene = X.scene; in.mix.silhouette = X.silhouette; in.mix.vertex_targets = X.vertex_targets;
    in.mix.w_in = X.w_in; in.mix.w_out = X.w_out; in.mix.sigma = X.sigma;
    in.mix.g_verts = X.g_verts; in.mix.loss = X.loss; in.mix.part = X.part; in.mix.rec_scene = X.rec_scene; in.mix.rec_verts = X.rec_verts;
    in.mix.parts = X.parts; in.mix.sums = X.sums;
    in.mix.scan = X.scan; in.mix.scan_w_s2m = X.scan_w_s2m; in.mix.scan_w_m2s = X.scan_w_m2s; in.mix.scan_sigma = X.scan_sigma;
    const ScanState& Z = c->scan;
    const ScanTerm& zt = c->scant;
    in.scan.on = Z.on; in.scan.term = zt.on; in.scan.ws = Z.ws.get(); in.scan.N = Z.N; in.scan.Pmax = Z.Pmax; in.scan.nf = Z.nf; in.scan.ns = Z.ns;
    in.scan.faces = c->d_faces; in.scan.w_s2m = zt.w_s2m; in.scan.w_m2s = zt.w_m2s; in.scan.sigma = zt.sigma;
    in.scan.g_verts = zt.g_verts; in.scan.loss = zt.loss; in.scan.part = zt.part;
    const LmState& lm = c->lm;
    in.lm.on = lm.on; in.lm.term = lm.term; in.lm.tab = lm.tab; in.lm.tgt = lm.tgt; in.lm.L = lm.L; in.lm.nt = lm.nt; in.lm.has3d = lm.has3d;
    in.lm.rho = lm.rho; in.lm.w3d = lm.w3d; in.lm.rho3d = lm.rho3d;
    in.lm.g_verts = lm.g_verts; in.lm.loss = lm.loss; in.lm.part = lm.part;
    return in;
}

extern "C" void mvfit_options_default(mvfit_options* o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->struct_size = (uint32_t)sizeof(mvfit_options);
    o->contraction = MVFIT_CONTRACTION_SPLIT_FP16;
    o->resident_pass = -1;
    o->sdf_two_phase = 1;
    o->sdf_face_lists = 1;
    o->vposer_helpers = 1;
    o->sdf_service = 1;
    o->work_queue = 1;
}

// a caller's struct (possibly shorter: an older header) over the defaults; range checks
static int read_options(mvfit_ctx* c, const mvfit_options* in, mvfit_options& o) {
    mvfit_options_default(&o);
    if (in) {
        if (in->struct_size < 8 || in->struct_size > 4096) return fail(c, MVFIT_E_ARG, "mvfit_options: struct_size %u", in->struct_size);
        memcpy(&o, in, std::min<size_t>(in->struct_size, sizeof(o)));
        o.struct_size = (uint32_t)sizeof(o);
    }
    if (o.contraction < 0 || o.contraction > MVFIT_CONTRACTION_HALF_BASIS) return fail(c, MVFIT_E_ARG, "mvfit_options: contraction %d", o.contraction);
    if (o.round_mode < 0 || o.round_mode > 1) return fail(c, MVFIT_E_ARG, "mvfit_options: round_mode %d", o.round_mode);
    if (o.resident_pass < -1 || o.resident_pass > 3) return fail(c, MVFIT_E_ARG, "mvfit_options: resident_pass %d", o.resident_pass);
    if (o.pass_kernel < 0 || o.pass_kernel > 2) return fail(c, MVFIT_E_ARG, "mvfit_options: pass_kernel %d", o.pass_kernel);
    if (o.vposer_sets < 0) return fail(c, MVFIT_E_ARG, "mvfit_options: vposer_sets %d", o.vposer_sets);
    return MVFIT_OK;
}

extern "C" int mvfit_create(mvfit_ctx** out, int device, void* hip_stream, const mvfit_model* m) {
    return mvfit_create_ex(out, device, hip_stream, m, nullptr);
}

extern "C" int mvfit_get_options(const mvfit_ctx* c, mvfit_options* o) {
    if (!c || !o) return MVFIT_E_ARG;
    *o = c->opt;
    return MVFIT_OK;
}

extern "C" int mvfit_set_options(mvfit_ctx* c, const mvfit_options* opts) {
    if (!c || !opts) return MVFIT_E_ARG;
    mvfit_options o;
    const int rc = read_options(c, opts, o);
    if (rc) return rc;
    if (o.contraction != c->opt.contraction || o.dense_skinning != c->opt.dense_skinning)
        return fail(c, MVFIT_E_ARG, "mvfit_set_options: contraction / dense_skinning are fixed at mvfit_create_ex");
    if (o.pass_kernel != c->opt.pass_kernel || o.sdf_face_lists != c->opt.sdf_face_lists) {
        HIP_OK(c, hipSetDevice(c->device));
        HIP_OK(c, hipStreamSynchronize(c->stream));
        drop_graph(c);                                   // the captured round graph bakes the kernel choice in
        if (o.sdf_face_lists != c->opt.sdf_face_lists) c->sdf_cull_refused = false;
    }
    c->opt = o;
    c->resident_auto_off = false;                        // (an explicit call re-arms the automatic resident_pass choice)
    return MVFIT_OK;
}

extern "C" int mvfit_sdf_info(const mvfit_ctx* c, int* op_path, int* term_path) {
    if (!c) return MVFIT_E_ARG;
    if (op_path) *op_path = c->sdf_op_path;
    if (term_path) *term_path = c->sdf_term_path;
    return MVFIT_OK;
}

extern "C" int mvfit_create_ex(mvfit_ctx** out, int device, void* hip_stream, const mvfit_model* m, const mvfit_options* opts) {
    if (!out || !m || !m->v_template || !m->shapedirs || !m->posedirs || !m->J_regressor || !m->parents ||
        !m->lbs_weights || !m->face_vertex_ids || !m->joint_map || m->num_verts <= 0) {
        if (out) *out = nullptr;
        return MVFIT_E_ARG;
    }
    // From here on *out is a ctx even when an error is returned: it holds the message for mvfit_last_error and owns
    // whatever was allocated so far - the caller releases both with mvfit_destroy (include/mvfit.h).
    mvfit_ctx* c = new mvfit_ctx();
    *out = c;
    c->device = device;
    HIP_OK(c, hipSetDevice(device));
    c->stream = (hipStream_t)hip_stream;
    if (const int rc = read_options(c, opts, c->opt)) return rc;
    if (persistent_lds(false) > 160 * 1024 || persistent_lds(true) > 160 * 1024)
        return fail(c, MVFIT_E_UNSUPPORTED, "LDS budget exceeded (%zu / %zu B)", persistent_lds(false), persistent_lds(true));
    static_assert(sizeof(VpHelperLds) <= sizeof(ClosureLds), "the decoder helpers share the fit kernel's dynamic LDS");
    {
        HostModel h;
        if (const int rc = prepare_model(*m, c->opt.contraction, c->opt.dense_skinning, h, c->err)) return rc;
        upload_model(c, h);
    }
    if (c->has_vposer) {    // request / answer granules of the decoder helpers (re-initialised before every launch that has them)
        c->vps_words = (size_t)VPS_MAX_SETS * VPS_PMAX * VPS_GRAN * (1 + VPS_SLICES);
        if (c->model_mem.alloc(&c->vps_mem, (c->vps_words + 1) * 8, true) != hipSuccess) c->alloc_failed = true;
    }
    if (c->alloc_failed) return fail(c, MVFIT_E_HIP, "device allocation failed");
    if (c->upload_failed) return fail(c, MVFIT_E_HIP, "copying the model constants to the device failed");
    HIP_OK(c, vertex_pass_configure());
    HIP_OK(c, vertex_backward_configure());
    HIP_OK(c, hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, device));
    HIP_OK(c, fit_kernels_configure());
    HIP_OK(c, c->h_done.reserve(8));
    HIP_OK(c, hipDeviceSynchronize());
    return MVFIT_OK;
}

// the scene term's obstacles go with the batch they were frozen for
void mvfit::free_obstacles(mvfit_ctx* c) {
    c->obst_mem.release();
    c->obst = Obstacles{};
}

void mvfit::free_term_mix(mvfit_ctx* c) {
    c->mix_mem.release();
    c->mix = TermMix{};
}

void mvfit::free_scan_term(mvfit_ctx* c) {
    c->scanterm_mem.release();
    c->scant = ScanTerm{};
}

void mvfit::free_landmark_targets(mvfit_ctx* c) {
    c->lmtgt_mem.release();
    c->lmterm_mem.release();
    LmState& S = c->lm;
    S.on = S.term = S.has3d = false;
    S.tgt_L = 0;
    S.tgt = S.g_verts = S.loss = S.part = nullptr;
}

void mvfit::free_vertex_targets(mvfit_ctx* c) {
    c->vtgt_mem.release();
    c->vtterm_mem.release();
    c->vt = VtxTargets{};
}

static void free_problem_buffers(mvfit_ctx* c) {
    drop_graph(c);
    c->problem_mem.release();
    c->ring_mem.release();
    c->sdf_cull.reset();
    c->B = c->V = c->Bpad = 0;          // nothing is allocated: a failed re-allocation cannot leave a stale shape behind
    c->pb = ProblemBufs{};
    c->P = DevPose{};
    c->F = FitBuffers{};
    c->ring = AsyncRing{};
    c->sdf_cull_refused = false;
    free_obstacles(c);
    c->silterm_mem.release();           // the silhouette term goes with the batch it was enabled for
    c->silt = SilTerm{};
    free_vertex_targets(c);             // and so do the vertex targets and their term
    free_term_mix(c);                   // and the term mix
    free_scan_term(c);                  // and the scan term (the scan set is not tied to the batch: it stays)
    free_landmark_targets(c);           // and the landmark targets with their term (the table stays too)
}

extern "C" void mvfit_destroy(mvfit_ctx* c) {
    if (!c) return;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    free_problem_buffers(c);
    for (hipEvent_t e : c->scene_copied) if (e) hipEventDestroy(e);
    for (hipEvent_t e : c->ev_done) if (e) hipEventDestroy(e);
    for (hipEvent_t e : c->ev_batch) if (e) hipEventDestroy(e);
    if (c->ev_init) hipEventDestroy(c->ev_init);
    if (c->pass_stream) hipStreamDestroy(c->pass_stream);
    for (auto& e : c->ev_vp) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
    for (auto& e : c->ev_step) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
    delete c;                           // the owners free the rest
}

extern "C" int mvfit_sync(mvfit_ctx* c) {
    if (!c) return MVFIT_E_ARG;
    HIP_OK(c, hipStreamSynchronize(c->stream));
    return MVFIT_OK;
}

extern "C" int mvfit_set_problems(mvfit_ctx* c, int B, int V, int cam_batched, const float* cam_R, const float* cam_t,
                                  const float* cam_f, const float* cam_c, const float* gt_xy, const float* w_conf) {
    if (!c) return MVFIT_E_ARG;
    if (B <= 0 || V <= 0 || V > MVFIT_MAX_VIEWS || !cam_R || !cam_t || !cam_f || !cam_c || !gt_xy || !w_conf)
        return fail(c, MVFIT_E_ARG, "set_problems: bad argument (B=%d V=%d, V <= %d)", B, V, MVFIT_MAX_VIEWS);
    HIP_OK(c, hipSetDevice(c->device));
    HIP_OK(c, hipStreamSynchronize(c->stream));
    if (B != c->B || V != c->V || (cam_batched != 0) != (c->Q.cam_batched != 0)) {
        free_problem_buffers(c);
        // caller-owned hook buffers were sized for the old batch (include/mvfit.h): switch both hooks off
        c->trace = nullptr; c->trace_cap = 0;
        c->capture_verts = nullptr; c->capture_round = -1;
        const size_t nc = cam_batched ? (size_t)B * V : (size_t)V;
        const int Bpad = (B + 31) / 32 * 32;
        DevPool& mem = c->problem_mem;
        ProblemBufs& pb = c->pb;
        HIP_OK(c, mem.alloc(&pb.camR, nc * 9 * 4)); HIP_OK(c, mem.alloc(&pb.camt, nc * 3 * 4));
        HIP_OK(c, mem.alloc(&pb.camf, nc * 4)); HIP_OK(c, mem.alloc(&pb.camc, nc * 2 * 4));
        HIP_OK(c, mem.alloc(&pb.gt, (size_t)B * V * NKP * 2 * 4)); HIP_OK(c, mem.alloc(&pb.wc, (size_t)B * V * NKP * 4));
        HIP_OK(c, mem.alloc(&c->P.coefT, (size_t)Bpad * KROWS * 4, true)); HIP_OK(c, mem.alloc(&c->P.Amat, (size_t)Bpad * 288 * 4));
        HIP_OK(c, mem.alloc(&c->P.tau, (size_t)Bpad * 4 * 4));
        HIP_OK(c, mem.alloc(&c->P.vposed_sel, (size_t)Bpad * NC_MAX * 4));
        HIP_OK(c, mem.alloc(&c->P.xs_sel, (size_t)Bpad * NC_MAX * 4));
        HIP_OK(c, mem.alloc(&c->P.coefH, (size_t)Bpad * KROWS * 4, true));
        HIP_OK(c, mem.alloc(&pb.verts, (size_t)B * c->nv * 3 * 4));
        HIP_OK(c, mem.alloc(&pb.obs, (size_t)B * sizeof(ObsBlock)));
        HIP_OK(c, mem.alloc(&c->F.opt, (size_t)B * sizeof(OptBlock)));
        HIP_OK(c, mem.alloc(&c->F.pose, (size_t)B * sizeof(PoseBlock)));
        HIP_OK(c, mem.alloc(&c->F.dirs, (size_t)B * LB_HIST * LB_D * 4));
        HIP_OK(c, mem.alloc(&c->F.stps, (size_t)B * LB_HIST * LB_D * 4));
        HIP_OK(c, mem.alloc(&c->F.rinv, (size_t)B * LB_RPACK * 4));
        HIP_OK(c, mem.alloc(&c->F.grow, (size_t)B * LB_GSIZE * 4, true));
        HIP_OK(c, mem.alloc(&c->F.gcol, (size_t)B * LB_GSIZE * 4, true));
        HIP_OK(c, mem.alloc(&c->F.stage_final, (size_t)B * MVFIT_MAX_STAGES * 8));
        HIP_OK(c, mem.alloc(&c->F.n_done, 12));
        HIP_OK(c, mem.alloc(&c->F.sdf_gate, (size_t)B * 4));
        HIP_OK(c, mem.alloc(&c->F.sdf_tag, (size_t)Bpad * 4));
        HIP_OK(c, mem.alloc(&c->F.vp, (size_t)B * sizeof(VpBlock)));
        HIP_OK(c, mem.alloc(&pb.gt3d, (size_t)B * NKP * 3 * 4));
        HIP_OK(c, mem.alloc(&pb.c3d, (size_t)B * NKP * 4));
        c->B = B; c->V = V; c->Bpad = Bpad;      // only now: every buffer of this shape exists
    }
    const size_t nc = cam_batched ? (size_t)B * V : (size_t)V;
    HIP_OK(c, hipMemcpyAsync(c->pb.camR, cam_R, nc * 9 * 4, hipMemcpyDefault, c->stream));
    HIP_OK(c, hipMemcpyAsync(c->pb.camt, cam_t, nc * 3 * 4, hipMemcpyDefault, c->stream));
    HIP_OK(c, hipMemcpyAsync(c->pb.camf, cam_f, nc * 4, hipMemcpyDefault, c->stream));
    HIP_OK(c, hipMemcpyAsync(c->pb.camc, cam_c, nc * 2 * 4, hipMemcpyDefault, c->stream));
    HIP_OK(c, hipMemcpyAsync(c->pb.gt, gt_xy, (size_t)B * V * NKP * 2 * 4, hipMemcpyDefault, c->stream));
    HIP_OK(c, hipMemcpyAsync(c->pb.wc, w_conf, (size_t)B * V * NKP * 4, hipMemcpyDefault, c->stream));
    c->Q = DevProblems{B, V, cam_batched ? 1 : 0, c->pb.camR, c->pb.camt, c->pb.camf, c->pb.camc, c->pb.gt, c->pb.wc};
    launch_pack_obs(B, c->stream, c->Q, c->pb.obs);
    c->has_joints3d = false;
    HIP_OK(c, hipGetLastError());
    HIP_OK(c, hipStreamSynchronize(c->stream));
    return MVFIT_OK;
}

extern "C" int mvfit_set_joints3d(mvfit_ctx* c, const float* gt3d, const float* conf3d) {
    if (!c || !gt3d || !conf3d) return MVFIT_E_ARG;
    if (c->B == 0) return fail(c, MVFIT_E_STATE, "call mvfit_set_problems first");
    HIP_OK(c, hipSetDevice(c->device));
    HIP_OK(c, hipMemcpyAsync(c->pb.gt3d, gt3d, (size_t)c->B * NKP * 3 * 4, hipMemcpyDefault, c->stream));
    HIP_OK(c, hipMemcpyAsync(c->pb.c3d, conf3d, (size_t)c->B * NKP * 4, hipMemcpyDefault, c->stream));
    launch_pack_joints3d(c->B, c->stream, c->pb.gt3d, c->pb.c3d, c->pb.obs);
    HIP_OK(c, hipGetLastError());
    c->has_joints3d = true;
    return MVFIT_OK;
}

extern "C" int mvfit_set_sdf(mvfit_ctx* c, const int32_t* faces, int num_faces, int grid_size) {
    if (!c) return MVFIT_E_ARG;
    if (c->obst.on && faces && num_faces != 0)
        return fail(c, MVFIT_E_STATE, "mvfit_set_sdf: scene obstacles are the interpenetration term (one per ctx): remove them first");
    if (c->silt.on && faces && num_faces != 0)
        return fail(c, MVFIT_E_STATE, "mvfit_set_sdf: the silhouette term uses the ctx's term slot: switch it off first");
    if (c->vt.term && faces && num_faces != 0)
        return fail(c, MVFIT_E_STATE, "mvfit_set_sdf: the vertex-target term uses the ctx's term slot: switch it off first");
    if (c->scant.on && faces && num_faces != 0)
        return fail(c, MVFIT_E_STATE, "mvfit_set_sdf: the scan term uses the ctx's term slot: switch it off first");
    if (c->lm.term && faces && num_faces != 0)
        return fail(c, MVFIT_E_STATE, "mvfit_set_sdf: the landmark term uses the ctx's term slot: switch it off first");
    if (c->mix.on && faces && num_faces != 0)
        return fail(c, MVFIT_E_STATE, "mvfit_set_sdf: the term mix uses the ctx's term slot (the one-person term is not part of it): switch it off first");
    HIP_OK(c, hipSetDevice(c->device));
    HIP_OK(c, hipStreamSynchronize(c->stream));
    drop_graph(c);
    c->sdf_faces.reset();
    c->sdf_cull.reset();                                           // sized by the face count
    c->sdf_cull_refused = false;
    c->sdf_num_faces = 0; c->sdf_grid = 0;
    if (!faces || num_faces == 0) return MVFIT_OK;                 // term switched off
    if (num_faces < 0 || grid_size < 2 || grid_size > 1024)
        return fail(c, MVFIT_E_ARG, "mvfit_set_sdf: bad argument (num_faces=%d grid_size=%d)", num_faces, grid_size);
    if (c->nv > 8192) return fail(c, MVFIT_E_UNSUPPORTED, "the SDF term supports up to 8192 vertices (model has %d)", c->nv);
    HIP_OK(c, c->sdf_faces.reserve((size_t)num_faces * 3 * 4));
    HIP_OK(c, hipMemcpy(c->sdf_faces.as<int32_t>(), faces, (size_t)num_faces * 3 * 4, hipMemcpyDefault));
    std::vector<int32_t> h((size_t)num_faces * 3);
    HIP_OK(c, hipMemcpy(h.data(), c->sdf_faces.as<int32_t>(), h.size() * 4, hipMemcpyDeviceToHost));
    for (int32_t vi : h)
        if (vi < 0 || vi >= c->nv) {
            c->sdf_faces.reset();
            return fail(c, MVFIT_E_ARG, "mvfit_set_sdf: face vertex index %d outside [0, %d)", (int)vi, c->nv);
        }
    c->sdf_num_faces = num_faces; c->sdf_grid = grid_size;
    return MVFIT_OK;
}

extern "C" int mvfit_sdf_term_read(mvfit_ctx* c, float* samples, float* sums) {
    if (!c) return MVFIT_E_ARG;
    if (!c->pb.sdf_adj) return fail(c, MVFIT_E_STATE, "no interpenetration term has been evaluated yet");
    const RoundTermPlan plan = plan_round_term(term_inputs(c));    // (where the round leaves the sums comes with the plan)
    if (samples && plan.kind != TERM_SDF)
        return fail(c, MVFIT_E_UNSUPPORTED, "mvfit_sdf_term_read: the %s term keeps no per-vertex samples (sums only)", term_name(c));
    HIP_OK(c, hipSetDevice(c->device));
    if (samples) HIP_OK(c, hipMemcpyAsync(samples, c->pb.sdf_samp, (size_t)c->B * c->nv * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    if (sums && plan.sums_stride == sizeof(float))
        HIP_OK(c, hipMemcpyAsync(sums, plan.sums, (size_t)c->B * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    else if (sums)
        HIP_OK(c, hipMemcpy2DAsync(sums, sizeof(float), plan.sums, plan.sums_stride, sizeof(float), c->B, hipMemcpyDeviceToDevice, c->stream));
    return MVFIT_OK;
}

// work buffers of the SDF term for the current batch
int mvfit::ensure_sdf_buffers(mvfit_ctx* c) {
    // all faces (or any list too long for the staged walk): the per-round face lists of sdf_term.hip.
    // mvfit_options::sdf_face_lists = 0 keeps the brute-force kernel (the check of the culled one).
    if (c->sdf_cull.get() && !c->opt.sdf_face_lists) {          // switched off since the workspace was made
        HIP_OK(c, hipStreamSynchronize(c->stream));
        c->sdf_cull.reset();
    }
    c->sdf_term_path = c->sdf_cull.get() ? 1 : 0;
    if (!c->sdf_cull.get() && c->opt.sdf_face_lists && c->sdf_num_faces >= sdf_cull_min_faces() && !c->sdf_cull_refused) {
        // (11.6 MB of lists, records and bins per problem at 13,776 faces: a batch whose workspace would not fit keeps the
        // walk - decided ONCE per (batch, face list): the refusal is remembered (and reported by mvfit_sdf_info) instead of
        // querying the free memory on every fit)
        size_t free_b = 0, total_b = 0;
        HIP_OK(c, hipMemGetInfo(&free_b, &total_b));
        if (sdf_cull_bytes(c->B, c->sdf_num_faces) < free_b / 2) {
            HIP_OK(c, c->sdf_cull.reserve(sdf_cull_bytes(c->B, c->sdf_num_faces)));
            HIP_OK(c, hipMemset(c->sdf_cull.as<unsigned char>() + sdf_cull_zero_offset(c->B, c->sdf_num_faces), 0, sdf_cull_zero_bytes(c->B)));
            c->sdf_term_path = 1;
        } else {
            c->sdf_cull_refused = true;
            c->sdf_term_path = 2;
        }
    } else if (!c->sdf_cull.get() && c->sdf_cull_refused) c->sdf_term_path = 2;
    if (c->pb.sdf_adj) return MVFIT_OK;
    unsigned char* work = nullptr;
    HIP_OK(c, c->problem_mem.alloc(&c->pb.sdf_box, (size_t)c->B * sizeof(SdfBox)));
    HIP_OK(c, c->problem_mem.alloc(&c->pb.sdf_samp, (size_t)c->B * c->nv * sizeof(float4)));
    HIP_OK(c, c->problem_mem.alloc(&work, sdf_work_bytes(c->B, c->nv)));      // entry lists + slice partials + heads + tickets
    HIP_OK(c, hipMemset(work + sdf_ticket_offset(c->B, c->nv), 0, (size_t)c->B * sizeof(int)));
    c->pb.sdf_entries = work;
    HIP_OK(c, c->problem_mem.alloc(&c->pb.sdf_adj, (size_t)c->B * sizeof(SdfAdj)));
    HIP_OK(c, c->problem_mem.alloc(&c->pb.sdf_gate_round, (size_t)c->B * 4));
    HIP_OK(c, c->problem_mem.alloc(&c->pb.sdf_boxpart, (size_t)c->Bpad * c->M.ntiles * 6 * 8));
    return MVFIT_OK;
}

// the per-round pass over problems [b_lo, b_hi) runs as lbs_vertex_pass_split_kernel (which writes the tile keys of the term's box when
// DevPose::box_part is set) when the split-fp16 basis exists and the launch is one 32-problem chunk per workgroup
bool mvfit::pass_writes_box_parts(const mvfit_ctx* c, int b_lo, int b_hi) {
    const int chunks = (b_hi + 31) / 32 - b_lo / 32;
    return !round_term(c) && c->M.bs_h2 != nullptr && c->pb.sdf_boxpart != nullptr && c->sdf_num_faces <= 128 && (chunks == 1 || c->opt.pass_kernel == 1);
}

// the interpenetration term of a chained round behind its vertex pass: the steps of its plan (round_term.cpp decides which), each
// one launch on the round's stream with no host work.  Everything a launcher takes is in the plan, but the model, the pose
// operands, the problems' cameras (the landmark term projects with them; a new batch drops the graph) and what the round itself brings: its vertices, gate, stream and the pass's tile keys of the box.
hipError_t mvfit::launch_term(const RoundTermPlan& plan, const DevModel& M, const DevPose& P, const DevProblems& Q, SilState& sil, ScanState& scan,
                              std::string& err, const float* verts, const int* gate, hipStream_t st, const unsigned long long* box_part) {
    const int B = plan.B, nv = plan.nv;
    hipError_t e = hipSuccess;
    for (int i = 0; i < plan.n && e == hipSuccess; ++i) {
        const TermStep& s = plan.step[i];
        switch (s.kind) {
        case STEP_SIL_EVAL:
            if (sil_round(sil, verts, B, s.sil.w_in, s.sil.w_out, s.sil.sigma, gate, s.sil.loss, s.sil.g_verts, st, err)) e = hipErrorLaunchFailure;
            break;
        case STEP_VT_EVAL:
            e = launch_vertex_target(verts, nv, B, s.vt.K, s.vt.targets, s.vt.weights, gate, s.vt.partial, s.vt.loss, s.vt.g_verts, st);
            break;
        case STEP_MIX_COTANGENT:
            e = launch_term_mix_cotangent(nv, B, s.cot.lam_sil, s.cot.g_sil, s.cot.L_sil, s.cot.lam_vt, s.cot.g_vt, s.cot.L_vt, s.cot.lam_scan,
                                          s.cot.g_scan, s.cot.L_scan, gate, s.cot.g, s.cot.L_v, s.cot.parts, s.cot.sums, st);
            break;
        case STEP_SCAN_EVAL:
            if (scan_round(scan, s.scan.faces, verts, s.scan.w_s2m, s.scan.w_m2s, s.scan.sigma, gate, s.scan.loss, s.scan.g_verts, st, err))
                e = hipErrorLaunchFailure;
            break;
        case STEP_LM_EVAL:
            e = launch_landmarks(verts, nv, B, s.lm.tab, s.lm.L, s.lm.nt, s.lm.tgt, s.lm.has3d != 0,
                                 LmCams{Q.V, Q.cam_batched, Q.cam_R, Q.cam_t, Q.cam_f, Q.cam_c}, s.lm.rho, s.lm.w3d, s.lm.rho3d, gate, s.lm.loss,
                                 s.lm.g_verts, st);
            break;
        case STEP_PULLBACK:
            e = launch_silhouette_pullback(M, P, B, plan.Bpad, gate, s.pull.g_verts, s.pull.loss, s.pull.part, s.pull.rec, st);
            break;
        case STEP_SCENE:
            e = launch_scene_term(M, P, verts, B, s.scene.tab, static_cast<const float4*>(s.scene.box), s.scene.phi, s.scene.grid, s.scene.rob, gate,
                                  s.scene.null_box, s.scene.entries, s.scene.rec, st);
            break;
        case STEP_MIX_RECORD:
            e = launch_term_mix_record(B, s.rec.lam_sc, s.rec.rec_scene, s.rec.rec_verts, s.rec.lam_sil, s.rec.L_sil, s.rec.lam_vt, s.rec.L_vt,
                                       s.rec.lam_scan, s.rec.L_scan, gate, s.rec.rec, s.rec.parts, s.rec.sums, st);
            break;
        case STEP_SDF:
            e = launch_sdf_term(M, P, verts, B, B, s.sdf.faces, s.sdf.num_faces, s.sdf.grid, gate, s.sdf.box, static_cast<float4*>(s.sdf.samp),
                                s.sdf.entries, s.sdf.adj, st, s.sdf.cull, nullptr, 0u, box_part);
            break;
        default:
            e = hipErrorInvalidValue;
        }
    }
    return e;
}

int mvfit::run_sdf_term(mvfit_ctx* c, const float* verts, const int* gate, hipStream_t st) {
    const hipError_t e = launch_term(plan_round_term(term_inputs(c)), c->M, c->P, c->Q, c->sil, c->scan, c->err, verts, gate, st, nullptr);
    if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "%s term launch: %s", term_name(c), hipGetErrorString(e));
    return MVFIT_OK;
}

int mvfit::check_flags(mvfit_ctx* c, uint32_t flags) {
    if ((flags & MVFIT_F_USE_3D) && !c->has_joints3d) return fail(c, MVFIT_E_STATE, "MVFIT_F_USE_3D set but mvfit_set_joints3d was not called");
    if ((flags & MVFIT_F_VPOSER) && !c->has_vposer) return fail(c, MVFIT_E_STATE, "MVFIT_F_VPOSER set but the model has no VPoser decoder");
    if ((flags & MVFIT_F_PRIOR_GMM) && c->gmm_M == 0) return fail(c, MVFIT_E_STATE, "MVFIT_F_PRIOR_GMM set but the model has no GMM");
    return MVFIT_OK;
}

DevWeights mvfit::to_dev(const mvfit_weights& w) {
    DevWeights d;
    d.data_w2 = w.data_weight * w.data_weight;
    d.pose_w = w.body_pose_weight; d.shape_w = w.shape_weight; d.bend_w = w.bending_prior_weight;
    d.coll_w = w.coll_loss_weight; d.rho2 = w.rho * w.rho; d.flags = w.flags; d.pad = 0;
    return d;
}

void mvfit::prof_begin(mvfit_ctx* c, std::vector<std::pair<hipEvent_t, hipEvent_t>>& evs) {
    if (!c->profile || evs.size() >= 4096) return;
    hipEvent_t a, b;
    hipEventCreate(&a); hipEventCreate(&b);
    hipEventRecord(a, c->stream);
    evs.emplace_back(a, b);
}
void mvfit::prof_end(mvfit_ctx* c, std::vector<std::pair<hipEvent_t, hipEvent_t>>& evs) {
    if (!c->profile || evs.empty()) return;
    hipEventRecord(evs.back().second, c->stream);
}

int mvfit::run_vertex_pass(mvfit_ctx* c, float* verts) {
    prof_begin(c, c->ev_vp);
    hipError_t e = launch_vertex_pass(c->M, c->P, c->B, verts, c->opt.pass_kernel, c->stream);
    prof_end(c, c->ev_vp);
    if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "vertex pass launch: %s", hipGetErrorString(e));
    return MVFIT_OK;
}

extern "C" int mvfit_vertices(mvfit_ctx* c, const float* params, uint32_t flags, float* verts, float* joints) {
    if (!c || !params || !verts) return MVFIT_E_ARG;
    if (c->B == 0) return fail(c, MVFIT_E_STATE, "call mvfit_set_problems first");
    int rc = check_flags(c, flags);
    if (rc) return rc;
    HIP_OK(c, hipSetDevice(c->device));
    launch_prep(c->B, c->stream, c->M, c->pb.obs, c->P, params, flags, nullptr);
    HIP_OK(c, hipGetLastError());
    rc = run_vertex_pass(c, verts);
    if (rc) return rc;
    if (joints) {
        launch_joints(c->B, c->stream, c->M, verts, c->P.Amat, params, joints);
        HIP_OK(c, hipGetLastError());
    }
    return MVFIT_OK;
}

extern "C" int mvfit_vertices_backward(mvfit_ctx* c, const float* params, uint32_t flags, const float* g_verts,
                                       const float* g_joints, float* g_params) {
    if (!c || !params || !g_params) return MVFIT_E_ARG;
    if (c->B == 0) return fail(c, MVFIT_E_STATE, "call mvfit_set_problems first");
    flags &= MVFIT_F_VPOSER | MVFIT_F_FIX_SHAPE | MVFIT_F_FIX_SCALE;       // the other bits have no effect here
    int rc = check_flags(c, flags);
    if (rc) return rc;
    HIP_OK(c, hipSetDevice(c->device));
    if (g_verts) {
        const size_t need = vjp_part_bytes(c->Bpad, c->nv);
        const size_t need_rec = (size_t)c->B * sizeof(SdfAdj);
        if (need > c->vjp_part.size() || need_rec > c->vjp_rec.size())
            HIP_OK(c, hipStreamSynchronize(c->stream));          // (a previous call may still read the old buffers)
        HIP_OK(c, c->vjp_part.reserve(need));
        HIP_OK(c, c->vjp_rec.reserve(need_rec));
    }
    launch_prep(c->B, c->stream, c->M, c->pb.obs, c->P, params, flags, nullptr);
    HIP_OK(c, hipGetLastError());
    HIP_OK(c, launch_vertices_backward(c->M, c->P, c->B, c->Bpad, params, flags, g_verts, g_joints, c->vjp_part.as<float>(), c->vjp_rec.as<SdfAdj>(),
                                       g_params, c->stream));
    return MVFIT_OK;
}

extern "C" int mvfit_full_pose(mvfit_ctx* c, const float* params, uint32_t flags, float* full_pose) {
    if (!c || !params || !full_pose) return MVFIT_E_ARG;
    if (c->B == 0) return fail(c, MVFIT_E_STATE, "call mvfit_set_problems first");
    int rc = check_flags(c, flags);
    if (rc) return rc;
    HIP_OK(c, hipSetDevice(c->device));
    launch_prep(c->B, c->stream, c->M, c->pb.obs, c->P, params, flags, full_pose);
    HIP_OK(c, hipGetLastError());
    return MVFIT_OK;
}

// Test route of mvfit_closure (MVFIT_CLOSURE_VP_HELPERS=1, read per call; VPoser flag, no SDF term): the closure decodes
// the body pose on helper workgroups of its own launch - the decoder of the production single-launch fits
// (vposer_service.h), whose summation order differs from the in-workgroup decoder - and, like those fits, evaluates the
// objective from the vertices it computes itself while the full vertex pass runs on the operands it published.
static int closure_via_helpers(mvfit_ctx* c, const mvfit_weights* w, const float* params, float* loss, float* grad,
                               float* verts, float* joints) {
    const int n = c->B;
    if (n > kVpsMaxSparse) return fail(c, MVFIT_E_ARG, "MVFIT_CLOSURE_VP_HELPERS: at most %d problems (all workgroups resident)", kVpsMaxSparse);
    DevModel M = c->M;
    const int nsets = plan_nsets(plan_inputs(c), n, 0, false);       // (the automatic count: the route does not read vposer_sets)
    HIP_OK(c, hipMemsetAsync(c->vps_mem, 0, c->vps_words * 8 + 8, c->stream));
    M.vps.req = c->vps_mem;
    M.vps.resp = c->vps_mem + (size_t)VPS_MAX_SETS * VPS_PMAX * VPS_GRAN;
    M.vps.stat = reinterpret_cast<unsigned*>(c->vps_mem + c->vps_words);
    M.vps.nsets = nsets;
    M.vps.nprob = n;
    M.vps.fault = 0;
    c->vps_stats[0] = 1;
    launch_closure(true, n + nsets * VPS_SLICES, c->stream, M, c->pb.obs, c->V, to_dev(*w), c->P, params, 0, loss, grad, joints, nullptr);
    HIP_OK(c, hipGetLastError());
    if (verts) return run_vertex_pass(c, verts);
    return MVFIT_OK;
}

extern "C" int mvfit_closure(mvfit_ctx* c, const mvfit_weights* w, const float* params, float* loss, float* grad,
                             float* verts, float* joints) {
    if (!c || !w || !params || !loss) return MVFIT_E_ARG;
    if (c->B == 0) return fail(c, MVFIT_E_STATE, "call mvfit_set_problems first");
    int rc = check_flags(c, w->flags);
    if (rc) return rc;
    const bool sdf = w->coll_loss_weight > 0.f;
    if (sdf && !c->sdf_num_faces && !round_term(c))
        return fail(c, MVFIT_E_STATE, "coll_loss_weight > 0 needs the SDF term's faces: call mvfit_set_sdf first");
    HIP_OK(c, hipSetDevice(c->device));
    if (c->opt.closure_vposer_helpers && (w->flags & MVFIT_F_VPOSER) && c->vps_mem && !sdf)
        return closure_via_helpers(c, w, params, loss, grad, verts, joints);
    float* vbuf = verts ? verts : c->pb.verts;
    // the interpenetration term reads every vertex: it forces the vertex pass
    const bool sparse = (w->flags & MVFIT_F_SPARSE_VERTS) != 0 && !sdf;
    if (!sparse || verts) {
        launch_prep(c->B, c->stream, c->M, c->pb.obs, c->P, params, w->flags, nullptr);
        HIP_OK(c, hipGetLastError());
        rc = run_vertex_pass(c, vbuf);
        if (rc) return rc;
    }
    if (sdf) {
        rc = ensure_sdf_buffers(c);
        if (!rc) rc = run_sdf_term(c, vbuf, nullptr, c->stream);
        if (rc) return rc;
    }
    prof_begin(c, c->ev_step);
    launch_closure(false, c->B, c->stream, c->M, c->pb.obs, c->V, to_dev(*w), c->P, params, sparse ? 0 : 1, loss, grad, joints,
                   sdf ? c->pb.sdf_adj : nullptr);
    prof_end(c, c->ev_step);
    HIP_OK(c, hipGetLastError());
    return MVFIT_OK;
}

// The path's only collective: all-gather of the ranks' fitted parameters over RCCL, for hosts that own a
// communicator.  libmvfit does not link RCCL: the communicator belongs to the RCCL copy the host process loaded (PyTorch
// ships its own), so ncclAllGather is bound at run time to THAT library - the one already resident - never to a second one.
extern "C" int mvfit_gather(mvfit_ctx* c, void* rccl_comm, const void* send, void* recv, size_t bytes_per_rank) {
    if (!c) return MVFIT_E_ARG;
    if (!rccl_comm || !send || !recv) return fail(c, MVFIT_E_ARG, "mvfit_gather: null communicator or buffer");
    if (bytes_per_rank == 0) return MVFIT_OK;
    typedef int (*allgather_fn)(const void*, void*, size_t, int, void*, hipStream_t);     // ncclAllGather
    static allgather_fn fn = nullptr;
    if (!fn) {
        fn = reinterpret_cast<allgather_fn>(dlsym(RTLD_DEFAULT, "ncclAllGather"));
        for (const char* so : {"librccl.so", "librccl.so.1"}) {
            if (fn) break;
            if (void* h = dlopen(so, RTLD_NOW | RTLD_NOLOAD)) fn = reinterpret_cast<allgather_fn>(dlsym(h, "ncclAllGather"));
        }
    }
    if (!fn) return fail(c, MVFIT_E_STATE, "mvfit_gather: no RCCL library is loaded in this process (ncclAllGather not found)");
    HIP_OK(c, hipSetDevice(c->device));
    const int rc = fn(send, recv, bytes_per_rank, /* ncclInt8 */ 0, rccl_comm, c->stream);
    if (rc != 0) return fail(c, MVFIT_E_HIP, "mvfit_gather: ncclAllGather returned %d", rc);
    return MVFIT_OK;
}

extern "C" int mvfit_profile(mvfit_ctx* c, int enable) {
    if (!c) return MVFIT_E_ARG;
    c->profile = enable != 0;
    return MVFIT_OK;
}

// n back-to-back launches of the vertex pass on the pose operands the last closure / fit left behind,
// bracketed by ONE hipEvent pair on the ctx stream: elapsed / n is the per-launch duration with the event
// markers' own ~2-4 us amortised away (a pair around a single launch over-reports by about that much).
static int profile_vertex_pass(mvfit_ctx* c, int launches, int flavour, double* avg_ms) {
    if (!c || !avg_ms || launches <= 0) return MVFIT_E_ARG;
    if (c->B == 0) return fail(c, MVFIT_E_STATE, "call mvfit_set_problems first");
    HIP_OK(c, hipSetDevice(c->device));
    DevPose P = c->P;
    if (flavour == 1) {
        // the pass as the asynchronous fit launches it: operands from ring slot 0 (whatever trial points the last fit
        // left there), non-temporal basis stream / vertex stores, no side outputs; round 0 is live for every problem
        if (!c->ring.tag) return fail(c, MVFIT_E_STATE, "no asynchronous fit has run on this batch yet");
        P.coefH = c->ring.coefH; P.coefT = nullptr; P.Amat = c->ring.Amat; P.tau = c->ring.tau;
        P.tag = c->ring.tag; P.done_round = c->ring.done_round; P.stats = c->ring.stats; P.round = 0;
    }
    if (flavour == 2) {
        // the RESIDENT pass alone: `launches` (<= ring slots) closure rounds whose operands are already in the ring (whatever
        // trial points the last fit left in slots 0 .. launches - 1) and whose tags say so - ONE kernel launch inside one
        // hipEvent pair serves them back to back; elapsed / launches = the service time of a round with no optimiser next door
        if (!c->ring.tag || !c->resident_tpw) return fail(c, MVFIT_E_STATE, "no asynchronous fit with the resident pass has run on this batch yet");
        const AsyncRing& R = c->ring;
        const int n = std::min(c->B, R.Bpad), rounds = std::min(launches, R.nslots);
        std::vector<unsigned> tg((size_t)R.nslots * R.Bpad, 0u), dn((size_t)c->Bpad, 0u);
        for (int sl = 0; sl < rounds; ++sl) for (int q = 0; q < n; ++q) tg[(size_t)sl * R.Bpad + q] = (unsigned)sl + 1u;
        for (int q = 0; q < n; ++q) dn[q] = (unsigned)rounds;
        HIP_OK(c, hipStreamSynchronize(c->stream));
        HIP_OK(c, hipMemcpy(R.tag, tg.data(), tg.size() * 4, hipMemcpyHostToDevice));
        HIP_OK(c, hipMemcpy(R.done_round, dn.data(), dn.size() * 4, hipMemcpyHostToDevice));
        HIP_OK(c, hipMemset(R.pass_done, 0, 4 * kPassWords));
        ResidentArgs RA{};
        RA.coefH = R.coefH; RA.Amat = R.Amat; RA.tau = R.tau; RA.tag = R.tag; RA.done_round = R.done_round; RA.stats = R.stats;
        RA.wg_round = R.pass_done; RA.verts = c->pb.verts; RA.capture_round = -1; RA.nslots = R.nslots; RA.rb = R.Bpad;
        RA.b_lo = 0; RA.n = n; RA.max_rounds = (unsigned)rounds + 1u;
        hipEvent_t a, b;
        HIP_OK(c, hipEventCreate(&a)); HIP_OK(c, hipEventCreate(&b));
        HIP_OK(c, hipEventRecord(a, c->stream));
        hipError_t e = launch_vertex_pass_resident(c->M, RA, c->resident_tpw, c->stream);
        HIP_OK(c, hipEventRecord(b, c->stream));
        HIP_OK(c, hipStreamSynchronize(c->stream));
        float ms = 0.f;
        hipError_t e2 = hipEventElapsedTime(&ms, a, b);
        hipEventDestroy(a); hipEventDestroy(b);
        if (e != hipSuccess || e2 != hipSuccess) return fail(c, MVFIT_E_HIP, "resident vertex pass timing failed");
        *avg_ms = (double)ms / rounds;
        return MVFIT_OK;
    }
    hipEvent_t a, b;
    HIP_OK(c, hipEventCreate(&a)); HIP_OK(c, hipEventCreate(&b));
    hipError_t e = launch_vertex_pass(c->M, P, c->B, c->pb.verts, c->opt.pass_kernel, c->stream);      // warm
    HIP_OK(c, hipEventRecord(a, c->stream));
    for (int i = 0; i < launches && e == hipSuccess; ++i) e = launch_vertex_pass(c->M, P, c->B, c->pb.verts, c->opt.pass_kernel, c->stream);
    HIP_OK(c, hipEventRecord(b, c->stream));
    HIP_OK(c, hipStreamSynchronize(c->stream));
    float ms = 0.f;
    hipError_t e2 = hipEventElapsedTime(&ms, a, b);
    hipEventDestroy(a); hipEventDestroy(b);
    if (e != hipSuccess || e2 != hipSuccess) return fail(c, MVFIT_E_HIP, "vertex pass timing failed");
    *avg_ms = (double)ms / launches;
    return MVFIT_OK;
}

extern "C" int mvfit_profile_vertex_pass(mvfit_ctx* c, int launches, double* avg_ms) {
    return profile_vertex_pass(c, launches, 0, avg_ms);
}

extern "C" int mvfit_profile_vertex_pass_ex(mvfit_ctx* c, int launches, int flavour, double* avg_ms) {
    return profile_vertex_pass(c, launches, flavour, avg_ms);
}

static double drain(std::vector<std::pair<hipEvent_t, hipEvent_t>>& evs, int* n) {
    double tot = 0.0;
    int cnt = 0;
    for (auto& e : evs) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e.first, e.second) == hipSuccess) { tot += ms; ++cnt; }
        hipEventDestroy(e.first); hipEventDestroy(e.second);
    }
    evs.clear();
    *n = cnt;
    return cnt ? tot / cnt : 0.0;
}

extern "C" int mvfit_pass_profile(mvfit_ctx* c, int* tiles_per_wg, int* workgroups, int* rounds, double* span_ms, double* busy_ms,
                                  double* slowest_ms) {
    if (!c) return MVFIT_E_ARG;
    if (tiles_per_wg) *tiles_per_wg = c->resident_tpw;
    if (workgroups) *workgroups = plan_resident_grid(c->resident_tpw, c->M.ntiles);
    if (rounds) *rounds = c->res_rounds;
    if (span_ms) *span_ms = c->res_span_ms;
    if (busy_ms) *busy_ms = c->res_busy_ms;
    if (slowest_ms) *slowest_ms = c->res_slowest_ms;
    return MVFIT_OK;
}

extern "C" int mvfit_profile_read(mvfit_ctx* c, double* vp_ms, int* launches, double* step_ms, int* step_launches) {
    if (!c) return MVFIT_E_ARG;
    HIP_OK(c, hipStreamSynchronize(c->stream));
    int n1 = 0, n2 = 0;
    double a = drain(c->ev_vp, &n1), b = drain(c->ev_step, &n2);
    // resident pass (one launch per fit): the per-round service span stamped inside the kernel stands for the launch duration
    if (n1 == 0 && c->res_rounds > 0) { a = c->res_span_ms; n1 = c->res_rounds; }
    if (vp_ms) *vp_ms = a;
    if (launches) *launches = n1;
    if (step_ms) *step_ms = b;
    if (step_launches) *step_launches = n2;
    return MVFIT_OK;
}
