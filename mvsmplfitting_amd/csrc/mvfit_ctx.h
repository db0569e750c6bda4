// The ctx of the C ABI and what the host files that implement it share: mvfit_api.hip (lifetime, problems, closure, profile),
// mvfit_fit.hip (the optimiser's drivers) and mvfit_scene.hip (entries that never run the optimiser).  Included by those three only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "dev_mem.h"
#include "fit_kernels.h"
#include "fit_plan.h"
#include "landmark.h"
#include "launchers.h"
#include "round_term.h"
#include "scan_loss.h"
#include "silhouette.h"
#include "term_mix.h"
#include "vertex_target.h"

using namespace mvfit;          // (the three host files only: their bodies name the library's types unqualified)

// device buffers sized by the batch, owned by mvfit_ctx::problem_mem (the SDF term's: ensure_sdf_buffers)
struct ProblemBufs {
    float *camR = nullptr, *camt = nullptr, *camf = nullptr, *camc = nullptr, *gt = nullptr, *wc = nullptr;
    ObsBlock* obs = nullptr;           // [B] packed observations (LDS image block)
    float* verts = nullptr;            // [B][nv][3] internal vertex buffer
    float *gt3d = nullptr, *c3d = nullptr;       // staging of mvfit_set_joints3d ([B][17][3], [B][17])
    SdfBox* sdf_box = nullptr;         // [B]
    float4* sdf_samp = nullptr;        // [B][nv]
    void* sdf_entries = nullptr;       // [B][nv] entry list
    SdfAdj* sdf_adj = nullptr;         // [B]
    int* sdf_gate_round = nullptr;     // [B] service rounds: the gate words as the round's gate kernel found them (what the term's kernels read)
    unsigned long long* sdf_boxpart = nullptr;   // [B][ntiles][6] the vertex pass's own per-tile keys of the term's bounding box (single-chunk split kernel)
};

// frozen obstacles of the scene term (mvfit_set_scene_obstacles): per problem its scene's row, its box and its field, owned
// by mvfit_ctx::obst_mem.  The buffers keep their addresses while (B, grid) stay the same, so a re-freeze leaves the
// captured round graph valid.
struct Obstacles {
    bool on = false;
    int grid = 0;
    float rob = 0.f;
    int32_t* tab = nullptr;            // [B] SceneBody rows
    float4* box = nullptr;             // [B] (centre, scale)
    float* phi = nullptr;              // [B][G^3]
};

// the silhouette term inside the fit (mvfit_set_silhouette_term): weights and the buffers of a chained round, owned by
// mvfit_ctx::silterm_mem.  They are allocated by the first enable for the batch and keep their addresses while B stays.
struct SilTerm {
    bool on = false;
    float w_in = 1.f, w_out = 1.f, sigma = 0.f;
    float* g_verts = nullptr;          // [B][nv][3] the round's vertex cotangent
    float* loss = nullptr;             // [B] L_j of the last evaluation
    float* part = nullptr;             // slice partials of the pull-back (vjp_part_bytes)
};

// the scan term inside the fit (mvfit_set_scan_term): scalars and the buffers of a chained round, owned by
// mvfit_ctx::scanterm_mem.  They are allocated by the first enable for the batch and keep their addresses while B stays; the
// scan set itself (ScanState) is not tied to the batch.
struct ScanTerm {
    bool on = false;
    float w_s2m = 1.f, w_m2s = 0.f, sigma = 0.f;
    float* g_verts = nullptr;          // [B][nv][3] the round's vertex cotangent
    float* loss = nullptr;             // [B] L_j of the last evaluation
    float* part = nullptr;             // slice partials of the pull-back (vjp_part_bytes)
};

struct mvfit_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // ---- memory: every allocation belongs to one of these owners (dev_mem.h), grouped by lifetime; the structs handed to
    // ---- kernels (M, Q, P, F, ring) and pb / obst are plain views of it, reset by assignment.  A new buffer is added here only.
    // model lifetime (mvfit_create_ex .. mvfit_destroy): the model's tables, the renderer's faces, vps_mem
    DevPool model_mem;
    // problem lifetime (free_problem_buffers): what mvfit_set_problems and ensure_sdf_buffers allocate; the ring (its done_round
    // is sized by Bpad) and the obstacles go whenever the problems go, and each may be replaced on its own before that
    DevPool problem_mem, ring_mem, obst_mem, silterm_mem;
    DevPool vtgt_mem, vtterm_mem;      // the vertex-target set (re-made when (B, K) change) and its term's round buffers
    DevPool mix_mem;                   // the term mix's round buffers (mvfit_set_term_mix)
    DevPool scanterm_mem;              // the scan term's round buffers (mvfit_set_scan_term)
    DevPool lmtgt_mem, lmterm_mem;     // the landmark targets (re-made when (B, V, L, 3-D or not) change) and the term's round buffers
    // table lifetime (mvfit_set_landmarks .. the next one): the landmark table, independent of the problems
    DevPool lmtab_mem;
    // own lifetime: one buffer each, grown (or replaced) by the call that uses it, freed with the ctx
    DevBuf sdf_faces;                  // mvfit_set_sdf: faces as the reference's caller hands them to the op
    DevBuf sdf_cull;                   // face lists of the all-faces term (sdf_term.hip), sized for (B, sdf_num_faces): goes with either
    DevBuf sdf_op_ws;                  // face lists of the stand-alone op (mvfit_sdf), kept between calls of one shape
    DevBuf vp_log;                     // mvfit_profile: per-round stamps of the resident pass [kVpLogRounds][grid][2]
    DevBuf render_nrm, render_ws;      // overlay rendering: [B][nv][3] vertex normals of the call; workspace of the largest group seen
    DevBuf scene_tab;                  // image / instance tables of the last mvfit_render_scene
    PinnedBuf h_scene_tab[2];          // their staging, two slots used in turn: a slot is rewritten once the copy out of it (two calls back) is done
    DevBuf vjp_part, vjp_rec;          // mvfit_vertices_backward (vertex_backward.hip): slice partials and one record per problem, grown with the batch
    DevBuf scn_ws;                     // mvfit_scene_sdf_loss (scene_sdf.hip): tables, boxes, local vertices, fields, face lists and partials of one
    PinnedBuf h_scn_tab;               // group of scenes, grown to the largest call seen; the pinned staging of the call's tables
    DevBuf assoc_ws;                   // mvfit_associate_views (associate.hip): ray origins, then rays and linkage matrices of one group of frames
    DevBuf queue;                      // work queue of a single-launch fit with more problems than rows: next problem to hand out
    PinnedBuf h_done;                  // 2 slots
    PinnedBuf h_async_done;            // host word the last finishing problem writes
    // mask set of the silhouette term (mvfit_set_silhouettes, silhouette.hip): fields, contours, tables and work areas
    SilState sil;
    SilTerm silt;
    // scan set of the scan loss (mvfit_set_scans, scan_loss.hip): points, face records and work areas
    ScanState scan;
    ScanTerm scant;
    // target set and term of mvfit_set_vertex_targets / mvfit_set_vertex_target_term (vertex_target.hip)
    VtxTargets vt;
    // table, targets and term of mvfit_set_landmarks / mvfit_set_landmark_targets / mvfit_set_landmark_term (landmark.hip)
    LmState lm;
    // the weighted sum of the scene, silhouette, vertex-target and scan terms (mvfit_set_term_mix, term_mix.hip)
    TermMix mix;
    // ---- model ----
    DevModel M{};
    bool upload_failed = false, alloc_failed = false;
    int nv = 0;
    bool has_vposer = false;
    int gmm_M = 0;
    int32_t *d_faces = nullptr, *d_vf_ptr = nullptr, *d_vf_idx = nullptr;    // the model's faces and the vertex -> face CSR (faces in ascending id), when it has faces
    int num_faces = 0;
    // decoder helpers of the single-launch fit (vposer_service.h): granule memory [requests | answers | 2 counters]
    unsigned long long* vps_mem = nullptr;
    size_t vps_words = 0;
    unsigned vps_stats[3] = {0, 0, 0};     // launches with helpers in the last fit, answers timed out, helpers that gave up
    // ---- problems and their work buffers ----
    DevProblems Q{};
    int B = 0, Bpad = 0, V = 0;
    ProblemBufs pb;
    DevPose P{};
    FitBuffers F{};
    bool has_joints3d = false;
    hipEvent_t ev_done[2] = {nullptr, nullptr};
    // asynchronous full-mode fit: ring of pose operands + the side stream the vertex passes are queued on
    AsyncRing ring{};
    hipStream_t pass_stream = nullptr;
    hipEvent_t ev_batch[4] = {nullptr, nullptr, nullptr, nullptr}, ev_init = nullptr;
    unsigned async_stats[4] = {0, 0, 0, 0};
    mvfit_options opt{};               // precision / path selectors (include/mvfit.h); the library reads no environment variable
    int n_cu = 0;                      // compute units of the device (residency of the resident vertex pass)
    int resident_tpw = 0;              // tiles per workgroup of the resident pass in the last asynchronous fit (0: per-round launches)
    int h_queue0 = 0;
    bool resident_auto_off = false;    // automatic resident_pass: a fit on this ctx timed out waiting - later fits use per-round launches
    double res_span_ms = 0.0, res_busy_ms = 0.0, res_slowest_ms = 0.0;   // per round: service span / mean workgroup busy time / slowest workgroup (last profiled fit)
    int res_rounds = 0;
    float* capture_verts = nullptr;    // mvfit_debug_capture_pass: the pass of closure round capture_round writes here
    int capture_round = -1;
    float* trace = nullptr;            // caller's device buffer (mvfit_fit_trace), not owned
    int trace_cap = 0;
    // full-mode round loop captured as a graph: key = everything baked into the kernel nodes
    hipGraphExec_t round_graph = nullptr;
    std::vector<unsigned char> graph_key;
    int graph_rounds = 0;
    unsigned graph_builds = 0;         // round graphs captured on this ctx so far (mvfit_round_graph_info)
    // SDF interpenetration term (mvfit_set_sdf)
    int sdf_num_faces = 0, sdf_grid = 0;
    int sdf_op_B = 0, sdf_op_F = 0;
    // which path served the last mvfit_sdf / the SDF term of the last fit (mvfit_sdf_info): 0 walk over every face (short
    // list or lists switched off), 1 face lists, 2 walk because the lists' workspace did not fit
    int sdf_op_path = 0, sdf_term_path = 0;
    bool sdf_cull_refused = false;      // the term's workspace did not fit for the current (batch, face list)
    Obstacles obst;
    hipEvent_t scene_copied[2] = {nullptr, nullptr};
    int scene_slot = 0;
    // profiling
    bool profile = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_vp, ev_step;
};

namespace mvfit {

inline int fail(mvfit_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

}  // namespace mvfit

#define HIP_OK(c, call)                                                                          \
    do {                                                                                         \
        hipError_t e__ = (call);                                                                 \
        if (e__ != hipSuccess) return fail(c, MVFIT_E_HIP, "%s: %s", #call, hipGetErrorString(e__)); \
    } while (0)

namespace mvfit {

// Developer hooks (fault injection, experiment switches) exist only in the -DMVFIT_DEBUG_HOOKS variant build the tests that
// need them load (libmvfit_hooks.so); the released library has no trace of them and reads no environment variable.
#ifdef MVFIT_DEBUG_HOOKS
inline int debug_hook(const char* name) { const char* e = getenv(name); return e ? atoi(e) : 0; }
#else
constexpr int debug_hook(const char*) { return 0; }
#endif

// ---- helpers of mvfit_api.hip that the other host files use too ----
int check_flags(mvfit_ctx* c, uint32_t flags);
DevWeights to_dev(const mvfit_weights& w);
FitPlanIn plan_inputs(const mvfit_ctx* c);
void prof_begin(mvfit_ctx* c, std::vector<std::pair<hipEvent_t, hipEvent_t>>& evs);
void prof_end(mvfit_ctx* c, std::vector<std::pair<hipEvent_t, hipEvent_t>>& evs);
int run_vertex_pass(mvfit_ctx* c, float* verts);
int ensure_sdf_buffers(mvfit_ctx* c);
bool pass_writes_box_parts(const mvfit_ctx* c, int b_lo, int b_hi);
// the round's term: what launch_term needs is in the plan (round_term.h) - it never sees the ctx
TermInputs term_inputs(const mvfit_ctx* c);
hipError_t launch_term(const RoundTermPlan& plan, const DevModel& M, const DevPose& P, const DevProblems& Q, SilState& sil, ScanState& scan,
                       std::string& err, const float* verts, const int* gate, hipStream_t st, const unsigned long long* box_part);
int run_sdf_term(mvfit_ctx* c, const float* verts, const int* gate, hipStream_t st);
void drop_graph(mvfit_ctx* c);
void free_obstacles(mvfit_ctx* c);
void free_vertex_targets(mvfit_ctx* c);
void free_term_mix(mvfit_ctx* c);
void free_scan_term(mvfit_ctx* c);
void free_landmark_targets(mvfit_ctx* c);   // the targets, the term and its round buffers; the table stays
int ensure_scan_round(mvfit_ctx* c);        // mvfit_scan.hip: the scan term's round buffers, for its own setter and for the mix
inline const char* term_name(const mvfit_ctx* c) { return term_kind_name(term_slot(term_inputs(c))); }
// a term other than mvfit_set_sdf's is configured: it runs in chained rounds only and keeps no per-vertex samples
inline bool round_term(const mvfit_ctx* c) { return term_slot(term_inputs(c)) != TERM_SDF; }

// A data set a term reads went away (or is about to be re-made): its own term goes off, and so does a mix that gives it a share.
enum TermSource { SRC_OBSTACLES = 0, SRC_MASKS, SRC_TARGETS, SRC_SCANS };
inline bool& term_flag(mvfit_ctx* c, TermSource src) {
    return src == SRC_OBSTACLES ? c->obst.on : src == SRC_MASKS ? c->silt.on : src == SRC_TARGETS ? c->vt.term : c->scant.on;
}
inline void term_source_gone(mvfit_ctx* c, TermSource src) {
    const float share[] = {c->mix.scene, c->mix.silhouette, c->mix.vertex_targets, c->mix.scan};
    term_flag(c, src) = false;
    if (share[src] > 0.f) c->mix.on = false;
}
// the same around a re-make that can fail: a failure leaves no term behind, restore() after success brings both flags back
struct TermSuspend {
    mvfit_ctx* c;
    TermSource src;
    bool term, mix;
    TermSuspend(mvfit_ctx* c_, TermSource s) : c(c_), src(s), term(term_flag(c_, s)), mix(c_->mix.on) { term_source_gone(c, s); }
    void restore() { term_flag(c, src) = term; c->mix.on = mix; }
};

}  // namespace mvfit
