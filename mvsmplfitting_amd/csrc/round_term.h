// The term of a chained round behind coll_loss_weight, decided before anything is launched (plain C++17, no HIP): which of the
// terms holds the ctx's one term slot, and the launches a round makes for it, each with every pointer and scalar its launcher
// takes.  launch_term (mvfit_api.hip) executes the plan and decides nothing; the captured round graph is keyed by the plan's
// bytes (mvfit_fit.hip), so what a kernel node bakes in and what the key compares are one list.  The table: DESIGN.md §4.6.
#pragma once
#include <stdint.h>

namespace mvfit {

struct SdfAdj;
struct SdfBox;

// The facts the plan depends on, as mvfit_api.hip reads them off the ctx (term_inputs).  Pointers are device addresses: the
// plan copies them and never follows one.  Buffers of a HIP vector type are held as void.
struct TermInputs {
    int B = 0, Bpad = 0, nv = 0;
    // mvfit_set_sdf's term and its cull workspace
    const int32_t* sdf_faces = nullptr;
    int sdf_num_faces = 0, sdf_grid = 0;
    void* sdf_cull = nullptr;
    // the per-problem work buffers of ensure_sdf_buffers (ProblemBufs)
    SdfBox* sdf_box = nullptr;
    void* sdf_samp = nullptr;
    void* sdf_entries = nullptr;
    SdfAdj* sdf_adj = nullptr;
    struct {            // frozen obstacles (Obstacles)
        bool on = false;
        const void *tab = nullptr, *box = nullptr;
        const float* phi = nullptr;
        int grid = 0;
        float rob = 0.f;
    } obst;
    struct {            // the mask set (SilState): what a silhouette evaluation's nodes bake in
        bool on = false;
        const void *ws = nullptr, *cs = nullptr;
        int M = 0, H = 0, W = 0, C = 0, nchunks = 0, stride = 0;
        const void* occ = nullptr;
        bool occ_on = false;
        float occ_margin = 0.f;
    } sil;
    struct {            // the silhouette term and its round buffers (SilTerm)
        bool on = false;
        float w_in = 0.f, w_out = 0.f, sigma = 0.f;
        float *g_verts = nullptr, *loss = nullptr, *part = nullptr;
    } silt;
    struct {            // the target set, the vertex-target term and its round buffers (VtxTargets)
        bool on = false, term = false;
        int K = 0;
        const float *targets = nullptr, *weights = nullptr;
        double* partial = nullptr;
        float *g_verts = nullptr, *loss = nullptr, *part = nullptr;
    } vt;
    struct {            // the term mix (TermMix)
        bool on = false;
        float scene = 0.f, silhouette = 0.f, vertex_targets = 0.f;
        float w_in = 0.f, w_out = 0.f, sigma = 0.f;
        float *g_verts = nullptr, *loss = nullptr, *part = nullptr;
        SdfAdj *rec_scene = nullptr, *rec_verts = nullptr;
        float *parts = nullptr, *sums = nullptr;
        float scan = 0.f;               // the scan share, and the scan term's scalars of a mix with one
        float scan_w_s2m = 0.f, scan_w_m2s = 0.f, scan_sigma = 0.f;
    } mix;
    struct {            // the scan set (ScanState), the scan term and its round buffers (ScanTerm)
        bool on = false, term = false;
        const void* ws = nullptr;
        int N = 0, Pmax = 0, nf = 0, ns = 0;
        const int32_t* faces = nullptr;
        float w_s2m = 0.f, w_m2s = 0.f, sigma = 0.f;
        float *g_verts = nullptr, *loss = nullptr, *part = nullptr;
    } scan;
    struct {            // the landmark table and targets (LmState), the landmark term and its round buffers
        bool on = false, term = false;
        const void* tab = nullptr;
        const float* tgt = nullptr;
        int L = 0, nt = 0;
        bool has3d = false;
        float rho = 0.f, w3d = 0.f, rho3d = 0.f;
        float *g_verts = nullptr, *loss = nullptr, *part = nullptr;
    } lm;
};

enum TermKind { TERM_SDF = 0, TERM_SCENE, TERM_SILHOUETTE, TERM_VERTEX_TARGET, TERM_MIX, TERM_SCAN, TERM_LANDMARK };

// who holds the term slot: the mix, else the vertex-target term, the silhouette term, the scan term, the landmark term, the
// obstacles, else mvfit_set_sdf's term
TermKind term_slot(const TermInputs& in);
const char* term_kind_name(TermKind kind);

enum StepKind { STEP_SIL_EVAL = 1, STEP_VT_EVAL, STEP_MIX_COTANGENT, STEP_PULLBACK, STEP_SCENE, STEP_MIX_RECORD, STEP_SDF,
                STEP_SCAN_EVAL, STEP_LM_EVAL };

// sil_round: the mask set's baked values (occluders only when they are set), the scalars, the round buffers it writes
struct SilEvalStep {
    const void *ws, *cs, *occ;
    int M, H, W, C, nchunks, stride, occ_on;
    float occ_margin, w_in, w_out, sigma;
    float *loss, *g_verts;
};
// launch_vertex_target
struct VtEvalStep {
    int K;
    const float *targets, *weights;
    double* partial;
    float *loss, *g_verts;
};
// launch_term_mix_cotangent (a component with share 0 has null pointers: they are never read)
struct MixCotangentStep {
    float lam_sil, lam_vt;
    const float *g_sil, *L_sil, *g_vt, *L_vt;
    float *g, *L_v, *parts, *sums;
    float lam_scan;
    const float *g_scan, *L_scan;
};
// launch_silhouette_pullback: a vertex cotangent and its loss -> a record
struct PullbackStep {
    const float *g_verts, *loss;
    float* part;
    SdfAdj* rec;
};
// launch_scene_term
struct SceneStep {
    const void *tab, *box;
    const float* phi;
    int grid;
    float rob;
    const SdfBox* null_box;
    void* entries;
    SdfAdj* rec;
};
// launch_term_mix_record
struct MixRecordStep {
    float lam_sc, lam_sil, lam_vt;
    const SdfAdj *rec_scene, *rec_verts;
    const float *L_sil, *L_vt;
    SdfAdj* rec;
    float *parts, *sums;
    float lam_scan;
    const float* L_scan;
};
// launch_sdf_term (the tile keys of the box come with the round's pass, not with the plan)
struct SdfStep {
    const int32_t* faces;
    int num_faces, grid;
    SdfBox* box;
    void *samp, *entries;
    SdfAdj* adj;
    void* cull;
};

// scan_round: the scan set's baked values (the workspace's layout follows from the sizes), the scalars, the round buffers it writes
struct ScanEvalStep {
    const void* ws;
    const int32_t* faces;
    int N, Pmax, nf, ns;
    float w_s2m, w_m2s, sigma;
    float *loss, *g_verts;
};

// launch_landmarks: the table and the targets (each one buffer whose layout follows from the sizes), the scalars, the round
// buffers it writes; the cameras are the problems' and come with the round
struct LmEvalStep {
    const void* tab;
    const float* tgt;
    int L, nt, has3d;
    float rho, w3d, rho3d;
    float *loss, *g_verts;
};
static_assert(sizeof(LmEvalStep) <= sizeof(SilEvalStep), "the plan's step union keeps its size");

struct TermStep {
    int kind;           // StepKind
    union {
        SilEvalStep sil;
        VtEvalStep vt;
        MixCotangentStep cot;
        PullbackStep pull;
        SceneStep scene;
        MixRecordStep rec;
        SdfStep sdf;
        ScanEvalStep scan;
        LmEvalStep lm;
    };
};

constexpr int kMaxTermSteps = 7;

// Zero-filled, then assigned field by field: the bytes are a function of the fields (they are the graph key), and a plan of
// all zeros is the round without a term.
struct RoundTermPlan {
    int kind;           // TermKind
    int B, Bpad, nv;
    int n;              // steps
    int sums_stride;    // bytes between two problems' sums
    const void* sums;   // where the round leaves every problem's sum: mvfit_sdf_term_read
    TermStep step[kMaxTermSteps];
};

// live = false: the round of a fit without coll_loss_weight runs no term - the plan of all zeros
RoundTermPlan plan_round_term(const TermInputs& in, bool live = true);

}  // namespace mvfit
