// The plan of a round's term (round_term.h): who holds the slot, and the step list of each slot (the table: DESIGN.md §4.6).
#include "round_term.h"

#include <string.h>

#include "../../include/mvfit.h"

namespace mvfit {

TermKind term_slot(const TermInputs& in) {
    return in.mix.on ? TERM_MIX : in.vt.term ? TERM_VERTEX_TARGET : in.silt.on ? TERM_SILHOUETTE : in.scan.term ? TERM_SCAN :
           in.lm.term ? TERM_LANDMARK : in.obst.on ? TERM_SCENE : TERM_SDF;
}

const char* term_kind_name(TermKind kind) {
    static const char* const names[] = {"sdf", "scene", "silhouette", "vertex-target", "mix", "scan", "landmark"};
    return names[kind];
}

namespace {

// the steps the single terms and the mix share; every field of a step is assigned here or stays zero
struct Builder {
    const TermInputs& in;
    RoundTermPlan& p;

    TermStep& add(StepKind kind) {
        TermStep& s = p.step[p.n++];
        s.kind = kind;
        return s;
    }
    // the evaluation writes the silhouette term's round buffers, whoever asks for it
    void sil_eval(float w_in, float w_out, float sigma) {
        SilEvalStep& s = add(STEP_SIL_EVAL).sil;
        s.ws = in.sil.ws; s.cs = in.sil.cs;
        s.M = in.sil.M; s.H = in.sil.H; s.W = in.sil.W; s.C = in.sil.C; s.nchunks = in.sil.nchunks; s.stride = in.sil.stride;
        if (in.sil.occ_on) { s.occ = in.sil.occ; s.occ_on = 1; s.occ_margin = in.sil.occ_margin; }
        s.w_in = w_in; s.w_out = w_out; s.sigma = sigma;
        s.loss = in.silt.loss; s.g_verts = in.silt.g_verts;
    }
    void vt_eval() {
        VtEvalStep& s = add(STEP_VT_EVAL).vt;
        s.K = in.vt.K; s.targets = in.vt.targets; s.weights = in.vt.weights; s.partial = in.vt.partial;
        s.loss = in.vt.loss; s.g_verts = in.vt.g_verts;
    }
    // the evaluation writes the scan term's round buffers, whoever asks for it
    void scan_eval(float w_s2m, float w_m2s, float sigma) {
        ScanEvalStep& s = add(STEP_SCAN_EVAL).scan;
        s.ws = in.scan.ws; s.faces = in.scan.faces;
        s.N = in.scan.N; s.Pmax = in.scan.Pmax; s.nf = in.scan.nf; s.ns = in.scan.ns;
        s.w_s2m = w_s2m; s.w_m2s = w_m2s; s.sigma = sigma;
        s.loss = in.scan.loss; s.g_verts = in.scan.g_verts;
    }
    void lm_eval() {
        LmEvalStep& s = add(STEP_LM_EVAL).lm;
        s.tab = in.lm.tab; s.tgt = in.lm.tgt; s.L = in.lm.L; s.nt = in.lm.nt; s.has3d = in.lm.has3d ? 1 : 0;
        s.rho = in.lm.rho; s.w3d = in.lm.w3d; s.rho3d = in.lm.rho3d;
        s.loss = in.lm.loss; s.g_verts = in.lm.g_verts;
    }
    void pullback(const float* g_verts, const float* loss, float* part, SdfAdj* rec) {
        PullbackStep& s = add(STEP_PULLBACK).pull;
        s.g_verts = g_verts; s.loss = loss; s.part = part; s.rec = rec;
    }
    void scene(SdfAdj* rec) {
        SceneStep& s = add(STEP_SCENE).scene;
        s.tab = in.obst.tab; s.box = in.obst.box; s.phi = in.obst.phi; s.grid = in.obst.grid; s.rob = in.obst.rob;
        s.null_box = in.sdf_box; s.entries = in.sdf_entries; s.rec = rec;
    }
    void sums_at(const void* sums, size_t stride) { p.sums = sums; p.sums_stride = (int)stride; }

    // the live vertex terms' evaluations, their mixed cotangent in front of ONE pull-back and - with a scene share - the scene
    // term into a record of its own and the merge of the two records
    void mix() {
        const auto& X = in.mix;
        const bool sil = X.silhouette > 0.f, vt = X.vertex_targets > 0.f, scan = X.scan > 0.f, sc = X.scene > 0.f;
        if (sil) sil_eval(X.w_in, X.w_out, X.sigma);
        if (vt) vt_eval();
        if (scan) scan_eval(X.scan_w_s2m, X.scan_w_m2s, X.scan_sigma);
        const float *g = X.g_verts, *L = X.loss;
        // one live vertex term with share 1: its own buffers go to the pull-back as they are
        if (sil && !vt && !scan && X.silhouette == 1.f) { g = in.silt.g_verts; L = in.silt.loss; }
        else if (vt && !sil && !scan && X.vertex_targets == 1.f) { g = in.vt.g_verts; L = in.vt.loss; }
        else if (scan && !sil && !vt && X.scan == 1.f) { g = in.scan.g_verts; L = in.scan.loss; }
        else {
            MixCotangentStep& s = add(STEP_MIX_COTANGENT).cot;
            s.lam_sil = X.silhouette; s.lam_vt = X.vertex_targets;
            if (sil) { s.g_sil = in.silt.g_verts; s.L_sil = in.silt.loss; }
            if (vt) { s.g_vt = in.vt.g_verts; s.L_vt = in.vt.loss; }
            if (scan) { s.lam_scan = X.scan; s.g_scan = in.scan.g_verts; s.L_scan = in.scan.loss; }
            s.g = X.g_verts; s.L_v = X.loss;
            if (!sc) { s.parts = X.parts; s.sums = X.sums; }       // (with a scene share the record merge writes them)
        }
        pullback(g, L, X.part, sc ? X.rec_verts : in.sdf_adj);
        if (sc) {
            scene(X.rec_scene);
            MixRecordStep& s = add(STEP_MIX_RECORD).rec;
            s.lam_sc = X.scene; s.lam_sil = X.silhouette; s.lam_vt = X.vertex_targets;
            s.rec_scene = X.rec_scene; s.rec_verts = X.rec_verts;
            if (sil) s.L_sil = in.silt.loss;
            if (vt) s.L_vt = in.vt.loss;
            if (scan) { s.lam_scan = X.scan; s.L_scan = in.scan.loss; }
            s.rec = in.sdf_adj; s.parts = X.parts; s.sums = X.sums;
        }
        sums_at(X.sums, sizeof(float));                              // the weighted sum of the parts: penalty = w^2 sums
    }
};

}  // namespace

RoundTermPlan plan_round_term(const TermInputs& in, bool live) {
    RoundTermPlan p;
    memset(&p, 0, sizeof(p));
    if (!live) return p;
    p.kind = term_slot(in);
    p.B = in.B; p.Bpad = in.Bpad; p.nv = in.nv;
    Builder b{in, p};
    switch (p.kind) {
    case TERM_MIX:
        b.mix();
        break;
    case TERM_VERTEX_TARGET:
        b.vt_eval();
        b.pullback(in.vt.g_verts, in.vt.loss, in.vt.part, in.sdf_adj);
        b.sums_at(in.vt.loss, sizeof(float));                        // L_j itself (the record holds its root)
        break;
    case TERM_SILHOUETTE:
        b.sil_eval(in.silt.w_in, in.silt.w_out, in.silt.sigma);
        b.pullback(in.silt.g_verts, in.silt.loss, in.silt.part, in.sdf_adj);
        b.sums_at(in.silt.loss, sizeof(float));
        break;
    case TERM_SCAN:
        b.scan_eval(in.scan.w_s2m, in.scan.w_m2s, in.scan.sigma);
        b.pullback(in.scan.g_verts, in.scan.loss, in.scan.part, in.sdf_adj);
        b.sums_at(in.scan.loss, sizeof(float));
        break;
    case TERM_LANDMARK:
        b.lm_eval();
        b.pullback(in.lm.g_verts, in.lm.loss, in.lm.part, in.sdf_adj);
        b.sums_at(in.lm.loss, sizeof(float));
        break;
    case TERM_SCENE:
        b.scene(in.sdf_adj);
        b.sums_at(in.sdf_adj, MVFIT_TERM_RECORD_FLOATS * sizeof(float));
        break;
    default: {
        SdfStep& s = b.add(STEP_SDF).sdf;
        s.faces = in.sdf_faces; s.num_faces = in.sdf_num_faces; s.grid = in.sdf_grid;
        s.box = in.sdf_box; s.samp = in.sdf_samp; s.entries = in.sdf_entries; s.adj = in.sdf_adj; s.cull = in.sdf_cull;
        b.sums_at(in.sdf_adj, MVFIT_TERM_RECORD_FLOATS * sizeof(float));
    }
    }
    return p;
}

}  // namespace mvfit
