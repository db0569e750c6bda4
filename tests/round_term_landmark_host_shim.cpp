// Host build of csrc/round_term.cpp for tests/test_round_term_landmark_cpu.py (clang++ -O2 -shared -fPIC, no HIP): the sibling
// of round_term_scan_host_shim.cpp that also fills TermInputs' lm block - the fields of that shim in its order, then the lm
// block in the order of LM_FIELDS in the test - and writes out the landmark evaluation's step.
#include <cstdint>
#include <cstring>
#include <initializer_list>

#include "../mvsmplfitting_amd/csrc/round_term.h"

using namespace mvfit;

template <typename T>
static T* ptr(double v) { return reinterpret_cast<T*>(static_cast<uintptr_t>(v)); }
static double num(const void* p) { return static_cast<double>(reinterpret_cast<uintptr_t>(p)); }

static TermInputs inputs(const double* v, int* count = nullptr) {
    TermInputs in;
    int i = 0;
    in.B = (int)v[i++]; in.Bpad = (int)v[i++]; in.nv = (int)v[i++];
    in.sdf_faces = ptr<const int32_t>(v[i++]); in.sdf_num_faces = (int)v[i++]; in.sdf_grid = (int)v[i++]; in.sdf_cull = ptr<void>(v[i++]);
    in.sdf_box = ptr<SdfBox>(v[i++]); in.sdf_samp = ptr<void>(v[i++]); in.sdf_entries = ptr<void>(v[i++]); in.sdf_adj = ptr<SdfAdj>(v[i++]);
    in.obst.on = v[i++] != 0; in.obst.tab = ptr<void>(v[i++]); in.obst.box = ptr<void>(v[i++]); in.obst.phi = ptr<float>(v[i++]);
    in.obst.grid = (int)v[i++]; in.obst.rob = (float)v[i++];
    in.sil.on = v[i++] != 0; in.sil.ws = ptr<void>(v[i++]); in.sil.cs = ptr<void>(v[i++]);
    in.sil.M = (int)v[i++]; in.sil.H = (int)v[i++]; in.sil.W = (int)v[i++]; in.sil.C = (int)v[i++]; in.sil.nchunks = (int)v[i++];
    in.sil.stride = (int)v[i++]; in.sil.occ = ptr<void>(v[i++]); in.sil.occ_on = v[i++] != 0; in.sil.occ_margin = (float)v[i++];
    in.silt.on = v[i++] != 0; in.silt.w_in = (float)v[i++]; in.silt.w_out = (float)v[i++]; in.silt.sigma = (float)v[i++];
    in.silt.g_verts = ptr<float>(v[i++]); in.silt.loss = ptr<float>(v[i++]); in.silt.part = ptr<float>(v[i++]);
    in.vt.on = v[i++] != 0; in.vt.term = v[i++] != 0; in.vt.K = (int)v[i++]; in.vt.targets = ptr<float>(v[i++]);
    in.vt.weights = ptr<float>(v[i++]); in.vt.partial = ptr<double>(v[i++]);
    in.vt.g_verts = ptr<float>(v[i++]); in.vt.loss = ptr<float>(v[i++]); in.vt.part = ptr<float>(v[i++]);
    in.mix.on = v[i++] != 0; in.mix.scene = (float)v[i++]; in.mix.silhouette = (float)v[i++]; in.mix.vertex_targets = (float)v[i++];
    in.mix.w_in = (float)v[i++]; in.mix.w_out = (float)v[i++]; in.mix.sigma = (float)v[i++];
    in.mix.g_verts = ptr<float>(v[i++]); in.mix.loss = ptr<float>(v[i++]); in.mix.part = ptr<float>(v[i++]);
    in.mix.rec_scene = ptr<SdfAdj>(v[i++]); in.mix.rec_verts = ptr<SdfAdj>(v[i++]);
    in.mix.parts = ptr<float>(v[i++]); in.mix.sums = ptr<float>(v[i++]);
    in.scan.on = v[i++] != 0; in.scan.term = v[i++] != 0; in.scan.ws = ptr<void>(v[i++]);
    in.scan.N = (int)v[i++]; in.scan.Pmax = (int)v[i++]; in.scan.nf = (int)v[i++]; in.scan.ns = (int)v[i++];
    in.scan.faces = ptr<const int32_t>(v[i++]);
    in.scan.w_s2m = (float)v[i++]; in.scan.w_m2s = (float)v[i++]; in.scan.sigma = (float)v[i++];
    in.scan.g_verts = ptr<float>(v[i++]); in.scan.loss = ptr<float>(v[i++]); in.scan.part = ptr<float>(v[i++]);
    in.lm.on = v[i++] != 0; in.lm.term = v[i++] != 0; in.lm.tab = ptr<void>(v[i++]); in.lm.tgt = ptr<float>(v[i++]);
    in.lm.L = (int)v[i++]; in.lm.nt = (int)v[i++]; in.lm.has3d = v[i++] != 0;
    in.lm.rho = (float)v[i++]; in.lm.w3d = (float)v[i++]; in.lm.rho3d = (float)v[i++];
    in.lm.g_verts = ptr<float>(v[i++]); in.lm.loss = ptr<float>(v[i++]); in.lm.part = ptr<float>(v[i++]);
    if (count) *count = i;
    return in;
}

extern "C" int round_term_num_inputs() {
    const double zeros[128] = {0};
    int n = 0;
    inputs(zeros, &n);
    return n;
}
extern "C" int round_term_key_bytes() { return (int)sizeof(RoundTermPlan); }
extern "C" int round_term_slot(const double* in) { return term_slot(inputs(in)); }
extern "C" const char* round_term_name(int kind) { return term_kind_name((TermKind)kind); }

// out: kind, B, Bpad, nv, sums, sums_stride, steps, then per step its StepKind, the number of values and the values in the
// order of the step's struct (round_term.h).  key: the plan's bytes.  Returns the words written to out (up to out_cap).
extern "C" int round_term_plan(const double* in, int live, double* out, int out_cap, unsigned char* key) {
    const RoundTermPlan p = plan_round_term(inputs(in), live != 0);
    memcpy(key, &p, sizeof(p));
    int n = 0;
    auto put = [&](double v) { if (n < out_cap) out[n] = v; ++n; };
    auto row = [&](int kind, std::initializer_list<double> vals) {
        put(kind); put((double)vals.size());
        for (double v : vals) put(v);
    };
    put(p.kind); put(p.B); put(p.Bpad); put(p.nv); put(num(p.sums)); put(p.sums_stride); put(p.n);
    for (int i = 0; i < p.n; ++i) {
        const TermStep& s = p.step[i];
        switch (s.kind) {
        case STEP_SIL_EVAL:
            row(s.kind, {num(s.sil.ws), num(s.sil.cs), num(s.sil.occ), (double)s.sil.M, (double)s.sil.H, (double)s.sil.W, (double)s.sil.C,
                         (double)s.sil.nchunks, (double)s.sil.stride, (double)s.sil.occ_on, s.sil.occ_margin, s.sil.w_in, s.sil.w_out, s.sil.sigma,
                         num(s.sil.loss), num(s.sil.g_verts)});
            break;
        case STEP_VT_EVAL:
            row(s.kind, {(double)s.vt.K, num(s.vt.targets), num(s.vt.weights), num(s.vt.partial), num(s.vt.loss), num(s.vt.g_verts)});
            break;
        case STEP_MIX_COTANGENT:
            row(s.kind, {s.cot.lam_sil, s.cot.lam_vt, num(s.cot.g_sil), num(s.cot.L_sil), num(s.cot.g_vt), num(s.cot.L_vt), num(s.cot.g),
                         num(s.cot.L_v), num(s.cot.parts), num(s.cot.sums)});
            break;
        case STEP_PULLBACK:
            row(s.kind, {num(s.pull.g_verts), num(s.pull.loss), num(s.pull.part), num(s.pull.rec)});
            break;
        case STEP_SCENE:
            row(s.kind, {num(s.scene.tab), num(s.scene.box), num(s.scene.phi), (double)s.scene.grid, s.scene.rob, num(s.scene.null_box),
                         num(s.scene.entries), num(s.scene.rec)});
            break;
        case STEP_MIX_RECORD:
            row(s.kind, {s.rec.lam_sc, s.rec.lam_sil, s.rec.lam_vt, num(s.rec.rec_scene), num(s.rec.rec_verts), num(s.rec.L_sil), num(s.rec.L_vt),
                         num(s.rec.rec), num(s.rec.parts), num(s.rec.sums)});
            break;
        case STEP_SDF:
            row(s.kind, {num(s.sdf.faces), (double)s.sdf.num_faces, (double)s.sdf.grid, num(s.sdf.box), num(s.sdf.samp), num(s.sdf.entries),
                         num(s.sdf.adj), num(s.sdf.cull)});
            break;
        case STEP_SCAN_EVAL:
            row(s.kind, {num(s.scan.ws), num(s.scan.faces), (double)s.scan.N, (double)s.scan.Pmax, (double)s.scan.nf, (double)s.scan.ns,
                         s.scan.w_s2m, s.scan.w_m2s, s.scan.sigma, num(s.scan.loss), num(s.scan.g_verts)});
            break;
        case STEP_LM_EVAL:
            row(s.kind, {num(s.lm.tab), num(s.lm.tgt), (double)s.lm.L, (double)s.lm.nt, (double)s.lm.has3d, s.lm.rho, s.lm.w3d, s.lm.rho3d,
                         num(s.lm.loss), num(s.lm.g_verts)});
            break;
        default:
            row(-1, {});
        }
    }
    return n;
}
