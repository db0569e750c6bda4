// Host build of csrc/model_prep.cpp for tests/test_model_prep_cpu.py (clang++ -O2 -shared -fPIC, no HIP): prepare_model's
// tables copied by name into caller buffers, so the model constants can be checked without a GPU.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>

#include "../mvsmplfitting_amd/csrc/model_prep.h"

using mvfit::HostModel;

extern "C" void* prep_run(const mvfit_model* m, int contraction, int dense_skinning, int* rc, char* err, int errlen) {
    HostModel* h = new HostModel();
    std::string e;
    *rc = mvfit::prepare_model(*m, contraction, dense_skinning, *h, e);
    snprintf(err, errlen, "%s", e.c_str());
    return h;
}

extern "C" void prep_free(void* h) { delete static_cast<HostModel*>(h); }

// member `name` of HostModel ("lds.<field>" for the ModelLds image): its size in bytes (-1: no such member), copied to dst
// when dst is not null
extern "C" long prep_get(void* hp, const char* name, void* dst) {
    HostModel& h = *static_cast<HostModel*>(hp);
    std::pair<const void*, size_t> r{nullptr, 0};
    bool found = false;
#define VEC(f) if (!found && !strcmp(name, #f)) { r = {h.f.data(), h.f.size() * sizeof(h.f[0])}; found = true; }
#define VAL(f) if (!found && !strcmp(name, #f)) { r = {&h.f, sizeof(h.f)}; found = true; }
#define LDS(f) if (!found && !strcmp(name, "lds." #f)) { r = {&h.lds.f, sizeof(h.lds.f)}; found = true; }
    VAL(nv) VAL(ntiles) VAL(nv_pad) VAL(ns) VAL(nc) VAL(nc_pad) VAL(bs_scale) VAL(half_basis) VAL(has_vposer) VAL(gmm_M)
    VAL(num_faces) VAL(lds)
    VEC(bs4) VEC(bs_h2) VEC(bs_vm) VEC(vt_planes) VEC(wt_tiles) VEC(w_vm) VEC(wsp_w) VEC(wsp_j) VEC(sel_v) VEC(pd_sub)
    VEC(pd_subT) VEC(tile_sel_start) VEC(tile_sel_local) VEC(tile_sel_slot) VEC(vp_w1) VEC(vp_b1) VEC(vp_w2) VEC(vp_b2)
    VEC(vp_w3) VEC(vp_b3) VEC(vp_w1T) VEC(vp_w2T) VEC(vp_w3T) VEC(vp_tw2) VEC(vp_tw3) VEC(gmm_means) VEC(gmm_prec)
    VEC(gmm_precT) VEC(gmm_lognw) VEC(faces) VEC(vf_ptr) VEC(vf_idx)
    LDS(wT) LDS(J_t) LDS(J_S) LDS(vt_sub) LDS(sel_v) LDS(kp_start) LDS(kp_s) LDS(kp_w) LDS(vs_start) LDS(vs_k) LDS(vs_w)
    LDS(kpp_s) LDS(kpp_w) LDS(vsp_k) LDS(vsp_w) LDS(padded) LDS(kp_joint) LDS(parents) LDS(nlevels) LDS(level_start)
    LDS(level_joints) LDS(child_start) LDS(child_list) LDS(n_fwd) LDS(n_bwd) LDS(fwd_tab) LDS(bwd_tab) LDS(anc_tab)
    LDS(n_jump) LDS(n_skel) LDS(ns) LDS(nc) LDS(nc_pad) LDS(selw) LDS(selj) LDS(sel_sparse)
#undef VEC
#undef VAL
#undef LDS
    if (!found) return -1;
    if (dst && r.second) memcpy(dst, r.first, r.second);
    return (long)r.second;
}
