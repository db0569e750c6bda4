// Host interface of the term mix (term_mix.hip) as mvfit_api.hip and mvfit_scene.hip drive it: the weighted sum of the scene,
// silhouette, vertex-target and scan terms behind coll_loss_weight (include/mvfit.h: mvfit_set_term_mix).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace mvfit {

struct SdfAdj;

// state of mvfit_set_term_mix and views of mvfit_ctx::mix_mem.  The buffers are allocated by the first enable for the batch
// and keep their addresses while B stays: a re-freeze of obstacles or targets leaves the captured round graph valid.
struct TermMix {
    bool on = false;
    float scene = 0.f, silhouette = 0.f, vertex_targets = 0.f, scan = 0.f;     // the shares
    float w_in = 1.f, w_out = 1.f, sigma = 0.f;                      // the silhouette term's scalars
    float scan_w_s2m = 0.f, scan_w_m2s = 0.f, scan_sigma = 0.f;      // the scan term's scalars (scan > 0)
    float* g_verts = nullptr;           // [B][nv][3] the mixed vertex cotangent
    float* loss = nullptr;              // [B] L_v, the mixed loss of the vertex terms
    float* part = nullptr;              // slice partials of the pull-back (vjp_part_bytes)
    SdfAdj* rec_scene = nullptr;        // [B] the scene term's record, when its share is > 0
    SdfAdj* rec_verts = nullptr;        // [B] the pull-back's record, when the scene share is > 0
    float* parts = nullptr;             // [B][4] S_sc^2, L_sil, L_vt, L_scan of the last evaluation, unweighted
    float* sums = nullptr;              // [B] their weighted sum
};

// workgroups a problem's 3 nv floats are split over (the second grid dimension is the problem)
int term_mix_blocks(int nv);

// The mixed cotangent g[B][nv][3] and loss L_v[B] of the vertex terms - silhouette, vertex targets, scan, in this order (the
// arithmetic: include/mvfit.h).  A component with share 0 is skipped: its pointers are never read.  parts / sums ([B][4] /
// [B]), unless null, get (0, L_sil, L_vt, L_scan) and the weighted sum: the caller passes them when no record merge follows.
// gate[b] == 0 skips problem b (its rows keep what they held), a null gate keeps every problem.  One kernel node, no host
// work: capturable.
hipError_t launch_term_mix_cotangent(int nv, int B, float lam_sil, const float* g_sil, const float* L_sil, float lam_vt,
                                     const float* g_vt, const float* L_vt, float lam_scan, const float* g_scan,
                                     const float* L_scan, const int* gate, float* g, float* L_v, float* parts, float* sums,
                                     hipStream_t stream);

// rec[b] = the record of lam_sc S_sc^2 + S_v^2 from the scene term's record and the pull-back's, and parts / sums of the
// evaluation unless parts is null (L_sil / L_vt / L_scan: the loss buffers of the live vertex terms, null for a share of 0).
// One kernel node: capturable.
hipError_t launch_term_mix_record(int B, float lam_sc, const SdfAdj* rec_scene, const SdfAdj* rec_verts, float lam_sil,
                                  const float* L_sil, float lam_vt, const float* L_vt, float lam_scan, const float* L_scan,
                                  const int* gate, SdfAdj* rec, float* parts, float* sums, hipStream_t stream);

}  // namespace mvfit
