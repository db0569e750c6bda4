// Host interface of the vertex-target term (vertex_target.hip) as mvfit_scene.hip and mvfit_api.hip drive it: the target set
// a ctx keeps between mvfit_set_vertex_targets and the loss calls, and the buffers of the term inside the fit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace mvfit {

constexpr int VT_MAX_K = 4;             // target sets per problem (include/mvfit.h: MVFIT_VERTEX_TARGETS_MAX)

// views of mvfit_ctx::vtgt_mem (the set) and mvfit_ctx::vtterm_mem (the term's round buffers).  The set's buffers keep their
// addresses while (B, K) stay, the term's while B stays: a re-freeze leaves the captured round graph valid.
struct VtxTargets {
    bool on = false;                    // a target set is present
    bool term = false;                  // mvfit_set_vertex_target_term: the term of closure and fit
    int K = 0;
    float* targets = nullptr;           // [B][K][nv][3]
    float* weights = nullptr;           // [B][K] (device: read by the kernel, not baked into its node)
    double* partial = nullptr;          // [B][vertex_target_blocks(nv)] the workgroups' float64 sums of one evaluation
    float* g_verts = nullptr;           // [B][nv][3] the round's vertex cotangent
    float* loss = nullptr;              // [B] L_j of the last evaluation inside closure / fit
    float* part = nullptr;              // slice partials of the pull-back (vjp_part_bytes)
};

// workgroups a problem's 3 nv floats are split over (the second grid dimension is the problem)
int vertex_target_blocks(int nv);

// loss[B] and, unless g_verts is null, g_verts[B][nv][3] of the contract in include/mvfit.h; gate[b] == 0 skips problem b
// (its rows keep what they held), a null gate keeps every problem.  Two kernel nodes, no host work: capturable.
hipError_t launch_vertex_target(const float* verts, int nv, int B, int K, const float* targets, const float* weights,
                                const int* gate, double* partial, float* loss, float* g_verts, hipStream_t stream);

}  // namespace mvfit
