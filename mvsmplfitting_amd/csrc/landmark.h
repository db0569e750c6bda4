// Host interface of the surface landmark term (landmark.hip) as mvfit_landmark.hip and mvfit_api.hip drive it: the landmark
// table a ctx keeps (mvfit_set_landmarks), the targets of the current batch (mvfit_set_landmark_targets) and the buffers of
// the term inside the fit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace mvfit {

constexpr int LM_MAX = 256;             // landmarks of a table (include/mvfit.h: MVFIT_LANDMARKS_MAX)
constexpr int LM_NNZ = 4;               // vertices per landmark (MVFIT_LANDMARK_NNZ)
constexpr int LM_MAX_VIEWS = 16;        // MVFIT_MAX_VIEWS

// The table is ONE device buffer of 4-byte words, its layout a function of (L, nt, nnz):
//   vid [L][4] int32 | w [L][4] float | tv [nt] int32 | tptr [nt + 1] int32 | tent [nnz] int32
// tv: the vertices that a slot of non-zero weight names, ascending; tptr / tent: the CSR of their entries, entry = 4 l + k
// in ascending order.  The targets are ONE buffer too:  xy [B][V][L][2] | conf [B][V][L] | xyz [B][L][3] | conf3 [B][L]
// (the last two only with has3d).
inline size_t lm_table_words(int L, int nt, int nnz) { return (size_t)L * 8 + nt + (nt + 1) + nnz; }
inline size_t lm_target_words(int B, int V, int L, bool has3d) { return (size_t)B * V * L * 3 + (has3d ? (size_t)B * L * 4 : 0); }

// views of mvfit_ctx::lmtab_mem (the table: its own lifetime), lmtgt_mem (the targets: re-made when (B, V, L, has3d) change)
// and lmterm_mem (the term's round buffers: kept while B stays)
struct LmState {
    bool table = false;                 // a table is present
    bool on = false;                    // targets are present
    bool term = false;                  // mvfit_set_landmark_term: the term of closure and fit
    int L = 0, nt = 0, nnz = 0;
    void* tab = nullptr;
    int tgt_L = 0;                      // the L the target buffer was made for
    bool has3d = false;
    float* tgt = nullptr;
    float rho = 100.f, w3d = 0.f, rho3d = 0.f;
    float* g_verts = nullptr;           // [B][nv][3] the round's vertex cotangent
    float* loss = nullptr;              // [B] L_j of the last evaluation inside closure / fit
    float* part = nullptr;              // slice partials of the pull-back (vjp_part_bytes)
};

// the cameras of mvfit_set_problems ([., V, 9], [., V, 3], [., V], [., V, 2]; batched: one rig per problem)
struct LmCams {
    int V, batched;
    const float *R, *t, *f, *c;
};

// loss[B] and, unless g_verts is null, g_verts[B][nv][3] of the contract in include/mvfit.h; gate[b] == 0 skips problem b
// (its rows keep what they held), a null gate keeps every problem.  One kernel node, no host work: capturable.
hipError_t launch_landmarks(const float* verts, int nv, int B, const void* tab, int L, int nt, const float* tgt, bool has3d,
                            const LmCams& cams, float rho, float w3d, float rho3d, const int* gate, float* loss, float* g_verts,
                            hipStream_t stream);

}  // namespace mvfit
