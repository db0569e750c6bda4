// Host interface of the optimiser kernels (fit_kernels.hip): the structs they take by value, their dynamic LDS sizes and one
// launcher per kernel.  A launcher is the kernel launch and nothing else: the caller reads hipGetLastError where it wants the
// error consumed.
#pragma once
#include <hip/hip_runtime.h>

#include "closure_device.h"
#include "fit_plan.h"
namespace mvfit {

struct StageWeights { DevWeights w[MVFIT_MAX_STAGES]; };

// per-problem optimiser storage in HBM
struct FitBuffers {
    OptBlock* opt;       // [B] trial point + L-BFGS scalars / working vectors / ro (LDS image block)
    PoseBlock* pose;     // [B] pose state of the current trial point (handed from launch to launch)
    float* dirs;         // [B][100][LB_D]
    float* stps;         // [B][100][LB_D]
    float* grow;         // [B][LB_GSIZE] pre-scaled Gram matrices (lbfgs_device.h:LbHist)
    float* gcol;         // [B][LB_GSIZE]
    float* rinv;         // [B][LB_RPACK] packed R^-1 of the compact direction form: the single-launch fit keeps it in LDS and parks
                         // it here only when a launch ends at its round cap
    double* stage_final; // [B][MVFIT_MAX_STAGES] run_fitting's return value per stage
    int* n_done;         // [3]: problems finished | problems of the current sub-batch that left the asynchronous phase (finished or
                         // paused at a stage boundary) | the same, all sub-batches of the fit
    VpBlock* vp;             // [B] VPoser decoder state of the current trial point (handed from launch to launch)
    const SdfAdj* sdf_adj;   // SDF term per problem (null: term not configured)
    int* sdf_gate;           // [B] 1 while the problem's current stage has coll_loss_weight > 0 and it is not done
    unsigned* sdf_tag;       // [B] service rounds of the single-launch fit: answer tag (round + 1) written behind the SdfAdj
    float* trace;            // [B][trace_cap][DV + 1] (x_trial, loss) of the first closures of a fit (mvfit_fit_trace); may be null
    int trace_cap;
};

// dynamic LDS of prep / closure / fit_init, of fit_step (+ the staged Gram window) and of the single-launch kernel
size_t step_lds();
size_t step_gram_lds();
size_t persistent_lds(bool vp);

// hipFuncAttributeMaxDynamicSharedMemorySize of every kernel above that takes dynamic LDS, every PersistentVariant included
hipError_t fit_kernels_configure();

// grid (B: one workgroup per problem) and stream, then the kernel's arguments in its own order
void launch_pack_obs(int B, hipStream_t stream, const DevProblems& Q, ObsBlock* obs);
void launch_pack_joints3d(int B, hipStream_t stream, const float* gt3d, const float* conf3d, ObsBlock* obs);
void launch_prep(int B, hipStream_t stream, const DevModel& M, const ObsBlock* obs, const DevPose& P, const float* params,
                 uint32_t flags, float* full_pose);
void launch_closure(bool remote, int grid, hipStream_t stream, const DevModel& M, const ObsBlock* obs, int nviews, const DevWeights& W,
                    const DevPose& P, const float* params, int from_pass, float* loss, float* grad, float* joints,
                    const SdfAdj* sdf_adj);
void launch_joints(int B, hipStream_t stream, const DevModel& M, const float* verts, const float* Amat, const float* params,
                   float* joints);
void launch_fit_init(int B, hipStream_t stream, const DevModel& M, const ObsBlock* obs, const DevPose& P, const FitBuffers& F,
                     const float* params, uint32_t flags, int publish);
void launch_fit_step(bool reuse, int B, hipStream_t stream, const DevModel& M, const ObsBlock* obs, int nviews, const StageWeights& SW,
                     const LbOpts& O, const DevPose& P, const FitBuffers& F);
void launch_fit_persistent(PersistentVariant variant, int grid, hipStream_t stream, const DevModel& M, const ObsBlock* obs, int nviews,
                           const StageWeights& SW, const LbOpts& O, const DevPose& P, const FitBuffers& F, int max_rounds,
                           const AsyncRing& ring, int b_lo, int done_target, int pause_stage, int* queue, int b_end);
void launch_fit_finish(int B, hipStream_t stream, const FitBuffers& F, float* params, float* final_loss, int32_t* n_closure,
                       int32_t* n_iter, int num_stages);
void launch_lbfgs_kat(int kind, int D, const LbOpts& O, double* x_io, double* trace, int max_trace, int* n_closure,
                      double* final_loss, double* dirs, double* stps, double* ro, double* grow, double* gcol, double* cmat);

}  // namespace mvfit
