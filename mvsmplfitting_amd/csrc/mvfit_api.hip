// libmvfit: C ABI (include/mvfit.h) + the per-problem step kernels.
//
// Kernels in this file (one workgroup per problem, see closure_device.h / lbfgs_device.h):
//   prep_kernel        params -> pose operands of the vertex pass
//   closure_kernel     one closure evaluation (loss, grad, keypoints) - the drop-in closure
//   fit_step_kernel    one closure round of the device-resident fit: objective + adjoint from the
//                      vertex-pass output, L-BFGS state-machine advance, pose operands of the next
//                      trial point
//   fit_persistent_kernel  the whole fit of one problem in a single launch: closures restricted to the vertices
//                      the objective reads, or full closures whose vertex passes run beside it (asynchronous fit:
//                      AsyncRing); optionally VPoser decoder helpers behind the problems' workgroups
//   lbfgs_kat_kernel   float64 instantiation of the state machine on analytic objectives
// Host side: the C ABI; the model's tables are built by model_prep.cpp and uploaded by mvfit_create_ex; how a fit runs is
// decided by fit_plan.cpp and executed by mvfit_fit; every allocation of a ctx has an owner of dev_mem.h, which does all the freeing.
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "closure_device.h"
#include "fit_plan.h"
#include "dev_mem.h"
#include "model_prep.h"
#include "silhouette.h"

namespace mvfit {

hipError_t launch_vertex_pass(const DevModel& M, const DevPose& P, int B, float* verts, int ksplit,
                              hipStream_t stream, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
hipError_t vertex_pass_configure();
hipError_t launch_pass_gate(const DevPose& P, int b_lo, int B, hipStream_t stream);
hipError_t launch_vertex_pass_resident(const DevModel& M, const ResidentArgs& RA, int tpw, hipStream_t stream);
hipError_t launch_sdf_term(const DevModel& M, const DevPose& P, const float* verts, int B, const int32_t* faces, int num_faces,
                           int G, const int* gate, SdfBox* box, float4* samp, void* entries, SdfAdj* adj, hipStream_t stream,
                           void* cull, unsigned* answer_tag = nullptr, unsigned answer = 0u, const unsigned long long* box_parts = nullptr);
size_t sdf_cull_bytes(int B, int num_faces);
size_t sdf_op_ws_bytes(int B, int num_faces);
bool sdf_op_uses_lists(int num_faces);
hipError_t launch_sdf_voxelize_culled(const int32_t* faces, int num_faces, const float* vertices, int B, int num_vertices, int G,
                                      float* phi, void* ws, hipStream_t stream);
size_t sdf_cull_zero_offset(int B, int num_faces);
size_t sdf_cull_zero_bytes(int B);
int sdf_cull_min_faces();
size_t sdf_work_bytes(int B, int nv);
size_t sdf_ticket_offset(int B, int nv);
hipError_t launch_triangulate(const float* kps, const double* intris, const double* extris, int B, int V, int J, double* out,
                              hipStream_t stream);
hipError_t launch_depth_guess(const double* rest, const double* extri, const double* intri, const float* kps, int B, int J,
                              double* out, hipStream_t stream);
hipError_t launch_umeyama(const double* src, const double* dst, int B, int npts, int estimate_scale, double* rot, double* rvec,
                          double* trans, double* scale, hipStream_t stream);
hipError_t launch_project_points(const DevProblems& Q, const float* pts, int N, float* uv, hipStream_t stream);
hipError_t launch_sdf_voxelize(const int32_t* faces, int num_faces, const float* vertices, int B, int num_vertices, int G,
                               float* phi, hipStream_t stream);
size_t render_ws_bytes(int G, int Nv, int Nf, int H, int W);
hipError_t launch_render_normals(const float* verts, int B, int Nv, const int32_t* faces, const int32_t* vf_ptr,
                                 const int32_t* vf_idx, double* nrm, hipStream_t stream);
hipError_t vertex_backward_configure();
hipError_t launch_vertices_backward(const DevModel& M, const DevPose& P, int B, int Bpad, const float* params, uint32_t flags,
                                    const float* g_verts, const float* g_joints, float* part, SdfAdj* rec, float* g_params,
                                    hipStream_t stream);
size_t vjp_part_bytes(int Bpad, int nv);
hipError_t launch_render_group(const DevProblems& Q, const int* prob, const int* view, int n, const float* verts,
                               const double* nrm, int Nv, const int32_t* faces, int Nf, const float* points, int num_points,
                               int H, int W, const uint8_t* in, uint8_t* out, int32_t* face_id, void* ws_mem,
                               hipStream_t stream);
size_t scene_ws_bytes(int n, int m, int Nv, int Nf, int H, int W);
size_t assoc_frame_bytes(int D);
size_t assoc_head_bytes();
hipError_t launch_associate_group(const float* kps, const int32_t* count, const double* intris, const double* extris, int f0,
                                  int nf, int V, int Nmax, double max_cost, int min_joints, int min_views, void* ws,
                                  double* cost_out, int32_t* labels, int32_t* num_clusters, hipStream_t stream);
int scene_sdf_blocks(int nv);
hipError_t launch_scene_boxes(const float* verts, int nv, int b0, int n, float factor, float4* box, float* local,
                              hipStream_t stream);
hipError_t launch_scene_pairs(const float* verts, int nv, int b0, int n, int s0, int ns, const void* tab, const int32_t* first,
                              const float4* box, const float* phi, int G, float rob, float* g_verts, float* part, float* loss,
                              hipStream_t stream);
hipError_t launch_scene_null_boxes(SdfBox* box, int B, hipStream_t stream);
hipError_t launch_scene_term(const DevModel& M, const DevPose& P, const float* verts, int B, const void* tab, const float4* box,
                             const float* phi, int G, float rob, const int* gate, const SdfBox* null_box, void* entries,
                             SdfAdj* adj, hipStream_t stream);
hipError_t launch_scene_group(const DevProblems& Q, const int32_t* tab, int num_images, int i0, int n, int j0, int m,
                              const float* verts, const double* nrm, int Nv, const int32_t* faces, int Nf, const float* points,
                              int num_points, int H, int W, const uint8_t* in, uint8_t* out, int32_t* face_id, int32_t* body_id,
                              void* ws_mem, hipStream_t stream);

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

// compact optimiser index (reference final_params order, non_linear_solver.py:164-170) -> flat x slot
__device__ __forceinline__ int cmap(int i, bool use_vp) {
    if (!use_vp) return i;                         // betas go body_pose transl scale = x[0:86]
    return i < 13 ? i : (i < 17 ? X_TR + (i - 13) : X_EMB + (i - 17));   // betas go transl scale embedding
}
__device__ __forceinline__ int dact(bool use_vp) { return use_vp ? 49 : 86; }

// pose operands of the vertex pass only: E1 + chain
template <bool CALL = false>
__device__ __forceinline__ void pose_and_chain(const DevModel& M, ClosureLds& L, uint32_t flags, int tid) {
    pose_prep<CALL>(M, L, flags, tid);
    chain_forward_block(L, tid);
}

__device__ __forceinline__ void store_block16(void* dst_g, const void* src_l, int nbytes, int tid) {
    const int n = nbytes / 16;
    for (int i = tid; i < n; i += STEP_NT) reinterpret_cast<float4*>(dst_g)[i] = reinterpret_cast<const float4*>(src_l)[i];
}

// per-problem observations -> ObsBlock image (one launch per mvfit_set_problems)
__global__ void pack_obs_kernel(DevProblems Q, ObsBlock* __restrict__ obs) {
    const int b = blockIdx.x, V = Q.V;
    const size_t cb = Q.cam_batched ? (size_t)b * V : 0;
    ObsBlock& O = obs[b];
    for (int i = threadIdx.x; i < (int)(sizeof(ObsBlock) / 4); i += blockDim.x) reinterpret_cast<float*>(&O)[i] = 0.f;
    __syncthreads();
    for (int i = threadIdx.x; i < V * 9; i += blockDim.x) (&O.camR[0][0])[i] = Q.cam_R[cb * 9 + i];
    for (int i = threadIdx.x; i < V * 3; i += blockDim.x) (&O.camt[0][0])[i] = Q.cam_t[cb * 3 + i];
    for (int i = threadIdx.x; i < V; i += blockDim.x) O.camf[i] = Q.cam_f[cb + i];
    for (int i = threadIdx.x; i < V * 2; i += blockDim.x) (&O.camc[0][0])[i] = Q.cam_c[cb * 2 + i];
    for (int i = threadIdx.x; i < V * NKP * 2; i += blockDim.x) O.gt[i] = Q.gt_xy[(size_t)b * V * NKP * 2 + i];
    for (int i = threadIdx.x; i < V * NKP; i += blockDim.x) O.wc[i] = Q.w_conf[(size_t)b * V * NKP + i];
}

__global__ void pack_joints3d_kernel(const float* __restrict__ gt3d, const float* __restrict__ conf3d,
                                     ObsBlock* __restrict__ obs) {
    const int b = blockIdx.x;
    for (int i = threadIdx.x; i < NKP * 3; i += blockDim.x) obs[b].gt3d[i] = gt3d[(size_t)b * NKP * 3 + i];
    for (int i = threadIdx.x; i < NKP; i += blockDim.x) obs[b].c3d[i] = conf3d[(size_t)b * NKP + i];
}

__global__ __launch_bounds__(STEP_NT) void prep_kernel(DevModel M, const ObsBlock* __restrict__ obs, DevPose P,
                                                       const float* __restrict__ params, uint32_t flags,
                                                       float* __restrict__ full_pose = nullptr) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    ClosureLds& L = *reinterpret_cast<ClosureLds*>(smem_raw);
    const int b = blockIdx.x, tid = threadIdx.x;
    prologue(L, M, obs + b, nullptr, nullptr, nullptr, nullptr, params + (size_t)b * DV, tid);
    __syncthreads();
    pose_and_chain(M, L, flags, tid);
    publish_pose(L, P, b, tid);
    // ModelOutput.full_pose (body_models_scale.py:392-412): global_orient | body_pose, the latter decoded from the
    // embedding with MVFIT_F_VPOSER (fitting.py:170-173)
    if (full_pose && tid < 72) full_pose[(size_t)b * 72 + tid] = L.pose.theta[tid];
}

// REMOTE (test route, MVFIT_CLOSURE_VP_HELPERS=1): the launch carries VPoser decoder helpers behind the problems'
// workgroups and the closure decodes through them - the decoder arithmetic of the production single-launch fit
// (vposer_service.h) under the closure-level goldens; the pose operands of the trial point are published for the
// vertex pass that follows (like the asynchronous fit: objective from its own vertices, full pass beside it).
template <bool REMOTE>
__global__ __launch_bounds__(STEP_NT) void closure_kernel(DevModel M, const ObsBlock* __restrict__ obs, int nviews,
                                                          DevWeights W, DevPose P, const float* __restrict__ params,
                                                          int from_pass, float* __restrict__ loss,
                                                          float* __restrict__ grad, float* __restrict__ joints,
                                                          const SdfAdj* __restrict__ sdf_adj) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    if (REMOTE && (int)blockIdx.x >= M.vps.nprob) {
        vposer_helper(M.vpt, M.vps, smem_raw, (int)blockIdx.x % M.vps.nsets, ((int)blockIdx.x - M.vps.nprob) / M.vps.nsets);
        return;
    }
    ClosureLds& L = *reinterpret_cast<ClosureLds*>(smem_raw);
    const int b = blockIdx.x, tid = threadIdx.x;
    prologue(L, M, obs + b, nullptr, nullptr, from_pass ? P.vposed_sel + (size_t)b * NC_MAX : nullptr,
             from_pass ? P.xs_sel + (size_t)b * NC_MAX : nullptr, params + (size_t)b * DV, tid, sdf_adj ? sdf_adj + b : nullptr);
    __syncthreads();
    if constexpr (REMOTE) {
        pose_prep_decode_inl<true>(M, L, W.flags, tid);
        pose_prep_elems(M, L, W.flags, tid);
    } else {
        pose_prep(M, L, W.flags, tid);
    }
    sparse_forward(M, L, from_pass != 0, tid);
    if constexpr (REMOTE) publish_pose(L, P, b, tid);
    const bool want_grad = grad != nullptr;
    const double total = loss_and_keypoint_grad(M, L, nviews, W, want_grad, tid);
    if (tid == 0 && loss) loss[b] = (float)total;
    if (joints && tid < NKP * 3) joints[(size_t)b * NKP * 3 + tid] = (&L.kp[0][0])[tid];
    if (want_grad) {
        closure_backward<REMOTE>(M, L, nviews, W, tid);
        if (tid < DV) grad[(size_t)b * DV + tid] = L.grad[tid];
    }
    if constexpr (REMOTE) {
        __syncthreads();
        if (tid == 0 && L.vp_remote) vps_store(vps_request_slot(M.vps), 0.f, (L.vp_seq + 1u) << 2 | VPS_BYE);
    }
}

// keypoints only (mvfit_vertices): gather from the vertex buffer; a skeleton keypoint (model without a regressor) from the
// skinning transforms prep_kernel wrote: G_t = A_t + G_r J (A_j = [G_r | G_t - G_r J], lbs.py:365-368), J = J_t + J_S beta
// formed as pose_prep_elems forms it, + transl
__global__ __launch_bounds__(64) void joints_kernel(DevModel M, const float* __restrict__ verts, const float* __restrict__ Amat,
                                                    const float* __restrict__ params, float* __restrict__ joints) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const ModelLds& C = *M.mlds;
    if (tid < NKP * 3) {
        const int k = tid / 3, a = tid - 3 * k;
        float s = 0.f;
        const int j = kp_joint_of(C, k);
        if (j >= 0) {
            const float* x = params + (size_t)b * DV;
            const float* A = Amat + (size_t)b * 288 + j * 12 + 4 * a;
            float J[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float v = C.J_t[3 * j + c];
#pragma unroll
                for (int l = 0; l < 10; ++l) v = fmaf(C.J_S[3 * j + c][l], x[X_BETAS + l], v);
                J[c] = v;
            }
            s = A[3] + (A[0] * J[0] + A[1] * J[1] + A[2] * J[2]) + x[X_TR + a];
        } else {
            for (int t = C.kp_start[k]; t < C.kp_start[k + 1]; ++t)
                s = fmaf(C.kp_w[t], verts[((size_t)b * M.nv + C.sel_v[C.kp_s[t]]) * 3 + a], s);
        }
        joints[(size_t)b * NKP * 3 + tid] = s;      // rows of the selection sum to 1 (+transl already in verts)
    }
}

__device__ __forceinline__ void opts_in(ClosureLds& L, const StageWeights& SW, const LbOpts& O, int tid) {
    constexpr int nsw = sizeof(StageWeights) / 4, nop = sizeof(LbOpts) / 4;
    if (tid < nsw) reinterpret_cast<int*>(&L.sw[0])[tid] = reinterpret_cast<const int*>(&SW)[tid];
    if (tid >= 128 && tid < 128 + nop) reinterpret_cast<int*>(&L.opts)[tid - 128] = reinterpret_cast<const int*>(&O)[tid - 128];
}

// initialise the optimiser state of every problem: x = params, first trial point = x
__global__ __launch_bounds__(STEP_NT) void fit_init_kernel(DevModel M, const ObsBlock* __restrict__ obs, DevPose P,
                                                           FitBuffers F, const float* __restrict__ params,
                                                           uint32_t flags, int publish) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    ClosureLds& L = *reinterpret_cast<ClosureLds*>(smem_raw);
    const int b = blockIdx.x, tid = threadIdx.x;
    const bool use_vp = (flags & MVFIT_F_VPOSER) != 0;
    const float xv = (tid < DV) ? params[(size_t)b * DV + tid] : 0.f;
    const float xc = (tid < dact(use_vp)) ? params[(size_t)b * DV + cmap(tid, use_vp)] : 0.f;
    prologue(L, M, obs + b, nullptr, nullptr, nullptr, nullptr, nullptr, tid);
    for (int i = tid; i < (int)(sizeof(OptBlock) / 4); i += STEP_NT) reinterpret_cast<float*>(&L.opt)[i] = 0.f;
    __syncthreads();
    if (tid < DPAD) L.opt.x[tid] = xv;
    if (tid < LB_D) L.opt.lbV[tid / LB_EPL].x[tid % LB_EPL] = xc;
    if (tid == 0) { L.opt.lbS.phase = PH_STEP_START; L.opt.lbS.H = 1.0; }
    if (tid < MVFIT_MAX_STAGES) F.stage_final[(size_t)b * MVFIT_MAX_STAGES + tid] = (double)NAN;
    __syncthreads();
    store_block16(F.opt + b, &L.opt, sizeof(OptBlock), tid);
    if (publish) {
        pose_and_chain(M, L, flags, tid);
        publish_pose(L, P, b, tid);
        store_block16(F.pose + b, &L.pose, sizeof(PoseBlock), tid);
        if (flags & MVFIT_F_VPOSER) store_block16(F.vp + b, L.vp_pre1, sizeof(VpBlock), tid);
    }
}

// shared by the two fit kernels: evaluate the closure at L.opt.x, advance the optimiser, leave the
// next trial point in L.opt.x.  Returns true when the problem is finished.
// REMOTE: the launch may carry VPoser decoder helpers (fit_persistent_kernel only); REUSE: MVFIT_F_REUSE_OUTER_VALUE;
// LEAN: the stage flags carry none of VPoser / GMM / 3-D term (the host checks) - said to the compiler as a fact about
// the flag word, which lets it drop those branches from the round: 13 KB less code to stream through the instruction
// cache every round (86 -> 73 KB), 1.2-1.6 % per fit (speed only: the result does not depend on it)
// SDFS: the launch serves stages with the SDF term by asking for it (closure_device.h: publish_sdf_request, loss_combine<true>);
// sv = {pass operands of the chained layout (coefT), gate words, answer tags, global problem index, round offset of the launch}
// SDFT = false: no SdfAdj ever reaches the kernel's prologue (fit_persistent_kernel without SDFS): the adjoint is compiled without
// the term's branches (the chained step kernel gets the term through its prologue and keeps them)
struct SdfService { const DevPose* P; int* gate; const unsigned* tag; int b; int round0; };
template <bool REMOTE = false, bool REUSE = false, bool LEAN = false, bool COMPACT = false, bool SDFS = false, bool ROFF = SDFS,
          bool SDFT = true>
__device__ __forceinline__ bool fit_round(const DevModel& M, ClosureLds& L, int nviews, const LbHist<float>& H,
                          bool from_pass, bool have_pose, double* stage_final, int tid,
                          LbGramLds GL = LbGramLds{nullptr, 0, 0}, float* trace = nullptr, int trace_cap = 0,
                          const AsyncRing& ring = AsyncRing{}, bool use_ring = false, int pb = 0,
                          const SdfService& sv = SdfService{nullptr, nullptr, nullptr, 0, 0}) {
    DevWeights W = L.sw[L.sh_stage];
    W.flags = __builtin_amdgcn_readfirstlane(W.flags);
    if constexpr (LEAN) {
        W.flags &= ~(uint32_t)(MVFIT_F_VPOSER | MVFIT_F_PRIOR_GMM | MVFIT_F_USE_3D);
        __builtin_assume((W.flags & (MVFIT_F_VPOSER | MVFIT_F_PRIOR_GMM | MVFIT_F_USE_3D)) == 0);
    }
    const LbOpts& O = L.opts;
    const bool use_vp = (W.flags & MVFIT_F_VPOSER) != 0;
    PH_T0();
    // have_pose: the previous launch left the pose block of this x (and, with VPoser, the decoder state the
    // adjoint needs - the VpBlock)
    if (!have_pose) {
        pose_prep_decode_inl<REMOTE>(M, L, W.flags, tid);
        pose_prep_elems(M, L, W.flags, tid);
    }
    PH_T(0);
    sparse_forward(M, L, from_pass, tid, !have_pose);
    PH_T(2);
    // asynchronous fit: the 6890-vertex pass of THIS trial point is already queued on the other CUs and waits for the
    // operands (coefficients, skinning transforms, translation: all complete here) in the ring slot of this round
    // closures consumed so far by this ring row = this round (sv.round0: the problem's closures before this launch, minus the
    // rounds the row spent on earlier problems of the launch - refill)
    const unsigned a_round = use_ring ? (unsigned)(L.opt.lbS.n_closure - (ROFF ? sv.round0 : 0)) : 0u;
    const int a_slot = use_ring ? (int)(a_round % (unsigned)ring.nslots) : 0;
    if (use_ring) publish_pose_async(L, ring, a_slot, a_round, pb, tid);
    bool sdf_round = false;
    if constexpr (SDFS) {
        // a stage that carries the interpenetration term: ask for S and its adjoint at this trial point (the tag goes out at
        // once: the round's passes and the term's kernels are queued behind it) and wait for the answer
        sdf_round = use_ring && L.sdf_adj != nullptr && W.coll_w > 0.f;           // block-uniform
        if (use_ring) publish_sdf_request(L, *sv.P, sv.gate, sv.b, sdf_round ? 1 : 0, tid);
        if (sdf_round) publish_tag(ring, a_slot, pb, a_round, tid);
        // the answer is waited for where S is first needed: by the wave that combines the loss's scalar terms, under E5
        // (closure_device.h: loss_combine<true>) - the keypoint phase overlaps the term's kernels.  Never a silently missing
        // term: a wait that times out makes the loss NaN and is counted (stats[3]: the host fails the fit)
        if (tid == 0) {
            L.sdf_wait_tag = sdf_round ? sv.tag + sv.b : nullptr;
            L.sdf_wait_want = a_round + 1u;
            L.sdf_wait_stats = ring.stats + 3;
        }
    }
    loss_and_keypoint_grad<true>(M, L, nviews, W, true, tid);          // (scalar terms combined under the adjoint's first phase)
    PH_T(3);
    closure_backward<REMOTE, true, SDFS, SDFT>(M, L, nviews, W, tid);
    const double total = L.total;
    if (trace) {                                           // (x_trial, loss) of this closure call (mvfit_fit_trace)
        const int k = L.opt.lbS.n_closure;                 // closures consumed so far = index of this one
        if (k < trace_cap) {
            if (tid < DV) trace[(size_t)k * (DV + 1) + tid] = L.opt.x[tid];
            if (tid == 0) trace[(size_t)k * (DV + 1) + DV] = (float)total;
        }
    }
    if (use_ring && !sdf_round) publish_tag(ring, a_slot, pb, a_round, tid);             // the stores have long drained by now
    PH_T(8);
    float gnew[LB_EPL], xt[LB_EPL];
    const int D = dact(use_vp);
    if (tid < 64) {
        PH_T(9);
#pragma unroll
        for (int e = 0; e < LB_EPL; ++e) {
            const int i = LB_EPL * tid + e;
            gnew[e] = i < D ? L.grad[cmap(i, use_vp)] : 0.f;
        }
    }
    // the optimiser state stays in LDS (L.opt.lbS, L.opt.lbV): lbfgs_round works on it in place
    // the reference reads the loss as a float32 tensor (float(closure()), lbfgs_ls.py:251,281)
    lbfgs_round<float, STEP_NT, REUSE>(&L.opt.lbS, &L.opt.lbV[0], H, L.lbW, O, (double)(float)total, gnew, xt, tid, stage_final, [&]() {
        PH_T(10);
        // the single-launch fit takes the direction in compact form (history and R^-1 in LDS, every phase on all waves);
        // the chained step kernel keeps the two-loop form over its Gram matrices in global memory
        if constexpr (COMPACT) lb_direction_compact<float, STEP_NT>(H, L.lbW, tid, lb_dir_general(O));
        else lb_direction_block<float, STEP_NT>(H, L.lbW, tid, GL);
        PH_T(11); PH_ADD(15, 1);
    });
    if (tid < 64) {
#pragma unroll
        for (int e = 0; e < LB_EPL; ++e) {
            const int i = LB_EPL * tid + e;
            if (i < D) L.opt.x[cmap(i, use_vp)] = xt[e];
        }
        if (tid == 0) { L.sh_stage = min(L.opt.lbS.stage, O.num_stages - 1); L.sh_status = L.opt.lbS.status; }
        PH_ADD(13, 1); PH_ADD(14, L.opt.lbS.hist_len);
    }
    __syncthreads();
    PH_T(12);
    return L.sh_status != 0;
}

// LDS layout of the single-launch fit behind the closure workspace: [s ring | y ring | packed R^-1].  Without VPoser the
// tail starts over the decoder's arrays (the last members of ClosureLds) and a row holds the 86 active parameters; with
// VPoser the active dimension is 49.
constexpr int kHistLdFull = 88, kHistLdVp = 52;
__host__ __device__ constexpr int persistent_hist_ld(bool vp) { return vp ? kHistLdVp : kHistLdFull; }
__host__ __device__ constexpr size_t persistent_tail_offset(bool vp) {
    return vp ? ((sizeof(ClosureLds) + 15) & ~(size_t)15) : offsetof(ClosureLds, vp_pre1);
}
__host__ __device__ constexpr size_t persistent_lds_bytes(bool vp) {
    return persistent_tail_offset(vp) + ((size_t)2 * LB_HIST * persistent_hist_ld(vp) + LB_RPACK) * sizeof(float);
}
static_assert(persistent_lds_bytes(false) <= 160 * 1024 && persistent_lds_bytes(true) <= 160 * 1024, "one workgroup per CU: 160 KB of LDS");

__device__ __forceinline__ size_t step_lds_dev() { return (sizeof(ClosureLds) + 15) & ~(size_t)15; }

// one closure round per launch (full mode): the objective reads the vertex pass's output for its
// vertices; afterwards the pose operands of the NEXT trial point are published for the next pass.
template <bool REUSE>
__global__ __launch_bounds__(STEP_NT) void fit_step_kernel(DevModel M, const ObsBlock* __restrict__ obs, int nviews,
                                                           StageWeights SW, LbOpts O, DevPose P, FitBuffers F) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    ClosureLds& L = *reinterpret_cast<ClosureLds*>(smem_raw);
    const int b = blockIdx.x, tid = threadIdx.x;
    PH_T0();
    prologue(L, M, obs + b, F.pose + b, F.opt + b, P.vposed_sel + (size_t)b * NC_MAX, P.xs_sel + (size_t)b * NC_MAX, nullptr, tid,
             F.sdf_adj ? F.sdf_adj + b : nullptr, (SW.w[0].flags & MVFIT_F_VPOSER) ? F.vp + b : nullptr);
    opts_in(L, SW, O, tid);
    __syncthreads();
    if (L.opt.lbS.status != 0) return;                    // uniform per block
    if (tid == 0) { L.sh_stage = L.opt.lbS.stage; L.sh_status = 0; }
    LbHist<float> H{F.dirs + (size_t)b * LB_HIST * LB_D, F.stps + (size_t)b * LB_HIST * LB_D, L.opt.lb_ro,
                    F.grow + (size_t)b * LB_GSIZE, F.gcol + (size_t)b * LB_GSIZE};
    __syncthreads();
    // Gram rows of the first recurrence -> LDS while the closure runs (the window covers the current head / length and
    // the one after an insertion); lb_direction_block waits for it
    // Touch every 128-byte line of the live history rows (s and y) once, now: after a launch boundary they are
    // ~2.5 k cycles away, and the direction's row dots and mat-vecs - 18 k cycles from here - would each start with
    // that round trip; afterwards they hit L2.  One load per thread, value never used (kept alive to the end so that
    // the register is not recycled under the load).
    float warm = 0.f;
    {
        const int n0 = L.opt.lbS.hist_len, head0 = L.opt.lbS.hist_head;
        constexpr int LPR = LB_D * 4 / 128;                      // 3 lines per row
        if (tid < 2 * LPR * n0) {
            const int which = tid / (LPR * n0), r = tid - which * LPR * n0, age = r / LPR, ln = r - age * LPR;
            int slot = head0 + age;
            slot = slot >= LB_HIST ? slot - LB_HIST : slot;
            warm = (which ? H.stps : H.dirs)[slot * LB_D + ln * 32];
        }
    }
    LbGramLds GL{reinterpret_cast<float*>(smem_raw + step_lds_dev()), L.opt.lbS.hist_head,
                 min(L.opt.lbS.hist_len + 1, LB_HIST) + 3 + 4 * LB_PD};
    lb_gram_dma<STEP_NT>(H.gcol, GL.row0, GL.buf, GL.nrows, tid);
    PH_T(24);
    const bool done = fit_round<false, REUSE>(M, L, nviews, H, true, true, F.stage_final + (size_t)b * MVFIT_MAX_STAGES, tid, GL,
                                F.trace ? F.trace + (size_t)b * F.trace_cap * (DV + 1) : nullptr, F.trace_cap);
    PH_T0();
    store_block16(F.opt + b, &L.opt, sizeof(OptBlock), tid);
    if (tid == 0 && done) atomicAdd(F.n_done, 1);
    if (tid == 0 && F.sdf_adj) F.sdf_gate[b] = (!done && L.sw[L.sh_stage].coll_w > 0.f) ? 1 : 0;
    // pose operands of the next trial point (also after the last round: final vertices)
    pose_and_chain(M, L, __builtin_amdgcn_readfirstlane(L.sw[L.sh_stage].flags), tid);
    publish_pose(L, P, b, tid);
    store_block16(F.pose + b, &L.pose, sizeof(PoseBlock), tid);
    if (SW.w[0].flags & MVFIT_F_VPOSER) store_block16(F.vp + b, L.vp_pre1, sizeof(VpBlock), tid);
    if (__builtin_expect(warm == 1.7014118e38f, 0)) atomicAdd(F.n_done, 0);       // sink of the warm-up loads
    PH_T(25);
}

// the whole fit of one problem in a single launch (objective-vertices-only closure): the L-BFGS
// history ring lives in LDS behind the closure workspace.
// REMOTE: the launch carries VPoser decoder helpers behind the problems' workgroups (vposer_service.h); launches without
// them run the instantiation that has no trace of the service.
// QUEUE: the launch has a work queue (more problems than ring rows): its own instantiations - the loop over a row's problems around
// the round loop costs the round loop registers (22 instead of 7 spilled, +12 % instructions), which launches without a queue do
// not pay
template <bool REMOTE, bool REUSE, bool LEAN, bool SDFS = false, bool QUEUE = false>
__global__ __launch_bounds__(STEP_NT) void fit_persistent_kernel(DevModel M, const ObsBlock* __restrict__ obs, int nviews,
                                                                 StageWeights SW, LbOpts O, DevPose P, FitBuffers F,
                                                                 int max_rounds, AsyncRing ring, int b_lo, int done_target,
                                                                 int pause_stage, int* queue, int b_end) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    if (REMOTE && (int)blockIdx.x >= M.vps.nprob) {
        // decoder helper of this launch (vposer_service.h): workgroups behind the problems' ones; set = blockIdx % nsets
        // like the problems it serves (dispatch is round-robin over the XCDs: same L2 when nsets == 8 - speed only)
        vposer_helper(M.vpt, M.vps, smem_raw, (int)blockIdx.x % M.vps.nsets, ((int)blockIdx.x - M.vps.nprob) / M.vps.nsets);
        return;
    }
    ClosureLds& L = *reinterpret_cast<ClosureLds*>(smem_raw);
    // behind (or, without VPoser, over the decoder's arrays at the end of) the closure workspace: the (s, y) ring, row
    // stride = the active dimension rounded up, and the packed R^-1 of the compact direction form
    const bool vp_mode = (SW.w[0].flags & MVFIT_F_VPOSER) != 0;                        // (flags are the same in all stages)
    const int ldh = LEAN ? kHistLdFull : persistent_hist_ld(vp_mode);
    float* hist = reinterpret_cast<float*>(smem_raw + (LEAN ? persistent_tail_offset(false) : persistent_tail_offset(vp_mode)));   // [2][100][ldh]
    float* rinv = hist + 2 * LB_HIST * ldh;                                              // [LB_RPACK]
    const int tid_k = threadIdx.x;
    const int row = b_lo + (int)blockIdx.x;                        // this workgroup's ring row / done_round word
    int b = row;                                                   // problems [b_lo, b_lo + nprob): one sub-batch of mvfit_fit ...
    // ... and, with a work queue (round 6: `queue` counts the problems handed out, b_end = one past the last), whatever problem
    // the workgroup takes when its own has finished: more problems than optimiser workgroups overlap in ONE launch instead of
    // running as sub-batches one after the other, and a workgroup whose problem converged early does not idle through the
    // tail of the slowest.  The ring row keeps counting closure rounds across its problems (rounds_before); the passes write a
    // round's vertices to the problem the row held in that round (its index travels in the translation word's spare lane).
    int rounds_before = 0, slot_rounds = 0;
  for (;;) {
    // (opaque per problem: nothing derived from the thread index is invariant across this loop - hoisted into its preheader, the
    // prologue's and epilogue's addresses would be live through every round loop: 179 spilled registers, 1.55 -> 1.42 M closures/s)
    int tid = tid_k;
    if constexpr (QUEUE) asm volatile("" : "+v"(tid));
    prologue(L, M, obs + b, nullptr, F.opt + b, nullptr, nullptr, nullptr, tid, SDFS && F.sdf_adj ? F.sdf_adj + b : nullptr);
    opts_in(L, SW, O, tid);
    __syncthreads();
    // closure rounds of THIS launch count from 0 (ring slots, tags, done_round): a service launch continues fits whose problems
    // have spent different numbers of closures in the stages before it
    const int round0 = (SDFS || QUEUE) ? L.opt.lbS.n_closure - rounds_before : 0;
    if (L.opt.lbS.status != 0) {
        if (REMOTE && tid == 0 && L.vp_remote) vps_store(vps_request_slot(M.vps), 0.f, 1u << 2 | VPS_BYE);
        if (tid == 0 && ring.tag) {         // finished in an earlier launch: no pass waits for this problem
            __hip_atomic_store(ring.done_round + row, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (SDFS) {                     // (the host counts the problems that left this launch)
                __hip_atomic_store(F.sdf_gate + b, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const int left = atomicAdd(F.n_done + 1, 1) + 1;
                atomicAdd(F.n_done + 2, 1);
                if (left == done_target) __hip_atomic_store(ring.host_done, left, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
        return;
    }
    if (tid == 0) { L.sh_stage = L.opt.lbS.stage; L.sh_status = 0; L.sh_sdf_ok = 1u; L.sh_prob = b; }
    if (tid == 64 * PUBLISH_WAVE) L.sh_pass_done = 0u;
    float* gd = F.dirs + (size_t)b * LB_HIST * LB_D;
    float* gs = F.stps + (size_t)b * LB_HIST * LB_D;
    float* gr = F.rinv + (size_t)b * LB_RPACK;
    const bool resume = L.opt.lbS.n_closure > 0;          // relaunch after a round cap: restore the ring
    if (resume) {
        for (int i = tid; i < LB_HIST * ldh; i += STEP_NT) {
            const int r = i / ldh, e = i - r * ldh;
            hist[i] = gd[r * LB_D + e]; hist[LB_HIST * ldh + i] = gs[r * LB_D + e];
        }
        for (int i = tid; i < LB_RPACK; i += STEP_NT) rinv[i] = gr[i];
    } else {
        // dead history rows / R^-1 entries are read with zero coefficients (branch-free phases): they must hold finite values
        for (int i = tid; i < 2 * LB_HIST * ldh + LB_RPACK; i += STEP_NT) hist[i] = 0.f;
    }
    LbHist<float> H{hist, hist + LB_HIST * ldh, L.opt.lb_ro, nullptr, nullptr};
    H.ys = L.opt.lb_ys; H.rinv = rinv; H.ld = ldh;
    __syncthreads();
    bool done = false, paused = false;
    int stage_prev = L.sh_stage;
    for (; max_rounds <= 0 || slot_rounds < max_rounds; ++slot_rounds) {
        // opaque copy of the thread index: keeps the compiler from hoisting every tid-derived address
        // of the closure out of the round loop (which costs >256 live VGPRs and spills)
        int t = tid;
        asm volatile("" : "+v"(t));
        done = fit_round<REMOTE, REUSE, LEAN, true, SDFS, SDFS || QUEUE, SDFS>(M, L, nviews, H, false, false, F.stage_final + (size_t)b * MVFIT_MAX_STAGES, t, LbGramLds{nullptr, 0, 0},
                         F.trace ? F.trace + (size_t)b * F.trace_cap * (DV + 1) : nullptr, F.trace_cap,
                         ring, ring.tag != nullptr, (int)blockIdx.x,        // ring slots: sub-batch-relative problem index
                         SdfService{SDFS ? &P : nullptr, SDFS ? F.sdf_gate : nullptr, SDFS ? F.sdf_tag : nullptr, b, round0});
        if (done) break;                                  // block-uniform
        if (L.sh_stage != stage_prev) {
            // a new stage starts with a fresh optimiser (non_linear_solver.py:172): its history is empty, and the branch-free
            // phases of the compact direction read dead rows with zero coefficients - a leftover inf / NaN row of a stage that
            // ran off would turn 0 * inf into NaN there.  Dead rows are zeros, as at the launch's start.
            for (int i = tid; i < 2 * LB_HIST * ldh + LB_RPACK; i += STEP_NT) hist[i] = 0.f;
            stage_prev = L.sh_stage;
            __syncthreads();
        }
        // two-phase fit (stages without the SDF term run here, the rest in chained rounds): leave at the stage boundary -
        // the trial point in L.opt.x is the first one of the next stage, the optimiser is fresh (non_linear_solver.py:172)
        if (L.sh_stage >= pause_stage) { paused = true; break; }
    }
    store_block16(F.opt + b, &L.opt, sizeof(OptBlock), tid);
    // the next problem of the batch, if the launch has a queue and this one is finished (a paused problem or the round cap ends
    // the workgroup): decided here, before the row says "nothing more comes"
    int b_next = -1;
    if (QUEUE && queue && done) {                                       // uniform
        if (tid == 0) L.sh_next = atomicAdd(queue, 1);
        __syncthreads();
        if (L.sh_next < b_end) b_next = L.sh_next;
    }
    // passes of later rounds have nothing to wait for from this row - whatever ended the launch for it (finished, paused at a
    // stage boundary, or the round cap: the resident pass ends when every row has said so)
    if (tid == 0 && ring.tag) {
        if (b_next < 0) __hip_atomic_store(ring.done_round + row, (unsigned)(L.opt.lbS.n_closure - round0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (SDFS) __hip_atomic_store(F.sdf_gate + b, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (tid == 0 && (done || paused)) {
        if (done) atomicAdd(F.n_done, 1);
        const int left = atomicAdd(F.n_done + 1, 1) + 1;
        atomicAdd(F.n_done + 2, 1);
        // the last problem tells the host (per-round pass launches: it stops queueing them)
        if (ring.tag && left == done_target) __hip_atomic_store(ring.host_done, left, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (!done) {
        for (int i = tid; i < LB_HIST * ldh; i += STEP_NT) {
            const int r = i / ldh, e = i - r * ldh;
            gd[r * LB_D + e] = hist[i]; gs[r * LB_D + e] = hist[LB_HIST * ldh + i];
        }
        for (int i = tid; i < LB_RPACK; i += STEP_NT) gr[i] = rinv[i];
    }
    if (REMOTE && L.vp_remote) {
        // goodbye to the helpers; the pose of the final point is decoded here (with the pre-activations the chained
        // rounds of a two-phase fit expect from their predecessor)
        __syncthreads();
        if (tid == 0) { vps_store(vps_request_slot(M.vps), 0.f, (L.vp_seq + 1u) << 2 | VPS_BYE); L.vp_remote = 0; }
        __syncthreads();
    }
    pose_and_chain<false>(M, L, __builtin_amdgcn_readfirstlane(L.sw[L.sh_stage].flags), tid);
    publish_pose(L, P, b, tid);
    if (paused) {
        // what the chained rounds' step kernel expects from its predecessor: the pose block of the trial point (+ the
        // decoder state with VPoser) and the SDF gate of the stage that starts
        store_block16(F.pose + b, &L.pose, sizeof(PoseBlock), tid);
        if (SW.w[0].flags & MVFIT_F_VPOSER) store_block16(F.vp + b, L.vp_pre1, sizeof(VpBlock), tid);
        if (tid == 0 && F.sdf_adj) F.sdf_gate[b] = L.sw[L.sh_stage].coll_w > 0.f ? 1 : 0;
    }
    if (!QUEUE || b_next < 0) break;
    rounds_before = L.opt.lbS.n_closure - round0;                      // the row's rounds so far
    b = b_next;
    __syncthreads();                                                   // (every thread is done with the finished problem's LDS image)
  }
}

__global__ void fit_finish_kernel(FitBuffers F, float* __restrict__ params, float* __restrict__ final_loss,
                                  int32_t* __restrict__ n_closure, int32_t* __restrict__ n_iter, int B,
                                  int num_stages) {
    const int b = blockIdx.x;
    for (int i = threadIdx.x; i < DV; i += blockDim.x) params[(size_t)b * DV + i] = F.opt[b].x[i];
    if (threadIdx.x == 0) {
        const LbState& s = F.opt[b].lbS;
        if (final_loss) final_loss[b] = (float)F.stage_final[(size_t)b * MVFIT_MAX_STAGES + num_stages - 1];
        if (n_closure) n_closure[b] = s.n_closure;
        if (n_iter) n_iter[b] = s.n_lbfgs;
    }
}

// ------------------------------------------------------------------ float64 known-answer test
__device__ double kat_eval(int kind, int D, const double* x, double* g) {
    // mirrors oracle/lbfgs_np.py:kat_objective (serial: one lane)
    double f = 0.0;
    if (kind == 0) {
        for (int i = 0; i < D; ++i) {
            double c = 1.0 + 99.0 * i / (D - 1), r = x[i] - sin((double)i);
            f += c * r * r; g[i] = c * r;
        }
        f *= 0.5;
    } else if (kind == 1) {
        for (int i = 0; i < D; ++i) g[i] = 0.0;
        for (int i = 0; i < D - 1; ++i) {
            double a = x[i + 1] - x[i] * x[i], bb = 1.0 - x[i];
            f += 100.0 * a * a + bb * bb;
            g[i] += -400.0 * a * x[i] - 2.0 * bb;
            g[i + 1] += 200.0 * a;
        }
    } else {
        const double rho2 = 1e4;
        for (int i = 0; i < D; ++i) g[i] = x[i];
        double q = 0.0;
        for (int i = 0; i < D; ++i) {
            int n = (i + 1) % D;
            double r = 50.0 * (x[i] - sin((double)i)) + 20.0 * sin(3.0 * x[n]);
            double r2 = r * r;
            f += rho2 * r2 / (r2 + rho2);
            q += x[i] * x[i];
            double dr = 2.0 * r * rho2 * rho2 / ((r2 + rho2) * (r2 + rho2));
            g[i] += 50.0 * dr;
            g[n] += dr * 60.0 * cos(3.0 * x[n]);
        }
        f += 0.5 * q;
    }
    return f;
}

__global__ __launch_bounds__(64) void lbfgs_kat_kernel(int kind, int D, LbOpts O, double* x_io, double* trace,
                                                       int max_trace, int* n_closure, double* final_loss,
                                                       double* dirs, double* stps, double* ro, double* grow,
                                                       double* gcol, double* cmat) {
    __shared__ double xs[LB_D], gs[LB_D];
    __shared__ double fsh;
    __shared__ LbWork<double> W;
    const bool compact = (kind & 0x100) != 0;              // direction in compact form (lb_direction_compact)
    kind &= 0xff;
    const int lane = threadIdx.x;
    // the state in memory, like the fit kernels keep it (lbfgs_round works on it in place)
    __shared__ LbState S;
    __shared__ LbVecs<double> Vm[LB_LANES];
    if (lane == 0) {
        memset(&S, 0, sizeof(S));
        S.phase = PH_STEP_START; S.H = 1.0;
    }
    LbHist<double> H{dirs, stps, ro, grow, gcol};
    H.rinv = cmat; H.ys = cmat + LB_RPACK;                // compact form: packed R^-1 and the diagonal y.s
    double xt[LB_EPL];
#pragma unroll
    for (int e = 0; e < LB_EPL; ++e) {
        const int i = LB_EPL * lane + e;
        xt[e] = i < D ? x_io[i] : 0.0;
    }
    {
        LbVecs<double> z;
#pragma unroll
        for (int e = 0; e < LB_EPL; ++e) { z.x[e] = xt[e]; z.d[e] = z.g[e] = z.pg[e] = z.gprev[e] = z.bg0[e] = z.bg1[e] = 0.0; }
        Vm[lane] = z;
    }
    __syncthreads();
    int ncl = 0;
    for (int round = 0; round < 100000; ++round) {
#pragma unroll
        for (int e = 0; e < LB_EPL; ++e) if (LB_EPL * lane + e < LB_D) xs[LB_EPL * lane + e] = xt[e];
        __syncthreads();
        if (lane == 0) fsh = kat_eval(kind, D, xs, gs);
        __syncthreads();
        const double f = fsh;
        if (ncl < max_trace && lane == 0) {
            for (int i = 0; i < D; ++i) trace[(size_t)ncl * (D + 1) + i] = xs[i];
            trace[(size_t)ncl * (D + 1) + D] = f;
        }
        ncl += 1;
        double gnew[LB_EPL];
#pragma unroll
        for (int e = 0; e < LB_EPL; ++e) gnew[e] = (LB_EPL * lane + e < D) ? gs[LB_EPL * lane + e] : 0.0;
        __syncthreads();
        lbfgs_round<double, 64, false>(&S, &Vm[0], H, W, O, f, gnew, xt, lane, final_loss, [&]() {   // the production round
            if (compact) lb_direction_compact<double, 64>(H, W, lane, lb_dir_general(O));
            else lb_direction_block<double, 64>(H, W, lane);
        });
        __syncthreads();
        if (S.status) break;
    }
#pragma unroll
    for (int e = 0; e < LB_EPL; ++e) if (LB_EPL * lane + e < D) x_io[LB_EPL * lane + e] = Vm[lane].x[e];
    if (lane == 0) *n_closure = ncl;
}

}  // namespace mvfit

// ==================================================================================== host side
using namespace mvfit;

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
    DevPool problem_mem, ring_mem, obst_mem;
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

static int fail(mvfit_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}
#define HIP_OK(c, call)                                                                          \
    do {                                                                                         \
        hipError_t e__ = (call);                                                                 \
        if (e__ != hipSuccess) return fail(c, MVFIT_E_HIP, "%s: %s", #call, hipGetErrorString(e__)); \
    } while (0)

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
    M.mlds = dev_upload(c, &h.lds, 1);
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

static size_t step_lds() { return (sizeof(ClosureLds) + 15) & ~(size_t)15; }
static size_t step_gram_lds() { return step_lds() + LB_GW_BYTES; }       // fit_step_kernel: + the staged Gram window
static size_t persistent_lds(bool vp) { return std::max(persistent_lds_bytes(vp), sizeof(VpHelperLds)); }

static void drop_graph(mvfit_ctx* c) {
    if (c->round_graph) { hipGraphExecDestroy(c->round_graph); c->round_graph = nullptr; }
    c->graph_key.clear();
}

extern "C" const char* mvfit_last_error(const mvfit_ctx* ctx) { return ctx ? ctx->err.c_str() : "null ctx"; }

// Developer hooks (fault injection, experiment switches) exist only in the -DMVFIT_DEBUG_HOOKS variant build the tests that
// need them load (libmvfit_hooks.so); the released library has no trace of them and reads no environment variable.
#ifdef MVFIT_DEBUG_HOOKS
static int debug_hook(const char* name) { const char* e = getenv(name); return e ? atoi(e) : 0; }
#else
static constexpr int debug_hook(const char*) { return 0; }
#endif

// what the fit's plan (fit_plan.h) depends on in this ctx; mvfit_fit adds the fit's own stages and options
static FitPlanIn plan_inputs(const mvfit_ctx* c) {
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
    HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(prep_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)step_lds()));
    HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(closure_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)step_lds()));
    HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(closure_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)step_lds()));
    HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(fit_init_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)step_lds()));
    HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(fit_step_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)step_gram_lds()));
    HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(fit_step_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)step_gram_lds()));
    for (const void* k : {reinterpret_cast<const void*>(fit_persistent_kernel<false, false, true>),
                          reinterpret_cast<const void*>(fit_persistent_kernel<false, false, false>),
                          reinterpret_cast<const void*>(fit_persistent_kernel<true, false, false>),
                          reinterpret_cast<const void*>(fit_persistent_kernel<false, true, false>),
                          reinterpret_cast<const void*>(fit_persistent_kernel<false, true, true>),
                          reinterpret_cast<const void*>(fit_persistent_kernel<true, true, false>)})
        HIP_OK(c, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)std::max(persistent_lds(false), persistent_lds(true))));
    HIP_OK(c, c->h_done.reserve(8));
    HIP_OK(c, hipDeviceSynchronize());
    return MVFIT_OK;
}

// the scene term's obstacles go with the batch they were frozen for
static void free_obstacles(mvfit_ctx* c) {
    c->obst_mem.release();
    c->obst = Obstacles{};
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
    hipLaunchKernelGGL(pack_obs_kernel, dim3(B), dim3(256), 0, c->stream, c->Q, c->pb.obs);
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
    hipLaunchKernelGGL(pack_joints3d_kernel, dim3(c->B), dim3(64), 0, c->stream, (const float*)c->pb.gt3d, (const float*)c->pb.c3d, c->pb.obs);
    HIP_OK(c, hipGetLastError());
    c->has_joints3d = true;
    return MVFIT_OK;
}

extern "C" int mvfit_set_sdf(mvfit_ctx* c, const int32_t* faces, int num_faces, int grid_size) {
    if (!c) return MVFIT_E_ARG;
    if (c->obst.on && faces && num_faces != 0)
        return fail(c, MVFIT_E_STATE, "mvfit_set_sdf: scene obstacles are the interpenetration term (one per ctx): remove them first");
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
    if (samples && c->obst.on)
        return fail(c, MVFIT_E_UNSUPPORTED, "mvfit_sdf_term_read: the scene term keeps no per-vertex samples (sums only)");
    HIP_OK(c, hipSetDevice(c->device));
    if (samples) HIP_OK(c, hipMemcpyAsync(samples, c->pb.sdf_samp, (size_t)c->B * c->nv * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    if (sums) HIP_OK(c, hipMemcpy2DAsync(sums, sizeof(float), c->pb.sdf_adj, sizeof(SdfAdj), sizeof(float), c->B, hipMemcpyDeviceToDevice, c->stream));
    return MVFIT_OK;
}

// work buffers of the SDF term for the current batch
static int ensure_sdf_buffers(mvfit_ctx* c) {
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
    HIP_OK(c, c->problem_mem.alloc(&c->pb.sdf_boxpart, (size_t)c->Bpad * c->M.ntiles * 6 * 8));
    return MVFIT_OK;
}

// the per-round pass over problems [b_lo, b_hi) runs as lbs_vertex_pass_split_kernel (which writes the tile keys of the term's box when
// DevPose::box_part is set) when the split-fp16 basis exists and the launch is one 32-problem chunk per workgroup
static bool pass_writes_box_parts(const mvfit_ctx* c, int b_lo, int b_hi) {
    const int chunks = (b_hi + 31) / 32 - b_lo / 32;
    return !c->obst.on && c->M.bs_h2 != nullptr && c->pb.sdf_boxpart != nullptr && c->sdf_num_faces <= 128 && (chunks == 1 || c->opt.pass_kernel == 1);
}

// the interpenetration term of a chained round behind its vertex pass: against the frozen obstacles when they are set,
// else the one-person term of mvfit_set_sdf
static hipError_t launch_term(mvfit_ctx* c, const float* verts, const int* gate, hipStream_t st, const unsigned long long* box_part) {
    if (c->obst.on)
        return launch_scene_term(c->M, c->P, verts, c->B, c->obst.tab, c->obst.box, c->obst.phi, c->obst.grid, c->obst.rob, gate,
                                 c->pb.sdf_box, c->pb.sdf_entries, c->pb.sdf_adj, st);
    return launch_sdf_term(c->M, c->P, verts, c->B, c->sdf_faces.as<int32_t>(), c->sdf_num_faces, c->sdf_grid, gate, c->pb.sdf_box, c->pb.sdf_samp,
                           c->pb.sdf_entries, c->pb.sdf_adj, st, c->sdf_cull.get(), nullptr, 0u, box_part);
}

static int run_sdf_term(mvfit_ctx* c, const float* verts, const int* gate, hipStream_t st) {
    const hipError_t e = launch_term(c, verts, gate, st, nullptr);
    if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "%s term launch: %s", c->obst.on ? "scene" : "sdf", hipGetErrorString(e));
    return MVFIT_OK;
}

static int check_flags(mvfit_ctx* c, uint32_t flags) {
    if ((flags & MVFIT_F_USE_3D) && !c->has_joints3d) return fail(c, MVFIT_E_STATE, "MVFIT_F_USE_3D set but mvfit_set_joints3d was not called");
    if ((flags & MVFIT_F_VPOSER) && !c->has_vposer) return fail(c, MVFIT_E_STATE, "MVFIT_F_VPOSER set but the model has no VPoser decoder");
    if ((flags & MVFIT_F_PRIOR_GMM) && c->gmm_M == 0) return fail(c, MVFIT_E_STATE, "MVFIT_F_PRIOR_GMM set but the model has no GMM");
    return MVFIT_OK;
}

static DevWeights to_dev(const mvfit_weights& w) {
    DevWeights d;
    d.data_w2 = w.data_weight * w.data_weight;
    d.pose_w = w.body_pose_weight; d.shape_w = w.shape_weight; d.bend_w = w.bending_prior_weight;
    d.coll_w = w.coll_loss_weight; d.rho2 = w.rho * w.rho; d.flags = w.flags; d.pad = 0;
    return d;
}

static void prof_begin(mvfit_ctx* c, std::vector<std::pair<hipEvent_t, hipEvent_t>>& evs) {
    if (!c->profile || evs.size() >= 4096) return;
    hipEvent_t a, b;
    hipEventCreate(&a); hipEventCreate(&b);
    hipEventRecord(a, c->stream);
    evs.emplace_back(a, b);
}
static void prof_end(mvfit_ctx* c, std::vector<std::pair<hipEvent_t, hipEvent_t>>& evs) {
    if (!c->profile || evs.empty()) return;
    hipEventRecord(evs.back().second, c->stream);
}

static int run_vertex_pass(mvfit_ctx* c, float* verts) {
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
    hipLaunchKernelGGL(prep_kernel, dim3(c->B), dim3(STEP_NT), step_lds(), c->stream, c->M, (const ObsBlock*)c->pb.obs, c->P, params, flags,
                       (float*)nullptr);
    HIP_OK(c, hipGetLastError());
    rc = run_vertex_pass(c, verts);
    if (rc) return rc;
    if (joints) {
        hipLaunchKernelGGL(joints_kernel, dim3(c->B), dim3(64), 0, c->stream, c->M, (const float*)verts, (const float*)c->P.Amat,
                           params, joints);
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
    hipLaunchKernelGGL(prep_kernel, dim3(c->B), dim3(STEP_NT), step_lds(), c->stream, c->M, (const ObsBlock*)c->pb.obs, c->P, params, flags,
                       (float*)nullptr);
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
    hipLaunchKernelGGL(prep_kernel, dim3(c->B), dim3(STEP_NT), step_lds(), c->stream, c->M, (const ObsBlock*)c->pb.obs, c->P, params, flags,
                       full_pose);
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
    hipLaunchKernelGGL(closure_kernel<true>, dim3(n + nsets * VPS_SLICES), dim3(STEP_NT), step_lds(), c->stream, M,
                       (const ObsBlock*)c->pb.obs, c->V, to_dev(*w), c->P, params, 0, loss, grad, joints, (const SdfAdj*)nullptr);
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
    if (sdf && !c->sdf_num_faces && !c->obst.on)
        return fail(c, MVFIT_E_STATE, "coll_loss_weight > 0 needs the SDF term's faces: call mvfit_set_sdf first");
    HIP_OK(c, hipSetDevice(c->device));
    if (c->opt.closure_vposer_helpers && (w->flags & MVFIT_F_VPOSER) && c->vps_mem && !sdf)
        return closure_via_helpers(c, w, params, loss, grad, verts, joints);
    float* vbuf = verts ? verts : c->pb.verts;
    // the interpenetration term reads every vertex: it forces the vertex pass
    const bool sparse = (w->flags & MVFIT_F_SPARSE_VERTS) != 0 && !sdf;
    if (!sparse || verts) {
        hipLaunchKernelGGL(prep_kernel, dim3(c->B), dim3(STEP_NT), step_lds(), c->stream, c->M, (const ObsBlock*)c->pb.obs, c->P, params, w->flags,
                           (float*)nullptr);
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
    hipLaunchKernelGGL(closure_kernel<false>, dim3(c->B), dim3(STEP_NT), step_lds(), c->stream, c->M, (const ObsBlock*)c->pb.obs, c->V,
                       to_dev(*w), c->P, params,
                       sparse ? 0 : 1, loss, grad, joints, sdf ? (const SdfAdj*)c->pb.sdf_adj : (const SdfAdj*)nullptr);
    prof_end(c, c->ev_step);
    HIP_OK(c, hipGetLastError());
    return MVFIT_OK;
}

// the optimiser's scalar options (the gtol segments are the caller's)
static LbOpts lb_opts(const mvfit_lbfgs_opts& o, int num_stages) {
    LbOpts O;
    memset(&O, 0, sizeof(O));
    O.lr = o.lr; O.tol_grad = o.tolerance_grad; O.tol_change = o.tolerance_change; O.ftol = o.ftol; O.gtol = o.gtol;
    O.max_iter = o.max_iter; O.max_eval = o.max_iter * 5 / 4; O.history = o.history; O.maxiters = o.maxiters;
    O.num_stages = num_stages;
    O.dir_general = debug_hook("MVFIT_DIR_GENERAL") != 0;      // (hooks build only) the general form of the direction's triangular products
    return O;
}

// What every entry that runs the optimiser requires of them.  The ring has LB_HIST slots and a new pair goes to slot
// (hist_head + hist_len - 1) % LB_HIST: history <= 0 makes that slot negative (hist_len stays 0), history > LB_HIST lets
// hist_len grow past the ring.
static_assert(MVFIT_HISTORY == LB_HIST, "mvfit_lbfgs_opts::history is checked against the size of the device ring");
static bool lb_opts_ok(const mvfit_lbfgs_opts& o) {
    return o.max_iter > 0 && o.history > 0 && o.history <= MVFIT_HISTORY && o.maxiters > 0;
}

static int make_opts(mvfit_ctx* c, const mvfit_lbfgs_opts* o, uint32_t flags, LbOpts& O) {
    if (!lb_opts_ok(*o) || o->num_stages <= 0 || o->num_stages > MVFIT_MAX_STAGES)
        return fail(c, MVFIT_E_ARG, "bad lbfgs options");
    O = lb_opts(*o, o->num_stages);
    O.reuse_outer = (flags & MVFIT_F_REUSE_OUTER_VALUE) ? 1 : 0;
    // parameter tensors that take part in the gtol test (fitting.py:115-116): requires_grad ones,
    // as index ranges of the compact optimiser vector (reference final_params order)
    int n = 0;
    auto add = [&](int lo, int hi) { O.seg_lo[n] = lo; O.seg_hi[n] = hi; ++n; };
    if (flags & MVFIT_F_VPOSER) {
        if (!(flags & MVFIT_F_FIX_SHAPE)) add(0, 10);
        add(10, 13); add(13, 16);
        if (!(flags & MVFIT_F_FIX_SCALE)) add(16, 17);
        add(17, 49);
    } else {
        if (!(flags & MVFIT_F_FIX_SHAPE)) add(0, 10);
        add(10, 13); add(13, 82); add(82, 85);
        if (!(flags & MVFIT_F_FIX_SCALE)) add(85, 86);
    }
    O.nseg = n;
    return MVFIT_OK;
}

// rounds of (vertex pass, step kernel) between two looks at the done counter, replayed as one graph
static const int kGraphRounds = 24;

static int ensure_round_graph(mvfit_ctx* c, const StageWeights& SW, const LbOpts& O) {
    // (the scene term's obstacles: buffers and scalars baked into its kernel node; a re-freeze changes none of them)
    struct { const void *tab, *box, *phi; int grid; float rob; } obst = {nullptr, nullptr, nullptr, 0, 0.f};
    if (c->obst.on) { obst.tab = c->obst.tab; obst.box = c->obst.box; obst.phi = c->obst.phi; obst.grid = c->obst.grid; obst.rob = c->obst.rob; }
    std::vector<unsigned char> key(sizeof(SW) + sizeof(O) + sizeof(DevPose) + sizeof(FitBuffers) + sizeof(DevProblems) + sizeof(int) + sizeof(obst));
    unsigned char* k = key.data();
    memcpy(k, &SW, sizeof(SW)); k += sizeof(SW);
    memcpy(k, &O, sizeof(O)); k += sizeof(O);
    memcpy(k, &c->P, sizeof(DevPose)); k += sizeof(DevPose);
    memcpy(k, &c->F, sizeof(FitBuffers)); k += sizeof(FitBuffers);
    memcpy(k, &c->Q, sizeof(DevProblems)); k += sizeof(DevProblems);
    memcpy(k, &c->opt.pass_kernel, sizeof(int)); k += sizeof(int);
    memcpy(k, &obst, sizeof(obst));
    if (c->round_graph && key == c->graph_key) return MVFIT_OK;
    drop_graph(c);
    hipStream_t cs;
    HIP_OK(c, hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
    if (e == hipSuccess) {
        // rounds with the SDF term: the pass writes its tiles' keys of the term's bounding box (single-chunk split kernel), the
        // front kernel reduces the box from them
        DevPose Pg = c->P;
        if (c->F.sdf_adj && pass_writes_box_parts(c, 0, c->B)) Pg.box_part = c->pb.sdf_boxpart;
        for (int r = 0; r < kGraphRounds && e == hipSuccess; ++r) {
            e = launch_vertex_pass(c->M, Pg, c->B, c->pb.verts, c->opt.pass_kernel, cs);
            if (e == hipSuccess && c->F.sdf_adj)
                e = launch_term(c, c->pb.verts, c->F.sdf_gate, cs, Pg.box_part);
            hipLaunchKernelGGL(O.reuse_outer ? fit_step_kernel<true> : fit_step_kernel<false>, dim3(c->B), dim3(STEP_NT), step_gram_lds(), cs, c->M, (const ObsBlock*)c->pb.obs, c->V, SW, O,
                               c->P, c->F);
        }
        hipError_t e2 = hipStreamEndCapture(cs, &g);
        if (e == hipSuccess) e = e2;
    }
    if (e == hipSuccess) e = hipGraphInstantiate(&c->round_graph, g, nullptr, nullptr, 0);
    if (g) hipGraphDestroy(g);
    hipStreamDestroy(cs);
    if (e != hipSuccess) { c->round_graph = nullptr; return fail(c, MVFIT_E_HIP, "round graph: %s", hipGetErrorString(e)); }
    c->graph_key = key;
    c->graph_rounds = kGraphRounds;
    return MVFIT_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Asynchronous full-mode fit (default when no SDF term is active and the batch leaves CUs for the passes).
//
// The objective reads 69 of the 6890 vertices and the optimiser kernel evaluates those itself (sparse_forward: the
// same arithmetic as the pass on the selected vertices), so the 6890-vertex LBS pass of a trial point is not on the
// optimiser's critical path - but every closure still gets its full pass, like the reference's return_verts=True:
//   ctx stream   ONE fit_persistent_kernel launch (one workgroup per problem, L-BFGS history in LDS) runs the whole
//                staged fit; in closure round r it publishes the pose operands of the trial point into ring slot
//                r % kRingSlots (write-through stores + a per-problem tag);
//   pass stream  one lbs_vertex_pass launch per closure round, queued ahead by the host in batches of kPassBatch;
//                the pass of round r waits (bounded spin on the tags of its 32 problems) until the optimiser has
//                published round r, then computes all 6890 vertices of those trial points on the CUs the optimiser
//                does not occupy - concurrently with the optimiser's own work on closure r.
// Nothing the optimiser does waits on a pass (one-directional hand-off: no deadlock; a pass that times out just runs
// on whatever the slot holds).  Passes whose 32 problems have all finished return at once.  stats: passes run /
// skipped / operands overwritten before their pass could read them (ring too short for the drift between problems;
// expected 0) / timed out (expected 0).
// Measured alternatives on configs[1]: chaining pass -> step per round costs pass + step (37 us per round, 766 k
// closures/s); forking the two inside one hipGraph round overlaps them but the cross-queue join costs ~12 us per round
// (632 k); windows of 24 rounds of the persistent kernel followed by their 24 passes lose the lock-step at every
// window end (947 k).
// ---------------------------------------------------------------------------------------------------------
static const int kRingSlots = 128;
static const int kPassBatch = 24;
static const int kVpLogRounds = 1024;     // mvfit_profile: rounds of the resident pass that are stamped

// The ring is sized by the SUB-BATCH (rb problems, a multiple of 32), not by the batch: only one sub-batch uses it at a
// time (128 slots x 2.06 KB per problem: 34 MB at 128 problems whatever the batch size).  Everything indexed by ring slot
// takes sub-batch-relative problem indices; done_round stays indexed by the global problem index.
static int ensure_async(mvfit_ctx* c, int rb) {
    if (!c->pass_stream) {
        HIP_OK(c, hipStreamCreateWithFlags(&c->pass_stream, hipStreamNonBlocking));
        for (hipEvent_t& e : c->ev_batch) HIP_OK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        HIP_OK(c, hipEventCreateWithFlags(&c->ev_init, hipEventDisableTiming));
        HIP_OK(c, c->h_async_done.reserve(64));
        HIP_OK(c, c->queue.reserve(64));
    }
    AsyncRing& R = c->ring;
    if (R.tag && R.Bpad >= rb) return MVFIT_OK;
    if (R.tag) {
        HIP_OK(c, hipStreamSynchronize(c->stream));
        HIP_OK(c, hipStreamSynchronize(c->pass_stream));
    }
    DevPool& mem = c->ring_mem;
    mem.release();                       // (also what an earlier call that failed half-way left)
    R = AsyncRing{};
    const size_t Bp = (size_t)rb;
    R.nslots = kRingSlots; R.Bpad = rb;
    HIP_OK(c, mem.alloc(&R.coefH, kRingSlots * Bp * KROWS * 4, true));
    HIP_OK(c, mem.alloc(&R.Amat, kRingSlots * Bp * 288 * 4, true));
    HIP_OK(c, mem.alloc(&R.tau, kRingSlots * Bp * 4 * 4, true));
    HIP_OK(c, mem.alloc(&R.done_round, (size_t)c->Bpad * 4));
    HIP_OK(c, mem.alloc(&R.stats, 4 * 4));
    HIP_OK(c, mem.alloc(&R.pass_done, 4 * kPassWords));
    HIP_OK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&R.host_done), c->h_async_done.get(), 0));
    HIP_OK(c, mem.alloc(&R.tag, kRingSlots * Bp * 4));          // last: a ring with a tag is complete
    return MVFIT_OK;
}

// Decoder helpers (vposer_service.h) ride on the single-launch fits with the VPoser prior: `nsets` sets of 8 helper
// workgroups behind the n problems' ones, every set serving the problems b with b % nsets == s (the count comes with the
// plan: fit_plan.cpp).  All workgroups of the launch must be resident at once (the problems wait for their helpers' answers)
// - every problem's arithmetic is the same whatever the slicing.  mvfit_options::vposer_helpers = 0 keeps the decoder in the
// problems' own workgroups (another summation order: results differ in the last bits).
static int launch_persistent(mvfit_ctx* c, const StageWeights& SW, const LbOpts& O, int cap, const AsyncRing& R, const FitLaunch& L,
                             int pause_stage, bool sdfs = false, int* queue = nullptr, int b_end = 0) {
    const int n = L.b_hi - L.b_lo;
    DevModel M = c->M;
    int grid = n;
    if (L.nsets) {
        HIP_OK(c, hipMemsetAsync(c->vps_mem, 0, c->vps_words * 8, c->stream));
        M.vps.req = c->vps_mem;
        M.vps.resp = c->vps_mem + (size_t)VPS_MAX_SETS * VPS_PMAX * VPS_GRAN;
        M.vps.stat = reinterpret_cast<unsigned*>(c->vps_mem + c->vps_words);
        M.vps.nsets = L.nsets;
        M.vps.nprob = n;
        M.vps.fault = debug_hook("MVFIT_VP_FAULT") != 0;                                     // test hook (hooks build only): helpers that never answer
        grid = n + L.nsets * VPS_SLICES;
        c->vps_stats[0] += 1;
    }
    const bool lean = !(SW.w[0].flags & (MVFIT_F_VPOSER | MVFIT_F_PRIOR_GMM | MVFIT_F_USE_3D));    // (flags are the same in all stages)
    // (service launches - the stages with the SDF term, mvfit_options::sdf_service - have their own instantiations: the other
    // kernels carry no trace of the service; MVFIT_F_REUSE_OUTER_VALUE fits keep the chained rounds, see fit_plan.cpp)
    auto kern = sdfs ? (M.vps.nsets ? fit_persistent_kernel<true, false, false, true> : fit_persistent_kernel<false, false, false, true>)
                : queue ? (lean ? fit_persistent_kernel<false, false, true, false, true> : fit_persistent_kernel<false, false, false, false, true>)
                : M.vps.nsets ? (O.reuse_outer ? fit_persistent_kernel<true, true, false> : fit_persistent_kernel<true, false, false>)
                : O.reuse_outer ? (lean ? fit_persistent_kernel<false, true, true> : fit_persistent_kernel<false, true, false>)
                : lean ? fit_persistent_kernel<false, false, true> : fit_persistent_kernel<false, false, false>;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(STEP_NT), persistent_lds((SW.w[0].flags & MVFIT_F_VPOSER) != 0), c->stream, M,
                       (const ObsBlock*)c->pb.obs, c->V, SW, O, c->P, c->F, cap, R, L.b_lo, L.n_target, pause_stage, queue, b_end);
    HIP_OK(c, hipGetLastError());
    return MVFIT_OK;
}

// mvfit_profile: the resident pass's stamp log -> per round: service span = last workgroup's stores drained - first workgroup saw
// the operands; busy = a workgroup's own drained - seen (wall clock, 100 MHz)
static int reduce_pass_log(mvfit_ctx* c, int res_grid) {
    std::vector<unsigned long long> lg((size_t)kVpLogRounds * res_grid * 2);
    HIP_OK(c, hipMemcpy(lg.data(), c->vp_log.as<unsigned long long>(), lg.size() * 8, hipMemcpyDeviceToHost));
    double span = 0.0, busy = 0.0, slowest = 0.0;
    int n = 0;
    for (int r = 0; r < kVpLogRounds; ++r) {
        unsigned long long lo = ~0ull, hi = 0ull, bsum = 0ull, bmax = 0ull;
        bool all = true;
        for (int w = 0; w < res_grid; ++w) {
            const unsigned long long a = lg[((size_t)r * res_grid + w) * 2], z = lg[((size_t)r * res_grid + w) * 2 + 1];
            if (!z) { all = false; break; }
            lo = std::min(lo, a); hi = std::max(hi, z); bsum += z - a; bmax = std::max(bmax, z - a);
        }
        if (!all) break;
        span += (double)(hi - lo) * 1e-5; busy += (double)bsum / res_grid * 1e-5;      // ticks of 10 ns -> ms
        slowest += (double)bmax * 1e-5;
        ++n;
    }
    c->res_rounds = n;
    c->res_span_ms = n ? span / n : 0.0;
    c->res_busy_ms = n ? busy / n : 0.0;
    c->res_slowest_ms = n ? slowest / n : 0.0;
    return MVFIT_OK;
}

// ---- the four drivers of a planned phase (fit_plan.h); *complete = problems that finished (a lead phase: that left it) ----

// DRIVER_ASYNC / DRIVER_ASYNC_SDF: per planned launch one fit_persistent_kernel on the ctx stream and its vertex passes on the
// pass stream (the mechanism: the block comment above; sub-batches, work queue and pass form come with the plan).  With the SDF
// service the launch continues fits that are paused in front of their first stage with the term, and every round's pass is
// followed by the term's kernels (launch_sdf_term, whose pull-back publishes the answer tag) - per-round launches by
// construction (the term's kernels need the round's vertices complete: a launch boundary).
static int run_async(mvfit_ctx* c, const StageWeights& SW, const LbOpts& O, const FitPhase& ph, int* complete) {
    const int B = c->B, tpw = ph.form, res_grid = ph.res_grid;
    const bool sdf_service = ph.driver == DRIVER_ASYNC_SDF, refill = ph.refill;
    const bool dbg_nopass = debug_hook("MVFIT_DEBUG_NOPASS") != 0;          // (hooks build only)
    if (sdf_service) HIP_OK(c, hipMemsetAsync(c->F.n_done + 1, 0, 8, c->stream));       // (a lead phase has counted its leavers there)
    int rc = ensure_async(c, ph.per);
    if (rc) return rc;
    AsyncRing R = c->ring;
    const size_t rb = (size_t)R.Bpad;                       // ring stride in problems (>= per)
    volatile int* h_done = c->h_async_done.as<int>();
    // polled words: re-initialised every call
    HIP_OK(c, hipMemsetAsync(R.done_round, 0xff, (size_t)c->Bpad * 4, c->stream));
    HIP_OK(c, hipMemsetAsync(R.stats, 0, 16, c->stream));
    c->resident_tpw = tpw;
    R.npass = tpw ? res_grid : 1;
    c->res_rounds = 0; c->res_span_ms = c->res_busy_ms = c->res_slowest_ms = 0.0;
    const bool log_on = tpw && c->profile;
    if (log_on) {
        HIP_OK(c, c->vp_log.reserve((size_t)kVpLogRounds * res_grid * 2 * 8));
    }
    for (const FitLaunch& L : ph.launches) {
        const int b_lo = L.b_lo, b_hi = L.b_hi, n_target = L.n_target;
        *h_done = 0;
        // per sub-batch: its tags (the slots are reused by other problems), the pass counter and the count of problems
        // that left the launch (finished or paused) - a sub-batch that stops at the round cap does not keep the later ones
        // from seeing theirs complete.  (The ctx stream is behind the previous sub-batch's last passes here.)
        HIP_OK(c, hipMemsetAsync(R.tag, 0, (size_t)kRingSlots * rb * 4, c->stream));
        HIP_OK(c, hipMemsetAsync(R.pass_done, 0, 4 * kPassWords, c->stream));
        HIP_OK(c, hipMemsetAsync(c->F.n_done + 1, 0, 4, c->stream));
        if (sdf_service) {
            // per sub-batch: no answer yet, and no gate open - a problem opens its own in front of every round's tag (the gates of
            // the problems outside this sub-batch stay shut: the term's kernels cover all problems up to b_hi)
            HIP_OK(c, hipMemsetAsync(c->F.sdf_tag, 0, (size_t)c->Bpad * 4, c->stream));
            HIP_OK(c, hipMemsetAsync(c->F.sdf_gate, 0, (size_t)B * 4, c->stream));
        }
        if (log_on) HIP_OK(c, hipMemsetAsync(c->vp_log.get(), 0, c->vp_log.size(), c->stream));      // (a profiled fit keeps the last sub-batch's stamps)
        HIP_OK(c, hipEventRecord(c->ev_init, c->stream));
        HIP_OK(c, hipStreamWaitEvent(c->pass_stream, c->ev_init, 0));
        if (refill) {
            c->h_queue0 = b_hi;                                   // problems [0, rows) start on their rows, the queue hands out the rest
            HIP_OK(c, hipMemcpyAsync(c->queue.as<int>(), &c->h_queue0, 4, hipMemcpyHostToDevice, c->stream));
        }
        rc = launch_persistent(c, SW, O, ph.launch_cap, R, L, ph.pause_stage, sdf_service, refill ? c->queue.as<int>() : nullptr, B);
        if (rc) return rc;
        int k = 0;
        if (tpw) {
            // ---- resident pass: ONE launch serves every closure round of this sub-batch from the ring; it ends when every
            //      problem has left the optimiser kernel (finished, paused at a stage boundary, or the round cap) ----
            ResidentArgs RA{};
            RA.coefH = R.coefH; RA.Amat = R.Amat; RA.tau = R.tau; RA.tag = R.tag;
            RA.done_round = R.done_round; RA.stats = R.stats; RA.wg_round = R.pass_done;
            RA.log = log_on ? c->vp_log.as<unsigned long long>() : nullptr; RA.log_rounds = kVpLogRounds;
            RA.verts = c->pb.verts;
            RA.capture_verts = c->capture_verts; RA.capture_round = c->capture_verts ? c->capture_round : -1;
            RA.nslots = kRingSlots; RA.rb = (int)rb;
            RA.b_lo = b_lo; RA.n = b_hi - b_lo;
            RA.flags = (unsigned)debug_hook("MVFIT_DEBUG_NT_OFF");         // (hooks build only) bit 1 = plain vertex stores
            RA.max_rounds = (unsigned)ph.launch_cap;
            hipError_t e = launch_vertex_pass_resident(c->M, RA, tpw, c->pass_stream);
            if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "resident vertex pass launch: %s", hipGetErrorString(e));
            HIP_OK(c, hipEventRecord(c->ev_batch[0], c->pass_stream));
        } else {
        // the passes: one per closure round, queued at most two batches ahead of the ones that have completed
        for (;; ++k) {
            for (int i = 0; i < kPassBatch && !dbg_nopass; ++i) {
                const unsigned r = (unsigned)(k * kPassBatch + i);
                const int slot = (int)(r % (unsigned)kRingSlots);
                DevPose P = c->P;                                          // side outputs / unused fields as in the chained mode
                // the pass addresses its operands by the global problem / chunk index: slot bases shifted by the sub-batch start
                P.coefH = R.coefH + ((ptrdiff_t)slot * (ptrdiff_t)rb - (ptrdiff_t)b_lo) * (KROWS / 4);
                P.coefT = nullptr;
                P.Amat = R.Amat + ((ptrdiff_t)slot * (ptrdiff_t)rb - (ptrdiff_t)b_lo) * 288;
                P.tau = R.tau + ((ptrdiff_t)slot * (ptrdiff_t)rb - (ptrdiff_t)b_lo) * 4;
                P.tag = R.tag + ((ptrdiff_t)slot * (ptrdiff_t)rb - (ptrdiff_t)b_lo);
                P.done_round = R.done_round;
                P.stats = R.stats;
                P.pass_done = R.pass_done;
                P.round = r;
                P.chunk0 = b_lo / 32;
                P.pad_ = (unsigned)debug_hook("MVFIT_DEBUG_NT_OFF");      // (hooks build only) bit 0 = plain basis loads, bit 1 = plain vertex stores
                float* vout = c->pb.verts;
                if (c->capture_verts && (int)r == c->capture_round) vout = c->capture_verts;      // test hook
                if (sdf_service && pass_writes_box_parts(c, b_lo, b_hi)) P.box_part = c->pb.sdf_boxpart;      // (the term's box from the pass's tile keys)
                hipError_t e = launch_pass_gate(P, b_lo, b_hi, c->pass_stream);
                hipEvent_t ea = nullptr, eb = nullptr;
                if (c->profile && c->ev_vp.size() < 4096) {            // mvfit_profile: the dispatch's own begin / end stamps
                    hipEventCreate(&ea); hipEventCreate(&eb);
                    c->ev_vp.emplace_back(ea, eb);
                }
                if (e == hipSuccess) e = launch_vertex_pass(c->M, P, b_hi, vout, c->opt.pass_kernel, c->pass_stream, ea, eb);
                if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "vertex pass launch: %s", hipGetErrorString(e));
                if (sdf_service) {
                    // the term at the round's vertices for the problems whose gate word is set (written by the optimiser in
                    // front of the round's tag); transforms from the ring slot, float32 coefficients from the chained layout
                    DevPose Ps = P;
                    Ps.coefT = c->P.coefT;
                    e = launch_sdf_term(c->M, Ps, vout, b_hi, c->sdf_faces.as<int32_t>(), c->sdf_num_faces, c->sdf_grid, c->F.sdf_gate, c->pb.sdf_box,
                                        c->pb.sdf_samp, c->pb.sdf_entries, c->pb.sdf_adj, c->pass_stream, c->sdf_cull.get(), c->F.sdf_tag, r + 1u, P.box_part);
                    if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "SDF term launch: %s", hipGetErrorString(e));
                }
            }
            HIP_OK(c, hipEventRecord(c->ev_batch[k & 3], c->pass_stream));
            if (k >= 2) HIP_OK(c, hipEventSynchronize(c->ev_batch[(k - 2) & 3]));
            if (*h_done >= n_target) break;
            if ((k + 1) * kPassBatch >= ph.launch_cap) break;
        }
        }
        // behind the optimiser kernel (all problems of the sub-batch, or the round cap) the ctx stream continues behind the
        // last passes (nothing of the fit's result depends on them: ordering only)
        HIP_OK(c, hipStreamWaitEvent(c->stream, c->ev_batch[k & 3], 0));
    }
    // one host wait for all of it
    HIP_OK(c, hipMemcpyAsync(c->async_stats, R.stats, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(c, hipMemcpyAsync(c->h_done.as<int>(), c->F.n_done, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(c, hipMemcpyAsync(c->h_done.as<int>() + 1, c->F.n_done + 2, 4, hipMemcpyDeviceToHost, c->stream));   // problems that left, all sub-batches
    HIP_OK(c, hipStreamSynchronize(c->stream));
    // a lead phase: every problem must have LEFT the single-launch kernel at the stage boundary (or finished): one that stopped
    // at the round cap mid-history would be continued by the chained step kernel, whose two-loop direction reads Gram rows the
    // single-launch kernel (compact direction form) does not maintain
    *complete = c->h_done.as<int>()[ph.pause_stage <= MVFIT_MAX_STAGES ? 1 : 0];
    // automatic mode: a fit whose resident workgroups (or whose optimiser) gave up waiting has shown that the launch does not get
    // the CUs the choice assumes (a shared device, a CU mask): later fits on this ctx use the per-round launches
    if (tpw && c->opt.resident_pass < 0 && c->async_stats[3]) c->resident_auto_off = true;
    if (log_on) return reduce_pass_log(c, res_grid);
    return MVFIT_OK;
}

// DRIVER_SPARSE: the persistent kernel alone, sub-batch after sub-batch
static int run_sparse(mvfit_ctx* c, const StageWeights& SW, const LbOpts& O, const FitPhase& ph, int* complete) {
    int* h_done = c->h_done.as<int>();
    *h_done = 0;
    for (const FitLaunch& L : ph.launches) {
        const int done_before = *h_done;          // (synchronised: problems finished by the earlier sub-batches)
        for (int rounds = 0; rounds < ph.launch_cap;) {
            const int chunk = std::min(ph.launch_cap - rounds, 1 << 20);
            if (const int rc = launch_persistent(c, SW, O, chunk, AsyncRing{}, L, MVFIT_MAX_STAGES + 1)) return rc;
            rounds += chunk;
            HIP_OK(c, hipMemcpyAsync(h_done, c->F.n_done, 4, hipMemcpyDeviceToHost, c->stream));
            HIP_OK(c, hipStreamSynchronize(c->stream));
            if (*h_done >= done_before + (L.b_hi - L.b_lo)) break;      // this sub-batch is complete (an earlier one may have hit the cap)
        }
    }
    *complete = *h_done;
    return MVFIT_OK;
}

// DRIVER_EAGER: chained rounds as eager launches bracketed by events (bench.py's per-launch timing of the vertex pass)
static int run_eager(mvfit_ctx* c, const StageWeights& SW, const LbOpts& O, const FitPhase& ph, int* complete) {
    int* h_done = c->h_done.as<int>();
    for (int rounds = 0; rounds < ph.launch_cap;) {
        for (int r = 0; r < kGraphRounds; ++r) {
            int rc = run_vertex_pass(c, c->pb.verts);
            if (!rc && c->F.sdf_adj) rc = run_sdf_term(c, c->pb.verts, c->F.sdf_gate, c->stream);
            if (rc) return rc;
            prof_begin(c, c->ev_step);
            hipLaunchKernelGGL(O.reuse_outer ? fit_step_kernel<true> : fit_step_kernel<false>, dim3(c->B), dim3(STEP_NT), step_gram_lds(), c->stream, c->M, (const ObsBlock*)c->pb.obs, c->V, SW, O,
                               c->P, c->F);
            prof_end(c, c->ev_step);
        }
        HIP_OK(c, hipGetLastError());
        rounds += kGraphRounds;
        HIP_OK(c, hipMemcpyAsync(h_done, c->F.n_done, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_OK(c, hipStreamSynchronize(c->stream));
        if (*h_done >= c->B) break;
    }
    *complete = *h_done;
    return MVFIT_OK;
}

// DRIVER_GRAPH: chained rounds, kGraphRounds of them per graph replay
static int run_graph(mvfit_ctx* c, const StageWeights& SW, const LbOpts& O, const FitPhase& ph, int* complete) {
    const int B = c->B;
    int* h_done = c->h_done.as<int>();
    if (const int rc = ensure_round_graph(c, SW, O)) return rc;
    // While at most half of the problems have finished, the next replay is queued before the host looks at the
    // done counter of the current one (the GPU does not idle through the ~30 us host turnaround); later the
    // replays go one at a time, so that no replay runs after the last problem finished.
    if (!c->ev_done[0]) {
        HIP_OK(c, hipEventCreateWithFlags(&c->ev_done[0], hipEventDisableTiming));
        HIP_OK(c, hipEventCreateWithFlags(&c->ev_done[1], hipEventDisableTiming));
    }
    auto enqueue = [&](int slot) -> hipError_t {
        hipError_t e = hipGraphLaunch(c->round_graph, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&h_done[slot], c->F.n_done, 4, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipEventRecord(c->ev_done[slot], c->stream);
        return e;
    };
    int rounds = 0, launched = 0, waited = 0, seen = 0;
    h_done[0] = h_done[1] = 0;
    const bool ahead_ok = B >= 8;
    while (true) {
        while (launched - waited < ((ahead_ok && seen <= B / 2) ? 2 : 1) && rounds < ph.launch_cap) {
            HIP_OK(c, enqueue(launched & 1));
            rounds += c->graph_rounds;
            ++launched;
        }
        if (launched == waited) break;                     // round cap reached
        HIP_OK(c, hipEventSynchronize(c->ev_done[waited & 1]));
        seen = h_done[waited & 1];
        ++waited;
        if (seen >= B) break;
    }
    HIP_OK(c, hipStreamSynchronize(c->stream));
    *complete = seen;
    return MVFIT_OK;
}

extern "C" int mvfit_debug_capture_pass(mvfit_ctx* c, int round, float* verts) {
    if (!c) return MVFIT_E_ARG;
    c->capture_round = verts ? round : -1;
    c->capture_verts = verts;
    return MVFIT_OK;
}

extern "C" int mvfit_fit_stats(mvfit_ctx* c, uint32_t* out4) {
    if (!c || !out4) return MVFIT_E_ARG;
    for (int i = 0; i < 4; ++i) out4[i] = c->async_stats[i];
    return MVFIT_OK;
}

extern "C" int mvfit_decoder_stats(mvfit_ctx* c, uint32_t* out3) {
    if (!c || !out3) return MVFIT_E_ARG;
    unsigned st[2] = {0, 0};
    if (c->vps_mem && c->vps_stats[0]) {
        HIP_OK(c, hipSetDevice(c->device));
        HIP_OK(c, hipStreamSynchronize(c->stream));
        HIP_OK(c, hipMemcpy(st, c->vps_mem + c->vps_words, 8, hipMemcpyDeviceToHost));
    }
    out3[0] = c->vps_stats[0]; out3[1] = st[0]; out3[2] = st[1];
    return MVFIT_OK;
}

extern "C" int mvfit_fit(mvfit_ctx* c, const mvfit_weights* sw, const mvfit_lbfgs_opts* o, float* params,
                         float* final_loss, int32_t* n_closure, int32_t* n_iter) {
    if (!c || !sw || !o || !params) return MVFIT_E_ARG;
    if (c->B == 0) return fail(c, MVFIT_E_STATE, "call mvfit_set_problems first");
    HIP_OK(c, hipSetDevice(c->device));
    // ---- validate ----
    StageWeights SW;
    memset(&SW, 0, sizeof(SW));
    FitPlanIn in = plan_inputs(c);
    if (o->num_stages <= 0 || o->num_stages > MVFIT_MAX_STAGES) return fail(c, MVFIT_E_ARG, "num_stages");
    for (int s = 0; s < o->num_stages; ++s) {
        int rc = check_flags(c, sw[s].flags);
        if (rc) return rc;
        if (sw[s].flags != sw[0].flags) return fail(c, MVFIT_E_ARG, "flags must be identical for all stages");
        if (sw[s].coll_loss_weight > 0.f) in.sdf_stages |= 1u << s;
        SW.w[s] = to_dev(sw[s]);
    }
    const bool any_sdf = in.sdf_stages != 0;
    if (any_sdf && !c->sdf_num_faces && !c->obst.on)
        return fail(c, MVFIT_E_STATE, "coll_loss_weight > 0 needs the SDF term's faces: call mvfit_set_sdf first");
    if (c->obst.on) in.sdf_service = 0;          // the scene term runs in chained rounds only (no service path for it)
    if (any_sdf) {
        int rc = ensure_sdf_buffers(c);
        if (rc) return rc;
    }
    c->F.sdf_adj = any_sdf ? c->pb.sdf_adj : nullptr;
    c->F.trace = c->trace; c->F.trace_cap = c->trace ? c->trace_cap : 0;
    LbOpts O;
    int rc = make_opts(c, o, sw[0].flags, O);
    if (rc) return rc;
    const int cap = o->max_rounds > 0 ? o->max_rounds : (o->num_stages * o->maxiters * (O.max_eval + 30) + 8);
    // ---- plan: phases, drivers, sub-batches, pass form, queue (fit_plan.cpp; the table: DESIGN.md §4.4) ----
    in.flags = sw[0].flags; in.num_stages = o->num_stages; in.reuse_outer = O.reuse_outer != 0; in.cap = cap;
    const FitPlan plan = plan_fit(in);
    if (plan.rc) return fail(c, plan.rc, "%s", plan.err.c_str());
    // ---- initialise ----
    for (unsigned& v : c->async_stats) v = 0;
    for (unsigned& v : c->vps_stats) v = 0;
    if (c->vps_mem) HIP_OK(c, hipMemsetAsync(c->vps_mem + c->vps_words, 0, 8, c->stream));
    const int B = c->B;
    HIP_OK(c, hipMemsetAsync(c->F.n_done, 0, 12, c->stream));
    HIP_OK(c, hipMemsetAsync(c->F.sdf_gate, sw[0].coll_loss_weight > 0.f ? 1 : 0, (size_t)B * 4, c->stream));
    hipLaunchKernelGGL(fit_init_kernel, dim3(B), dim3(STEP_NT), step_lds(), c->stream, c->M, (const ObsBlock*)c->pb.obs, c->P, c->F,
                       (const float*)params,
                       sw[0].flags, plan.init_full_pass ? 1 : 0);
    HIP_OK(c, hipGetLastError());
    // ---- run the phases; one that does not complete (the round cap) ends the fit ----
    static int (*const drivers[])(mvfit_ctx*, const StageWeights&, const LbOpts&, const FitPhase&, int*) = {run_async, run_async, run_sparse,
                                                                                                           run_graph, run_eager};
    unsigned stats[4] = {0, 0, 0, 0}, sv_lost = 0, sv_gave_up = 0;
    const FitPhase* capped = nullptr;
    for (int i = 0; i < plan.nphases && !capped; ++i) {
        const FitPhase& ph = plan.phase[i];
        int complete = 0;
        rc = drivers[ph.driver](c, SW, O, ph, &complete);
        if (rc) return rc;
        if (ph.driver == DRIVER_ASYNC_SDF) { sv_lost = c->async_stats[2]; sv_gave_up = c->async_stats[3]; }
        if (ph.driver <= DRIVER_ASYNC_SDF) for (int k = 0; k < 4; ++k) stats[k] += c->async_stats[k];
        if (complete < B) capped = &ph;
    }
    for (int k = 0; k < 4; ++k) c->async_stats[k] = stats[k];               // mvfit_fit_stats: the whole fit
    // ---- results, then the verdict ----
    hipLaunchKernelGGL(fit_finish_kernel, dim3(B), dim3(128), 0, c->stream, c->F, params, final_loss, n_closure, n_iter, B,
                       o->num_stages);
    HIP_OK(c, hipGetLastError());
    // a gate that timed out lets the term's kernels run on another round's operands, a problem whose answer never came ends
    // with a NaN loss: neither is a result
    if (sv_lost || sv_gave_up)
        return fail(c, MVFIT_E_STATE, "SDF service rounds degraded (%u operand sets lost, %u waits given up): the fit is not valid - "
                    "is the GPU shared?  (mvfit_options::sdf_service = 0 runs these stages as chained rounds)", sv_lost, sv_gave_up);
    if (capped)
        return fail(c, MVFIT_E_STATE, "fit hit the round cap (%d) before all problems finished%s", cap,
                    capped->pause_stage <= MVFIT_MAX_STAGES ? " the stages without the SDF term" : "");
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

extern "C" int mvfit_fit_trace(mvfit_ctx* c, float* trace, int max_closures) {
    if (!c || max_closures < 0 || (trace && max_closures == 0)) return MVFIT_E_ARG;
    c->trace = trace;
    c->trace_cap = trace ? max_closures : 0;
    return MVFIT_OK;
}

#ifdef MVFIT_LB_CHECK
// check build: [0] fast optimiser transitions cross-checked against the general state machine, [1] mismatches, [2] first word
extern "C" __attribute__((visibility("default"))) int mvfit_debug_lb_check(unsigned* out4, int reset) {
    hipDeviceSynchronize();
    hipMemcpyFromSymbol(out4, HIP_SYMBOL(mvfit::g_lb_check), sizeof(unsigned) * 4);
    if (reset) { unsigned z[4] = {0, 0, 0, 0}; hipMemcpyToSymbol(HIP_SYMBOL(mvfit::g_lb_check), z, sizeof(z)); }
    return 0;
}
#endif
#ifdef MVFIT_TIMING
extern "C" __attribute__((visibility("default"))) int mvfit_debug_timing(long long* out32, int reset) {
    hipDeviceSynchronize();
    hipMemcpyFromSymbol(out32, HIP_SYMBOL(mvfit::g_dbg), sizeof(long long) * 32);
    if (reset) { long long z[32] = {0}; hipMemcpyToSymbol(HIP_SYMBOL(mvfit::g_dbg), z, sizeof(z)); }
    return 0;
}
extern "C" __attribute__((visibility("default"))) int mvfit_debug_timing_adv(long long* out16, int reset) {           // g_dbg[48..63]: inside lbfgs_advance
    hipDeviceSynchronize();
    hipMemcpyFromSymbol(out16, HIP_SYMBOL(mvfit::g_dbg), sizeof(long long) * 16, sizeof(long long) * 48);
    if (reset) { long long z[16] = {0}; hipMemcpyToSymbol(HIP_SYMBOL(mvfit::g_dbg), z, sizeof(z), sizeof(long long) * 48); }
    return 0;
}
extern "C" __attribute__((visibility("default"))) int mvfit_debug_timing_calls(long long* out16, int reset) {          // g_dbg[64..79]: optimiser calls by kind (lbfgs_round)
    hipDeviceSynchronize();
    hipMemcpyFromSymbol(out16, HIP_SYMBOL(mvfit::g_dbg), sizeof(long long) * 16, sizeof(long long) * 64);
    if (reset) { long long z[16] = {0}; hipMemcpyToSymbol(HIP_SYMBOL(mvfit::g_dbg), z, sizeof(z), sizeof(long long) * 64); }
    return 0;
}
extern "C" __attribute__((visibility("default"))) int mvfit_debug_timing_helpers(long long* out16, int reset) {       // g_dbg[32..47]: decoder helper (set 0, slice 0)
    hipDeviceSynchronize();
    hipMemcpyFromSymbol(out16, HIP_SYMBOL(mvfit::g_dbg), sizeof(long long) * 16, sizeof(long long) * 32);
    if (reset) { long long z[16] = {0}; hipMemcpyToSymbol(HIP_SYMBOL(mvfit::g_dbg), z, sizeof(z), sizeof(long long) * 32); }
    return 0;
}
#endif

extern "C" int mvfit_sdf(mvfit_ctx* c, const int32_t* faces, int num_faces, const float* vertices, int B, int num_vertices,
                         int G, float* phi) {
    if (!c) return MVFIT_E_ARG;
    if (!faces || !vertices || !phi || num_faces < 0 || B <= 0 || num_vertices <= 0 || G < 2 || G > 1024)
        return fail(c, MVFIT_E_ARG, "mvfit_sdf: bad argument (num_faces=%d B=%d num_vertices=%d G=%d)", num_faces, B, num_vertices, G);
    HIP_OK(c, hipSetDevice(c->device));
    // long face lists: exact culling on face lists (sdf_term.hip), bit-identical to the walk; mvfit_options::sdf_face_lists = 0
    // keeps the walk
    c->sdf_op_path = 0;
    if (sdf_op_uses_lists(num_faces) && c->opt.sdf_face_lists) {
        if (c->sdf_op_B != B || c->sdf_op_F != num_faces) {       // a new shape: decide once (the decision, also a refusal, is kept)
            HIP_OK(c, hipStreamSynchronize(c->stream));
            c->sdf_op_ws.reset();
            size_t free_b = 0, total_b = 0;
            HIP_OK(c, hipMemGetInfo(&free_b, &total_b));
            if (sdf_op_ws_bytes(B, num_faces) < free_b / 2) {
                HIP_OK(c, c->sdf_op_ws.reserve(sdf_op_ws_bytes(B, num_faces)));
                HIP_OK(c, hipMemsetAsync(c->sdf_op_ws.as<unsigned char>() + sdf_cull_zero_offset(B, num_faces), 0, sdf_cull_zero_bytes(B),
                                         c->stream));
            }
            c->sdf_op_B = B; c->sdf_op_F = num_faces;
        }
        if (c->sdf_op_ws.get()) {
            hipError_t e = launch_sdf_voxelize_culled(faces, num_faces, vertices, B, num_vertices, G, phi, c->sdf_op_ws.get(), c->stream);
            if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "sdf launch: %s", hipGetErrorString(e));
            c->sdf_op_path = 1;
            return MVFIT_OK;
        }
        c->sdf_op_path = 2;                                       // the workspace did not fit: the walk
    }
    hipError_t e = launch_sdf_voxelize(faces, num_faces, vertices, B, num_vertices, G, phi, c->stream);
    if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "sdf launch: %s", hipGetErrorString(e));
    return MVFIT_OK;
}

// SDFLoss.forward for num_scenes scenes (scene_sdf.hip).  Groups of consecutive whole scenes whose fields and local vertices
// stay under the 256 MB cap the renderer uses (one scene's, when that alone needs more); inside a group the bodies are
// voxelised in runs whose face lists stay under 2 GB.
// scene_first[num_scenes + 1]: starts at 0, 1 .. MVFIT_SCENE_BODIES_MAX bodies per scene
static int check_scene_first(mvfit_ctx* c, const char* who, const int32_t* scene_first, int num_scenes) {
    if (scene_first[0] != 0) return fail(c, MVFIT_E_ARG, "%s: scene_first[0] = %d, not 0", who, scene_first[0]);
    for (int s = 0; s < num_scenes; ++s) {
        const long long cnt = (long long)scene_first[s + 1] - scene_first[s];
        if (cnt < 0) return fail(c, MVFIT_E_ARG, "%s: scene_first decreases at scene %d", who, s);
        if (cnt == 0) return fail(c, MVFIT_E_ARG, "%s: scene %d is empty", who, s);
        if (cnt > MVFIT_SCENE_BODIES_MAX)
            return fail(c, MVFIT_E_ARG, "%s: scene %d has %lld bodies (at most %d)", who, s, cnt, MVFIT_SCENE_BODIES_MAX);
    }
    return MVFIT_OK;
}

// keep_box / keep_tab (both or neither; then phi_out is set too): the freeze of mvfit_set_scene_obstacles - boxes and table
// rows go to the caller's buffers as well, the faces are the model's own (checked at mvfit_create) and the pair kernels do
// not run (no loss).  Boxes and fields are what the loss call computes: the same kernels on the same inputs.
static int scene_sdf_run(mvfit_ctx* c, const char* who, const float* vertices, int num_vertices, const int32_t* faces, int num_faces,
                         const int32_t* scene_first, int num_scenes, int grid_size, float scale_factor, float robustifier,
                         float* loss, float* g_vertices, float* phi_out, float4* keep_box, int32_t* keep_tab) {
    const bool freeze = keep_box != nullptr;
    if (!vertices || !faces || !scene_first || (!loss && !freeze))
        return fail(c, MVFIT_E_ARG, "%s: null %s", who, !vertices ? "vertices" : !faces ? "faces" : !scene_first ? "scene_first" : "loss");
    if (num_vertices <= 0 || num_faces <= 0 || num_scenes <= 0)
        return fail(c, MVFIT_E_ARG, "%s: bad argument (num_vertices=%d num_faces=%d num_scenes=%d)", who, num_vertices,
                    num_faces, num_scenes);
    if (grid_size < 2 || grid_size > 128) return fail(c, MVFIT_E_ARG, "%s: grid_size %d outside [2, 128]", who, grid_size);
    if (const int rc = check_scene_first(c, who, scene_first, num_scenes)) return rc;
    const int N = scene_first[num_scenes];
    HIP_OK(c, hipSetDevice(c->device));
    // the voxelisation reads vertices through the face indices: checked on the host, as mvfit_set_sdf does (this also
    // orders the call behind the earlier ones: the staging below is free again)
    HIP_OK(c, hipStreamSynchronize(c->stream));
    if (!freeze) {
        std::vector<int32_t> h((size_t)num_faces * 3);
        HIP_OK(c, hipMemcpy(h.data(), faces, h.size() * 4, hipMemcpyDefault));
        for (int32_t vi : h)
            if (vi < 0 || vi >= num_vertices)
                return fail(c, MVFIT_E_ARG, "%s: face vertex index %d outside [0, %d)", who, (int)vi, num_vertices);
    }
    const int G = grid_size, nblk = scene_sdf_blocks(num_vertices);
    const size_t nvox = (size_t)G * G * G, cap = (size_t)256 << 20;
    const bool lists = sdf_op_uses_lists(num_faces) && c->opt.sdf_face_lists;
    const size_t per_body = (phi_out ? 0 : nvox * 4) + (size_t)num_vertices * 12;
    std::vector<int> group_end;                  // scene index one past each group
    int nb_max = 0;
    for (int s0 = 0; s0 < num_scenes;) {
        int s1 = s0 + 1;
        while (s1 < num_scenes && (size_t)(scene_first[s1 + 1] - scene_first[s0]) * per_body <= cap &&
               scene_first[s1 + 1] - scene_first[s0] <= 4096)
            ++s1;
        group_end.push_back(s1);
        nb_max = std::max(nb_max, scene_first[s1] - scene_first[s0]);
        s0 = s1;
    }
    // bodies voxelised per run of the face-list kernels: as many as the group has while the lists stay under 2 GB (11.6 MB per
    // body at 13,776 faces; one run of 128 bodies takes half the time of six runs of 22 - every run ends in a tail of few busy
    // workgroups) and, when the workspace has to grow, under half of the free memory, as mvfit_sdf decides it
    int run = lists ? (int)std::min<size_t>((size_t)nb_max, std::max<size_t>(1, ((size_t)2 << 30) / sdf_op_ws_bytes(1, num_faces))) : 0;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_tab = 0, o_first = o_tab + al((size_t)N * 16), o_box = o_first + al((size_t)(num_scenes + 1) * 4);
    const size_t o_part = o_box + al((size_t)N * 16), o_local = o_part + al((size_t)nb_max * nblk * 4);
    const size_t o_phi = o_local + al((size_t)nb_max * num_vertices * 12), o_cull = o_phi + (phi_out ? 0 : al((size_t)nb_max * nvox * 4));
    size_t need = o_cull + (lists ? sdf_op_ws_bytes(run, num_faces) : 0);
    if (need > c->scn_ws.size()) {
        c->scn_ws.reset();
        size_t free_b = 0, total_b = 0;
        HIP_OK(c, hipMemGetInfo(&free_b, &total_b));
        while (run > 1 && need > free_b / 2) {
            run = (run + 1) / 2;
            need = o_cull + sdf_op_ws_bytes(run, num_faces);
        }
        HIP_OK(c, c->scn_ws.reserve(need));
    }
    const size_t tb = o_box;                     // tables: a row per body, then scene_first
    HIP_OK(c, c->h_scn_tab.reserve(tb));
    int32_t* h_tab = c->h_scn_tab.as<int32_t>();
    for (int s = 0; s < num_scenes; ++s)
        for (int b = scene_first[s]; b < scene_first[s + 1]; ++b) {
            int32_t* r = h_tab + (size_t)b * 4;
            r[0] = scene_first[s]; r[1] = scene_first[s + 1] - scene_first[s]; r[2] = 0; r[3] = 0;
        }
    memcpy(c->h_scn_tab.as<unsigned char>() + o_first, scene_first, (size_t)(num_scenes + 1) * 4);
    unsigned char* ws = c->scn_ws.as<unsigned char>();
    HIP_OK(c, hipMemcpyAsync(ws, h_tab, tb, hipMemcpyHostToDevice, c->stream));
    if (freeze) HIP_OK(c, hipMemcpyAsync(keep_tab, h_tab, (size_t)N * 16, hipMemcpyHostToDevice, c->stream));
    float4* box = freeze ? keep_box : reinterpret_cast<float4*>(ws + o_box);
    float* part = reinterpret_cast<float*>(ws + o_part);
    float* local = reinterpret_cast<float*>(ws + o_local);
    const float factor = (float)((1.0 + (double)scale_factor) * 0.5);
    c->sdf_op_path = lists ? 1 : 0;
    int s0 = 0;
    for (int s1 : group_end) {
        const int b0 = scene_first[s0], n = scene_first[s1] - b0;
        float* phi = phi_out ? phi_out + (size_t)b0 * nvox : reinterpret_cast<float*>(ws + o_phi);
        hipError_t e = launch_scene_boxes(vertices, num_vertices, b0, n, factor, box, local, c->stream);
        if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "%s: box launch: %s", who, hipGetErrorString(e));
        if (lists) {
            for (int r0 = 0; r0 < n; r0 += run) {
                const int rn = std::min(run, n - r0);
                // the lists' count area must be zero where this run's layout puts it
                HIP_OK(c, hipMemsetAsync(ws + o_cull + sdf_cull_zero_offset(rn, num_faces), 0, sdf_cull_zero_bytes(rn), c->stream));
                e = launch_sdf_voxelize_culled(faces, num_faces, local + (size_t)r0 * num_vertices * 3, rn, num_vertices, G,
                                               phi + (size_t)r0 * nvox, ws + o_cull, c->stream);
                if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "%s: sdf launch: %s", who, hipGetErrorString(e));
            }
        } else {
            e = launch_sdf_voxelize(faces, num_faces, local, n, num_vertices, G, phi, c->stream);
            if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "%s: sdf launch: %s", who, hipGetErrorString(e));
        }
        if (freeze) { s0 = s1; continue; }
        e = launch_scene_pairs(vertices, num_vertices, b0, n, s0, s1 - s0, ws + o_tab, reinterpret_cast<const int32_t*>(ws + o_first),
                               box, phi, G, robustifier, g_vertices, part, loss, c->stream);
        if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "%s: pair launch: %s", who, hipGetErrorString(e));
        s0 = s1;
    }
    return MVFIT_OK;
}

extern "C" int mvfit_scene_sdf_loss(mvfit_ctx* c, const float* vertices, int num_vertices, const int32_t* faces, int num_faces,
                                    const int32_t* scene_first, int num_scenes, int grid_size, float scale_factor,
                                    float robustifier, float* loss, float* g_vertices, float* phi_out) {
    if (!c) return MVFIT_E_ARG;
    return scene_sdf_run(c, "mvfit_scene_sdf_loss", vertices, num_vertices, faces, num_faces, scene_first, num_scenes, grid_size,
                         scale_factor, robustifier, loss, g_vertices, phi_out, nullptr, nullptr);
}

// Freeze the obstacles of the scene term at `vertices` (scene_sdf.hip: scene_entries_kernel reads them in every chained round).
extern "C" int mvfit_set_scene_obstacles(mvfit_ctx* c, const float* vertices, const int32_t* scene_first, int num_scenes,
                                         int grid_size, float scale_factor, float robustifier) {
    if (!c) return MVFIT_E_ARG;
    HIP_OK(c, hipSetDevice(c->device));
    if (!vertices) {                                         // remove: the buffers stay for the next freeze of this batch
        c->obst.on = false;
        return MVFIT_OK;
    }
    if (c->B == 0) return fail(c, MVFIT_E_STATE, "call mvfit_set_problems first");
    if (!c->num_faces) return fail(c, MVFIT_E_STATE, "mvfit_set_scene_obstacles: the model was created without (valid) faces");
    if (c->sdf_num_faces)
        return fail(c, MVFIT_E_STATE, "mvfit_set_scene_obstacles: mvfit_set_sdf's term is the interpenetration term (one per ctx): remove it first");
    if (c->nv > 8192) return fail(c, MVFIT_E_UNSUPPORTED, "the scene term supports up to 8192 vertices (model has %d)", c->nv);
    if (!scene_first || num_scenes <= 0) return fail(c, MVFIT_E_ARG, "mvfit_set_scene_obstacles: bad argument (num_scenes=%d)", num_scenes);
    if (grid_size < 2 || grid_size > 128) return fail(c, MVFIT_E_ARG, "mvfit_set_scene_obstacles: grid_size %d outside [2, 128]", grid_size);
    int rc = check_scene_first(c, "mvfit_set_scene_obstacles", scene_first, num_scenes);
    if (rc) return rc;
    if (scene_first[num_scenes] != c->B)
        return fail(c, MVFIT_E_ARG, "mvfit_set_scene_obstacles: the scenes hold %d bodies, the ctx %d problems", scene_first[num_scenes], c->B);
    const size_t nvox = (size_t)grid_size * grid_size * grid_size;
    if (c->obst.grid != grid_size || !c->obst.phi) {
        HIP_OK(c, hipStreamSynchronize(c->stream));
        free_obstacles(c);
        HIP_OK(c, c->obst_mem.alloc(&c->obst.tab, (size_t)c->B * 16));
        HIP_OK(c, c->obst_mem.alloc(&c->obst.box, (size_t)c->B * sizeof(float4)));
        HIP_OK(c, c->obst_mem.alloc(&c->obst.phi, (size_t)c->B * nvox * 4));
        c->obst.grid = grid_size;
    }
    c->obst.on = false;                                      // a failed freeze leaves no term behind
    rc = ensure_sdf_buffers(c);
    if (rc) return rc;
    hipError_t e = launch_scene_null_boxes(c->pb.sdf_box, c->B, c->stream);
    if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "mvfit_set_scene_obstacles: box launch: %s", hipGetErrorString(e));
    rc = scene_sdf_run(c, "mvfit_set_scene_obstacles", vertices, c->nv, c->d_faces, c->num_faces, scene_first, num_scenes, grid_size,
                       scale_factor, robustifier, nullptr, nullptr, c->obst.phi, c->obst.box, c->obst.tab);
    if (rc) return rc;
    c->obst.rob = robustifier;
    c->obst.on = true;
    return MVFIT_OK;
}

extern "C" int mvfit_scene_obstacles_read(mvfit_ctx* c, float* phi, float* boxes) {
    if (!c) return MVFIT_E_ARG;
    if (!c->obst.on) return fail(c, MVFIT_E_STATE, "mvfit_scene_obstacles_read: no obstacles are set");
    HIP_OK(c, hipSetDevice(c->device));
    const size_t nvox = (size_t)c->obst.grid * c->obst.grid * c->obst.grid;
    if (phi) HIP_OK(c, hipMemcpyAsync(phi, c->obst.phi, (size_t)c->B * nvox * 4, hipMemcpyDeviceToDevice, c->stream));
    if (boxes) HIP_OK(c, hipMemcpyAsync(boxes, c->obst.box, (size_t)c->B * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    return MVFIT_OK;
}

// The silhouette term (silhouette.hip): the mask set is prepared once, the loss calls sample it.
extern "C" int mvfit_set_silhouettes(mvfit_ctx* c, int num_images, int height, int width, const uint8_t* masks,
                                     const int32_t* image_body, const float* cam_R, const float* cam_t, const float* cam_f,
                                     const float* cam_c, int contour_stride) {
    if (!c) return MVFIT_E_ARG;
    HIP_OK(c, hipSetDevice(c->device));
    if (num_images == 0) {                                   // clear: the work areas stay for a next set of the same size
        c->sil.on = false;
        return MVFIT_OK;
    }
    if (num_images < 0 || num_images > 65535 || height < 2 || height > 8192 || width < 2 || width > 8192)
        return fail(c, MVFIT_E_ARG, "mvfit_set_silhouettes: sizes out of range (num_images=%d in [0, 65535], height=%d and "
                    "width=%d in [2, 8192])", num_images, height, width);
    if (contour_stride < 1) return fail(c, MVFIT_E_ARG, "mvfit_set_silhouettes: contour_stride %d < 1", contour_stride);
    if (!masks || !image_body || !cam_R || !cam_t || !cam_f || !cam_c)
        return fail(c, MVFIT_E_ARG, "mvfit_set_silhouettes: null %s", !masks ? "masks" : !image_body ? "image_body" : !cam_R ? "cam_R" :
                    !cam_t ? "cam_t" : !cam_f ? "cam_f" : "cam_c");
    return sil_set(c->sil, c->nv, num_images, height, width, masks, image_body, cam_R, cam_t, cam_f, cam_c, contour_stride,
                   c->stream, c->err);
}

extern "C" int mvfit_silhouettes_read(mvfit_ctx* c, float* field, int32_t* contour_first, int32_t* contour_xy, int32_t* num_points) {
    if (!c) return MVFIT_E_ARG;
    if (!c->sil.on) return fail(c, MVFIT_E_STATE, "mvfit_silhouettes_read: no mask set is present");
    HIP_OK(c, hipSetDevice(c->device));
    if (num_points) *num_points = c->sil.C;
    return sil_read(c->sil, field, contour_first, contour_xy, c->stream, c->err);
}

extern "C" int mvfit_silhouette_loss(mvfit_ctx* c, const float* vertices, int num_bodies, float w_in, float w_out, float sigma,
                                     float* loss, float* g_vertices, int32_t* winner) {
    if (!c) return MVFIT_E_ARG;
    if (!c->sil.on) return fail(c, MVFIT_E_STATE, "mvfit_silhouette_loss: no mask set is present (mvfit_set_silhouettes)");
    if (!vertices || !loss) return fail(c, MVFIT_E_ARG, "mvfit_silhouette_loss: null %s", !vertices ? "vertices" : "loss");
    if (num_bodies < 1 || num_bodies > 65535)
        return fail(c, MVFIT_E_ARG, "mvfit_silhouette_loss: num_bodies %d outside [1, 65535]", num_bodies);
    if (c->sil.body_min < 0 || c->sil.body_max >= num_bodies)
        return fail(c, MVFIT_E_ARG, "mvfit_silhouette_loss: image_body holds %d .. %d, outside [0, %d)", c->sil.body_min,
                    c->sil.body_max, num_bodies);
    HIP_OK(c, hipSetDevice(c->device));
    return sil_loss(c->sil, vertices, num_bodies, w_in, w_out, sigma, loss, g_vertices, winner, c->stream, c->err);
}

extern "C" int mvfit_triangulate(mvfit_ctx* c, int B, int V, const float* keypoints, const double* intris, const double* extris,
                                 double* joints3d) {
    if (!c) return MVFIT_E_ARG;
    if (B <= 0 || V <= 0 || !keypoints || !intris || !extris || !joints3d)
        return fail(c, MVFIT_E_ARG, "mvfit_triangulate: bad argument (B=%d V=%d)", B, V);
    HIP_OK(c, hipSetDevice(c->device));
    hipError_t e = launch_triangulate(keypoints, intris, extris, B, V, NKP, joints3d, c->stream);
    if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "triangulate launch: %s", hipGetErrorString(e));
    return MVFIT_OK;
}

// Cross-view association of a frame's detections (associate.hip).  Frames go through in groups whose rays and linkage
// matrices stay under the 256 MB cap of the renderer's and the scene op's workspaces; a frame's result does not depend on
// its group.
extern "C" int mvfit_associate_views(mvfit_ctx* c, int F, int V, int Nmax, const float* keypoints, const int32_t* count,
                                     const double* intris, const double* extris, double max_cost, int min_joints, int min_views,
                                     double* cost_out, int32_t* labels, int32_t* num_clusters) {
    if (!c) return MVFIT_E_ARG;
    if (!keypoints || !count || !intris || !extris || !labels)
        return fail(c, MVFIT_E_ARG, "mvfit_associate_views: null %s",
                    !keypoints ? "keypoints" : !count ? "count" : !intris ? "intris" : !extris ? "extris" : "labels");
    if (F <= 0 || V > MVFIT_MAX_VIEWS || Nmax < 1 || Nmax > MVFIT_ASSOC_MAX_DET || min_views < 2 || min_views > V)
        return fail(c, MVFIT_E_ARG, "mvfit_associate_views: bad argument (F=%d V=%d Nmax=%d min_views=%d): 2 <= min_views <= V <= %d, "
                    "1 <= Nmax <= %d", F, V, Nmax, min_views, MVFIT_MAX_VIEWS, MVFIT_ASSOC_MAX_DET);
    if (min_joints < 1 || min_joints > NKP)
        return fail(c, MVFIT_E_ARG, "mvfit_associate_views: min_joints %d outside [1, %d]", min_joints, NKP);
    if (!(max_cost >= 0.0) || std::isinf(max_cost))
        return fail(c, MVFIT_E_ARG, "mvfit_associate_views: max_cost %g is not a finite value >= 0", max_cost);
    if (max_cost == 0.0) max_cost = 0.0;                     // -0.0: the kernels compare bit patterns
    HIP_OK(c, hipSetDevice(c->device));
    const int D = V * Nmax;
    const size_t cap = (size_t)256 << 20, per = assoc_frame_bytes(D);
    const int group = (int)std::min<size_t>({(size_t)F, std::max<size_t>(1, (cap - assoc_head_bytes()) / per), (size_t)32768});
    const size_t need = assoc_head_bytes() + (size_t)group * per;
    if (need > c->assoc_ws.size()) HIP_OK(c, hipStreamSynchronize(c->stream));          // an earlier call may still run on the old one
    HIP_OK(c, c->assoc_ws.reserve(need));
    for (int f0 = 0; f0 < F; f0 += group) {
        const hipError_t e = launch_associate_group(keypoints, count, intris, extris, f0, std::min(group, F - f0), V, Nmax, max_cost,
                                                    min_joints, min_views, c->assoc_ws.get(), cost_out, labels, num_clusters, c->stream);
        if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "mvfit_associate_views: launch: %s", hipGetErrorString(e));
    }
    return MVFIT_OK;
}

extern "C" int mvfit_depth_guess(mvfit_ctx* c, int B, const double* rest_joints, const double* extri, const double* intri,
                                 const float* keypoints, double* joints3d) {
    if (!c) return MVFIT_E_ARG;
    if (B <= 0 || !rest_joints || !extri || !intri || !keypoints || !joints3d)
        return fail(c, MVFIT_E_ARG, "mvfit_depth_guess: bad argument (B=%d)", B);
    HIP_OK(c, hipSetDevice(c->device));
    hipError_t e = launch_depth_guess(rest_joints, extri, intri, keypoints, B, NKP, joints3d, c->stream);
    if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "depth guess launch: %s", hipGetErrorString(e));
    return MVFIT_OK;
}

extern "C" int mvfit_umeyama(mvfit_ctx* c, int B, int npts, const double* src, const double* dst, int estimate_scale,
                             double* rot, double* rvec, double* trans, double* scale) {
    if (!c) return MVFIT_E_ARG;
    if (B <= 0 || npts < 3 || !src || !dst || !rot || !rvec || !trans || !scale)
        return fail(c, MVFIT_E_ARG, "mvfit_umeyama: bad argument (B=%d npts=%d)", B, npts);
    HIP_OK(c, hipSetDevice(c->device));
    hipError_t e = launch_umeyama(src, dst, B, npts, estimate_scale, rot, rvec, trans, scale, c->stream);
    if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "umeyama launch: %s", hipGetErrorString(e));
    return MVFIT_OK;
}

extern "C" int mvfit_project_points(mvfit_ctx* c, const float* points, int num_points, float* uv) {
    if (!c) return MVFIT_E_ARG;
    if (!points || !uv || num_points <= 0) return fail(c, MVFIT_E_ARG, "mvfit_project_points: bad argument (num_points=%d)", num_points);
    if (c->B == 0) return fail(c, MVFIT_E_STATE, "call mvfit_set_problems first (the cameras come from there)");
    HIP_OK(c, hipSetDevice(c->device));
    hipError_t e = launch_project_points(c->Q, points, num_points, uv, c->stream);
    if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "projection launch: %s", hipGetErrorString(e));
    return MVFIT_OK;
}

// grows the renderer's workspace and normal buffer (kept in the ctx) to at least ws / nb bytes
static int render_reserve(mvfit_ctx* c, size_t ws, size_t nb) {
    if (ws > c->render_ws.size() || nb > c->render_nrm.size())
        HIP_OK(c, hipStreamSynchronize(c->stream));             // earlier calls may still read the old buffers
    HIP_OK(c, c->render_ws.reserve(ws));
    HIP_OK(c, c->render_nrm.reserve(nb));
    return MVFIT_OK;
}

extern "C" int mvfit_render_overlay(mvfit_ctx* c, const float* vertices, const float* points, int num_points, int num_images,
                                    const int32_t* image_problem, const int32_t* image_view, int height, int width,
                                    const uint8_t* images, uint8_t* out, int32_t* face_id) {
    if (!c) return MVFIT_E_ARG;
    if (!c->num_faces) return fail(c, MVFIT_E_STATE, "mvfit_render_overlay: the model was created without (valid) faces");
    if (c->B == 0) return fail(c, MVFIT_E_STATE, "call mvfit_set_problems first (the cameras come from there)");
    if (!vertices || !images || !out || !image_problem || !image_view || num_images < 1 || height < 1 || height > 8192 ||
        width < 1 || width > 8192 || num_points < 0 || num_points > 64)
        return fail(c, MVFIT_E_ARG, "mvfit_render_overlay: bad argument (num_images=%d height=%d width=%d num_points=%d)",
                    num_images, height, width, num_points);
    for (int i = 0; i < num_images; ++i)
        if (image_problem[i] < 0 || image_problem[i] >= c->B || image_view[i] < 0 || image_view[i] >= c->V)
            return fail(c, MVFIT_E_ARG, "mvfit_render_overlay: image %d names problem %d / view %d (B=%d V=%d)", i,
                        image_problem[i], image_view[i], c->B, c->V);
    HIP_OK(c, hipSetDevice(c->device));
    // images per group: at most RENDER_GROUP_MAX and a workspace of at most 256 MB - or one image's, when a single image
    // needs more (8 H W bytes of visibility, 512 MB at 8192 x 8192; images are not tiled)
    const size_t cap = (size_t)256 << 20;
    int G = std::min(num_images, RENDER_GROUP_MAX);
    while (G > 1 && render_ws_bytes(G, c->nv, c->num_faces, height, width) > cap) --G;
    const size_t ws = render_ws_bytes(G, c->nv, c->num_faces, height, width);
    const size_t nb = (size_t)c->B * c->nv * 3 * sizeof(double);
    if (int rc = render_reserve(c, ws, nb)) return rc;
    hipError_t e = launch_render_normals(vertices, c->B, c->nv, c->d_faces, c->d_vf_ptr, c->d_vf_idx, c->render_nrm.as<double>(), c->stream);
    const size_t px = (size_t)height * width;
    for (int i0 = 0; i0 < num_images && e == hipSuccess; i0 += G) {
        const int n = std::min(G, num_images - i0);
        e = launch_render_group(c->Q, image_problem + i0, image_view + i0, n, vertices, c->render_nrm.as<double>(), c->nv, c->d_faces,
                                c->num_faces, points, points ? num_points : 0, height, width, images + (size_t)i0 * px * 3,
                                out + (size_t)i0 * px * 3, face_id ? face_id + (size_t)i0 * px : nullptr, c->render_ws.get(),
                                c->stream);
    }
    if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "render launch: %s", hipGetErrorString(e));
    return MVFIT_OK;
}

// utils.py:904-912 Renderer.colors in dictionary order
static const float SCENE_PALETTE[7][3] = {{.8f, .1f, .1f}, {.1f, .1f, .8f}, {.1f, .8f, .1f}, {.7f, .7f, .9f},
                                          {.9f, .9f, .8f}, {.7f, .75f, .5f}, {.5f, .7f, .75f}};

extern "C" int mvfit_render_scene(mvfit_ctx* c, const float* vertices, const float* points, int num_points, int num_images,
                                  const int32_t* image_first, const int32_t* body_problem, const int32_t* image_view,
                                  const float* body_color, int height, int width, const uint8_t* images, uint8_t* out,
                                  int32_t* face_id, int32_t* body_id) {
    if (!c) return MVFIT_E_ARG;
    if (!c->num_faces) return fail(c, MVFIT_E_STATE, "mvfit_render_scene: the model was created without (valid) faces");
    if (c->B == 0) return fail(c, MVFIT_E_STATE, "call mvfit_set_problems first (the cameras come from there)");
    if (!vertices || !images || !out || !image_first || !image_view || num_images < 1 || height < 1 || height > 8192 ||
        width < 1 || width > 8192 || num_points < 0 || num_points > 64)
        return fail(c, MVFIT_E_ARG, "mvfit_render_scene: bad argument (num_images=%d height=%d width=%d num_points=%d)",
                    num_images, height, width, num_points);
    if (image_first[0] != 0) return fail(c, MVFIT_E_ARG, "mvfit_render_scene: image_first[0] = %d, not 0", image_first[0]);
    for (int i = 0; i < num_images; ++i) {
        const long long cnt = (long long)image_first[i + 1] - image_first[i];
        if (cnt < 0) return fail(c, MVFIT_E_ARG, "mvfit_render_scene: image_first decreases at image %d", i);
        if (cnt > SCENE_BODIES_MAX)
            return fail(c, MVFIT_E_ARG, "mvfit_render_scene: image %d lists %lld bodies (at most %d)", i, cnt, SCENE_BODIES_MAX);
        if (image_view[i] < 0 || image_view[i] >= c->V)
            return fail(c, MVFIT_E_ARG, "mvfit_render_scene: image %d names view %d (V=%d)", i, image_view[i], c->V);
    }
    const int total = image_first[num_images];
    if (total > 0 && !body_problem) return fail(c, MVFIT_E_ARG, "mvfit_render_scene: body_problem is NULL");
    for (int j = 0; j < total; ++j) {
        if (body_problem[j] < 0 || body_problem[j] >= c->B)
            return fail(c, MVFIT_E_ARG, "mvfit_render_scene: body %d names problem %d (B=%d)", j, body_problem[j], c->B);
        if (body_color)
            for (int k = 0; k < 3; ++k)
                if (!(body_color[j * 3 + k] >= 0.f && body_color[j * 3 + k] <= 1.f))        // NaN fails both
                    return fail(c, MVFIT_E_ARG, "mvfit_render_scene: colour of body %d outside [0, 1]", j);
    }
    HIP_OK(c, hipSetDevice(c->device));
    // the call's tables, built in a pinned staging slot so that the copy to the device does not block the host
    const size_t tab_words = (size_t)num_images * SCENE_IMAGE_WORDS + (size_t)total * SCENE_INST_WORDS;
    const size_t tb = tab_words * sizeof(int32_t);
    const int slot = c->scene_slot;
    c->scene_slot ^= 1;
    if (c->scene_copied[slot]) HIP_OK(c, hipEventSynchronize(c->scene_copied[slot]));
    else HIP_OK(c, hipEventCreateWithFlags(&c->scene_copied[slot], hipEventDisableTiming));
    HIP_OK(c, c->h_scene_tab[slot].reserve(tb));
    int32_t* ti = c->h_scene_tab[slot].as<int32_t>();
    int32_t* tj = ti + (size_t)num_images * SCENE_IMAGE_WORDS;
    for (int i = 0; i < num_images; ++i) {
        const int first = image_first[i], cnt = image_first[i + 1] - first;
        ti[i * 4 + 0] = first; ti[i * 4 + 1] = cnt; ti[i * 4 + 2] = image_view[i];
        ti[i * 4 + 3] = cnt ? body_problem[first] : 0;
        for (int k = 0; k < cnt; ++k) {
            int32_t* r = tj + (size_t)(first + k) * SCENE_INST_WORDS;
            r[0] = body_problem[first + k]; r[1] = i; r[2] = k;
            const float* col = body_color ? body_color + (size_t)(first + k) * 3 : SCENE_PALETTE[k % 7];
            memcpy(r + 3, col, 12);
        }
    }
    // groups of consecutive images: at most RENDER_GROUP_MAX images and a workspace of at most 256 MB counting instances -
    // or one image's, when that alone needs more
    const size_t cap = (size_t)256 << 20;
    std::vector<int> group_end;
    size_t ws = 0;
    for (int i0 = 0; i0 < num_images;) {
        int i1 = i0 + 1;
        while (i1 < num_images && i1 - i0 < RENDER_GROUP_MAX &&
               scene_ws_bytes(i1 + 1 - i0, image_first[i1 + 1] - image_first[i0], c->nv, c->num_faces, height, width) <= cap)
            ++i1;
        ws = std::max(ws, scene_ws_bytes(i1 - i0, image_first[i1] - image_first[i0], c->nv, c->num_faces, height, width));
        group_end.push_back(i1);
        i0 = i1;
    }
    const size_t nb = (size_t)c->B * c->nv * 3 * sizeof(double);
    if (int rc = render_reserve(c, ws, nb)) return rc;
    if (tb > c->scene_tab.size()) HIP_OK(c, hipStreamSynchronize(c->stream));
    HIP_OK(c, c->scene_tab.reserve(tb));
    HIP_OK(c, hipMemcpyAsync(c->scene_tab.get(), ti, tb, hipMemcpyHostToDevice, c->stream));
    HIP_OK(c, hipEventRecord(c->scene_copied[slot], c->stream));
    hipError_t e = launch_render_normals(vertices, c->B, c->nv, c->d_faces, c->d_vf_ptr, c->d_vf_idx, c->render_nrm.as<double>(), c->stream);
    const size_t px = (size_t)height * width;
    int i0 = 0;
    for (size_t g = 0; g < group_end.size() && e == hipSuccess; ++g) {
        const int i1 = group_end[g], j0 = image_first[i0], m = image_first[i1] - j0;
        e = launch_scene_group(c->Q, c->scene_tab.as<int32_t>(), num_images, i0, i1 - i0, j0, m, vertices, c->render_nrm.as<double>(), c->nv, c->d_faces,
                               c->num_faces, points, points ? num_points : 0, height, width, images + (size_t)i0 * px * 3,
                               out + (size_t)i0 * px * 3, face_id ? face_id + (size_t)i0 * px : nullptr,
                               body_id ? body_id + (size_t)i0 * px : nullptr, c->render_ws.get(), c->stream);
        i0 = i1;
    }
    if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "render launch: %s", hipGetErrorString(e));
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

extern "C" int mvfit_lbfgs_kat(int device, int kind, int D, const int32_t* segs, int nseg, const mvfit_lbfgs_opts* o,
                               double* x_inout, double* trace, int max_trace, int* n_closure, double* final_loss) {
    if (!o || !x_inout || D <= 1 || D > LB_D || nseg < 1 || nseg > 8 || !segs) return MVFIT_E_ARG;
    if (!lb_opts_ok(*o)) return MVFIT_E_ARG;
    if (hipSetDevice(device) != hipSuccess) return MVFIT_E_HIP;
    LbOpts O = lb_opts(*o, 1);
    O.nseg = nseg;
    for (int i = 0; i < nseg; ++i) { O.seg_lo[i] = segs[i]; O.seg_hi[i] = segs[i + 1]; }
    double *dx, *dtrace, *dfl, *ddirs, *dstps, *dro, *dgrow, *dgcol, *dcmat;
    int* dn;
    const size_t tb = (size_t)std::max(max_trace, 1) * (D + 1) * 8;
    DevPool mem;                         // (every return frees what was allocated)
    if (mem.alloc(&dx, LB_D * 8) || mem.alloc(&dtrace, tb, true) || mem.alloc(&dfl, 8) || mem.alloc(&dn, 4) ||
        mem.alloc(&ddirs, LB_HIST * LB_D * 8, true) || mem.alloc(&dstps, LB_HIST * LB_D * 8, true) || mem.alloc(&dro, LB_HIST * 8) ||
        mem.alloc(&dgrow, LB_GSIZE * 8, true) || mem.alloc(&dgcol, LB_GSIZE * 8, true) || mem.alloc(&dcmat, 3 * LB_HIST * LB_HIST * 8, true))
        return MVFIT_E_HIP;
    hipMemcpy(dx, x_inout, D * 8, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(lbfgs_kat_kernel, dim3(1), dim3(64), 0, 0, kind, D, O, dx, dtrace, max_trace, dn, dfl, ddirs, dstps, dro,
                       dgrow, dgcol, dcmat);
    hipError_t e = hipDeviceSynchronize();
    hipMemcpy(x_inout, dx, D * 8, hipMemcpyDeviceToHost);
    if (trace && max_trace > 0) hipMemcpy(trace, dtrace, tb, hipMemcpyDeviceToHost);
    if (n_closure) hipMemcpy(n_closure, dn, 4, hipMemcpyDeviceToHost);
    if (final_loss) hipMemcpy(final_loss, dfl, 8, hipMemcpyDeviceToHost);
    return e == hipSuccess ? MVFIT_OK : MVFIT_E_HIP;
}
