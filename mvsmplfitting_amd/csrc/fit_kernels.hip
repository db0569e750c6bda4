// The optimiser kernels of libmvfit (one workgroup per problem, see closure_device.h / lbfgs_device.h) and their launchers
// (fit_kernels.h) - everything device-side that the host files mvfit_api.hip, mvfit_fit.hip and mvfit_scene.hip launch directly:
//   pack_obs_kernel, pack_joints3d_kernel   observations -> ObsBlock images
//   prep_kernel        params -> pose operands of the vertex pass
//   closure_kernel     one closure evaluation (loss, grad, keypoints) - the drop-in closure
//   joints_kernel      keypoints from the vertex buffer (mvfit_vertices)
//   fit_init_kernel    optimiser state of every problem at the start of a fit
//   fit_step_kernel    one closure round of the device-resident fit: objective + adjoint from the
//                      vertex-pass output, L-BFGS state-machine advance, pose operands of the next
//                      trial point
//   fit_persistent_kernel  the whole fit of one problem in a single launch: closures restricted to the vertices
//                      the objective reads, or full closures whose vertex passes run beside it (asynchronous fit:
//                      AsyncRing); optionally VPoser decoder helpers behind the problems' workgroups
//   fit_finish_kernel  optimiser state -> the caller's result arrays
//   lbfgs_kat_kernel   float64 instantiation of the state machine on analytic objectives
// One translation unit: g_dbg and g_lb_check (wave_ops.h, lbfgs_device.h) are per-file device variables, and the debug entry
// points at the end of this file read the copies these kernels write.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <utility>

#include "closure_device.h"
#include "fit_kernels.h"
namespace mvfit {

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
    FwdEarly ev;                                   // the sparse closure: waves 5-7 load their forward item in E1
    ev.wave = fwd_early_wave(L, from_pass == 0, tid);
    if constexpr (REMOTE) {
        pose_prep_decode_inl<true>(M, L, W.flags, tid);
        pose_prep_elems(M, L, W.flags, tid, ev);
    } else {
        pose_prep(M, L, W.flags, tid, ev);
    }
    sparse_forward(M, L, from_pass != 0, tid, true, ev);
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
    // (the single-launch kernel: its waves 5-7 carry their forward item from E1 into E2; the chained step kernel reads the
    // vertex pass's side outputs - from_pass - and has no forward stream)
    FwdEarly ev;
    ev.wave = fwd_early_wave(L, !from_pass && !have_pose, tid);
    if (!have_pose) {
        pose_prep_decode_inl<REMOTE>(M, L, W.flags, tid);
        pose_prep_elems(M, L, W.flags, tid, ev);
    }
    PH_T(0);
    sparse_forward(M, L, from_pass, tid, !have_pose, ev);
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
        if constexpr (COMPACT) lb_direction_compact<float, STEP_NT>(H, L.lbW, tid, lb_dir_forms(O));
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
    // the next problem of the batch, if the launch has a queue and this one has left it - finished, or paused at the stage
    // boundary of a lead phase (what the tail needs of a paused problem is stored below, before the row moves on; every row
    // pauses there, so a row that ended instead would leave the queue's problems without their lead stages).  The round cap
    // ends the workgroup.  Decided here, before the row says "nothing more comes"
    int b_next = -1;
    if (QUEUE && queue && (done || paused)) {                           // uniform
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
    } else if (kind == 3) {                                    // 'linear': c . x, unbounded below
        for (int i = 0; i < D; ++i) {
            const double c = 1.0 + (double)i / D;
            f += c * x[i]; g[i] = c;
        }
    } else if (kind == 4 || kind == 5) {                       // 'wavy' / 'wavy2': sum 0.5 x^2 + a sin(b x)
        const double a = kind == 4 ? 5.0 : 0.5, b = kind == 4 ? 7.0 : 3.0;
        for (int i = 0; i < D; ++i) {
            f += 0.5 * x[i] * x[i] + a * sin(b * x[i]);
            g[i] = x[i] + (a * b) * cos(b * x[i]);
        }
    } else if (kind == 6) {                                    // 'steep': -sum c x^4, unbounded below and ever steeper
        for (int i = 0; i < D; ++i) {
            const double c = 1.0 + (double)i / D, x2 = x[i] * x[i];
            f += -c * (x2 * x2); g[i] = -4.0 * c * (x2 * x[i]);
        }
    } else if (kind == 7) {                                    // 'steep2': -sum c |x|^(31/16), unbounded below, its slope growing ever slower
        for (int i = 0; i < D; ++i) {
            const double c = 1.0 + (double)i / D, r = sqrt(sqrt(sqrt(sqrt(fabs(x[i])))));
            f += -c * (x[i] * x[i] / r); g[i] = -1.9375 * c * (x[i] / r);
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
            if (compact) lb_direction_compact<double, 64>(H, W, lane, lb_dir_forms(O));
            else lb_direction_block<double, 64>(H, W, lane);
        });
        __syncthreads();
        if (S.status) break;
    }
#pragma unroll
    for (int e = 0; e < LB_EPL; ++e) if (LB_EPL * lane + e < D) x_io[LB_EPL * lane + e] = Vm[lane].x[e];
    if (lane == 0) *n_closure = ncl;
}

// ------------------------------------------------------------------ launchers (fit_kernels.h)
size_t step_lds() { return (sizeof(ClosureLds) + 15) & ~(size_t)15; }
size_t step_gram_lds() { return step_lds() + LB_GW_BYTES; }       // fit_step_kernel: + the staged Gram window
size_t persistent_lds(bool vp) { return std::max(persistent_lds_bytes(vp), sizeof(VpHelperLds)); }

// every instantiation of the single-launch kernel, by its PersistentVariant (fit_plan.h): the one place that ties the two
using PersistentKernel = decltype(&fit_persistent_kernel<false, false, false>);
static PersistentKernel persistent_kernel(PersistentVariant variant) {
    switch (variant) {
    case PV_PLAIN:         return fit_persistent_kernel<false, false, false>;
    case PV_LEAN:          return fit_persistent_kernel<false, false, true>;
    case PV_REUSE:         return fit_persistent_kernel<false, true, false>;
    case PV_REUSE_LEAN:    return fit_persistent_kernel<false, true, true>;
    case PV_HELPERS:       return fit_persistent_kernel<true, false, false>;
    case PV_HELPERS_REUSE: return fit_persistent_kernel<true, true, false>;
    case PV_QUEUE:         return fit_persistent_kernel<false, false, false, false, true>;
    case PV_QUEUE_LEAN:    return fit_persistent_kernel<false, false, true, false, true>;
    case PV_SDF:           return fit_persistent_kernel<false, false, false, true>;
    case PV_SDF_HELPERS:   return fit_persistent_kernel<true, false, false, true>;
    case PV_COUNT:         break;
    }
    return nullptr;
}

hipError_t fit_kernels_configure() {
    const int lds = (int)step_lds(), gram = (int)step_gram_lds(), pers = (int)std::max(persistent_lds(false), persistent_lds(true));
    const std::pair<const void*, int> fixed[] = {
        {reinterpret_cast<const void*>(prep_kernel), lds},
        {reinterpret_cast<const void*>(closure_kernel<false>), lds},
        {reinterpret_cast<const void*>(closure_kernel<true>), lds},
        {reinterpret_cast<const void*>(fit_init_kernel), lds},
        {reinterpret_cast<const void*>(fit_step_kernel<false>), gram},
        {reinterpret_cast<const void*>(fit_step_kernel<true>), gram},
    };
    for (const auto& k : fixed)
        if (hipError_t e = hipFuncSetAttribute(k.first, hipFuncAttributeMaxDynamicSharedMemorySize, k.second)) return e;
    for (int v = 0; v < PV_COUNT; ++v) {
        const PersistentKernel k = persistent_kernel((PersistentVariant)v);
        if (!k) return hipErrorInvalidDeviceFunction;          // a PersistentVariant without its case above: no ctx is created
        if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, pers)) return e;
    }
    return hipSuccess;
}

void launch_pack_obs(int B, hipStream_t stream, const DevProblems& Q, ObsBlock* obs) {
    hipLaunchKernelGGL(pack_obs_kernel, dim3(B), dim3(256), 0, stream, Q, obs);
}
void launch_pack_joints3d(int B, hipStream_t stream, const float* gt3d, const float* conf3d, ObsBlock* obs) {
    hipLaunchKernelGGL(pack_joints3d_kernel, dim3(B), dim3(64), 0, stream, gt3d, conf3d, obs);
}
void launch_prep(int B, hipStream_t stream, const DevModel& M, const ObsBlock* obs, const DevPose& P, const float* params,
                 uint32_t flags, float* full_pose) {
    hipLaunchKernelGGL(prep_kernel, dim3(B), dim3(STEP_NT), step_lds(), stream, M, obs, P, params, flags, full_pose);
}
void launch_closure(bool remote, int grid, hipStream_t stream, const DevModel& M, const ObsBlock* obs, int nviews, const DevWeights& W,
                    const DevPose& P, const float* params, int from_pass, float* loss, float* grad, float* joints,
                    const SdfAdj* sdf_adj) {
    hipLaunchKernelGGL(remote ? closure_kernel<true> : closure_kernel<false>, dim3(grid), dim3(STEP_NT), step_lds(), stream, M, obs,
                       nviews, W, P, params, from_pass, loss, grad, joints, sdf_adj);
}
void launch_joints(int B, hipStream_t stream, const DevModel& M, const float* verts, const float* Amat, const float* params,
                   float* joints) {
    hipLaunchKernelGGL(joints_kernel, dim3(B), dim3(64), 0, stream, M, verts, Amat, params, joints);
}
void launch_fit_init(int B, hipStream_t stream, const DevModel& M, const ObsBlock* obs, const DevPose& P, const FitBuffers& F,
                     const float* params, uint32_t flags, int publish) {
    hipLaunchKernelGGL(fit_init_kernel, dim3(B), dim3(STEP_NT), step_lds(), stream, M, obs, P, F, params, flags, publish);
}
void launch_fit_step(bool reuse, int B, hipStream_t stream, const DevModel& M, const ObsBlock* obs, int nviews, const StageWeights& SW,
                     const LbOpts& O, const DevPose& P, const FitBuffers& F) {
    hipLaunchKernelGGL(reuse ? fit_step_kernel<true> : fit_step_kernel<false>, dim3(B), dim3(STEP_NT), step_gram_lds(), stream, M, obs,
                       nviews, SW, O, P, F);
}
void launch_fit_persistent(PersistentVariant variant, int grid, hipStream_t stream, const DevModel& M, const ObsBlock* obs, int nviews,
                           const StageWeights& SW, const LbOpts& O, const DevPose& P, const FitBuffers& F, int max_rounds,
                           const AsyncRing& ring, int b_lo, int done_target, int pause_stage, int* queue, int b_end) {
    hipLaunchKernelGGL(persistent_kernel(variant), dim3(grid), dim3(STEP_NT), persistent_lds((SW.w[0].flags & MVFIT_F_VPOSER) != 0),
                       stream, M, obs, nviews, SW, O, P, F, max_rounds, ring, b_lo, done_target, pause_stage, queue, b_end);
}
void launch_fit_finish(int B, hipStream_t stream, const FitBuffers& F, float* params, float* final_loss, int32_t* n_closure,
                       int32_t* n_iter, int num_stages) {
    hipLaunchKernelGGL(fit_finish_kernel, dim3(B), dim3(128), 0, stream, F, params, final_loss, n_closure, n_iter, B, num_stages);
}
void launch_lbfgs_kat(int kind, int D, const LbOpts& O, double* x_io, double* trace, int max_trace, int* n_closure,
                      double* final_loss, double* dirs, double* stps, double* ro, double* grow, double* gcol, double* cmat) {
    hipLaunchKernelGGL(lbfgs_kat_kernel, dim3(1), dim3(64), 0, 0, kind, D, O, x_io, trace, max_trace, n_closure, final_loss, dirs, stps,
                       ro, grow, gcol, cmat);
}

}  // namespace mvfit

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
