/*
 * mvfit.h - C ABI of the MI355X-native multi-view SMPL fitting hot path.
 *
 * The reference (boycehbz/MvSMPLfitting) has no FFI on this path except the SDF op; its
 * seams are Python callables.  Each entry point below names the reference interface it
 * replaces (file:line relative to the reference root).  INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns 0 on success, a negative MVFIT_E_* code on failure, never throws;
 *     mvfit_last_error(ctx) returns a NUL-terminated message owned by the ctx.
 *   - a ctx is bound to one HIP device and one hipStream_t, is not thread-safe; different
 *     ctxs are independent.  Calls enqueue their work on the ctx stream and return; the ones that
 *     block until the device has finished are mvfit_create, mvfit_set_problems, mvfit_set_sdf,
 *     mvfit_sync, mvfit_destroy, the profiling readers and mvfit_fit (it watches the problems'
 *     completion to stop queueing rounds; its outputs are complete when it returns).
 *   - "dev|host" pointers may be either (copied with hipMemcpyDefault); "dev" pointers must be
 *     device memory (e.g. a torch CUDA tensor's data_ptr()); all arrays row-major float32
 *     unless noted.  Caller-owned; nothing is retained beyond the call except by
 *     mvfit_create, which copies (and re-tiles) the model constants into HBM.
 *   - flat parameter vector x[D], D = MVFIT_D = 86 + 32:  the reference's final_params order
 *     (code/utils/non_linear_solver.py:164-170, code/smplx/body_models_scale.py:202-268)
 *       betas[0:10] global_orient[10:13] body_pose[13:82] transl[82:85] scale[85]
 *       pose_embedding[86:118]
 *     With MVFIT_F_VPOSER the body_pose slots are ignored on input (decoded from the
 *     embedding) and receive zero gradient; without it the embedding slots are ignored.
 *     MVFIT_F_FIX_SHAPE / MVFIT_F_FIX_SCALE freeze betas / scale (gradient forced to 0:
 *     code/utils/init_guess.py:205-210).
 */
#ifndef MVFIT_H_
#define MVFIT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libmvfit.so is built with -fvisibility=hidden: the functions declared in this header are its only exports */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define MVFIT_NUM_JOINTS 24
#define MVFIT_NUM_BETAS 10
#define MVFIT_NUM_POSE_BASIS 207
#define MVFIT_NUM_KP 17
#define MVFIT_D 118          /* 86 model scalars + 32 latent */
#define MVFIT_D_MODEL 86
#define MVFIT_MAX_VIEWS 16
#define MVFIT_MAX_STAGES 8
#define MVFIT_HISTORY 100

/* error codes */
#define MVFIT_OK 0
#define MVFIT_E_ARG (-1)
#define MVFIT_E_HIP (-2)
#define MVFIT_E_STATE (-3)
#define MVFIT_E_UNSUPPORTED (-4)
#define MVFIT_ASSOC_MAX_DET 16      /* detections per view of a frame (the association op) */
#define MVFIT_SCENE_BODIES_MAX 256   /* bodies per scene (mvfit_render_scene images, mvfit_scene_sdf_loss scenes) */

/* flags (mvfit_weights.flags) */
#define MVFIT_F_VPOSER 1u      /* use_vposer: code/utils/fitting.py:166-168,327-329 */
#define MVFIT_F_PRIOR_GMM 2u   /* body_prior_type 'gmm' (code/prior.py:100-231) instead of 'l2' */
#define MVFIT_F_FIX_SHAPE 4u   /* fix_shape: code/utils/fitting.py:340, init_guess.py:208-210 */
#define MVFIT_F_FIX_SCALE 8u   /* fix_scale: init_guess.py:205-207 */
#define MVFIT_F_USE_3D 32u      /* use_3d: 3-D joint term (code/utils/fitting.py:319-324); needs mvfit_set_joints3d */
#define MVFIT_F_SPARSE_VERTS 16u /* evaluate only the vertices the objective reads (same loss /
                                    gradient; skips the full 6890-vertex pass inside the closure) */
#define MVFIT_F_REUSE_OUTER_VALUE 64u /* mvfit_fit only, opt-in, NOT the reference's closure count: LBFGS.step() opens with a
                                    closure call (lbfgs_ls.py:279-283) at the point the previous step() of the stage ended on;
                                    with this flag the optimiser feeds the loss / gradient it still holds instead of evaluating
                                    again - same iterates and eval accounting, 8-10 % fewer closure evaluations */

typedef struct mvfit_ctx mvfit_ctx;

/* Host-side description of the body model; replaces the buffers registered by
 * SMPL.__init__ (code/smplx/body_models_scale.py:197-305). */
typedef struct mvfit_model {
    int32_t num_verts;               /* 6890 */
    int32_t num_faces;               /* 13776 (0 if faces == NULL) */
    const float* v_template;         /* [Nv,3] */
    const float* shapedirs;          /* [Nv,3,10]   (beta index fastest) */
    const float* posedirs;           /* [207, Nv*3] (column = 3*vertex + coord) */
    const float* J_regressor;        /* [24,Nv] dense */
    const int32_t* parents;          /* [24], parents[0] = -1 */
    const float* lbs_weights;        /* [Nv,24] dense */
    const float* kp_regressor;       /* [14,Nv] dense ('smpllsp' joint_regressor, :283-286), or NULL: model_type 'smpl' */
    const int32_t* face_vertex_ids;  /* [5]  (code/smplx/vertex_joint_selector.py:38-43) */
    const int32_t* joint_map;        /* [17] indices into the model's joint tensor (code/utils/utils.py:444-457):
                                      *   with kp_regressor ('smpllsp', 'lsp14'): 0..13 regressor rows, 14..18 face vertices;
                                      *   kp_regressor NULL ('smpl', 'coco17'): 0..23 posed skeleton joints (the translation
                                      *   column of the chained transforms, lbs.py:316-370, + transl), 24..28 face vertices.
                                      * An entry outside its range: MVFIT_E_ARG. */
    const int32_t* faces;            /* [Nf,3] or NULL; kept on the device for mvfit_render_overlay */
    /* optional VPoser decoder (code/model/VPoser.py:188-195), NULL if unused */
    const float* vp_fc1_w; const float* vp_fc1_b;   /* [512,32],[512] */
    const float* vp_fc2_w; const float* vp_fc2_b;   /* [512,512],[512] */
    const float* vp_out_w; const float* vp_out_b;   /* [138,512],[138] */
    /* optional max-mixture prior (code/prior.py:135-160), gmm_M = 0 if unused */
    int32_t gmm_M;
    const float* gmm_means;          /* [M,69] */
    const float* gmm_precisions;     /* [M,69,69] */
    const float* gmm_nll_weights;    /* [M] */
} mvfit_model;

/* One stage's loss weights; replaces SMPLifyLoss.reset_loss_weights
 * (code/utils/fitting.py:270-280) + the per-stage dict of non_linear_solver.py:109-124,177-180. */
typedef struct mvfit_weights {
    float data_weight;           /* 500/H, enters squared (fitting.py:315) */
    float body_pose_weight;      /* enters squared (fitting.py:329,333,337) */
    float shape_weight;          /* enters squared (fitting.py:342) */
    float bending_prior_weight;  /* 3.17*body_pose_weight, NOT squared (fitting.py:348) */
    float coll_loss_weight;      /* SDF term (fitting.py:354,392); 0 = off */
    float rho;                   /* GMoF rho (code/utils/utils.py:427-438) */
    uint32_t flags;              /* MVFIT_F_* */
} mvfit_weights;

/* Optimiser settings; replaces create_optimizer(..., 'lbfgsls') (code/optimizers/optim_factory.py:50-52,
 * lbfgs_ls.py:199-207) and FittingMonitor(maxiters, ftol, gtol) (code/utils/fitting.py:38-47). */
typedef struct mvfit_lbfgs_opts {
    float lr;                /* 1.0 */
    int32_t max_iter;        /* 30 (max_eval = max_iter*5/4) */
    int32_t history;         /* <= MVFIT_HISTORY (100) */
    float tolerance_grad;    /* 1e-5 */
    float tolerance_change;  /* 1e-9 */
    int32_t maxiters;        /* outer run_fitting iterations, 30 */
    float ftol;              /* 1e-9 */
    float gtol;              /* 1e-9 */
    int32_t num_stages;      /* <= MVFIT_MAX_STAGES */
    int32_t max_rounds;      /* safety cap on closure rounds per call (0 = no cap) */
} mvfit_lbfgs_opts;

/* SMPL.__init__ + .to(device) (body_models_scale.py:98-305, code/init.py:143-151): copies and
 * re-tiles the constants into HBM.  hip_stream may be NULL (default stream). */
/* Precision and path selectors of a ctx.  The released library reads NO environment variable: what used to be MVFIT_*
 * switches are fields here (mvfit_options_default fills the defaults; mvfit_create(...) = mvfit_create_ex(..., NULL) = the
 * defaults).  The first group decides what mvfit_create_ex uploads and is fixed for the ctx's life; the second group may be
 * changed between calls with mvfit_set_options. */
#define MVFIT_CONTRACTION_SPLIT_FP16 0   /* default: every fp32 product of the blendshape contraction as error-compensated
                                          * split-fp16 pairs on the fp16 matrix pipe, fp32 accumulate (5e-7 from float64) */
#define MVFIT_CONTRACTION_EXACT_FP32 1   /* the contraction as an exact fp32 MFMA chain (bitwise an fmaf chain) */
#define MVFIT_CONTRACTION_HALF_BASIS 2   /* BASELINE configs[4], half-width blendshape operands: only the fp16 hi halves of the
                                          * basis are streamed (2 bytes per element; vertices within ~2e-5 of the fp32 result) */
typedef struct mvfit_options {
    uint32_t struct_size;            /* sizeof(mvfit_options) of the caller */
    /* ---- fixed at mvfit_create_ex ---- */
    int32_t contraction;             /* MVFIT_CONTRACTION_* */
    int32_t dense_skinning;          /* 1: the dense 24-column skinning blend even when every vertex has <= 4 weights (0) */
    /* ---- mvfit_set_options ---- */
    int32_t round_mode;              /* 0: automatic (asynchronous single-launch fit wherever the objective allows);
                                      * 1: chained rounds always (vertex pass -> step kernel per closure round) */
    int32_t resident_pass;           /* vertex passes of the asynchronous fit: -1 automatic (resident when its workgroups fit
                                      * next to the optimiser's), 0 a gate + a pass launch per closure round, 1 / 2 resident with
                                      * that many vertex tiles per workgroup, 3 resident with two tiles per workgroup and the
                                      * workgroup split into contraction and worker waves (a forced value that does not fit
                                      * stalls the fit; round 6: forms 1 and 3 are the automatic choices - 216 workgroups beside
                                      * <= 36 optimiser workgroups, 108 beside <= 144 -, form 2 was dropped: it maps to 3).
                                      * The resident pass assumes what the path's deployment gives it - one process per GPU
                                      * (SURVEY 8(e)): a fit's ~250 workgroups are resident together.  Processes (or concurrent
                                      * ctxs) that SHARE a device should set 0: waiting for one another's CUs they would exhaust
                                      * the ring's patience (20 ms) and lose passes - counted by mvfit_fit_stats, never silent,
                                      * and without effect on the fitted parameters */
    int32_t sdf_two_phase;           /* 1 (default): a fit with the SDF term runs its leading coll_loss_weight == 0 stages
                                      * asynchronously and hands over to chained rounds; 0: chained rounds in every stage */
    int32_t sdf_face_lists;          /* 1 (default): long face lists are culled exactly on per-round face lists (bit-identical
                                      * to the walk); 0: the walk over every face for every vertex / voxel */
    int32_t vposer_helpers;          /* 1 (default): the single-launch fits decode VPoser on helper workgroups; 0: in the
                                      * problems' own workgroups (another summation order: last-bit differences) */
    int32_t vposer_sets;             /* 0: automatic (16 sets for <= 32 problems, else 8; asynchronous fits take 8 where 16 would
                                      * leave no CUs for the resident vertex pass); n: helper sets of a launch (clamped to what
                                      * the problems need / fit).  Results do not depend on it */
    int32_t closure_vposer_helpers;  /* 1: mvfit_closure (MVFIT_F_VPOSER, no SDF term, B <= 160) decodes on helper workgroups
                                      * of its own launch - the decoder arithmetic of the fits, for parity tests (0) */
    int32_t pass_kernel;             /* per-round launch kernels at more than 32 problems: 0 automatic (two-role pipeline; dense
                                      * skinning rows: the lock-step chunk loop; <= 4 weights per vertex and an odd num_verts: as
                                      * 1), 1 one workgroup per (tile, chunk); 2 = 0 (the lock-step loop for <= 4 weights per
                                      * vertex was dropped in round 6).  The vertices do not depend on it, bit for bit */
    int32_t sdf_service;             /* 1 (default): in a two-phase fit (sdf_two_phase) the stages WITH the SDF term also run in the
                                      * single-launch optimiser kernel, which asks for the term every closure round - gate ->
                                      * vertex pass -> term kernels per round on the pass stream, the pull-back answers through
                                      * memory (fitting.py:352-393 unchanged: the same kernels compute the same S and adjoint);
                                      * 0: those stages as chained rounds (pass -> term -> step kernel launch per round) */
    int32_t work_queue;              /* 1 (default): an asynchronous fit of more problems than optimiser workgroups (128 beside the
                                      * resident vertex pass) is ONE launch whose workgroups take the next unfitted problem when
                                      * theirs has finished; 0: sub-batches one after the other.  A problem's result does not depend
                                      * on it (problems are independent) */
} mvfit_options;
void mvfit_options_default(mvfit_options* opts);

/* Error contract: MVFIT_E_ARG for a null / incomplete model leaves *out = NULL.  Any later failure (unsupported
 * model, device allocation) still stores a ctx in *out: it carries the message (mvfit_last_error) and owns whatever
 * was allocated so far - release it with mvfit_destroy, it is not usable for anything else. */
int mvfit_create(mvfit_ctx** out, int device, void* hip_stream, const mvfit_model* model);
/* mvfit_create with explicit options (NULL = defaults).  MVFIT_E_ARG for an unknown selector value. */
int mvfit_create_ex(mvfit_ctx** out, int device, void* hip_stream, const mvfit_model* model, const mvfit_options* opts);
/* Change the second group of options between calls; the first group must equal what the ctx was created with
 * (MVFIT_E_ARG otherwise).  mvfit_get_options returns what is in force. */
int mvfit_set_options(mvfit_ctx* ctx, const mvfit_options* opts);
int mvfit_get_options(const mvfit_ctx* ctx, mvfit_options* opts);
/* Which path served the last mvfit_sdf call (*op_path) and the SDF term of the last mvfit_fit / mvfit_closure (*term_path):
 * 0 the walk over every face (short face list, or sdf_face_lists = 0), 1 face lists, 2 the walk because the lists'
 * workspace (11.6 MB per problem at 13,776 faces) did not fit in half of the free device memory - decided once per shape
 * and remembered, a ~10x slower path that is never taken silently: the Python adapter warns. */
int mvfit_sdf_info(const mvfit_ctx* ctx, int* op_path, int* term_path);
void mvfit_destroy(mvfit_ctx* ctx);
const char* mvfit_last_error(const mvfit_ctx* ctx);
int mvfit_sync(mvfit_ctx* ctx);

/* The per-frame inputs of create_fitting_closure (code/utils/fitting.py:144-156; shapes from
 * non_linear_solver.py:77-84, code/init.py:112-131):
 *   cameras: cam_batched = 0 -> one rig [V,...] shared by all problems; 1 -> [B,V,...].
 *   gt_xy[B,V,17,2] ; w_conf[B,V,17] = joint_weights * conf (0 for missing views, main.py:49-57).
 * B = number of independent (subject x frame) problems. */
int mvfit_set_problems(mvfit_ctx* ctx, int B, int V, int cam_batched,
                       const float* cam_R /*[.,V,3,3] dev|host*/, const float* cam_t /*[.,V,3]*/,
                       const float* cam_f /*[.,V]*/, const float* cam_c /*[.,V,2]*/,
                       const float* gt_xy /*dev|host*/, const float* w_conf /*dev|host*/);

/* Optional 3-D joint targets of the use_3d term (code/utils/non_linear_solver.py:86-99):
 * gt3d[B,17,3], conf3d[B,17] (dev|host).  Call after mvfit_set_problems (which clears them). */
int mvfit_set_joints3d(mvfit_ctx* ctx, const float* gt3d, const float* conf3d);

/* One closure evaluation for all B problems: fitting_func(backward=True)
 * (code/utils/fitting.py:162-203) = SMPL.forward + SMPLifyLoss.forward + backward.
 *   params[B,MVFIT_D] dev ; loss[B] dev ; grad[B,MVFIT_D] dev or NULL (forward only) ;
 *   verts[B,Nv,3] dev or NULL ; joints[B,17,3] dev or NULL.
 * mvfit_options::closure_vposer_helpers = 1 (with MVFIT_F_VPOSER, no SDF term, B <= 160) decodes the body pose on helper
 * workgroups of the closure's own launch - the decoder arithmetic of the single-launch fits (another summation order than
 * the in-workgroup decoder, ~1e-7 relative) - so that the parity tests can hold the shipping decoder against the
 * closure-level goldens (tests/test_gpu_closure_helpers.py); mvfit_decoder_stats reports that launch. */
int mvfit_closure(mvfit_ctx* ctx, const mvfit_weights* w, const float* params,
                  float* loss, float* grad, float* verts, float* joints);

/* ModelOutput.full_pose of SMPL.forward (body_models_scale.py:392-412): [B,72] = global_orient | body_pose, the body pose
 * decoded from the embedding with MVFIT_F_VPOSER (fitting.py:170-173, VPoser.decode 'aa') - what the reference's
 * save_results stores as 'pose' / 'body_pose' (code/utils/utils.py:744-766).  params[B,MVFIT_D] dev, full_pose[B,72] dev. */
int mvfit_full_pose(mvfit_ctx* ctx, const float* params, uint32_t flags, float* full_pose);

/* SMPL.forward only (body_models_scale.py:327-412): vertices (+transl) and the 17 keypoints. */
int mvfit_vertices(mvfit_ctx* ctx, const float* params /*[B,MVFIT_D] dev*/, uint32_t flags,
                   float* verts /*[B,Nv,3] dev*/, float* joints /*[B,17,3] dev or NULL*/);

/* Reverse mode of mvfit_vertices: the vector-Jacobian product of (vertices, joints) at params.
 *   g_verts[B,Nv,3] dev or NULL, g_joints[B,17,3] dev or NULL (NULL = zero cotangent);
 *   g_params[B,MVFIT_D] dev, overwritten.
 * flags as mvfit_vertices: MVFIT_F_VPOSER -> gradient in the embedding slots [86:118], body_pose slots 0
 * (otherwise the embedding slots are 0); MVFIT_F_FIX_SHAPE / MVFIT_F_FIX_SCALE zero those slots as in
 * mvfit_closure; the other bits have no effect. Needs mvfit_set_problems (for B) like mvfit_vertices.
 * The result is the gradient of exactly what mvfit_vertices returns (vertices and keypoints both include transl; the root
 * transform carries the scale, Rm[0] = s R[0]), for either model kind and skinning form.  It is the adjoint of the fp32
 * model in every contraction mode: with MVFIT_CONTRACTION_HALF_BASIS the forward is the approximation, not this.
 * Deterministic: no float atomics, every sum in a fixed order; a problem's gradient does not depend on B, its position
 * in the batch or the call.  The workspace is allocated by the first call with g_verts and grows with B. */
int mvfit_vertices_backward(mvfit_ctx* ctx, const float* params, uint32_t flags,
                            const float* g_verts, const float* g_joints, float* g_params);

/* The whole staged fit, device resident: for each stage (non_linear_solver.py:156-211) a fresh
 * LBFGS (lbfgs_ls.py:256-445, strong-Wolfe :39-167) driven by run_fitting (fitting.py:99-142),
 * every problem advancing its own state machine, no host synchronisation per closure.
 *   params[B,MVFIT_D] dev, in/out ; stage_weights[num_stages] host ;
 *   final_loss[B] dev (run_fitting's return of the last stage; NaN where the reference returns None)
 *   n_closure[B], n_iter[B] dev int32 (closure evaluations / L-BFGS iterations spent), may be NULL.
 * The vertices of the trial points (the reference's return_verts=True) are computed per closure round into an internal
 * buffer and are NOT an output of this call - mvfit_vertices(params) gives the vertices of the result.  In the
 * asynchronous mode (the default; with the SDF term: for the stages whose coll_loss_weight is 0) those per-round passes
 * run beside the optimiser and nothing of the result depends on them; mvfit_fit_stats reports how many ran and whether
 * any was lost (none: the operand ring has back-pressure).  Any number of problems: batches beyond what is resident at
 * once are fitted in sub-batches, a problem's result does not depend on the slicing. */
int mvfit_fit(mvfit_ctx* ctx, const mvfit_weights* stage_weights, const mvfit_lbfgs_opts* opts,
              float* params, float* final_loss, int32_t* n_closure, int32_t* n_iter);

/* Counters of the vertex passes of the last mvfit_fit in its asynchronous mode (all zero in the other modes):
 *   out4[0]  chunk passes (32 problems x 6890 vertices) run;
 *   out4[1]  chunk passes skipped because all their problems had finished;
 *   out4[2]  pose operands lost (expected 0): per-round launches - (problem, round) operand sets overwritten before their pass
 *            read them; resident pass - the LARGEST number of (problem, round) operand sets any one of its workgroups found
 *            overwritten (every workgroup reports; such a round is skipped by that workgroup, never computed from another
 *            round's operands);
 *   out4[3]  waits given up (expected 0): gate kernels that waited 3 ms and resident workgroups that waited 20 ms for operands
 *            and left + problems whose optimiser waited 20 ms for the ring's back-pressure and stopped honouring it + service
 *            rounds (SDF term, mvfit_options::sdf_service) whose problem waited 200 ms for the term's answer - once per problem:
 *            its later rounds do not wait again (mvfit_fit then fails).
 * A non-zero out4[2] or out4[3] means "every closure round got its full vertex pass" does not hold for that fit (the fitted
 * parameters never depend on the passes); with mvfit_options::resident_pass = -1 the ctx then runs its later fits with
 * per-round launches (until mvfit_set_options is called). */
int mvfit_fit_stats(mvfit_ctx* ctx, uint32_t* out4);

/* Counters of the decoder helpers of the last mvfit_fit.  With MVFIT_F_VPOSER the single-launch fits (asynchronous and
 * objective-vertices-only) run the VPoser decoder's layers (VPoser.py:218-232) on helper workgroups of the same launch
 * that keep the weights in registers (csrc/vposer_service.h; mvfit_options::vposer_helpers = 0 keeps them in the
 * problems' own workgroups):
 * out3 = { launches that carried helpers, answers that did not arrive within 50 ms (expected 0: that problem decodes
 * locally from then on), helpers that gave up after 0.2 s without a request (expected 0) }.  Waits for the ctx stream. */
int mvfit_decoder_stats(mvfit_ctx* ctx, uint32_t* out3);

/* Test hook for the asynchronous fit: the vertex pass that belongs to closure round `round` (0-based, of every
 * problem) writes its vertices to verts[B,Nv,3] (dev) instead of the internal buffer; together with mvfit_fit_trace
 * (the trial points) this lets a test check that the pass of round r really computed the trial point of round r.
 * verts = NULL switches it off.  The buffer is sized for the CURRENT batch: mvfit_set_problems with another B (or V)
 * switches the hook off. */
int mvfit_debug_capture_pass(mvfit_ctx* ctx, int round, float* verts);

/* Optional closure trace of the NEXT mvfit_fit calls (test / debugging hook; the reference equivalent is printing
 * inside fitting_func): for every problem the first max_closures closure evaluations are recorded as
 *   trace[b][k][0:MVFIT_D] = the trial point the closure was evaluated at, trace[b][k][MVFIT_D] = its loss.
 * trace[B, max_closures, MVFIT_D + 1] dev, caller-owned, must stay valid until tracing is switched off with
 * mvfit_fit_trace(ctx, NULL, 0) (or the ctx is destroyed).  Rows beyond a problem's closure count are not written.
 * The buffer is sized for the CURRENT batch: mvfit_set_problems with another B (or V) switches tracing off. */
int mvfit_fit_trace(mvfit_ctx* ctx, float* trace, int max_closures);

/* The SDF voxelisation op (reference sdf/sdf/sdf.py:21-26 -> sdf_cuda.cpp:14-28 -> sdf_cuda_kernel.cu:242-335):
 *   faces[num_faces,3] int32 dev ; vertices[B,num_vertices,3] dev, coordinates in [-1,1] ; phi[B,G,G,G] dev out
 *   (phi[b,k,j,i]: i fastest = x).  num_faces is the caller's faces.size(0), exactly as the reference launcher
 *   takes it (sdf_cuda_kernel.cu:314; the reference's own call site passes a [1,F,3] tensor, i.e. ONE triangle).
 * Stand-alone op; the loss term below evaluates the same voxel function without materialising phi.
 * Face lists of 512 faces and more are voxelised on per-call face lists (exact culling: the same bits as the walk
 * over every face for every voxel, which mvfit_options::sdf_face_lists = 0 keeps; the workspace, 11.6 MB per batch
 * element at 13,776 faces, is kept in the ctx between calls of one shape). */
int mvfit_sdf(mvfit_ctx* ctx, const int32_t* faces, int num_faces, const float* vertices, int B,
              int num_vertices, int G, float* phi);

/* The interpenetration term of SMPLifyLoss.forward (code/utils/fitting.py:352-393, boxes :282-288):
 *   pen = (coll_loss_weight * sum_v grid_sample(phi, (v - c) / s))^2,  phi = SDF(faces, (v - c) / s, grid_size)
 * switched on for mvfit_closure / mvfit_fit whenever a weight set has coll_loss_weight > 0 (fitting.py:354).
 *   faces[num_faces,3] int32 (host or device), copied; num_faces = what the reference's call site makes the
 *   op see: it passes body_model_faces.reshape(1, -1, 3) (fitting.py:367-368), so the op's faces.size(0)
 *   is 1 and only the FIRST triangle is voxelised - pass num_faces = 1 for the reference's behaviour, the
 *   full face count for the behaviour its author presumably intended.  grid_size: 128 in the reference (:368).
 *   faces = NULL or num_faces = 0 removes the term.
 * Every problem is one person (the reference asserts batch size 1, :366): boxes, phi and the sum are per problem.
 * The term reads all vertices, so MVFIT_F_SPARSE_VERTS is ignored while it is active.
 * With 512 faces and more the sampled corners take their values from per-round face lists (same bits as the walk over
 * every face; mvfit_options::sdf_face_lists = 0 keeps the walk; a batch whose workspace would not fit in half of the free
 * memory keeps it too - mvfit_sdf_info says which path ran). */
int mvfit_set_sdf(mvfit_ctx* ctx, const int32_t* faces, int num_faces, int grid_size);

/* Diagnostics of the last evaluated interpenetration term (after mvfit_closure with coll_loss_weight > 0):
 *   samples[B,num_verts,4] dev out = (phi_v, d phi_v / d local x, y, z) per vertex (may be NULL),
 *   sums[B] dev out = S = sum_v phi_v (may be NULL). */
int mvfit_sdf_term_read(mvfit_ctx* ctx, float* samples, float* sums);

/* Scene collision loss: SDFLoss.forward (reference sdf/sdf/sdf_loss.py:51-99) for num_scenes scenes in one call.
 *   vertices[N,num_vertices,3] dev: translation already added; bodies scene_first[s] .. scene_first[s+1]-1 form scene s
 *   faces[num_faces,3] int32 dev, shared by all bodies; scene_first[num_scenes+1] host, scene_first[0]=0, non-decreasing,
 *   1 .. MVFIT_SCENE_BODIES_MAX bodies per scene; 2 <= grid_size <= 128; robustifier <= 0: none.
 *   loss[num_scenes] dev out; g_vertices[N,num_vertices,3] dev out or NULL = d loss[s] / d vertices (cotangent 1 per scene);
 *   phi_out[N,G,G,G] dev out or NULL (diagnostics: the fields the samples were taken from).
 * Per scene of P bodies: box of body i = (centre c_i, scale s_i = float32((1 + scale_factor) / 2) * largest extent), no
 * gradient; phi_i = the voxel function of the SDF op above on (v_i - c_i) / s_i over ALL num_faces faces; for i != j and
 * every vertex v of body j, p = grid_sample(phi_i, (v - c_i) / s_i) (trilinear, zeros padding, align_corners = False),
 * with a robustifier r: p <- (p/r)^2 / ((p/r)^2 + 1); loss = sum p / P^2.  A scene of one body gives 0.
 * The reference's isolation filter is reproduced as it EXECUTES: its mask is the bitwise complement of a uint8 tensor,
 * never zero, so every body is kept and the divisor is P^2 even when a body is far from the others.
 * Deterministic: fixed-order sums, no atomics; a scene's loss and gradient do not depend on the other scenes of the call.
 * Needs no set_problems call.  The face indices are checked on the host in every call (one stream synchronisation);
 * the op's path (face lists from 512 faces on) is reported by the info call of the SDF op.
 * MVFIT_E_ARG: a null vertices / faces / scene_first / loss, scene_first[0] != 0 or decreasing, an empty scene, a scene
 * of more than MVFIT_SCENE_BODIES_MAX bodies, grid_size out of range, a face index outside [0, num_vertices). */
int mvfit_scene_sdf_loss(mvfit_ctx* ctx, const float* vertices, int num_vertices, const int32_t* faces, int num_faces,
                         const int32_t* scene_first, int num_scenes, int grid_size, float scale_factor, float robustifier,
                         float* loss, float* g_vertices, float* phi_out);

/* The collision term of a fit against the other bodies of a scene, with their fields FROZEN: the B problems of the ctx are
 * partitioned into num_scenes scenes, contiguous in problem order (scene_first as above, and scene_first[num_scenes] = B).
 *   vertices[B,num_verts,3] dev, world: where the obstacles are frozen.  For every body i the call stores its box
 *   (c_i, s_i) and its field phi_i exactly as mvfit_scene_sdf_loss computes them over the model's own faces (the same
 *   kernels: bit-identical to that op's phi_out).  vertices = NULL removes the obstacles.
 * While they are set, a weight set with coll_loss_weight > 0 adds to problem j
 *   pen_j = (coll_loss_weight * S_j)^2,  S_j = sum_{i != j in j's scene} sum_{v of j} rho(grid_sample(phi_i, (v - c_i) / s_i))
 * (sampling and robustifier rho as in mvfit_scene_sdf_loss; no 1/P^2 - the weight absorbs it).  The fields and boxes carry no
 * gradient, as in the reference's SDFLoss: the gradient flows through the sampled positions of body j only.  At the freeze
 * point sum_j S_j / P^2 is the scene's loss of mvfit_scene_sdf_loss and d S_j / d v_j is P^2 times its g_vertices[j].  A
 * scene of one body, or a body out of reach of every field, pays nothing.  A problem's numbers do not depend on B, on its
 * position in the batch or on the other scenes.
 * mvfit_fit runs the stages that carry this term as chained rounds (pass -> scene entries -> pull-back -> step kernel);
 * stages without it in front keep their single-launch phase.  mvfit_sdf_term_read returns S_j in sums; samples:
 * MVFIT_E_UNSUPPORTED.  Call again to re-freeze: for an unchanged (B, grid_size) the buffers keep their addresses and the
 * captured round graph stays valid.  mvfit_set_problems with another B removes the obstacles.
 * One interpenetration term per ctx: MVFIT_E_STATE while mvfit_set_sdf's term is configured (and mvfit_set_sdf returns it
 * while obstacles are set).  MVFIT_E_STATE also without mvfit_set_problems or for a model without faces; MVFIT_E_ARG for a
 * scene_first that mvfit_scene_sdf_loss would refuse or that does not end at B, or a grid_size outside [2, 128]. */
int mvfit_set_scene_obstacles(mvfit_ctx* ctx, const float* vertices, const int32_t* scene_first, int num_scenes,
                              int grid_size, float scale_factor, float robustifier);

/* Diagnostics: the frozen obstacles.  phi[B,G,G,G] dev out (may be NULL), boxes[B,4] dev out = (c_i, s_i) (may be NULL).
 * MVFIT_E_STATE when no obstacles are set. */
int mvfit_scene_obstacles_read(mvfit_ctx* ctx, float* phi, float* boxes);

/* ---- Silhouette loss against per-view person masks, with its gradient on the vertices (csrc/silhouette.hip).  The reference
 * has no term on the body's outline: this contract is the project's own.
 *
 * Images.  M mask images, all H x W (2 <= H, W <= 8192, M <= 65535).  Image i shows body image_body[i] through its own
 * pinhole camera (R_i, t_i, f_i, c_i) - given per image, not taken from mvfit_set_problems.  A body may have any number of
 * images, none included.  A mask pixel is "on" when its byte is non-zero.
 *
 * mvfit_set_silhouettes prepares, once per mask set:
 *   Field D_i[H,W] float32: d2 = the exact integer squared Euclidean distance, in pixels, from the pixel to the nearest on
 *     pixel (0 on the mask), computed in integer arithmetic; D = float32(sqrt(float64(d2))) - what
 *     scipy.ndimage.distance_transform_edt(mask == 0) gives, cast to float32.  An image with no on pixel is ignored by both
 *     terms, its field reads back as zeros and it has no contour points; an all-on image has field 0 and no contour.
 *   Contour of image i: the on pixels with at least one 4-neighbour that lies inside the image and is off (a mask running
 *     into the image border is a person cut by the frame, not an outline), in raster order; the k-th of them is kept iff
 *     k % contour_stride == 0.  Stored as CSR contour_first[M+1] over the kept points and contour_xy[C,2] int32 (x, y).
 *   The call waits for the stream (the contour sizes come back to the host); every other entry is asynchronous.
 *
 * mvfit_silhouette_loss evaluates at vertices[N,Nv,3] float32 (translation included, as mvfit_vertices returns them; Nv is
 * the model's):
 *   Projection, the rasteriser's fp32 sequence without contraction: p = ((R0 X + R1 Y) + R2 Z) + t, u = f (px / pz) + cx,
 *     v = f (py / pz) + cy.  A vertex is valid in image i iff pz > 0.05; an invalid one contributes to neither term.
 *   Term A (body inside mask).  Pixel-index coordinates x = u - 0.5, y = v - 0.5 (pixel (x, y) has its centre at
 *     (x + .5, y + .5), as the rasteriser); xc = min(max(x, 0), W-1), x0 = min(int(floorf(xc)), W-2), a = xc - x0 in fp32,
 *     likewise yc, y0, b.  In float64 from the fp32 a, b and the four field values:
 *     d = (1-b)((1-a) D00 + a D01) + b((1-a) D10 + a D11); dd/dx = (1-b)(D01-D00) + b(D11-D10) if x == xc, else 0, likewise
 *     dd/dy.  rho_A = d^2 when sigma <= 0, else sigma^2 d^2 / (sigma^2 + d^2) (the data term's GMoF form).
 *     A_i = sum_j rho_A.
 *   Term B (mask covered by body).  For a kept contour point with centre c = (x + .5, y + .5) and a valid vertex j:
 *     dx = u_j - cx, dy = v_j - cy, m_j = dx*dx + dy*dy, products and sum each rounded to fp32.  The winner is the valid j
 *     with the smallest m_j, ties to the lowest j; with no valid vertex the winner is -1 and the point contributes 0.
 *     rho_B = m when sigma <= 0, else sigma^2 m / (sigma^2 + m), in float64 from the fp32 m.
 *     B_i = contour_stride * sum_k rho_B; the gradient goes to the winner only: contour_stride * rho_B'(m) * 2 (dx, dy) in
 *     pixel space.  Term B measures the distance to the nearest projected vertex, not to the outline polygon.
 *   loss[n] = sum over the images of body n, in ascending image index, of (w_in A_i + w_out B_i), accumulated in float64,
 *     output float32.  g_vertices[n,j,:] = the pull-back of both terms through the projection (du/dp = (f/pz) [1, 0, -px/pz],
 *     dv/dp likewise, then R^T), summed in float64 over the body's images in ascending order and rounded to float32 once.
 *     The gradient flows through the vertex positions only: field, contour and winners are constants.
 *   Determinism: no float atomics; a body's loss and gradient are bit-identical alone, in any batch, at any position and from
 *     run to run; a body with no images gets loss 0 and an exactly zero gradient.  Term B's many-points-to-one-vertex sum is
 *     a 64-bit integer accumulation in units of 2^-28 pixel (each point's contribution is rounded to that unit; the sum of
 *     one vertex in one image must stay below 2^35 pixels in magnitude).
 *
 * masks[M,H,W] uint8 dev or host; image_body[M], cam_R[M,3,3], cam_t[M,3], cam_f[M], cam_c[M,2] host.  num_images = 0 clears
 * the mask set (the other arguments are ignored).  loss[N] dev out; g_vertices[N,Nv,3] dev out or NULL; winner[C] int32 dev
 * out or NULL (diagnostics: the winner of every kept contour point).
 * Workspace, kept in the ctx and reused by a second set of the same sizes:
 *     M H W * 5 + M H * 4 + M * (16 Nv + 8 ceil(Nv / 256) + 92) + 8   bytes   (field 4 H W and a copy of the mask H W per
 *     image, row offsets, the fixed-point accumulators, term A's partials, tables), each part rounded up to 256 bytes, plus
 *     C * 8 + ceil-sum(C_i / 512) * 24 bytes for the contour list, the search's chunk table and term B's partials (grows to
 *     the largest set seen).
 * MVFIT_E_ARG: sizes out of range, contour_stride < 1, a NULL required pointer, num_bodies outside [1, 65535], an
 * image_body[i] outside [0, num_bodies) (checked at loss time).  MVFIT_E_STATE: no mask set is present.
 * MVFIT_E_UNSUPPORTED: more than 2^31 - 1 kept contour points. */
int mvfit_set_silhouettes(mvfit_ctx* ctx, int num_images, int height, int width, const uint8_t* masks,
                          const int32_t* image_body, const float* cam_R, const float* cam_t, const float* cam_f,
                          const float* cam_c, int contour_stride);
/* field[M,H,W] dev out or NULL, contour_first[M+1] dev out or NULL, contour_xy[C,2] dev out or NULL, num_points host out (C;
 * known when the set returns, so a caller reads it first and sizes contour_xy). */
int mvfit_silhouettes_read(mvfit_ctx* ctx, float* field, int32_t* contour_first, int32_t* contour_xy, int32_t* num_points);
int mvfit_silhouette_loss(mvfit_ctx* ctx, const float* vertices, int num_bodies, float w_in, float w_out, float sigma,
                          float* loss, float* g_vertices, int32_t* winner);

/* The silhouette loss as a term of the fit, over the ctx's current mask set (enable != 0; enable = 0 switches it off and
 * ignores the other arguments).  While it is on, a weight set with coll_loss_weight > 0 adds to problem j
 *   pen_j = coll_loss_weight^2 * L_j,
 * L_j exactly loss[j] of mvfit_silhouette_loss(vertices of the trial point, num_bodies = B, w_in, w_out, sigma):
 * image_body[i] is the problem index.  The term is linear in L; the weight enters squared like every other weight of
 * mvfit_weights.  Its gradient is coll_loss_weight^2 times the pull-back of that call's g_vertices through the fp32 model to
 * the parameters (the adjoint mvfit_vertices_backward computes); field, contour and winners are constants, as in the op, and
 * the winners are searched anew at every trial point.  A problem with no image pays exactly 0: its loss and gradient have the
 * bits they have without the term.  A problem's numbers do not depend on B, on its position in the batch or on the other
 * problems' masks.
 * mvfit_closure and mvfit_fit both honour the term.  mvfit_fit runs the stages that carry it as chained rounds (pass ->
 * silhouette evaluation -> dense pull-back -> record -> step kernel, the term's kernels skipping finished problems);
 * stages without it in front keep their single-launch phase.  MVFIT_F_SPARSE_VERTS is ignored while the term is active;
 * MVFIT_F_VPOSER / FIX_SHAPE / FIX_SCALE behave as in the closure.  mvfit_sdf_term_read returns L_j in sums (the loss, not a
 * root of it); samples: MVFIT_E_UNSUPPORTED.
 * The mask set may be replaced while the term is on: the next fit uses the new set (the captured round graph is rebuilt when
 * the new set has other sizes or another contour, and kept otherwise).  mvfit_set_silhouettes(num_images = 0) switches the
 * term off, and so does a replacing set that fails or whose image_body reaches B (that call returns MVFIT_E_ARG);
 * mvfit_set_problems with another B switches it off too.  The round's buffers (12 B Nv + 4 bytes of cotangent and loss, and
 * 2112 ceil(Nv / 32) bytes of pull-back partials, per problem of the batch rounded up to 32) are allocated by the first enable
 * and keep their addresses while B stays.
 * One term slot per ctx: MVFIT_E_STATE while mvfit_set_sdf's term or scene obstacles are configured (and those two calls
 * return it while this term is on).  MVFIT_E_STATE also without mvfit_set_problems or without a mask set.  MVFIT_E_ARG: a
 * non-finite or negative w_in / w_out, a non-finite sigma, a mask set whose image_body lies outside [0, B). */
int mvfit_set_silhouette_term(mvfit_ctx* ctx, int enable, float w_in, float w_out, float sigma);

/* ---- Occlusion between the bodies of a scene (csrc/silhouette_occlusion.hip).  A person mask from a segmenter is modal: it
 * shows the visible part of the person only.  Where another body of the scene stands in front, an off pixel says nothing
 * about this body: term A would push the body out from behind the other one, term B would pull it onto the line where the
 * other one cuts its mask.  mvfit_set_silhouette_occluders freezes the other bodies as depth maps per mask image; while
 * they are set, mvfit_silhouette_loss, mvfit_closure, the term in mvfit_fit and the term mix ignore what the maps hide.
 * With no occluders set every entry returns the bits it returns without this section.
 *
 * Freeze, at vertices[N,Nv,3] dev with body_scene[N] host (N = num_bodies): image i shows body n = image_body[i].
 *   body_scene[n] < 0: the image has no occluders.  Otherwise its occluders are all bodies m != n with body_scene[m] ==
 *   body_scene[n], at vertices[m]; a body without images still occludes.
 *   Depth maps at the mask set's H x W through the image's own camera: Z_occ,i[y,x] = the smallest fp32 depth of any
 *     occluder face covering the pixel sample, Z_own,i the same from vertices[n] itself (every image has it), both +inf
 *     where nothing covers the sample.  Transform, coverage, depth formula, [znear, zfar] and guard band are exactly those
 *     of mvfit_render_overlay below (fp32 transform, 1/256-pixel integer edge functions with inclusive edges, float64
 *     perspective depth rounded to fp32, [0.05, 8000], 16384 px).  The minimum is taken over the fp32 bits (positive floats
 *     order like their bits): order-independent, deterministic, independent of any grouping of images or bodies.
 *   Point flags, one byte per kept contour point (contour list, CSR, chunk table and every buffer of the mask set stay as
 *     they are).  For point p of image i and a 4-neighbour q of p that lies inside the image and is off in the mask: q is
 *     explained iff Z_occ,i(q) < +inf and not (Z_own,i(p) <= Z_occ,i(q)) - an own depth of +inf counts as "not known to be
 *     in front".  The point is flagged iff all its off in-image 4-neighbours are explained.
 * Evaluation while occluders are set:
 *   A valid vertex (pz > 0.05) projected to (u, v) is hidden in image i iff 0 <= u < W and 0 <= v < H (fp32 compares) and
 *     Z_occ,i[(int)v][(int)u] + margin < pz, the add rounded to fp32, nothing fused.  A hidden vertex contributes to neither
 *     term, exactly like an invalid one: nothing to term A, no candidate in term B's search.
 *   A flagged contour point contributes 0: winner -2 in the diagnostic output, no gradient; B_i stays contour_stride * sum
 *     over the unflagged kept points.
 *   Everything else - rho forms, summation orders, fixed-point accumulators, determinism, independence of N, of the body's
 *     position and of other scenes - is the contract above.
 * mvfit_silhouette_occluders_read: z_occ[M,H,W], z_own[M,H,W] float32 and point_flag[C] uint8, dev out or NULL.
 * mvfit_silhouette_hidden: hidden[M,Nv] uint8 dev out, the hidden byte per (image, vertex) at vertices[num_bodies,Nv,3]; 0
 * for invalid vertices and 0 everywhere without occluders.
 * Lifetime.  The occluders belong to the mask set: every mvfit_set_silhouettes call clears them (a failing one and
 * num_images = 0 included).  num_bodies = 0 or vertices = NULL clears them; a failed freeze leaves none set.  A re-freeze
 * with unchanged (M, H, W, C) keeps every buffer address; the captured round graph's key holds the maps' buffer, whether
 * occluders are set and margin, so a re-freeze alone does not rebuild the graph.  The freeze waits for the stream.
 * Workspace, kept in the ctx: 8 M H W + C bytes (two maps and the flags, each part rounded up to 256 bytes), plus for the
 * raster 16 bytes per instance (an image's own body and each of its occluders) and, per instance of a group of at most
 * 512, 16 Nv + 4 Nf bytes of vertex records and large-face list, grown to the largest freeze seen like the renderer's.
 * A face whose pixel box exceeds 1024 pixels is rasterised by a whole workgroup, as in the renderer.
 * MVFIT_E_STATE: no mask set; a model without (valid) faces; mvfit_silhouette_occluders_read without occluders.
 * MVFIT_E_ARG: NULL body_scene, num_bodies outside [1, 65535] or not above the mask set's largest image_body, margin
 * negative or not finite; for mvfit_silhouette_hidden a NULL pointer or num_bodies as above.
 * Not built: a body's self-occlusion (its own mask covers it), label images shared between persons. */
int mvfit_set_silhouette_occluders(mvfit_ctx* ctx, const float* vertices, int num_bodies, const int32_t* body_scene, float margin);
int mvfit_silhouette_occluders_read(mvfit_ctx* ctx, float* z_occ, float* z_own, uint8_t* point_flag);
int mvfit_silhouette_hidden(mvfit_ctx* ctx, const float* vertices, int num_bodies, uint8_t* hidden);

/* The captured round graph of the chained rounds (mvfit_fit with a term other than mvfit_set_sdf's, or round_mode = 1) and the
 * buffers a re-freeze must keep.  out4 (host, or NULL): [0] round graphs captured on this ctx so far - a fit whose key
 * (buffers, sizes, weights, options; see the terms above) equals the last capture's replays that graph and does not count;
 * [1..3] the device addresses of the occluders' z_occ, z_own and point_flag (0 before the first freeze).  drop != 0 waits
 * for the stream and drops the captured graph: the next such fit captures a fresh one (about 1 ms).
 * silhouette.refine_fit_occluded does so before every sweep after the first: a default-length fit that replays a graph
 * captured before the frozen data changed has been measured not to be reproducible from ctx to ctx,
 * a fit on a graph of its own is. */
int mvfit_round_graph_info(mvfit_ctx* ctx, int drop, uint64_t* out4);

/* ---- Vertex-target term: squared distance of a problem's vertices to weighted target vertex sets ----
 * The frozen form of every "stay close to these bodies" energy (temporal smoothing against the neighbouring frames, a
 * registered mesh of another method): problem j has K target vertex sets T_jk [Nv,3] with weights a_jk >= 0.
 *
 * mvfit_set_vertex_targets copies targets[B,K,Nv,3] (device) and weights[B,K] (host) into buffers the ctx owns; the
 * caller may free its own afterwards.  1 <= K <= MVFIT_VERTEX_TARGETS_MAX, every weight finite and >= 0.  K = 0 or
 * targets = NULL clears the set and switches the term (mvfit_set_vertex_target_term) off.  A target row with a_jk == 0 is
 * never read: it may hold anything, NaN included.  A second set with the same (B, K) keeps every buffer address (the
 * weights live in a device buffer the kernel reads; a captured round graph stays valid), another K replaces the buffers and
 * keeps an enabled term on.  mvfit_set_problems with another B clears the set.  MVFIT_E_STATE without mvfit_set_problems;
 * MVFIT_E_ARG: K outside the range, a null weights pointer, a negative or non-finite weight (the set in place stays). */
#define MVFIT_VERTEX_TARGETS_MAX 4
int mvfit_set_vertex_targets(mvfit_ctx* ctx, int K, const float* targets, const float* weights);

/* The term at vertices[B,Nv,3] (device): loss[B] and, unless NULL, g_vertices[B,Nv,3] (device).  The contract, over a
 * problem's vertices as n = 3 Nv flat floats (the term is separable per float):
 *   d_k[e] = V[e] - T_k[e]                              one fp32 subtraction, for the k with a_k > 0 in ascending k;
 *   g[e]   = float32(2 * sum_k double(a_k) * double(d_k[e]))          the sum in float64, ascending k, from 0.0;
 *   L      = float32(sum_e sum_k double(a_k) * double(d_k[e])^2)      accumulated in float64.
 * A product of two floats is exact in float64, so a fused multiply-add changes no bit of g: g_vertices is reproducible bit
 * for bit by a NumPy restatement.  The order of L's sum is fixed by Nv and the kernel's shape (csrc/vertex_target.hip: 1024
 * pairs of floats per workgroup, a wave64 butterfly, the waves and then the workgroups in order), never by B or the
 * problem's position; float64 keeps its error far below the one final fp32 rounding.  No atomics: a problem's L and g are
 * bit-identical alone, in any batch, at any position and from run to run.  A problem whose weights are all zero gets L = 0
 * and an exactly zero gradient.
 * MVFIT_E_STATE when no target set is present; MVFIT_E_ARG for a null vertices or loss. */
int mvfit_vertex_target_loss(mvfit_ctx* ctx, const float* vertices, float* loss, float* g_vertices);

/* The vertex-target loss as a term of the fit (enable != 0; 0 switches it off).  While it is on, a weight set with
 * coll_loss_weight = w > 0 adds w^2 * L_j to problem j, L_j exactly loss[j] of mvfit_vertex_target_loss at the trial point's
 * vertices; its gradient is w^2 times the pull-back of that call's g_vertices through the fp32 model (the adjoint
 * mvfit_vertices_backward computes).  The form, the record and the L < FLT_MIN rule are the silhouette term's: a problem
 * whose weights are all zero keeps the loss and gradient bits it has without the term.
 * mvfit_closure and mvfit_fit both honour the term.  mvfit_fit runs the stages that carry it as chained rounds (pass ->
 * target kernel -> dense pull-back -> record -> step kernel, the term's kernels skipping finished problems); stages without it
 * in front keep their single-launch phase.  MVFIT_F_SPARSE_VERTS is ignored while the term is active.  mvfit_sdf_term_read
 * returns L_j in sums; samples: MVFIT_E_UNSUPPORTED.
 * The target set may be replaced while the term is on: the next fit uses the new set, and the captured round graph is kept
 * when (B, K) are the same.  The round's buffers (12 B Nv + 4 bytes of cotangent and loss, 2112 ceil(Nv / 32) bytes of
 * pull-back partials per problem of the batch rounded up to 32) are allocated by the first enable and keep their addresses
 * while B stays.
 * One term slot per ctx: MVFIT_E_STATE while mvfit_set_sdf's term, scene obstacles or the silhouette term are configured
 * (and those three setters return it while this term is on).  MVFIT_E_STATE also without mvfit_set_problems or without a
 * target set. */
int mvfit_set_vertex_target_term(mvfit_ctx* ctx, int enable);

/* ---- Scan loss: measured 3-D surface points against the posed body and back, with its gradient on the vertices
 * (csrc/scan_loss.hip).  The reference has no term on scan data: this contract is the project's own.  A scan has no
 * correspondences with the model; they are searched for at every evaluation.
 *
 * mvfit_set_scans keeps, once per scan set, up to max_points world points for each of num_bodies bodies.  Point i of body n
 * takes part iff i < count[n] and its weight is > 0 (weights = NULL: every weight is 1).  A point that does not take part is
 * never read and may hold anything, NaN included.  num_bodies = 0 clears the set (the other arguments are ignored).  Faces
 * are the model's.
 *
 * mvfit_scan_loss evaluates at vertices[N,Nv,3] float32 (translation included, as mvfit_vertices returns them), N the set's.
 * Distances are in the unit of the vertices, and so is sigma.  All fp32 arithmetic below is un-contracted (no FMA fusion).
 *   Term S (scan to mesh).  For a point p and a face (a, b, c) with ab = b - a, ac = c - a in fp32: the closest point of the
 *     triangle by region - with ap = p - a, bp = ap - ab, cp = ap - ac, d1 = ab.ap, d2 = ac.ap, d3 = ab.bp, d4 = ac.bp,
 *     d5 = ab.cp, d6 = ac.cp (dots as (x + y) + z), vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4, the first
 *     that matches of: vertex a (d1 <= 0, d2 <= 0): (v, w) = (0, 0); vertex b (d3 >= 0, d4 <= d3): (1, 0); edge ab (vc <= 0,
 *     d1 >= 0, d3 <= 0): (d1 / (d1 - d3), 0); vertex c (d6 >= 0, d5 <= d6): (0, 1); edge ac (vb <= 0, d2 >= 0, d6 <= 0):
 *     (0, d2 / (d2 - d6)); edge bc (va <= 0, d4 - d3 >= 0, d5 - d6 >= 0): (d5 - d6, d4 - d3) / ((d4 - d3) + (d5 - d6));
 *     interior: (vb, vc) / ((va + vb) + vc); every quotient as a product with one fp32 reciprocal.  q = a + v ab + w ac, the
 *     barycentrics of (a, b, c) are (b0, b1, b2) = ((1 - v) - w, v, w), and m = |q - p|^2 is recomputed from
 *     q - p = (v ab + w ac) - ap in fp32.  The winner is the face with the smallest fp32 m, ties to the lowest face index
 *     (a face whose m is NaN never wins; with no winner the point reports -1 and contributes 0).
 *     rho(m) = m when sigma <= 0, else sigma^2 m / (sigma^2 + m), in float64 from the fp32 m.  S_n = sum_p w_p rho(m_p).
 *     The gradient goes to the winner's three vertices with the barycentrics held fixed: w_p rho'(m) 2 (q - p) b_k - exact
 *     wherever the closest point is unique.
 *   Term M (mesh to scan).  For every vertex j of the model the participating point with the smallest fp32
 *     m = |v_j - p|^2 (differences, products and the sum (x + y) + z each rounded to fp32), ties to the lowest point index; a
 *     body without participating points contributes 0 and reports -1.  Same rho; M_n = sum_j rho(m_j), the gradient
 *     rho'(m) 2 (v_j - p) goes to the vertex.
 *   loss[n] = float32(w_s2m S_n + w_m2s M_n), g_vertices = w_s2m dS/dV + w_m2s dM/dV summed in float64 and rounded to float32
 *     once.  A term whose weight is 0 is not searched; its winner array, when asked for, is filled with -1.  The gradient
 *     flows through the vertex positions only: points, winners and barycentrics are constants.
 *   search: 0 (auto) or 1 (exhaustive: every point against every face).  Auto skips faces whose bounding sphere lies beyond
 *     a conservative bound of the point's distance; it returns the bits of the exhaustive search.
 *   Determinism: no float atomics; a body's loss, gradient and winners are bit-identical alone, in any batch, at any position
 *     and from run to run; a body without participating points gets, at w_m2s = 0, loss 0 and an exactly zero gradient.
 *     Term S's many-points-to-one-vertex sum is a 64-bit integer accumulation of the contributions scaled by 2^e_n,
 *     e_n = -ilogb(largest participating weight of body n) (0 for a body without one; computed once by mvfit_set_scans), in
 *     units of 2^-32 of the vertices' unit: with w' = 2^e_n w_p, so that the body's largest w' lies in [1, 2), each
 *     contribution w' rho'(m) 2 (q - p) b_k to a vertex coordinate is rounded to that unit, the sum of one coordinate must
 *     stay below 2^31 units of the vertices in magnitude, and 2^-e_n is applied to the sum in float64 before w_s2m and the
 *     one rounding to float32.  The unit is therefore relative to the body's weights - weights scaled by a power of two scale
 *     the loss and every gradient word by exactly that power, and a body whose largest weight lies in [1, 2) has e_n = 0 -
 *     but absolute in q - p: a contribution carries up to 2^-33 / (2 w' rho' |q - p| b_k) of relative rounding, 1e-8 at 5 mm
 *     (in metres) and weight 1, more where the distances or rho' are small.
 *     S_n and M_n are float64 sums whose order is fixed by max_points, Nv and the
 *     kernel shapes (256 points or vertices per workgroup: a wave64 butterfly, the waves, then the workgroups in order),
 *     never by N.
 *
 * points[N,max_points,3] float32 dev or host; count[N] int32 host; weights[N,max_points] float32 host or NULL.  loss[N] dev
 * out; g_vertices[N,Nv,3] dev out or NULL; nearest_face[N,max_points] int32 dev out or NULL (-1 for a point that does not
 * take part); nearest_point[N,Nv] int32 dev out or NULL.  mvfit_set_scans waits for the stream; mvfit_scan_loss is
 * asynchronous.
 * Workspace, kept in the ctx and reused - every address kept - by a second set of the same (N, max_points):
 *     N * (32 max_points + 8 + 64 Nf + 16 ceil(Nf / 8) + 24 Nv + 8 ceil(max_points / 256) + 8 ceil(Nv / 256))   bytes
 *     (points, weights and packed points; counts and the exponents e_n; face records; seed vertices; the fixed-point accumulators; the partials of
 *     both terms), each part rounded up to 256 bytes.
 * MVFIT_E_ARG: a NULL required pointer, sizes out of range (N <= 65535, max_points >= 1, N max_points <= 2^28), a count[n]
 * outside [0, max_points], a negative or non-finite weight below count[n], a negative or non-finite w_s2m, w_m2s or sigma,
 * search > 1, num_bodies other than the set's.  MVFIT_E_STATE: mvfit_scan_loss without a scan set; mvfit_set_scans on a
 * model without (valid) faces. */
int mvfit_set_scans(mvfit_ctx* ctx, int num_bodies, int max_points, const float* points, const int32_t* count,
                    const float* weights);
int mvfit_scan_loss(mvfit_ctx* ctx, const float* vertices, int num_bodies, float w_s2m, float w_m2s, float sigma, uint32_t search,
                    float* loss, float* g_vertices, int32_t* nearest_face, int32_t* nearest_point);

/* The scan loss as a term of the fit (enable != 0; 0 switches it off and ignores the scalars).  Scan body n is problem n, so
 * the set holds B bodies.  While it is on, a weight set with coll_loss_weight = w > 0 adds w^2 * L_j to problem j, L_j exactly
 * loss[j] of mvfit_scan_loss(w_s2m, w_m2s, sigma, search = 0) at the trial point's vertices; its gradient is w^2 times the
 * pull-back of that call's g_vertices through the fp32 model (the adjoint mvfit_vertices_backward computes).  The form, the
 * record and the L < FLT_MIN rule are the silhouette term's: a problem without participating points (at w_m2s = 0) keeps the
 * loss and gradient bits it has without the term.
 * mvfit_closure and mvfit_fit both honour the term.  mvfit_fit runs the stages that carry it as chained rounds (pass -> clear
 * -> face records -> scan to mesh -> mesh to scan -> sum -> dense pull-back -> record -> step kernel; kernel launches only, the
 * term's kernels skipping finished problems, whose loss, gradient rows, partials and accumulators stay as they are); stages
 * without it in front keep their single-launch phase.  MVFIT_F_SPARSE_VERTS is ignored while the term is active.
 * mvfit_sdf_term_read returns L_j in sums; samples: MVFIT_E_UNSUPPORTED.  mvfit_scan_loss stays available and returns the
 * bits it returns without the term; it shares the set's work areas with the rounds, on the ctx's stream.
 * The scan set may be replaced while the term is on: the next fit uses the new points, and the captured round graph is kept
 * when (N, max_points) are the same.  A set with num_bodies != B switches the term off and returns MVFIT_E_ARG; clearing the
 * set switches it off too.  mvfit_set_problems with another batch switches the term off and keeps the scan set.  The round's
 * buffers (12 B Nv + 4 bytes of cotangent and loss, 2112 ceil(Nv / 32) bytes of pull-back partials per problem of the batch
 * rounded up to 32) are allocated by the first enable and keep their addresses while B stays.
 * One term slot per ctx: MVFIT_E_STATE while mvfit_set_sdf's term, scene obstacles, the silhouette term, the vertex-target
 * term or the term mix are configured (and those five setters return it while this term is on; next to other terms the scan
 * loss runs as a share of the mix, mvfit_term_mix::scan).  MVFIT_E_STATE also without mvfit_set_problems or without a scan set.  MVFIT_E_ARG when the set's num_bodies
 * differs from B, for a negative or non-finite w_s2m, w_m2s or sigma, and when both weights are 0.  A refused call leaves
 * the state as it was. */
int mvfit_set_scan_term(mvfit_ctx* ctx, int enable, float w_s2m, float w_m2s, float sigma);

/* ---- Surface landmark term: named points of the body's surface against the pixels they were seen at and against measured
 * 3-D positions, with the gradient on the vertices (csrc/landmark.hip).  The reference has no such term (its body model
 * knows foot keypoints as surface vertices, its fitter drops the detector's foot points): this contract is the project's own.
 *
 * mvfit_set_landmarks keeps the landmark table, once per ctx and independent of the problems: 1 <= L <= MVFIT_LANDMARKS_MAX
 * landmarks, each an affine combination of up to MVFIT_LANDMARK_NNZ vertices, vertex_ids[L,4] int32 and weights[L,4] float32
 * (host).  A slot of weight 0 is never read and its id may be anything; every other slot has an id in [0, Nv) and a finite
 * weight, else MVFIT_E_ARG (the table in place stays).  Landmark l lies at p_l = sum_k w_lk V[vid_lk], in fp32 from 0 in
 * ascending k.  L = 0 or a NULL pointer clears the table, the targets and the term; so does a new table (the
 * targets belong to the table they were set for).
 *
 * mvfit_set_landmark_targets copies the targets of the current batch (B and V of mvfit_set_problems, whose cameras the term
 * uses): xy[B,V,L,2], conf[B,V,L] and, both or neither, xyz[B,L,3], conf3[B,L] (device or host).  Every confidence is finite
 * and >= 0 (MVFIT_E_ARG, the set in place stays); an entry of confidence 0 is never read and may hold NaN.  A second set at
 * the same (B, V, L, with or without 3-D) keeps every buffer address, so a captured round graph stays valid.  xy = NULL
 * clears the targets and switches the term off.  MVFIT_E_STATE without a table or without mvfit_set_problems;
 * mvfit_set_problems with another B or V clears the targets and the term and keeps the table.
 *
 * mvfit_landmark_loss evaluates at vertices[B,Nv,3] (device): loss[B] and, unless NULL, g_vertices[B,Nv,3] (device).
 *   L_b = sum_v sum_l conf_bvl^2 (g(u_bvlx - xy_bvlx; rho) + g(u_bvly - xy_bvly; rho))
 *       + sum_l w3d conf3_bl^2 ((g(p_blx - xyz_blx; rho3d) + g(p_bly - xyz_bly; rho3d)) + g(p_blz - xyz_blz; rho3d)),
 *   g(r; s) = s^2 r^2 / (r^2 + s^2) for s > 0 (the reference's GMoF, utils/utils.py:435-438), r^2 for s == 0,
 *   u = f (R p + t)_xy / (R p + t)_z + c in fp32 exactly as the closure's keypoint term computes it (no rule about depth:
 * bodies are in front of their cameras).  There is no data_weight inside.  Each item is an fp32 value; the items of a lane
 * are added in float64 in ascending (v, l), the 3-D items after them, the lanes through a fixed reduction network, and the
 * total is rounded to fp32 once.  The gradient is dense: a landmark's point gradient sums its views in ascending order, then
 * the 3-D part; a vertex's gradient sums w_lk g_l over its (landmark, slot) entries in ascending order; rows of vertices no
 * landmark uses are written as zero, whatever the buffer held.  No atomics: a problem's bits are the same alone, in any
 * batch, at any buffer alignment and from run to run; a problem whose confidences are all zero gets L = 0 and an exactly zero
 * gradient.  MVFIT_E_STATE without a table or targets; MVFIT_E_ARG for a null vertices or loss and for a negative or
 * non-finite rho, w3d or rho3d. */
#define MVFIT_LANDMARKS_MAX 256
#define MVFIT_LANDMARK_NNZ 4
int mvfit_set_landmarks(mvfit_ctx* ctx, int L, const int32_t* vertex_ids, const float* weights);
int mvfit_set_landmark_targets(mvfit_ctx* ctx, const float* xy, const float* conf, const float* xyz, const float* conf3);
int mvfit_landmark_loss(mvfit_ctx* ctx, const float* vertices, float rho, float w3d, float rho3d, float* loss, float* g_vertices);

/* The landmark loss as a term of the fit (enable != 0; 0 switches it off and ignores the scalars).  While it is on, a weight
 * set with coll_loss_weight = w > 0 adds w^2 * L_j to problem j, L_j exactly loss[j] of mvfit_landmark_loss(rho, w3d, rho3d)
 * at the trial point's vertices; its gradient is w^2 times the pull-back of that call's g_vertices through the fp32 model
 * (the adjoint mvfit_vertices_backward computes).  The form, the record and the L < FLT_MIN rule are the silhouette term's:
 * a problem whose confidences are all zero keeps the loss and gradient bits it has without the term.
 * mvfit_closure and mvfit_fit both honour the term.  mvfit_fit runs the stages that carry it as chained rounds (pass ->
 * landmark kernel -> dense pull-back -> record -> step kernel, the term's kernel skipping finished problems); stages without
 * it in front keep their single-launch phase.  MVFIT_F_SPARSE_VERTS is ignored while the term is active.
 * mvfit_sdf_term_read returns L_j in sums; samples: MVFIT_E_UNSUPPORTED.  The targets may be replaced while the term is on;
 * the captured round graph is kept when their sizes are the same.  The round's buffers are the vertex-target term's.
 * One term slot per ctx: MVFIT_E_STATE while mvfit_set_sdf's term, scene obstacles, the silhouette term, the vertex-target
 * term, the scan term or the term mix are configured (and those setters return it while this term is on; the term takes no
 * share of the mix).  MVFIT_E_STATE also without targets.  MVFIT_E_ARG for a negative or non-finite scalar.  A refused call
 * leaves the state as it was. */
int mvfit_set_landmark_term(mvfit_ctx* ctx, int enable, float rho, float w3d, float rho3d);

/* ---- Term mix: the scene, silhouette, vertex-target and scan terms together behind coll_loss_weight ----
 * With the mix on, a weight set with coll_loss_weight = w > 0 adds to problem j
 *   pen_j = w^2 * (scene * S_sc^2 + silhouette * L_sil + vertex_targets * L_vt + scan * L_scan),
 * S_sc what the scene term's record holds against the frozen obstacles (mvfit_set_scene_obstacles), L_sil, L_vt and L_scan
 * exactly loss[j] of mvfit_silhouette_loss(num_bodies = B, sil_w_in, sil_w_out, sil_sigma), of mvfit_vertex_target_loss and
 * of mvfit_scan_loss(scan_w_s2m, scan_w_m2s, scan_sigma, search = 0) at the trial point's vertices (scan body n is problem
 * n); the gradient is the same weighted sum of the four terms' gradients.  The shares are >= 0 and at
 * least two are > 0 (a single term keeps its own setter); a component with share 0 is never evaluated and its buffers are
 * never read.  The one-person SDF term of mvfit_set_sdf is NOT part of the mix.
 * Arithmetic (csrc/term_mix.hip; reproducible by a NumPy restatement).  The vertex terms share ONE dense pull-back: its
 * cotangent is, per float, g = (fl32(silhouette * g_sil) + fl32(vertex_targets * g_vt)) + fl32(scan * g_scan) - rounded products,
 * rounded adds in this order, nothing fused, a component with share 0 left out and not added as 0 - and its loss L_v =
 * float32((double(silhouette) * L_sil + double(vertex_targets) * L_vt) + double(scan) * L_scan); with one vertex term
 * live, only that product is formed, and with its share equal to 1 the term's own buffers go to the pull-back unchanged.
 * A problem whose scan body has no participating points (at scan_w_m2s = 0) has L_scan = 0 and an all-zero g_scan: it adds
 * exactly 0 to L_v and an exactly zero cotangent.
 * With scene = 0 the pull-back writes the closure's record.  With scene > 0 the scene term and the pull-back write records
 * (S_sc, a_sc) and (S_v, a_v) of their own, merged per problem in float64, every operation rounded on its own:
 *   Q = scene * (S_sc * S_sc) + S_v * S_v ;  S = float32(sqrt(Q)) ;
 *   a[e] = float32(((scene * S_sc) * a_sc[e] + S_v * a_v[e]) / sqrt(Q)) ;  Q < FLT_MIN: an all-zero record.
 * With scene = 1 and S_v = 0 the scene record passes through bit for bit.  A problem whose components are all zero keeps
 * the loss and gradient bits it has without any term; a problem's numbers do not depend on B, on its position in the batch
 * or on the other problems (beyond its scene's frozen obstacles).
 * mvfit_closure and mvfit_fit both honour the mix.  mvfit_fit runs the stages that carry it as chained rounds (pass ->
 * silhouette evaluation -> target kernel -> scan evaluation -> cotangent mix -> pull-back -> scene term -> record merge -> step kernel, every
 * kernel skipping finished problems); stages without it in front keep their single-launch phase.  MVFIT_F_SPARSE_VERTS is
 * ignored while the mix is on.
 * State.  While the mix is on, mvfit_set_silhouette_term(enable), mvfit_set_vertex_target_term(enable) and mvfit_set_sdf(faces)
 * and mvfit_set_scan_term(enable) return MVFIT_E_STATE.  Obstacles and targets may be re-frozen and the mask and scan sets
 * replaced (same shapes: the captured round graph is kept; other shapes, other shares or other silhouette or scan scalars
 * rebuild it).  Removing a data set whose share is > 0 switches the mix off, as does a replacing set that fails, a scan set
 * with num_bodies != B (MVFIT_E_ARG) and mvfit_set_problems with another B.  A mix with scan = 0 is untouched by any scan
 * call; mvfit_scan_loss stays available and returns its own bits between rounds.  Obstacles being set does
 * not by itself make the scene term run under the mix: only scene > 0 does.  With the mix off every other entry behaves as
 * it does without this one.  The round's buffers (those of the live single terms, 12 B Nv bytes of mixed cotangent, the
 * pull-back partials and two records per problem) are allocated by the first enable and keep their addresses while B stays.
 * mvfit_sdf_term_read: sums returns sum_k share_k * part_k per problem (float64, rounded once; penalty = w^2 * sums);
 * samples: MVFIT_E_UNSUPPORTED.
 * MVFIT_E_ARG: size neither MVFIT_TERM_MIX_SIZE_V1 (the layout up to vertex_targets: the scan fields read as 0) nor
 * sizeof(mvfit_term_mix), a negative or non-finite share, fewer than two shares > 0, bad silhouette scalars (as
 * mvfit_set_silhouette_term) or scan scalars (as mvfit_set_scan_term), a mask set whose image_body lies outside [0, B), a
 * scan set whose num_bodies differs from B.  MVFIT_E_STATE: without mvfit_set_problems, while mvfit_set_sdf's term or a
 * single term's own setter is on, or when a share > 0 has no data set.  A refused call leaves the state as it was. */
#define MVFIT_TERM_MIX_SIZE_V1 28u
typedef struct mvfit_term_mix {
    uint32_t size;                 /* sizeof(mvfit_term_mix) of the caller, or MVFIT_TERM_MIX_SIZE_V1 */
    float scene;                   /* share >= 0; > 0 needs obstacles (mvfit_set_scene_obstacles) */
    float silhouette;              /* share >= 0; > 0 needs a mask set (mvfit_set_silhouettes) */
    float sil_w_in, sil_w_out, sil_sigma;
    float vertex_targets;          /* share >= 0; > 0 needs a target set (mvfit_set_vertex_targets) */
    float scan;                    /* share >= 0; > 0 needs a scan set of B bodies (mvfit_set_scans) */
    float scan_w_s2m, scan_w_m2s, scan_sigma;
} mvfit_term_mix;
int mvfit_set_term_mix(mvfit_ctx* ctx, const mvfit_term_mix* mix /* NULL: off */);
/* parts[B,3] dev out: S_sc^2 (the float64 square of the scene record's S, rounded once), L_sil, L_vt of the last evaluation,
 * unweighted; 0 for a share of 0.  MVFIT_E_STATE while the mix is off. */
int mvfit_term_mix_read(mvfit_ctx* ctx, float* parts);
/* parts[B,4] dev out: the same three and L_scan. */
int mvfit_term_mix_read4(mvfit_ctx* ctx, float* parts);
/* The mix's two kernels on the caller's device buffers, for checks against a restatement of the arithmetic above (B and Nv
 * are the ctx's; nothing of the ctx's state is read or changed).
 * mvfit_term_mix_cotangent: g[B,Nv,3] and L_v[B] from g_sil / g_vt [B,Nv,3] and L_sil / L_vt [B]; the buffers of a component
 * with share 0 are never read (NULL is fine).  Buffers at addresses that are no multiple of 8 take the 4-byte-load form of the
 * kernel: the same bits.  MVFIT_E_ARG: a negative or non-finite share, both 0, a null buffer of a live component.
 * mvfit_term_mix_cotangent3: the same with the scan as third component, g_scan [B,Nv,3] and L_scan [B]; any of the three may
 * be live, and with scan = 0 it returns the bits of mvfit_term_mix_cotangent.
 * mvfit_term_mix_merge: rec[B,R] from the records rec_scene / rec_verts [B,R], R = MVFIT_TERM_RECORD_FLOATS floats each: S,
 * then the adjoint entries.  MVFIT_E_ARG: scene not finite and > 0, a null buffer.  Both: MVFIT_E_STATE without
 * mvfit_set_problems. */
#define MVFIT_TERM_RECORD_FLOATS 516
int mvfit_term_mix_cotangent(mvfit_ctx* ctx, float silhouette, const float* g_sil, const float* L_sil, float vertex_targets,
                             const float* g_vt, const float* L_vt, float* g, float* L_v);
int mvfit_term_mix_cotangent3(mvfit_ctx* ctx, float silhouette, const float* g_sil, const float* L_sil, float vertex_targets,
                              const float* g_vt, const float* L_vt, float scan, const float* g_scan, const float* L_scan, float* g,
                              float* L_v);
int mvfit_term_mix_merge(mvfit_ctx* ctx, float scene, const float* rec_scene, const float* rec_verts, float* rec);

/* Per-frame initial guess, stage 1 (code/utils/init_guess.py:80-83 -> code/utils/recompute3D.py:22-62): weighted linear
 * triangulation of the 17 keypoints from V calibrated views, batched over B frames.
 *   keypoints[B,V,17,3] float32 dev (u, v, confidence) ; intris[V,3,3], extris[V,4,4] float64 dev (the reference
 *   keeps the camera file in float64, code/utils/utils.py:352-394) ; joints3d[B,17,3] float64 dev out.
 * Same arithmetic as the reference: float64 accumulation, AtA rounded to float32 before the float64 solve (:54). */
int mvfit_triangulate(mvfit_ctx* ctx, int B, int V, const float* keypoints, const double* intris, const double* extris,
                      double* joints3d);

/* Association of 2-D detections across the views of a frame: which detections show the same person.  A detector run per
 * view lists its people in its own order; this op scores every cross-view pair of a frame's detections geometrically and
 * clusters them into persons.  Batched over F frames, asynchronous on the ctx stream, no set_problems call needed.
 *   keypoints[F,V,Nmax,17,3] float32 dev (u, v, confidence) ; count[F,V] int32 dev: detections of view v in frame f (slots
 *   k < count are read; a value above Nmax counts as Nmax, below 0 as 0) ; intris[V,3,3], extris[V,4,4] float64 dev as the
 *   triangulation takes them.  D = V * Nmax, detection (view v, slot k) has the flat index a = v * Nmax + k.
 *   cost_out[F,D,D] float64 dev out or NULL ; labels[F,V,Nmax] int32 dev out ; num_clusters[F] int32 dev out or NULL.
 * Limits: F >= 1, 2 <= min_views <= V <= MVFIT_MAX_VIEWS, 1 <= Nmax <= MVFIT_ASSOC_MAX_DET, 1 <= min_joints <= 17, max_cost
 * finite and >= 0 ; MVFIT_E_ARG otherwise and for a NULL keypoints / count / intris / extris / labels.
 *
 * Cost (float64, every product and sum rounded on its own - no fused multiply-add -, operands in the order written, sums
 * left to right unless bracketed; sqrt and / correctly rounded):
 *   view v:  Ki = inverse of intris[v] by cofactors, as the triangulation forms it: with K = (a b c; d e f; g h i),
 *            A = e*i - f*h, B = -(d*i - f*g), C = d*h - e*g, id = 1 / (a*A + b*B + c*C),
 *            Ki = (A*id, -(b*i - c*h)*id, (b*f - c*e)*id ; B*id, (a*i - c*g)*id, -(a*f - c*d)*id ;
 *                  C*id, -(a*h - b*g)*id, (a*e - b*d)*id) ;
 *            R, t = rotation and translation of extris[v] ; origin o_i = -((R0i*t0 + R1i*t1) + R2i*t2).
 *   detection a, joint j with pixel (x, y) and confidence cf, all converted to float64:
 *            n_r = Ki_r0*x + Ki_r1*y + Ki_r2, nn = sqrt(n0*n0 + n1*n1 + n2*n2), n_r = n_r / nn,
 *            direction d_i = (R0i*n0 + R1i*n1) + R2i*n2.
 *   pair a < b of different views, both slots below their count, joint j with both confidences > 0:
 *            b_ = o_b - o_a, c = d_a x d_b (c0 = da1*db2 - da2*db1, c1 = da2*db0 - da0*db2, c2 = da0*db1 - da1*db0),
 *            s2 = (c0*c0 + c1*c1) + c2*c2 ;
 *            s2 > 1e-18:  dist_j = |(b_0*c0 + b_1*c1) + b_2*c2| / sqrt(s2)      (distance of the two lines, world units)
 *            otherwise:   x = b_ x d_a (same component pattern), dist_j = sqrt((x0*x0 + x1*x1) + x2*x2)
 *            w_j = sqrt(cf_a * cf_b) ; num = num + w_j*dist_j, den = den + w_j in ascending j from 0.
 *   cost(a, b) = cost(b, a) = num / den when at least min_joints joints took part, +inf otherwise, and +inf for a == b, for
 *   two detections of one view and for a slot at or above its count.
 * Clustering, per frame (complete linkage, cannot-link within a view): every valid detection starts as its own cluster.
 * While a pair of clusters {A, B} has L(A, B) = max over a in A, b in B of cost(a, b) <= max_cost - two clusters that share a
 * view have L = +inf by the rule above -, the pair with the smallest L is merged; ties go to the lexicographically smallest
 * (smallest member of A, smallest member of B), A the cluster with the smaller smallest member.  Then clusters of fewer than
 * min_views members get label -1, as do slots at or above their count; the others are numbered 0, 1, ... in ascending order
 * of their smallest member, and num_clusters[f] is their number.  A cluster never holds two detections of one view.
 * A frame's costs and labels do not depend on F, on the frame's position in the call or on the groups of frames the op
 * works in (each group's rays and D x D linkage matrices, D * (17 * 32 + D * 8) bytes per frame behind a 512-byte head,
 * stay under 256 MB of a workspace the ctx keeps and grows to the largest call). */
int mvfit_associate_views(mvfit_ctx* ctx, int F, int V, int Nmax, const float* keypoints, const int32_t* count,
                          const double* intris, const double* extris, double max_cost, int min_joints, int min_views,
                          double* cost_out, int32_t* labels, int32_t* num_clusters);

/* Refinement of the rig's cameras against held bodies.  Every term of a fit takes the rig of mvfit_set_problems as exact; these
 * two ops hold the bodies' 17 keypoints and move the cameras, one independent problem per view: the keypoint data term of the
 * closure restricted to the view, as a function of the view's camera.  B, V, gt_xy and w_conf are those of mvfit_set_problems
 * (MVFIT_E_STATE before it); the ctx's own cameras are neither read nor changed - the caller passes the refined rig to
 * mvfit_set_problems.  Both ops are asynchronous on the ctx stream, do no host synchronisation and use no workspace.
 *   joints[B,17,3] float32 dev (the keypoints of mvfit_closure / mvfit_vertices) ; a camera is 15 float64: R (9, row-major),
 *   t (3), f, cx, cy ; cams[V,15] float64 dev.  The 9 parameters of a camera are omega (3), dt (3), f, cx, cy.
 *
 * Arithmetic of view v (float64, no fused multiply-add; the float32 inputs are widened first).  Point (b, j) with
 * X = joints[b,j], (gx, gy) = gt_xy[b,v,j], w = w_conf[b,v,j]; a point with w == 0 is not read further and adds nothing:
 *   p = R X + t, a = px / pz, b = py / pz, u = f a + cx, v = f b + cy, r_u = gx - u, r_v = gy - v, k = data_weight^2 w^2 ;
 *   E = sum k (G(r_u) + G(r_v)), G(r) = rho^2 r^2 / (r^2 + rho^2)          (the closure's data term, Geman-McClure) ;
 *   s(r) = rho^4 / (r^2 + rho^2)^2, so G'(r) = 2 r s(r) ; per residual with Jacobian row J (of u or v):
 *   g -= 2 k s(r) r J,  H += 2 k s(r) J^T J                                 (H positive semi-definite: the IRLS form).
 * The parameters perturb the camera frame, p' = exp([omega]x) p + dt, so
 *   du/dp = (f/pz, 0, -f a/pz), dv/dp = (0, f/pz, -f b/pz), dp/domega = -[p]x (rows (0, pz, -py), (-pz, 0, px), (py, -px, 0)),
 *   dp/ddt = I, du/df = a, dv/df = b, du/dcx = 1, dv/dcy = 1, every other entry 0 ;
 * and a step d means R' = exp([omega]x) R, t' = exp([omega]x) t + dt (Rodrigues in float64; below |omega|^2 = 1e-24 with
 * sin(x)/x = 1 and (1 - cos x)/x^2 = 1/2), f' = f + df, c' = c + dc.
 * count = the number of points with w != 0.  A view with a counted point at pz <= 1e-6 is "behind": E = +inf, and g and H are
 * not defined (mvfit_camera_normal_eqs writes NaN).  The points are summed strided over 256 threads, per wave and then in
 * wave order: a view's results depend on nothing but that view's inputs and B.
 *
 * mvfit_camera_normal_eqs: E[V], g[V,9] or NULL, H[V,9,9] (full, symmetric) or NULL, count[V] int32 or NULL, all dev out.
 * MVFIT_E_ARG: a NULL joints / cams / E, rho not finite and > 0, data_weight not finite and >= 0.
 *
 * mvfit_refine_cameras: Levenberg-Marquardt per view, the whole loop on the device.  free = the ascending list of the parameters
 * named by free_mask (bit 0: omega, bit 1: dt, bit 2: f, bit 3: cx and cy).
 *   E, g, H at theta ; E0 = E ; lam = lambda0 ; it = acc = 0
 *   while it < max_iter:
 *       it += 1
 *       A = H[free, free] with its diagonal multiplied by (1 + lam)
 *       Cholesky of A ; a pivot <= 0 (or not a number):  lam *= 10 ; continue
 *       d = -A^-1 g[free] ; theta' = step(theta, d)
 *       E' at theta'                                        (+inf when behind)
 *       if E' < E:  dec = E - E' ; theta = theta' ; E = E' ; g, H at theta ; lam = max(lam / 10, 1e-9) ; acc += 1
 *                   if dec <= ftol * max(E, 1): status 0, stop
 *       else:       lam *= 10 ; if lam > 1e12: status 2, stop
 *   the loop left by it == max_iter: status 1
 * E' of a candidate and E of the evaluation at the same camera are one summation, hence one number.  A view is skipped - its
 * 15 output doubles are the input's bits - with status 3 when its bit is set in fixed_views, else status 4 when
 * count < min_points, else status 5 when it is behind at the start.
 *   cams_out[V,15] dev out (cams_out == cams_in is allowed) ; report[V,8] float64 dev out:
 *   (E0, E1, it, acc, status, count, lam, 0) per view, E1 the energy at the returned camera.
 * MVFIT_E_ARG, the message naming the field: a NULL joints / cams_in / opts / cams_out / report, size below the struct's,
 * free_mask 0 or above 15, max_iter outside 1..64, min_points < 1, rho not finite and > 0, data_weight not finite and >= 0,
 * lambda0 not finite and > 0, ftol not >= 0.  Bits of fixed_views at or above V are ignored. */
typedef struct mvfit_camera_refine_opts {
    uint32_t size;                 /* sizeof of this struct at the caller, as in mvfit_term_mix */
    uint32_t free_mask;            /* bit 0: omega, 1: dt, 2: f, 3: c */
    uint32_t fixed_views;          /* bit v: view v is returned as given */
    int32_t max_iter;              /* 1..64 */
    int32_t min_points;            /* >= 1 */
    float rho, data_weight;
    double lambda0, ftol;          /* > 0 ; >= 0 */
} mvfit_camera_refine_opts;
int mvfit_camera_normal_eqs(mvfit_ctx* ctx, const float* joints, const double* cams, float rho, float data_weight, double* E,
                            double* g, double* H, int32_t* count);
int mvfit_refine_cameras(mvfit_ctx* ctx, const float* joints, const double* cams_in, const mvfit_camera_refine_opts* opts,
                         double* cams_out, double* report);

/* Per-frame initial guess, stage 1 for single-view input (code/utils/init_guess.py:54-74): the depth guess that replaces
 * the triangulation when a frame has ONE view - the model's rest-pose keypoints pushed along the camera's z axis by
 * est_d = fx * (torso height in camera space) / (torso height in the image) and mapped back with inv(extri); the
 * reference's arithmetic is kept (the left shoulder-hip pair taken twice in the 2-D height, over (u, v, confidence)
 * rows in float32; everything else float64).  Batched over B frames seen by the same camera.
 *   rest_joints[17,3] float64 dev (the 17 keypoints of mvfit_vertices at zero pose / shape / translation and the start
 *   scale, init_guess.py:31-52) ; extri[4,4], intri[3,3] float64 dev ; keypoints[B,17,3] float32 dev (u, v, confidence)
 *   -> joints3d[B,17,3] float64 dev: what mvfit_umeyama takes as dst. */
int mvfit_depth_guess(mvfit_ctx* ctx, int B, const double* rest_joints, const double* extri, const double* intri,
                      const float* keypoints, double* joints3d);

/* Per-frame initial guess, stage 2 (code/utils/init_guess.py:95-106): similarity alignment src -> dst by the
 * reference's umeyama (code/utils/umeyama.py:16-109, incl. its full-rank formula U diag(d) Vh^T and the two-candidate
 * choice with the translation of the second candidate) and cv2.Rodrigues of the chosen rotation; batched over B frames
 * that share the source points (the rest-pose keypoints).  All float64 like the reference's NumPy.
 *   src[npts,3] dev, dst[B,npts,3] dev (npts = 4: the torso joints 5, 6, 11, 12 with use_torso, or 17) ->
 *   rot[B,3,3], rvec[B,3] (the model's global_orient), trans[B,3], scale[B] dev.
 * The signs of the singular-vector pairs - which the reference's formula is sensitive to and LAPACK chooses for it -
 * are LAPACK's own: the device SVD walks dgesdd's path for a 3 x 3 matrix (dgebd2, dbdsqr, dormbr; csrc/lapack_svd3.h)
 * and returns numpy's pairs, so rot / trans / scale equal the reference's (tests/golden/init_guess_ref.npz). */
int mvfit_umeyama(mvfit_ctx* ctx, int B, int npts, const double* src, const double* dst, int estimate_scale,
                  double* rot, double* rvec, double* trans, double* scale);

/* Per-view projection of point sets with the cameras of mvfit_set_problems: the reference's visualisation path
 * cam(verts) / cam(joints) per view (code/utils/utils.py:581-583,603-607; PerspectiveCamera.forward code/camera.py:93-117).
 *   points[B,num_points,3] dev (e.g. the vertices of mvfit_vertices, num_points = 6890) ->
 *   uv[B,V,num_points,2] dev, float pixels (the reference truncates to int32 on the host afterwards). */
int mvfit_project_points(mvfit_ctx* ctx, const float* points, int num_points, float* uv);

/* The fitted body drawn over each view's image, with the 17 model keypoints as red dots: the reference's save_images
 * output (code/utils/utils.py:866-883 save_results -> :574-597 project_to_img -> :659-712 visualize_results ->
 * :977-1028 Renderer.__call__, pyrender + OpenCV on the host), as a depth-tested rasteriser with a fixed operation order
 * (csrc/render.hip; tests/render_oracle.py restates it in NumPy and reproduces the face-ID image bit for bit).
 *   vertices[B,Nv,3] dev (e.g. mvfit_vertices); points[B,num_points,3] dev or NULL (no dots), 0 <= num_points <= 64;
 *   image i (0 <= i < num_images) is problem image_problem[i] seen by view image_view[i] (both host arrays) with the
 *   cameras of mvfit_set_problems (the shared rig or the per-problem cameras);
 *   images[num_images,H,W,3] RGB uint8 dev -> out[num_images,H,W,3] dev (out == images renders in place);
 *   face_id[num_images,H,W] int32 dev or NULL: the visible face per pixel, -1 where no face is.  1 <= H, W <= 8192.
 * Contract (geometry without FP contraction, fp32 divides correctly rounded):
 *   transform  p = ((R0 X + R1 Y) + R2 Z) + t row by row in fp32; u = f (px / pz) + cx, v = f (py / pz) + cy.
 *   coverage   U = rintf(256 u), V = rintf(256 v) (int32); pixel (row y, column x) is sampled at (256 x + 128, 256 y + 128);
 *              the three edge functions in int64, oriented by the sign of the area (area 0: no pixels); covered when all
 *              three are >= 0 (inclusive edges).  A triangle is dropped when a vertex has pz <= znear or lies more than
 *              16384 px outside the image; nothing is clipped.
 *   depth      float64 from the exact edge values e_i (e_i = 0 on the edge opposite vertex i):
 *              w = ((e0 (1/z0) + e1 (1/z1)) + e2 (1/z2)), z = area / w, rounded to fp32; drawn when znear <= z <= zfar,
 *              [znear, zfar] = [0.05, 8000] (pyrender's default near plane; IntrinsicsCamera(zfar=8000), utils.py:998).
 *              The visible face is the minimum of (fp32 bits of z) << 32 | face id: ties go to the lower face id.
 *   shading    (a documented stand-in for pyrender's material, grey 0.5, one colour on all channels, no specular term)
 *              vertex normals = normalised sum, in ascending face id, of the un-normalised (p1 - p0) x (p2 - p0) of the
 *              vertex's faces, float64 in world space, rotated by R; at a covered pixel the normal and the camera-space
 *              point q are interpolated with the perspective-correct barycentrics (e_i / z_i) / w, the normal normalised
 *              and flipped when n.q > 0 (two-sided).  Nine point lights (add_pointLight, utils.py:937-950) at c + r d_k,
 *              c / r = centre / norm of the half-extent of the axis-aligned box of the image's camera-space vertices,
 *              d_k = (sin t cos p, sin t sin p, cos t), t in {pi/6, pi/2, 5pi/6}, p in {0, 2pi/3, 4pi/3};
 *              s = 0.5 * 0.3 + (0.5 / pi) sum_k r^2 max(0, n.l_k) / |L_k - q|^2 (l_k the unit vector to the light);
 *              value = floor(255 min(1, s)^(1/2.2) + 0.5).  Covered pixels take the value (opaque, visible_weight = 1),
 *              every other pixel keeps the input bytes.
 *   dots       drawn last (visualize_results' cv2.circle(radius 3, thickness 10) in BGR red): each point projected with
 *              the same fp32 sequence, truncated toward zero like astype(np.int32) to (cx, cy); every pixel with
 *              (x - cx)^2 + (y - cy)^2 <= 64 becomes (255, 0, 0).  Points with pz <= znear or more than 16384 px outside
 *              the image are skipped.
 * MVFIT_E_STATE: the model was created without faces (or with faces that index outside the vertices), or
 * mvfit_set_problems has not been called.  MVFIT_E_ARG: a problem or view index out of range, H or W outside 1..8192,
 * num_points outside 0..64, num_images < 1, or a NULL vertices / images / out / index array.  Asynchronous on the ctx
 * stream.  Images are processed in groups of at most 64; a group's workspace (per image 8 H W bytes of visibility,
 * 56 B x Nv of vertex records and 4 B x Nf of face list) is at most 256 MB, or one image's when a single image needs
 * more (512 MB of visibility at 8192 x 8192: images are not tiled).  On top of that the vertex normals take
 * 24 B x B x Nv.  Both buffers are kept in the ctx, grown to the largest call.  The result does not depend on the
 * grouping.  A face whose pixel box exceeds 1024 pixels is rasterised by a whole workgroup instead of one thread. */
int mvfit_render_overlay(mvfit_ctx* ctx, const float* vertices, const float* points, int num_points, int num_images,
                         const int32_t* image_problem, const int32_t* image_view, int height, int width,
                         const uint8_t* images, uint8_t* out, int32_t* face_id);

/* Several bodies in one image (the reference's Renderer.render_multiperson, utils.py:1030-1099, which nothing in the
 * reference calls: its save_images path is single-person).  Image i shows the problems
 * body_problem[image_first[i] .. image_first[i+1]) (host arrays, CSR) seen by view image_view[i], and is rendered EXACTLY
 * AS mvfit_render_overlay WOULD RENDER THE ONE MESH THAT CONCATENATES THE IMAGE'S BODIES IN LIST ORDER: body k of the image
 * (slot k = 0 .. n_i - 1) contributes vertex k Nv + j for its vertex j and face k Nf + f for its face f.  Hence
 *   transform, coverage, depth, znear / zfar, guard band: as above, per vertex and face;
 *   visibility key = (fp32 bits of z) << 32 | (k Nf + f), one 64-bit minimum per covered sample into the image's one
 *              visibility buffer: bodies occlude one another, a depth tie goes to the lower slot, then the lower face;
 *   vertex normals per body (bodies share no vertex);
 *   lights     placed from the axis-aligned box of the camera-space vertices of ALL bodies of the image;
 *   shading    with acc the light sum above and c the body's colour channel (float, widened to double):
 *              s = c * 0.3 + (c / pi) acc, byte = floor(255 min(1, s)^(1/2.2) + 0.5) per channel (c = 0.5: the grey of
 *              mvfit_render_overlay, term for term);
 *   colours    body_color[image_first[num_images]][3] host, RGB in [0, 1], or NULL: slot k takes entry k mod 7 of the
 *              reference's palette in its dictionary order (utils.py:904-912): (.8,.1,.1) (.1,.1,.8) (.1,.8,.1) (.7,.7,.9)
 *              (.9,.9,.8) (.7,.75,.5) (.5,.7,.75);
 *   dots       the num_points points of every body of the image, same rule, drawn last;
 *   outputs    face_id[num_images,H,W] = f (within the body), body_id[num_images,H,W] = slot k, int32 dev or NULL, both -1
 *              where nothing is drawn;
 *   cameras    the shared rig, or with per-problem cameras those of the image's first body's problem.
 * An image with an empty list is copied through (ids -1).  A problem may appear in several images and twice in one.
 * MVFIT_E_STATE as mvfit_render_overlay.  MVFIT_E_ARG: a NULL image_first / image_view (or body_problem with a body
 * listed), image_first not starting at 0 or decreasing, a problem or view out of range, a colour outside [0, 1] or not
 * finite, more than 256 bodies in one image, and the size limits of mvfit_render_overlay.  Asynchronous on the ctx stream
 * (the host arrays have been read when the call returns).  Consecutive images are processed in groups of at most 64 whose
 * workspace - per (image, body) instance 56 B x Nv + 4 B x Nf, per image 8 H W bytes - is at most 256 MB, or one image's
 * when that alone is larger; the result does not depend on the grouping. */
int mvfit_render_scene(mvfit_ctx* ctx, const float* vertices, const float* points, int num_points, int num_images,
                       const int32_t* image_first, const int32_t* body_problem, const int32_t* image_view,
                       const float* body_color, int height, int width, const uint8_t* images, uint8_t* out,
                       int32_t* face_id, int32_t* body_id);

/* The path's only collective (north_star: "RCCL over xGMI only for the final gather"; in the Python adapters it is one
 * torch.distributed.all_gather, mvsmplfitting_amd/sharding.py): all-gather over the caller's RCCL communicator on the ctx
 * stream - rank r's bytes_per_rank bytes at `send` land at recv + r * bytes_per_rank on every rank.  For hosts that own
 * a communicator (a C / C++ driver); the reference has no counterpart (single process, code/main.py:60-120).
 *   rccl_comm: the host's ncclComm_t.  libmvfit does not link RCCL - ncclAllGather is bound at run time to the RCCL
 *   library already loaded in the process (the one the communicator belongs to); MVFIT_E_STATE if there is none.
 *   send[bytes_per_rank], recv[nranks * bytes_per_rank] dev; asynchronous like every other call (mvfit_sync). */
int mvfit_gather(mvfit_ctx* ctx, void* rccl_comm, const void* send, void* recv, size_t bytes_per_rank);

/* Timing hook for bench.py: average duration (ms) of the LBS vertex-pass kernel launches since
 * the last call, measured with hipEvents on the ctx stream; *launches = number measured.
 * Enable with mvfit_profile(ctx, 1) (adds two event records per launch). */
int mvfit_profile(mvfit_ctx* ctx, int enable);
int mvfit_profile_read(mvfit_ctx* ctx, double* vertex_pass_ms_avg, int* launches,
                       double* step_kernel_ms_avg, int* step_launches);
/* `launches` back-to-back launches of the vertex pass (pose operands as the last closure / fit left them)
 * inside ONE hipEvent pair on the ctx stream; *avg_ms = elapsed / launches.  A pair around a single launch
 * (mvfit_profile_read) contains the markers' own few microseconds; this amortises them. */
int mvfit_profile_vertex_pass(mvfit_ctx* ctx, int launches, double* avg_ms);
/* flavour 0: as above; 1: the pass exactly as the asynchronous fit launches it (operands from its ring, non-temporal
 * basis stream and vertex stores, no side outputs) - needs a preceding asynchronous mvfit_fit on this batch. */
int mvfit_profile_vertex_pass_ex(mvfit_ctx* ctx, int launches, int flavour, double* avg_ms);
/* How the vertex passes of the last asynchronous mvfit_fit ran:
 *   *tiles_per_wg  the form of mvfit_options::resident_pass that ran.  1 / 2 / 3: the RESIDENT pass - one launch per (sub-batch)
 *                  fit whose workgroups keep the blendshape basis of their one / two / two vertex tile(s) in registers and serve
 *                  closure round after closure round from the operand ring (the basis crosses the memory system once per fit;
 *                  3 = two tiles with the workgroup split into contraction and worker waves, the automatic choice beside more
 *                  than 36 optimiser workgroups); 0: one gate + one pass launch per closure round (dense skinning rows,
 *                  exact-fp32 contraction, or launches that leave no CUs for resident workgroups);
 *   *workgroups    workgroups of the resident pass (ceil(tiles / tiles per workgroup));
 * and, when the fit ran under mvfit_profile(ctx, 1) with the resident pass, what its workgroups stamped per closure round
 * (wall clock, 10 ns ticks; the first 1024 rounds of the last sub-batch):
 *   *rounds        rounds stamped;
 *   *span_ms       mean over the rounds of (last workgroup's vertex stores acknowledged - first workgroup saw the round's
 *                  operands): the in-fit service time of a round - what mvfit_profile_read reports as the launch duration;
 *   *busy_ms       mean over rounds and workgroups of a workgroup's own (stores acknowledged - operands seen);
 *   *slowest_ms    mean over the rounds of the SLOWEST workgroup's (stores acknowledged - operands seen): the rate at which the
 *                  pass can serve rounds (when the passes are slower than the optimiser the workgroups drift apart by up to the
 *                  ring's depth and the span of a round says nothing about that rate).
 * Any pointer may be NULL.  flavour 2 of mvfit_profile_vertex_pass_ex runs the resident pass ALONE over `launches` (<= 128)
 * rounds whose operands the last fit left in the ring: one kernel launch inside one hipEvent pair, avg_ms = elapsed / rounds. */
int mvfit_pass_profile(mvfit_ctx* ctx, int* tiles_per_wg, int* workgroups, int* rounds, double* span_ms, double* busy_ms,
                       double* slowest_ms);

/* Known-answer test entry for the device L-BFGS state machine (same template as production,
 * instantiated in float64) on the analytic objectives of oracle/lbfgs_np.py:kat_objective.
 *   kind: 0 quad, 1 rosen, 2 gmof, 3 linear, 4 wavy, 5 wavy2, 6 steep, 7 steep2 (| 0x100: the direction in compact form) - any
 *   other kind is MVFIT_E_ARG ; D <= 96 ; x_inout[D] host ; trace[max_trace,(D+1)] host
 *   (x_trial, loss per closure) ; segs[nseg+1] parameter-tensor boundaries for the gtol test ;
 *   opts as for mvfit_fit (num_stages and max_rounds are not read): max_iter, maxiters > 0 and
 *   1 <= history <= MVFIT_HISTORY, else MVFIT_E_ARG before anything is launched. */
#define MVFIT_KAT_KINDS 8
int mvfit_lbfgs_kat(int device, int kind, int D, const int32_t* segs, int nseg,
                    const mvfit_lbfgs_opts* opts, double* x_inout, double* trace, int max_trace,
                    int* n_closure, double* final_loss);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* MVFIT_H_ */
