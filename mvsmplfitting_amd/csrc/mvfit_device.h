// Shared device-side structures of libmvfit (gfx950 / wave64 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mvfit.h"
#include "model_layout.h"
#include "wave_ops.h"
#include "lbfgs_device.h"
#include "vposer_service.h"

namespace mvfit {

// NJ, NKP, KROWS, TILE_V, NS_MAX, ... and ModelLds: model_layout.h
constexpr int RENDER_GROUP_MAX = 64;   // images per launch group of mvfit_render_overlay (render.hip)
// mvfit_render_scene: device tables of int32 words - per image {first instance, count, view, camera problem}, per instance
// {problem, image, slot, colour r g b as float bits}
constexpr int SCENE_IMAGE_WORDS = 4, SCENE_INST_WORDS = 6;
constexpr int SCENE_BODIES_MAX = 256;  // bodies per image
constexpr int DV = MVFIT_D;       // 118
constexpr int DPAD = 128;
constexpr int A_STRIDE = 288;     // per-problem stride of the 24x12 skinning transforms in LDS (vertex pass): the HBM stride, so that a chunk's
                                  // transforms are one linear global -> LDS copy
constexpr int STEP_NT = 512;      // threads of the per-problem kernels (8 waves)
constexpr int STEP_NW = STEP_NT / 64;

// flat parameter layout (include/mvfit.h)
constexpr int X_BETAS = 0, X_GO = 10, X_BP = 13, X_TR = 82, X_SC = 85, X_EMB = 86;

// skeleton joint whose posed position is keypoint k, or -1 (a vertex-selection row)
__host__ __device__ __forceinline__ int kp_joint_of(const ModelLds& C, int k) {
    const int j = (int)((C.kp_joint[k / 6] >> (5 * (k % 6))) & 31u);
    return j == 31 ? -1 : j;
}

// The model's constants on the device: HostModel's tables (model_prep.h documents every layout), uploaded by mvfit_create_ex
struct DevModel {
    int nv, nv_pad, ntiles;
    const float* bs4;        // blendshape basis in MFMA-B-operand order (see vertex pass)
    const float4* bs_h2;     // the same basis split into fp16 (hi, lo) pairs for the fp16 matrix pipe (null: exact-fp32 contraction)
    float bs_scale;          // the power of two bs_h2 is scaled by
    int half_basis;          // 1: the contraction reads only the hi halves of the split basis (2 bytes per element, configs[4])
    const float* vt_planes;
    const float* wt_tiles;
    const float4* wsp_w;     // sparse skinning (null unless every vertex has <= 4 non-zero weights)
    const int4* wsp_j;
    const float* bs_vm;      // vertex-major copies for the per-vertex pull-back of the SDF term (sdf_term.hip)
    const float* w_vm;
    // objective-relevant vertex subset
    int ns, nc, nc_pad;
    const ModelLds* mlds;    // LDS image (global copy)
    const int* sel_v;
    const float* pd_sub;
    const float* pd_subT;
    // vertex-pass side outputs for the selected vertices: per tile, which local vertices are selected
    const int* tile_sel_start;
    const int* tile_sel_local;
    const int* tile_sel_slot;
    // VPoser decoder (null if absent)
    const float* vp_w1; const float* vp_b1;
    const float* vp_w2; const float* vp_b2;
    const float* vp_w3; const float* vp_b3;
    const float* vp_w1T;
    const float* vp_w2T;
    const float* vp_w3T;
    VpTiles vpt;                                // the same weights as register tiles of the decoder helpers (vposer_service.h)
    VpService vps;                              // per launch: the helpers of THIS launch (nsets == 0: none)
    // GMM
    int gmm_M;
    const float* gmm_means;
    const float* gmm_prec;
    const float* gmm_precT;
    const float* gmm_lognw;
};

struct DevProblems {
    int B, V, cam_batched;
    const float* cam_R;   // [.,V,9]
    const float* cam_t;   // [.,V,3]
    const float* cam_f;   // [.,V]
    const float* cam_c;   // [.,V,2]
    const float* gt_xy;   // [B,V,17,2]
    const float* w_conf;  // [B,V,17]
};

struct DevWeights {          // one stage
    float data_w2;           // data_weight^2
    float pose_w;            // body_pose_weight
    float shape_w;
    float bend_w;
    float coll_w;
    float rho2;
    uint32_t flags;
    uint32_t pad;
};

// per-problem pose workspace handed from the step kernel to the vertex pass
//   coefT [B/32][KROWS][32]   (pose_feature | betas | 0), transposed per 32-problem chunk
//   coefH the same coefficients, split into fp16 (hi, lo) pairs in MFMA A-operand order
//   Amat  [B][24][12]
//   tau   [B][4]
// and back (vertex pass -> step kernel), for the selected vertices only:
//   vposed_sel [B][NC_MAX]   blendshaped rest positions  (lbs.py:203), c = 3 s + a
//   xs_sel     [B][NC_MAX]   skinned positions before "+ transl"
struct DevPose {
    float4* coefH;           // [B/32][14 blocks][hi, lo][64 lanes] 16-byte words: the coefficients of a chunk as
                             // split-fp16 MFMA A operands (problem = lane & 31, rows 16 G + 8 (lane >> 5) + t)
    float* coefT;
    float* Amat;
    float* tau;
    float* vposed_sel;
    float* xs_sel;
    // asynchronous fit (mvfit_fit without the SDF term): the operands are a ring slot that the optimiser kernel
    // publishes while this pass is already queued; tag != nullptr makes the pass wait for them (vertex_pass.hip)
    const unsigned* tag;         // [Bpad] of this slot: round + 1 of the trial point each problem's operands belong to
    const unsigned* done_round;  // [Bpad] closures evaluated by a finished problem (0xffffffff while it is running)
    unsigned* stats;             // [4] passes run / chunk passes skipped (all problems finished) / missed / timed out
    unsigned round;              // closure round this pass belongs to
    unsigned pad_;
    // sub-batch of the asynchronous fit (mvfit_fit time-slices batches with more problems than the optimiser gets CUs):
    // this launch covers the 32-problem chunks from chunk0 on, up to the problem count it is given
    int chunk0;
    unsigned* pass_done;         // [1] rounds whose pass has completed (written by the gate of the next round)
    unsigned long long* box_part; // [B][ntiles][6] min / max keys of the tile's vertices per axis (single-chunk split kernel; the SDF
                                 // term's bounding box is reduced from them), or null
};

// Pose-operand ring of the asynchronous fit: slot (r % nslots) holds, per problem, the vertex-pass operands of the
// trial point of that problem's closure round r.  Producer: fit_persistent_kernel (write-through sc1 stores, then
// the problem's tag); consumer: the vertex pass launched for round r (polls the tags of its 32 problems).
struct AsyncRing {
    float4* coefH;               // [nslots][Bpad / 32][KROWS / 16][hi, lo][64]
    float* Amat;                 // [nslots][Bpad][288]
    float* tau;                  // [nslots][Bpad][4]
    unsigned* tag;               // [nslots][Bpad]
    unsigned* done_round;        // [Bpad]
    unsigned* stats;             // [4]
    int* host_done;              // pinned host word: set to the number of problems by the last one to finish
    int nslots, Bpad;
    // back-pressure: rounds whose vertex pass has completed.  A problem publishes round r into slot r % nslots only once
    // the pass of round r - nslots has run (pass_done > r - nslots): a slot is never overwritten before its pass read it,
    // however slow the passes are (the optimiser is throttled to their rate instead).
    // npass words, the minimum counts: ONE written by the gate kernels of the per-round launches, or one per workgroup of
    // the resident pass (rounds whose operands that workgroup has read) - no atomics, every writer owns its word.
    unsigned* pass_done;
    int npass, rpad_;
};

// Resident vertex pass of the asynchronous fit (lbs_vertex_pass_resident_kernel, vertex_pass.hip): ONE launch per
// (sub-batch) fit; every workgroup keeps the basis of its vertex tile(s) in registers and serves closure round after
// closure round from the ring.
struct ResidentArgs {
    const float4* coefH;         // ring bases: slot 0, problem 0 of the sub-batch
    const float* Amat;
    const float* tau;
    const unsigned* tag;
    const unsigned* done_round;  // [Bpad] by global problem index
    unsigned* stats;             // [4] chunk passes run / skipped / missed / timed out
    unsigned* wg_round;          // [grid] back-pressure words (AsyncRing::pass_done)
    unsigned long long* log;     // mvfit_profile: [log_rounds][grid][2] wall-clock stamps {operands seen, stores drained}, or null
    float* verts;                // [B][nv][3] by global problem index
    float* capture_verts;        // test hook: the round capture_round is written here instead
    int capture_round;
    int nslots, rb;              // ring geometry: slots, problems per slot
    int b_lo, n;                 // the sub-batch: global index of its first problem, number of problems
    int log_rounds;
    unsigned flags;              // bit 1: plain (not non-temporal) vertex stores
    unsigned max_rounds;
};

// SDF interpenetration term (fitting.py:352-393), per problem
struct SdfBox {              // bounding box of the vertices: centre, scale, arg indices (fitting.py:282-288,356-359)
    float c[3];
    float s;
    int imin[3];
    int imax[3];
    int amax;                // axis of the largest extent
    int pad;
};
struct SdfAdj {              // S = sum_v phi_v and its adjoint w.r.t. the vertex pass operands
    float S;
    float gtau[3];
    float gA[NJ * 12];       // per joint [g_Ar (a-major 3x3) | g_At (3)]: the accumulator order of the closure's E6
    float gcoef[KROWS];
};
static_assert(sizeof(SdfAdj) % 16 == 0, "16-byte block");

}  // namespace mvfit
