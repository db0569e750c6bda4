// Layout of the model constants the kernels read: the sizes their tables depend on and the ModelLds image.  Shared by the
// device code (mvfit_device.h, vposer_service.h), the host builder of the tables (model_prep.cpp) and the fit's planning
// (fit_plan.cpp), so it includes no HIP header.
#pragma once
#include <stdint.h>

namespace mvfit {

constexpr int NJ = 24;            // SMPL joints
constexpr int NKP = 17;           // dataset keypoints
constexpr int KROWS = 224;        // blendshape rows: 207 pose + 10 shape, padded to 28*8
constexpr int KGROUPS = 28;       // groups of 4 MFMA k-steps (8 rows) each
constexpr int TILE_V = 32;        // vertices per MFMA tile
constexpr int NS_MAX = 96;        // selected (objective-relevant) vertices
constexpr int NS_STRIDE = 112;    // row stride of the transposed skinning weights (== 16 mod 32: the four
                                  // 16-lane rows of a wave hit disjoint LDS banks)
constexpr int NC_MAX = NS_MAX * 3;
constexpr int KNNZ_MAX = 160;     // non-zeros of the 17 x ns keypoint selection
constexpr int KP_NZ = 12;         // padded per-keypoint list length (LSP regressor rows have 4-9 non-zeros)
constexpr int VS_NZ = 2;          // padded per-vertex list length (a vertex usually feeds one keypoint)
constexpr int VPS_SLICES = 8;     // VPoser decoder helpers per set = slices of the 512 fc2 units (vposer_service.h)
constexpr int VPS_PMAX = 24;      // problems per helper set (wave w polls the slots w, w + 8, w + 16)
constexpr int VPS_MAX_SETS = 16;  // 16 for launches of <= 32 problems, else 8 (fit_plan.h)

// Who does what in the closure's first two phases (closure_device.h: pose_prep_elems, sparse_forward), as plain functions
// the host can evaluate (tests/test_fwd_items_cpu.py restates them).
// E1, 512 threads: thread tid < E1_POSE_T is (joint j, element e) = (tid / 12, tid % 12) - e < 9: one Rodrigues, the word
// R[j][e], its Mj word and, for j >= 1, the pose feature coef[9 (j - 1) + e]; e >= 9: J[j][e - 9] and Mj's translation column -,
// the next KROWS - 207 threads write the betas and the zero padding of coef.  Waves 5-7 have no E1 work.
constexpr int E1_POSE_T = NJ * 12;                          // 288
constexpr int E1_NPOSE = (NJ - 1) * 9;                      // 207 words of the pose feature
constexpr int E1_WORKERS = E1_POSE_T + (KROWS - E1_NPOSE);  // 305
constexpr int E1_IDLE_T0 = 320;                             // first thread of the waves without E1 work
static_assert(E1_WORKERS <= E1_IDLE_T0 && E1_IDLE_T0 % 64 == 0, "E1's workers leave whole waves free");
// E2's forward basis stream: FWD_SLICES k-slices x nc_pad / 4 float4 column groups = items; stream thread t (thread 64 + t
// of the workgroup, waves 1-7) owns the items t and t + FWD_THREADS that exist.  The threads of the waves that idle in E1
// (t >= FWD_EARLY_T0) never own a second item and load their first one there, one barrier ahead of its FMAs.
constexpr int FWD_SLICES = 8, FWD_RPS = KROWS / FWD_SLICES;      // 28 basis rows per k-slice of the forward contraction
constexpr int FWD_THREADS = 512 - 64, FWD_EARLY_T0 = E1_IDLE_T0 - 64;
static_assert(FWD_EARLY_T0 + FWD_THREADS >= (NC_MAX / 4) * FWD_SLICES, "an early thread owns one item at most");
struct FwdOwner { int first, n; bool early; };              // items first, first + FWD_THREADS, ... (n of them); early: the first one
constexpr FwdOwner fwd_item_owner(int nc_pad, int t) {
    const int nitems = (nc_pad >> 2) * FWD_SLICES;
    const int n = t >= nitems ? 0 : (t + FWD_THREADS < nitems ? 2 : 1);
    return FwdOwner{t, n, n > 0 && t >= FWD_EARLY_T0};
}

// Model constants every per-problem workgroup keeps in LDS (bulk-copied once per launch).
struct ModelLds {
    float wT[NJ][NS_STRIDE];          // lbs_weights of the selected vertices, transposed: wT[j][s]
    float J_t[NJ * 3];                // J_regressor . v_template
    float J_S[NJ * 3][11];            // J_regressor . shapedirs  (row padded to 11: conflict-free by lane)
    float vt_sub[NC_MAX];             // v_template of the selected vertices, c = 3 s + a
    int sel_v[NS_MAX];                // vertex id of selected vertex s
    int kp_start[NKP + 1];            // keypoint k = sum_t kp_w[t] * xs[kp_s[t]]  (ascending s)
    int kp_s[KNNZ_MAX];
    float kp_w[KNNZ_MAX];
    int vs_start[NS_MAX + 1];         // transpose: selected vertex s feeds keypoints vs_k[t] (ascending k)
    int vs_k[KNNZ_MAX];
    float vs_w[KNNZ_MAX];
    // the same selection as fixed-length zero-padded lists (all index loads of a thread in one LDS round
    // trip instead of one per CSR entry); padded = 0 when a row is longer than the padding (CSR is used)
    int kpp_s[NKP][KP_NZ];
    float kpp_w[NKP][KP_NZ];
    int vsp_k[NS_MAX][VS_NZ];
    float vsp_w[NS_MAX][VS_NZ];
    int padded;
    // source of each keypoint, 5 bits per keypoint, six keypoints per word (kp_joint_of): a posed skeleton joint j < 24 (model
    // without a keypoint regressor, 'smpl' / 'coco17': keypoint = G_j's translation column + transl) or 31 = a row of the
    // vertex selection above (every keypoint of a model with a regressor); n_skel = keypoints of the first kind
    unsigned kp_joint[3];
    int parents[NJ];
    int nlevels;
    int level_start[NJ + 1];
    int level_joints[NJ];
    int child_start[NJ + 1];
    int child_list[NJ];
    // kinematic chain schedules for ONE wave (12 lanes per joint, 5 joints per pass):
    //   fwd_tab[pass][q] = j | parent << 8 (or -1): joints whose parent transform is complete
    //   bwd_tab[pass][q] = parent | 0x80 if not its first entry | c0 << 8 | c1 << 16 | c2 << 24 (or -1), child 31 = none
    int n_fwd, n_bwd;
    int fwd_tab[NJ][5];
    int bwd_tab[NJ][5];
    // pointer-jumping form of the forward chain: anc_tab[s][j] = the 2^s-th ancestor of joint j (-1: above the root);
    // n_jump = steps until every path product is complete (2^n_jump >= joints on the longest path)
    int anc_tab[5][NJ];
    int n_jump, n_skel, jpad1, jpad2;
    int ns, nc, nc_pad, pad0;
    // the selected vertices' skinning weights as <= 4 (weight, joint) pairs in ascending joint order, zero-padded (the
    // non-zero products of the dense row in the same order: the same bits); sel_sparse = 0 when a row has more than 4
    float selw[NS_MAX][4];
    unsigned selj[NS_MAX];            // four joint indices, one per byte
    // e6_cells = 1: every cell of the adjoint's E6 (joint j, lane g = s mod 16) has <= E6_NZ non-zero weights and sel_sparse
    // is 1 - the kernels' prologue then lays HostModel::e6_cells over the first E6_ROW_BYTES of each row of wT, which nothing
    // else reads in that case (the image itself always holds the dense wT)
    // stream_late: always 0 in the image the host builds; the -DMVFIT_DEBUG_HOOKS build sets bit 0 on request (MVFIT_BWD_STREAM_LATE)
    // and only that build's kernels read it: every wave of the adjoint's transposed stream then loads inside E7; bit 1
    // (MVFIT_FWD_STREAM_LATE): every wave of the forward stream loads inside E2; bit 2 (MVFIT_VIEW_SUMS_SERIAL): E4 sums the
    // views' keypoint gradients and g_tau's parts in loops of conditional reads, the form before the batched loads
    int sel_sparse, e6_cells, stream_late, spad2;
};
constexpr int E6_NZ = 4;                                // padded entries per E6 cell
constexpr unsigned E6_INVALID = 0x8000u;                // entry = 4 s + t (the word selw[s][t]) | E6_INVALID for padding
constexpr int E6_ROW_BYTES = 16 * E6_NZ * 2;            // one joint's sixteen cells of 16-bit entries
static_assert(E6_ROW_BYTES % 16 == 0 && E6_ROW_BYTES <= NS_STRIDE * 4 && NS_MAX * 4 <= (int)E6_INVALID, "E6 cells fit a row of wT");
static_assert(sizeof(ModelLds) % 16 == 0, "ModelLds is bulk-copied as 16-byte words");
static_assert(NKP <= 18 && NJ < 31, "kp_joint packs six 5-bit entries per word");

}  // namespace mvfit
