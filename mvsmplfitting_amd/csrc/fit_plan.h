// How a fit runs, decided before anything is launched (plain C++17, no HIP): plan_fit turns the facts a fit's path depends on
// into its phases, each with its driver, sub-batch size, form of the vertex passes, work queue and list of launches.
// mvfit_fit executes the plan and decides nothing.  The rules as one table: DESIGN.md §4.4.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/mvfit.h"
#include "model_layout.h"

namespace mvfit {

// ---- sizing: workgroups of a single-launch fit hold a CU each (LDS), and all of them must be resident at once ----
constexpr int kAsyncMaxB = 160;        // asynchronous fit, per-round pass launches: one CU per problem, >= 96 CUs left to the passes
constexpr int kResidentMaxB = 128;     // beside the resident pass: its workgroups (ntiles / 2 at this size) hold a CU each for the whole fit
constexpr int kPassWords = 512;        // back-pressure words of the ring (one per resident-pass workgroup; the gate kernels use word 0)
// decoder helpers (vposer_service.h): sets of VPS_SLICES helper workgroups behind the problems' ones
constexpr int kVpsSets = 8;                                             // sets of a launch with more than 32 problems
constexpr int kVpsHelpers = kVpsSets * VPS_SLICES;                      // 64 CUs
constexpr int kVpsMaxSparse = 160, kVpsMaxAsync = 96;                   // problems per launch: objective vertices only / asynchronous
static_assert(kVpsMaxSparse <= kVpsSets * VPS_PMAX && kVpsMaxSparse + kVpsHelpers <= 256 && 32 + VPS_MAX_SETS * VPS_SLICES <= 160, "all workgroups resident");

// everything the decisions depend on
struct FitPlanIn {
    int B = 0, n_cu = 0, ntiles = 0;     // problems, compute units of the device, 32-vertex tiles of the model
    bool half_basis = false;             // the model has the split-fp16 basis (not MVFIT_CONTRACTION_EXACT_FP32)
    bool sparse_skinning = false;        // the model has the 4-weight skinning rows (not dense_skinning, no vertex with more weights)
    bool nv_even = false;                // the resident pass stores vertex pairs
    bool helper_memory = false;          // the ctx has the decoder helpers' granules (model with a VPoser decoder)
    bool profile = false;                // mvfit_profile is on
    bool resident_auto_off = false;      // automatic resident_pass: an earlier fit on this ctx timed out waiting
    bool debug_nopass = false;           // MVFIT_DEBUG_NOPASS (hooks build only)
    // mvfit_options
    int round_mode = 0, resident_pass = -1, sdf_two_phase = 1, sdf_service = 1, vposer_helpers = 1, vposer_sets = 0, work_queue = 1;
    // the fit
    uint32_t flags = 0;                  // MVFIT_F_* (the same in all stages)
    uint32_t sdf_stages = 0;             // bit s: stage s has coll_loss_weight > 0
    int num_stages = 1;
    bool reuse_outer = false;            // MVFIT_F_REUSE_OUTER_VALUE as the optimiser reads it
    int cap = 0;                         // closure rounds a problem may take
};

enum FitDriver {
    DRIVER_ASYNC = 0,      // single launch per sub-batch, full vertex passes beside it
    DRIVER_ASYNC_SDF = 1,  // the same with the SDF term as a service (per-round gate -> pass -> term launches)
    DRIVER_SPARSE = 2,     // single launch per sub-batch, objective vertices only
    DRIVER_GRAPH = 3,      // chained (vertex pass [-> term] -> step kernel) rounds replayed as a graph
    DRIVER_EAGER = 4,      // the same rounds as eager launches bracketed by events (profiled fits)
};

struct FitLaunch {
    int b_lo, b_hi;        // problems (refill: ring rows) of the launch
    int n_target;          // problems that leave it
    int nsets;             // decoder-helper sets it carries (0: none)
};

struct FitPhase {
    int driver = DRIVER_GRAPH;
    int pause_stage = MVFIT_MAX_STAGES + 1;     // lead phase: problems leave the launch in front of this stage
    // asynchronous drivers
    int per = 0;                                // sub-batch size = ring rows
    int form = 0;                               // vertex passes: 0 a gate + a pass launch per round; 1 / 3 the resident pass (tiles per workgroup / roles kernel)
    int res_grid = 0;                           // workgroups of the resident pass
    bool refill = false;                        // ONE launch with a work queue: a row takes the next problem when its own has finished
    int launch_cap = 0;                         // round cap of the phase's launches (refill: of a row over all its problems); every driver
    std::vector<FitLaunch> launches;            // asynchronous and sparse drivers: one per sub-batch
};

struct FitPlan {
    int rc = MVFIT_OK;                          // MVFIT_E_ARG: err says why
    std::string err;
    bool init_full_pass = false;                // fit_init_kernel publishes the pose operands of the first trial point (chained rounds from the start)
    int nphases = 0;
    FitPhase phase[2];                          // [lead phase that pauses at the first stage with the SDF term,] tail
};

FitPlan plan_fit(const FitPlanIn& in);

// decoder-helper sets behind n problems; vposer_sets: mvfit_options::vposer_sets (0 automatic); with_passes: vertex passes run
// beside the launch - the automatic choice then takes 8 sets where 16 would leave no room for the resident pass
int plan_nsets(const FitPlanIn& in, int n, int vposer_sets, bool with_passes);
// workgroups of the resident pass in form 1 / 3 (FitPhase::form)
int plan_resident_grid(int form, int ntiles);

// The instantiations of the single-launch kernel (fit_kernels.hip: persistent_kernel() names one kernel per value):
// fit_persistent_kernel<REMOTE, REUSE, LEAN, SDFS, QUEUE>
enum PersistentVariant {
    PV_PLAIN = 0,          // <0,0,0>
    PV_LEAN,               // <0,0,1>      the stage flags carry none of VPoser / GMM / 3-D term
    PV_REUSE,              // <0,1,0>      MVFIT_F_REUSE_OUTER_VALUE
    PV_REUSE_LEAN,         // <0,1,1>
    PV_HELPERS,            // <1,0,0>      the launch carries decoder helpers
    PV_HELPERS_REUSE,      // <1,1,0>
    PV_QUEUE,              // <0,0,0,0,1>  the launch has a work queue
    PV_QUEUE_LEAN,         // <0,0,1,0,1>
    PV_SDF,                // <0,0,0,1>    the launch serves stages with the SDF term
    PV_SDF_HELPERS,        // <1,0,0,1>
    PV_COUNT
};
// which one a launch runs: the service first, then the queue, then helpers; reuse_outer and lean count only where the row above
// has an instantiation for them
PersistentVariant plan_persistent_variant(bool sdf_service, bool queue, bool helpers, bool reuse_outer, bool lean);

// The kernels of a per-round vertex pass (vertex_pass.hip: launch_vertex_pass switches on the result)
enum PassKernel {
    PASS_EXACT = 0,        // lbs_vertex_pass_kernel<sparse>             exact fp32 MFMA chain, one workgroup per (tile, chunk)
    PASS_SPLIT,            // lbs_vertex_pass_split_kernel<sparse>       split-fp16, one workgroup per (tile, chunk)
    PASS_SPLIT_LOOP,       // lbs_vertex_pass_split_loop_kernel<false>   split-fp16, one workgroup per tile walks the chunks in lock-step
    PASS_PIPE,             // lbs_vertex_pass_pipe_kernel                split-fp16, the same walk as a two-role pipeline
    PASS_KERNEL_COUNT
};
struct PassLaunch {
    int kernel;            // PassKernel
    bool sparse;           // the 4-pair skinning blend (the SPARSE_W instantiation; the pipeline has no other)
    int grid_y;            // workgroups per vertex tile: the chunks, or 1 for the kernels that walk them
};
// split_basis: the model has the split-fp16 basis (full or half width); chunks = ceil(B / 32) - first chunk of the launch;
// pass_kernel: mvfit_options::pass_kernel (1: one workgroup per (tile, chunk) at any number of chunks; 2 = 0).
// The pipeline stores vertex pairs: an odd vertex count with sparse skinning rows takes one workgroup per (tile, chunk).
PassLaunch plan_pass_launch(bool split_basis, bool sparse_skinning, bool nv_even, int chunks, int pass_kernel);

}  // namespace mvfit
