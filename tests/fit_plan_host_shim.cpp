// Host build of csrc/fit_plan.cpp for tests/test_fit_plan_cpu.py (clang++ -O2 -shared -fPIC, no HIP): the plan's inputs as a
// flat int array in FitPlanIn's member order, the plan as a flat int array, so the decisions of mvfit_fit can be checked
// without a GPU.
#include <cstdint>
#include <cstdio>

#include "../mvsmplfitting_amd/csrc/fit_plan.h"

using namespace mvfit;

static FitPlanIn inputs(const int32_t* v) {
    FitPlanIn in;
    int i = 0;
    in.B = v[i++]; in.n_cu = v[i++]; in.ntiles = v[i++];
    in.half_basis = v[i++] != 0; in.sparse_skinning = v[i++] != 0; in.nv_even = v[i++] != 0; in.helper_memory = v[i++] != 0;
    in.profile = v[i++] != 0; in.resident_auto_off = v[i++] != 0; in.debug_nopass = v[i++] != 0;
    in.round_mode = v[i++]; in.resident_pass = v[i++]; in.sdf_two_phase = v[i++]; in.sdf_service = v[i++];
    in.vposer_helpers = v[i++]; in.vposer_sets = v[i++]; in.work_queue = v[i++];
    in.flags = (uint32_t)v[i++]; in.sdf_stages = (uint32_t)v[i++]; in.num_stages = v[i++]; in.reuse_outer = v[i++] != 0;
    in.cap = v[i++];
    return in;
}

// out: rc, init_full_pass, nphases, then per phase: driver, pause_stage, per, form, res_grid, refill, launch_cap, launches and
// (b_lo, b_hi, n_target, nsets) per launch.  Returns the words the plan takes (written up to out_cap).
extern "C" int fit_plan_run(const int32_t* in, int32_t* out, int out_cap, char* err, int errlen) {
    const FitPlan p = plan_fit(inputs(in));
    int n = 0;
    auto put = [&](int v) { if (n < out_cap) out[n] = v; ++n; };
    put(p.rc); put(p.init_full_pass); put(p.nphases);
    for (int i = 0; i < p.nphases; ++i) {
        const FitPhase& ph = p.phase[i];
        put(ph.driver); put(ph.pause_stage); put(ph.per); put(ph.form); put(ph.res_grid); put(ph.refill); put(ph.launch_cap);
        put((int)ph.launches.size());
        for (const FitLaunch& L : ph.launches) { put(L.b_lo); put(L.b_hi); put(L.n_target); put(L.nsets); }
    }
    snprintf(err, errlen, "%s", p.err.c_str());
    return n;
}

extern "C" int fit_plan_nsets(const int32_t* in, int n, int vposer_sets, int with_passes) {
    return plan_nsets(inputs(in), n, vposer_sets, with_passes != 0);
}

extern "C" int fit_plan_persistent_variant(int sdf_service, int queue, int helpers, int reuse_outer, int lean) {
    return plan_persistent_variant(sdf_service != 0, queue != 0, helpers != 0, reuse_outer != 0, lean != 0);
}
extern "C" int fit_plan_persistent_variant_count() { return PV_COUNT; }

// the kernel of a per-round vertex pass: out3 = kernel (PassKernel), sparse, grid_y
extern "C" void fit_plan_pass_launch(int split_basis, int sparse_skinning, int nv_even, int chunks, int pass_kernel, int32_t* out3) {
    const PassLaunch L = plan_pass_launch(split_basis != 0, sparse_skinning != 0, nv_even != 0, chunks, pass_kernel);
    out3[0] = L.kernel; out3[1] = L.sparse; out3[2] = L.grid_y;
}
extern "C" int fit_plan_pass_kernel_count() { return PASS_KERNEL_COUNT; }

// kAsyncMaxB, kResidentMaxB, kPassWords, kVpsSets, kVpsMaxSparse, kVpsMaxAsync, VPS_PMAX, VPS_MAX_SETS, VPS_SLICES, MVFIT_MAX_STAGES
extern "C" void fit_plan_constants(int32_t* out10) {
    const int v[10] = {kAsyncMaxB, kResidentMaxB, kPassWords, kVpsSets, kVpsMaxSparse, kVpsMaxAsync, VPS_PMAX, VPS_MAX_SETS, VPS_SLICES,
                       MVFIT_MAX_STAGES};
    for (int i = 0; i < 10; ++i) out10[i] = v[i];
}
