// plan_fit: the decisions of mvfit_fit (fit_plan.h).  The measured reasons behind the rules: DESIGN.md §4.4.
#include "fit_plan.h"

#include <algorithm>
#include <cstdio>

namespace mvfit {

int plan_resident_grid(int form, int ntiles) {
    if (!form) return 0;
    const int tiles = form >= 2 ? 2 : 1;
    return (ntiles + tiles - 1) / tiles;
}

namespace {

// Form of the vertex passes beside opt_grid optimiser-kernel workgroups (FitPhase::form).
// The resident pass (one launch per sub-batch, basis stationary in registers) needs the split-fp16 basis, sparse skinning rows
// and all of its workgroups resident next to the optimiser's opt_grid ones, every one of them a CU.
// mvfit_options::resident_pass = 0 / 1 / 2 forces the choice (a forced value that does not fit can stall the fit).
int resident_form(const FitPlanIn& in, int opt_grid) {
    if (!in.half_basis || !in.sparse_skinning || !in.nv_even) return 0;
    if (in.resident_pass >= 0) return in.resident_pass == 2 ? 3 : in.resident_pass;      // (form 2 was dropped: it maps to 3)
    if (in.resident_auto_off) return 0;
    const int room = in.n_cu - 4 - opt_grid;           // (4 CUs of slack: nothing in HIP promises that every CU takes a workgroup)
    if (in.ntiles <= room) return 1;
    if ((in.ntiles + 1) / 2 <= room) return 3;
    return 0;
}

}  // namespace

// with_passes, automatic count: 16 sets next to <= 32 problems are 160 optimiser-kernel workgroups, which leave no room for the
// resident pass's 108; 8 sets (96 workgroups) do, and measure the same closure rate (the mode is bound by the decoder hand-offs,
// profiles/r5_progress.md) - so the shipped yaml's default mode does not run its passes as per-round launches (round 6).
// Results do not depend on the number of sets (fixed summation order).
int plan_nsets(const FitPlanIn& in, int n, int vposer_sets, bool with_passes) {
    // few problems: 16 sets (two problems per helper at 32: less queueing behind another problem's request)
    const int cap = n <= 32 ? VPS_MAX_SETS : kVpsSets;
    // at least ceil(n / VPS_PMAX) sets: a set has VPS_PMAX request / answer slots (the knob cannot push problems past them)
    const int need = (n + VPS_PMAX - 1) / VPS_PMAX;
    int want = vposer_sets > 0 ? std::min(vposer_sets, cap) : cap;
    if (vposer_sets <= 0 && with_passes && want > kVpsSets) {
        const int full = std::max(need, std::min(want, n)), half = std::max(need, std::min(kVpsSets, n));
        if (!resident_form(in, n + full * VPS_SLICES) && resident_form(in, n + half * VPS_SLICES)) want = kVpsSets;
    }
    return std::max(need, std::min(want, n));
}

namespace {

// the fit decodes the body pose on helper workgroups
bool helpers_on(const FitPlanIn& in) { return (in.flags & MVFIT_F_VPOSER) && in.helper_memory && in.vposer_helpers != 0; }

int launch_nsets(const FitPlanIn& in, int n, bool with_passes) {
    return helpers_on(in) && n <= kVpsMaxSparse ? plan_nsets(in, n, in.vposer_sets, with_passes) : 0;
}

int fail(FitPlan& p, const char* fmt, int a, int b) {
    char buf[160];
    snprintf(buf, sizeof(buf), fmt, a, b);
    p.err = buf;
    return p.rc = MVFIT_E_ARG;
}

int plan_async(const FitPlanIn& in, bool service, int pause_stage, FitPlan& plan, FitPhase& ph) {
    const int B = in.B;
    const bool vps = helpers_on(in);
    // whole 32-problem chunks, the sub-batches of one size
    auto sub_batch = [&](int maxb) { const int nsub = (B + maxb - 1) / maxb; return ((B + nsub - 1) / nsub + 31) / 32 * 32; };
    ph.driver = service ? DRIVER_ASYNC_SDF : DRIVER_ASYNC;
    ph.pause_stage = pause_stage;
    // the sub-batch size follows from the form the passes really take for the optimiser grid it gives
    ph.per = sub_batch(vps ? kVpsMaxAsync : kResidentMaxB);
    const int n0 = std::min(B, ph.per);
    ph.form = (in.debug_nopass || service) ? 0 : resident_form(in, n0 + launch_nsets(in, n0, true) * VPS_SLICES);
    if (!ph.form && !vps) ph.per = sub_batch(kAsyncMaxB);
    // (no queue with decoder helpers: their request slots belong to problems; none in service launches)
    ph.refill = ph.form != 0 && !vps && !service && B > ph.per && in.work_queue != 0 && !in.reuse_outer;
    if (ph.refill) ph.per = kResidentMaxB;
    ph.launch_cap = ph.refill ? (int)std::min<long long>((long long)in.cap * ((B + ph.per - 1) / ph.per + 1), 1 << 30) : in.cap;
    ph.res_grid = plan_resident_grid(ph.form, in.ntiles);
    if (ph.res_grid > kPassWords) return fail(plan, "resident vertex pass: %d workgroups > %d back-pressure words", ph.res_grid, kPassWords);
    if (ph.form && ph.per > kResidentMaxB) return fail(plan, "resident vertex pass: %d ring rows > %d", ph.per, kResidentMaxB);
    for (int b_lo = 0; b_lo < B; b_lo += ph.refill ? B : ph.per) {
        const int b_hi = std::min(B, b_lo + ph.per);
        ph.launches.push_back({b_lo, b_hi, ph.refill ? B : b_hi - b_lo, launch_nsets(in, b_hi - b_lo, true)});
    }
    return MVFIT_OK;
}

// (with decoder helpers: sub-batches whose workgroups are all resident, one after the other)
void plan_sparse(const FitPlanIn& in, FitPhase& ph) {
    const int B = in.B, maxb = helpers_on(in) ? kVpsMaxSparse : B;
    const int nsub = (B + maxb - 1) / maxb, per = (B + nsub - 1) / nsub;
    ph.driver = DRIVER_SPARSE;
    ph.per = per;
    ph.launch_cap = in.cap;
    for (int b_lo = 0; b_lo < B; b_lo += per) {
        const int b_hi = std::min(B, b_lo + per);
        ph.launches.push_back({b_lo, b_hi, b_hi - b_lo, launch_nsets(in, b_hi - b_lo, false)});
    }
}

}  // namespace

FitPlan plan_fit(const FitPlanIn& in) {
    FitPlan plan;
    const bool any_sdf = in.sdf_stages != 0;
    // the interpenetration term reads every vertex: MVFIT_F_SPARSE_VERTS is ignored while it is active
    const bool sparse = (in.flags & MVFIT_F_SPARSE_VERTS) != 0 && !any_sdf;
    // the single-launch kernel needs the split-fp16 basis; round_mode = 1 keeps the chained rounds
    const bool single = in.half_basis && in.round_mode != 1;
    // With the term: the leading stages whose coll_loss_weight is 0 (stages 1-2 of the yaml) do not need the vertices before the
    // loss - they run asynchronously like a fit without the term, every problem leaves at the stage boundary, and the tail takes
    // over from the stored optimiser / pose state (a fresh optimiser starts there anyway).
    int lead = 0;
    while (lead < in.num_stages && !(in.sdf_stages >> lead & 1u)) ++lead;
    const bool two_phase = any_sdf && lead >= 1 && lead < in.num_stages && single && in.sdf_two_phase != 0;
    // The stages that carry the term run in the single-launch kernel too, with the term as a service (also when the FIRST stage
    // carries it: no lead phase then).  sdf_service = 0 keeps the chained rounds - pass -> term -> step kernel per round -, which
    // stay the checker of this path and the structure of profiled fits and of MVFIT_F_REUSE_OUTER_VALUE fits.
    const bool service = any_sdf && single && in.sdf_two_phase != 0 && in.sdf_service != 0 && !in.reuse_outer && !in.profile;
    const bool async = !sparse && !any_sdf && single;
    plan.init_full_pass = !(sparse || async || two_phase || service);
    if (two_phase && plan_async(in, false, lead, plan, plan.phase[plan.nphases++])) return plan;
    FitPhase& tail = plan.phase[plan.nphases++];
    if (service || async) plan_async(in, service, MVFIT_MAX_STAGES + 1, plan, tail);
    else if (sparse) plan_sparse(in, tail);
    else { tail.driver = in.profile ? DRIVER_EAGER : DRIVER_GRAPH; tail.launch_cap = in.cap; }
    return plan;
}

PersistentVariant plan_persistent_variant(bool sdf_service, bool queue, bool helpers, bool reuse_outer, bool lean) {
    if (sdf_service) return helpers ? PV_SDF_HELPERS : PV_SDF;
    if (queue) return lean ? PV_QUEUE_LEAN : PV_QUEUE;
    if (helpers) return reuse_outer ? PV_HELPERS_REUSE : PV_HELPERS;
    if (reuse_outer) return lean ? PV_REUSE_LEAN : PV_REUSE;
    return lean ? PV_LEAN : PV_PLAIN;
}

PassLaunch plan_pass_launch(bool split_basis, bool sparse_skinning, bool nv_even, int chunks, int pass_kernel) {
    if (!split_basis) return {PASS_EXACT, sparse_skinning, chunks};
    // more than one 32-problem chunk: one workgroup per vertex tile walks ALL chunks with the tile's basis held in registers
    if (chunks == 1 || pass_kernel == 1) return {PASS_SPLIT, sparse_skinning, chunks};
    if (!sparse_skinning) return {PASS_SPLIT_LOOP, false, 1};
    if (nv_even) return {PASS_PIPE, true, 1};
    return {PASS_SPLIT, true, chunks};
}

}  // namespace mvfit
