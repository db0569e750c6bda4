// libmvfit: the C ABI (include/mvfit.h), part 2 of 3 - mvfit_fit and what belongs to it.  How a fit runs is decided by
// fit_plan.cpp; the four drivers here execute the plan with the kernels of fit_kernels.hip and the vertex passes of
// vertex_pass.hip.  Also the host half of the float64 known-answer test of the optimiser (mvfit_lbfgs_kat).
#include "mvfit_ctx.h"

// the optimiser's scalar options (the gtol segments are the caller's)
static LbOpts lb_opts(const mvfit_lbfgs_opts& o, int num_stages) {
    LbOpts O;
    memset(&O, 0, sizeof(O));
    O.lr = o.lr; O.tol_grad = o.tolerance_grad; O.tol_change = o.tolerance_change; O.ftol = o.ftol; O.gtol = o.gtol;
    O.max_iter = o.max_iter; O.max_eval = o.max_iter * 5 / 4; O.history = o.history; O.maxiters = o.maxiters;
    O.num_stages = num_stages;
    // (hooks build only) the general form of the direction's triangular products; the LDS form of its mat-vecs
    O.dir_forms = (debug_hook("MVFIT_DIR_GENERAL") != 0 ? LB_DIR_GENERAL : 0) | (debug_hook("MVFIT_DIR_MATVEC_LDS") != 0 ? LB_DIR_MATVEC_LDS : 0);
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
    // the key: everything baked into the kernel nodes.  The term's part of it is the plan launch_term executes below - what a
    // step does not take is not in the plan, so a re-freeze or re-set that keeps the buffers and sizes keeps the graph
    const RoundTermPlan term = plan_round_term(term_inputs(c), c->F.sdf_adj != nullptr);
    std::vector<unsigned char> key(sizeof(SW) + sizeof(O) + sizeof(DevPose) + sizeof(FitBuffers) + sizeof(DevProblems) + sizeof(int) + sizeof(term));
    unsigned char* k = key.data();
    memcpy(k, &SW, sizeof(SW)); k += sizeof(SW);
    memcpy(k, &O, sizeof(O)); k += sizeof(O);
    memcpy(k, &c->P, sizeof(DevPose)); k += sizeof(DevPose);
    memcpy(k, &c->F, sizeof(FitBuffers)); k += sizeof(FitBuffers);
    memcpy(k, &c->Q, sizeof(DevProblems)); k += sizeof(DevProblems);
    memcpy(k, &c->opt.pass_kernel, sizeof(int)); k += sizeof(int);
    memcpy(k, &term, sizeof(term));
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
                e = launch_term(term, c->M, c->P, c->Q, c->sil, c->scan, c->err, c->pb.verts, c->F.sdf_gate, cs, Pg.box_part);
            launch_fit_step(O.reuse_outer != 0, c->B, cs, c->M, c->pb.obs, c->V, SW, O, c->P, c->F);
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
    ++c->graph_builds;
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
    const PersistentVariant variant = plan_persistent_variant(sdfs, queue != nullptr, M.vps.nsets != 0, O.reuse_outer != 0, lean);
    launch_fit_persistent(variant, grid, c->stream, M, c->pb.obs, c->V, SW, O, c->P, c->F, cap, R, L.b_lo, L.n_target, pause_stage, queue,
                          b_end);
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
            // (the rounds' own copies of the gates, written by the gate kernels for [b_lo, b_hi) and read by the term's kernels)
            HIP_OK(c, hipMemsetAsync(c->pb.sdf_gate_round, 0, (size_t)B * 4, c->stream));
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
                hipError_t e = launch_pass_gate(P, b_lo, b_hi, c->pass_stream, sdf_service ? c->F.sdf_gate : nullptr,
                                                sdf_service ? c->pb.sdf_gate_round : nullptr);
                hipEvent_t ea = nullptr, eb = nullptr;
                if (c->profile && c->ev_vp.size() < 4096) {            // mvfit_profile: the dispatch's own begin / end stamps
                    hipEventCreate(&ea); hipEventCreate(&eb);
                    c->ev_vp.emplace_back(ea, eb);
                }
                if (e == hipSuccess) e = launch_vertex_pass(c->M, P, b_hi, vout, c->opt.pass_kernel, c->pass_stream, ea, eb);
                if (e != hipSuccess) return fail(c, MVFIT_E_HIP, "vertex pass launch: %s", hipGetErrorString(e));
                if (sdf_service) {
                    // the term at the round's vertices for the problems whose gate word was set (written by the optimiser in
                    // front of the round's tag, copied for the round by its gate kernel); transforms from the ring slot, float32
                    // coefficients from the chained layout.  The grid ends at b_hi; the work areas keep the layout of the batch
                    DevPose Ps = P;
                    Ps.coefT = c->P.coefT;
                    e = launch_sdf_term(c->M, Ps, vout, b_hi, B, c->sdf_faces.as<int32_t>(), c->sdf_num_faces, c->sdf_grid, c->pb.sdf_gate_round, c->pb.sdf_box,
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
            launch_fit_step(O.reuse_outer != 0, c->B, c->stream, c->M, c->pb.obs, c->V, SW, O, c->P, c->F);
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

extern "C" int mvfit_round_graph_info(mvfit_ctx* c, int drop, uint64_t* out4) {
    if (!c) return MVFIT_E_ARG;
    if (drop) {
        HIP_OK(c, hipSetDevice(c->device));
        HIP_OK(c, hipStreamSynchronize(c->stream));          // (a replay may still run)
        drop_graph(c);
    }
    if (out4) {
        const unsigned char* oc = c->sil.occ.as<unsigned char>();
        out4[0] = c->graph_builds;
        out4[1] = oc ? reinterpret_cast<uintptr_t>(oc + c->sil.o_zocc) : 0;
        out4[2] = oc ? reinterpret_cast<uintptr_t>(oc + c->sil.o_zown) : 0;
        out4[3] = oc ? reinterpret_cast<uintptr_t>(oc + c->sil.o_pflag) : 0;
    }
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
    if (any_sdf && !c->sdf_num_faces && !round_term(c))
        return fail(c, MVFIT_E_STATE, "coll_loss_weight > 0 needs the SDF term's faces: call mvfit_set_sdf first");
    if (round_term(c)) in.sdf_service = 0;      // the scene, silhouette, vertex-target and scan terms and the mix run in chained rounds only (no service path for them)
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
    launch_fit_init(B, c->stream, c->M, c->pb.obs, c->P, c->F, params, sw[0].flags, plan.init_full_pass ? 1 : 0);
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
    launch_fit_finish(B, c->stream, c->F, params, final_loss, n_closure, n_iter, o->num_stages);
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

extern "C" int mvfit_fit_trace(mvfit_ctx* c, float* trace, int max_closures) {
    if (!c || max_closures < 0 || (trace && max_closures == 0)) return MVFIT_E_ARG;
    c->trace = trace;
    c->trace_cap = trace ? max_closures : 0;
    return MVFIT_OK;
}

extern "C" int mvfit_lbfgs_kat(int device, int kind, int D, const int32_t* segs, int nseg, const mvfit_lbfgs_opts* o,
                               double* x_inout, double* trace, int max_trace, int* n_closure, double* final_loss) {
    if (!o || !x_inout || D <= 1 || D > LB_D || nseg < 1 || nseg > 8 || !segs) return MVFIT_E_ARG;
    if (!lb_opts_ok(*o)) return MVFIT_E_ARG;
    if ((kind & ~0x100) < 0 || (kind & ~0x100) >= MVFIT_KAT_KINDS) return MVFIT_E_ARG;      // (an unknown kind used to run 'gmof')
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
    launch_lbfgs_kat(kind, D, O, dx, dtrace, max_trace, dn, dfl, ddirs, dstps, dro, dgrow, dgcol, dcmat);
    hipError_t e = hipDeviceSynchronize();
    hipMemcpy(x_inout, dx, D * 8, hipMemcpyDeviceToHost);
    if (trace && max_trace > 0) hipMemcpy(trace, dtrace, tb, hipMemcpyDeviceToHost);
    if (n_closure) hipMemcpy(n_closure, dn, 4, hipMemcpyDeviceToHost);
    if (final_loss) hipMemcpy(final_loss, dfl, 8, hipMemcpyDeviceToHost);
    return e == hipSuccess ? MVFIT_OK : MVFIT_E_HIP;
}
