"""GPU: staged fits with the interpenetration (SDF) term outside the one shape the other tests of that path stay in - more
problems than one sub-batch of the service tail, a lead phase with a work queue, a term whose pull-back takes the ticket path
(more than 16 entries per problem: eight slice workgroups, the last arriver adds the partials), face lists, and more than one
fit per engine.

References, none of them new: problems are independent and every summation order is fixed, so the reference of a fit at a
large batch is the same problems fitted in one sub-batch - bit equality on parameters, closure counts and final losses (as
tests/test_gpu_large_batch.py and test_service_rounds_... of tests/test_gpu_sdf_term.py); the reference of a service round's
value is mvfit_closure at the traced trial point within 1e-5 |L| + 4e-4 pen (tests/test_gpu_sdf_term.py); the reference of
the closure is the float64 oracle within that file's tolerances (loss 1e-5 relative, gradient 2e-4 of its max).

Every fit also has to end without an error, on finite losses, with no pass missed and no wait given up (and no decoder
answer timed out where there is a decoder).

The gate words' copy per round (pass_gate_copy_kernel) closes a window that cannot be opened on purpose: a problem in a round
without the term inside a service launch moves on and rewrites its gate while that round's term kernels run.  The argument
for it is the code; test_zero_weight_stage_inside_the_service_launch guards the schedule that has such rounds."""
import numpy as np
import pytest

from mvsmplfitting_amd import _lib
from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import stage_weights as eng_stage_weights
from tests.gpu_helpers import make_engine, to118
from tests.helpers import body_model, load_case, oracle_for
from tests.test_gpu_large_batch import _inputs
from tests.test_gpu_sdf_term import _closure_case
from tests.test_sdf_term_ref import load_term_case

pytestmark = pytest.mark.gpu

NF, G = 64, 32                        # the term of test_sdf_adjoint_is_the_same_bits_in_every_run: eight slices
COLL = [0.0, 0.0, 0.05, 0.1]          # lead phase (stages 0-1), then the service tail; small, so that the term does not push the
                                      # body out of the voxels that carry it: the fits end where the pull-back has > 16 entries
NSMALL = 37                           # the reference batch: one sub-batch, two chunks, ragged


def _checked_fit(eng, x0, stages, use_vp=False, **fit_opts):
    """one fit (an error of the library raises MvFitError: the test fails) -> (params, n_closure, final_loss)"""
    xf, st = eng.fit(x0, stages, **fit_opts)
    fl = st['final_loss'].cpu().numpy()
    assert np.all(np.isfinite(fl)), fl
    assert st['passes']['missed'] == 0 and st['passes']['timed_out'] == 0, st['passes']
    if use_vp:
        ds = eng.decoder_stats()
        assert ds['answers_timed_out'] == 0 and ds['helpers_gave_up'] == 0, ds
    return xf.cpu().numpy(), st['n_closure'].cpu().numpy(), fl


def _same(a, b, what):
    for k, name in enumerate(('parameters', 'n_closure', 'final_loss')):
        assert np.array_equal(a[k], b[k]), (what, name, np.nonzero((a[k] != b[k]).reshape(a[k].shape[0], -1).any(1))[0][:8])


def _term_problems(name, B, star=None, model=None):
    """B problems of the term's golden case `name` as test_service_rounds_... builds them: one set of observations, the start
    a body in the triangle's shadow plus 1e-3 of noise, problem i of a large batch = problem i % 37.  star: the observations
    are the projections (2 px of noise, seed `star`) of the body at that start pose instead of the recorded ones, with which
    every fit ends (measured) where no vertex samples a non-zero voxel of the 64-face term.  model: another model of the
    same body (sparse skinning) for the same inputs."""
    cfg, c, model_c, vpw, cams = load_term_case(name)
    model = model_c if model is None else model
    use_vp = cfg['use_vposer']
    gt1, conf1 = c['gt_xy'], c['conf']
    if star is not None:
        x = np.asarray(c['x'], np.float64)
        body = oracle_for(model_c, vpw, None).body(dict(betas=x[0:10], global_orient=x[10:13], body_pose=x[13:82], transl=x[82:85],
                                                        scale=x[85:86], use_vposer=False), want_cache=False)
        gt, conf = syn.make_observations(body['joints'][None], cams, seed=star, noise_px=2.0)
        gt1, conf1 = gt[0], conf[0]
    noise = 1e-3 * np.random.default_rng(7).normal(0, 1, (NSMALL, 86))[np.arange(B) % NSMALL]
    if use_vp:
        x0 = np.stack([to118(c['x'] + noise[b, :49], True) for b in range(B)]).astype(np.float32)
    else:
        x0 = np.repeat(to118(c['x'], False).astype(np.float32)[None], B, 0)
        x0[:, :86] += noise.astype(np.float32)
    return model, vpw, use_vp, cams, np.repeat(gt1[None], B, 0), np.repeat(conf1[None], B, 0), x0


def _active_vertices(eng, x, w):
    """per problem: the vertices whose sample carries gradient at x - the entry criterion of sdf_entries_kernel (the pull-back
    takes the ticket path from 17 entries on; the six vertices of the box come on top)"""
    eng.closure(x, w, want_grad=False)
    smp, S = eng.sdf_term_read()
    return (smp.cpu().numpy()[:, :, 1:] != 0).any(2).sum(1), S.cpu().numpy()


def _check_traced_rounds(eng, tr, ncl, stages, probs, B, step):
    """every step-th traced round of the problems `probs` returned what mvfit_closure returns at that trial point
    (test_service_rounds_... of tests/test_gpu_sdf_term.py, its bound); -> rounds that touched the term, per problem"""
    n_pos = {}
    for b in probs:
        ks = [k for k in range(min(tr.shape[1], ncl[b])) if np.isfinite(tr[b, k, 118])]
        n_pos[b] = 0
        for k in ks[::step]:
            xk = np.repeat(tr[b, k, :118][None], B, 0).astype(np.float32)
            Lr, best = tr[b, k, 118], None
            for s_ in range(len(stages)):                      # (the trace does not say which stage a round belongs to)
                Ls = float(eng.closure(xk, stages[s_], want_grad=False)['loss'][b])
                _, S = eng.sdf_term_read()
                pen = (float(stages[s_]['coll_loss_weight']) * float(S[b])) ** 2
                err = abs(Ls - Lr) - (1e-5 * abs(Lr) + 4e-4 * pen)
                if best is None or err < best[0]:
                    best = (err, s_, Ls, pen)
            print('traced round: problem %d round %d loss %.6g closure %.6g pen %.4g excess %.3g' % (b, k, Lr, best[2], best[3], best[0]))
            assert best[0] <= 0.0, (b, k, Lr, best)
            n_pos[b] += int(best[3] > 0.0)
    return n_pos


# ---- B1: the lead phase with a work queue (131 problems on 128 rows; the service tail is one launch) ----
def test_lead_phase_with_a_work_queue_fits_every_problem():
    """Two-phase fit of 131 problems with sparse skinning: the lead phase is ONE launch of 128 rows with a work queue, every row
    pauses at the stage boundary, and the three problems of the queue run their lead stages on rows that paused (a row that
    ended there left them unfitted and mvfit_fit returned 'hit the round cap ... the stages without the SDF term').  work_queue 1
    against 0 (sub-batches), with the service tail and with the chained one: the same bits per problem."""
    model = body_model(0, 4)
    B = 131
    stages = eng_stage_weights(1536.0, coll_w=[0.0, 0.0, 1000.0, 1000.0])
    x0 = np.zeros((B, 118), np.float32)
    x0[:, 85] = 1.0
    res = {}
    for svc, wq in ((0, 1), (0, 0), (1, 1), (1, 0)):
        eng = make_engine(model, work_queue=wq, sdf_service=svc)
        _inputs(eng, B, 8, seed0=8000)
        eng.set_sdf(model['faces'], num_faces=1, grid_size=128)
        res[svc, wq] = _checked_fit(eng, x0, stages)
        form = eng.pass_profile()['form']
        eng.close()
        if (svc, wq) == (0, 1) and form == 0:
            # (the chained tail leaves the lead phase's form in place; 0: per-round launches, no queue was planned)
            pytest.skip('the resident vertex pass was not planned on this device (shared or masked): no work queue in the lead phase')
    _same(res[0, 1], res[0, 0], 'chained tail, queue against sub-batches')
    _same(res[1, 1], res[1, 0], 'service tail, queue against sub-batches')


# ---- B2: service sub-batches on the ticket path (dense skinning: no queue is planned) ----
B2_STAR = 7          # (measured: all 37 fits end with 250 vertices or so in non-zero voxels)


def test_service_sub_batches_on_the_ticket_path_and_two_fits_per_engine():
    """165 problems: the service tail runs as sub-batches [0, 96) and [96, 165) whose term kernels cover problems [0, b_hi) inside
    work areas laid out - and zeroed - for 165.  Two fits in a row on one engine, both bit-equal to the 37-problem fit; traced
    rounds of problems 0 and 96 return the closure's values; the term has more than 16 vertices with gradient at the start and
    at the returned parameters of the problems checked (the ticket path of the pull-back)."""
    model, vpw, use_vp, cams, gt, conf, x0 = _term_problems('l2_s3_v6', 165, B2_STAR)
    stages = eng_stage_weights(1536.0, coll_w=COLL)
    ref_eng = make_engine(model)
    ref_eng.set_problems(cams, gt[:NSMALL], conf[:NSMALL])
    ref_eng.set_sdf(model['faces'], num_faces=NF, grid_size=G)
    ref = _checked_fit(ref_eng, x0[:NSMALL], stages)
    ref_eng.close()
    idx = np.arange(165) % NSMALL
    eng = make_engine(model)
    eng.set_problems(cams, gt, conf)
    eng.set_sdf(model['faces'], num_faces=NF, grid_size=G)
    tr = eng.fit_trace(400)
    first = _checked_fit(eng, x0, stages)
    tr = tr.cpu().numpy().astype(np.float64)
    eng.fit_trace(0)
    _same(first, tuple(r[idx] for r in ref), 'first fit of 165 against 37')
    n_pos = _check_traced_rounds(eng, tr, first[1], stages, (0, 96), 165, step=max(1, int(first[1][[0, 96]].max()) // 16))
    second = _checked_fit(eng, x0, stages)
    _same(second, first, 'second fit on the engine')
    print('B2_BITS_OK')
    n0, S0 = _active_vertices(eng, x0, stages[-1])
    n1, S1 = _active_vertices(eng, first[0], stages[-1])
    eng.close()
    print('vertices with gradient at the start %s, at the returned parameters %s; rounds with pen > 0: %s' % (n0[[0, 96]], n1[[0, 96]], n_pos))
    print('problems on the ticket path at the start %d, at the end %d of 165' % ((n0 >= 17).sum(), (n1 >= 17).sum()))
    assert min(n_pos.values()) >= 1, n_pos
    assert n0[0] >= 17 and n0[96] >= 17 and n1[0] >= 17 and n1[96] >= 17, (n0[[0, 96]], n1[[0, 96]])


# ---- B3: both together: sparse skinning, 165 problems, the ticket-path term ----
def test_work_queue_and_service_sub_batches_together():
    """The model with at most four skinning weights per vertex (a work queue in the lead phase) on B2's problems and term: 165
    problems, two fits per engine, work_queue 1 against 0 and against 37 problems."""
    model, vpw, use_vp, cams, gt, conf, x0 = _term_problems('l2_s3_v6', 165, B2_STAR, model=body_model(0, 4))
    stages = eng_stage_weights(1536.0, coll_w=COLL)
    ref_eng = make_engine(model)
    ref_eng.set_problems(cams, gt[:NSMALL], conf[:NSMALL])
    ref_eng.set_sdf(model['faces'], num_faces=NF, grid_size=G)
    ref = _checked_fit(ref_eng, x0[:NSMALL], stages)
    ref_eng.close()
    idx = np.arange(165) % NSMALL
    res = {}
    for wq in (1, 0):
        eng = make_engine(model, work_queue=wq)
        eng.set_problems(cams, gt, conf)
        eng.set_sdf(model['faces'], num_faces=NF, grid_size=G)
        res[wq] = _checked_fit(eng, x0, stages)
        _same(_checked_fit(eng, x0, stages), res[wq], 'second fit on the engine, work_queue %d' % wq)
        if wq:
            n1, _ = _active_vertices(eng, res[wq][0], stages[-1])
            print('problems on the ticket path at the returned parameters: %d of 165' % (n1 >= 17).sum())
        eng.close()
    _same(res[1], res[0], 'queue against sub-batches')
    _same(res[1], tuple(r[idx] for r in ref), '165 against 37')


# ---- B4: decoder helpers in both phases: sub-batches [0, 64) and [64, 100) ----
def test_service_sub_batches_with_decoder_helpers():
    model, vpw, use_vp, cams, gt, conf, x0 = _term_problems('vp_s0_v8', 100)
    assert use_vp
    stages = eng_stage_weights(1536.0, flags=_lib.F_VPOSER, coll_w=COLL)
    res = {}
    for B in (NSMALL, 100):
        eng = make_engine(model, vpw)
        eng.set_problems(cams, gt[:B], conf[:B])
        eng.set_sdf(model['faces'], num_faces=NF, grid_size=G)
        res[B] = _checked_fit(eng, x0[:B], stages, use_vp=True)
        # helpers in the lead phase and in the service tail, every sub-batch of both
        assert eng.decoder_stats()['launches'] == (4 if B == 100 else 2), eng.decoder_stats()
        if B == 100:
            _same(_checked_fit(eng, x0[:B], stages, use_vp=True), res[B], 'second fit on the engine')
        eng.close()
    idx = np.arange(100) % NSMALL
    _same(res[100], tuple(r[idx] for r in res[NSMALL]), '100 against 37')


# ---- B6: a stage without the term inside the service launch ----
def test_zero_weight_stage_inside_the_service_launch():
    """coll weights [c, 0, c, c]: no lead phase, and rounds that do not ask for the term sit between rounds that do, in one
    service launch.  5 problems against 37, and a second fit on each engine against the first."""
    stages = eng_stage_weights(1536.0, coll_w=[5.0, 0.0, 5.0, 20.0])
    model, vpw, use_vp, cams, gt, conf, x0 = _term_problems('l2_s3_v6', NSMALL, B2_STAR)
    res = {}
    for B in (5, NSMALL):
        eng = make_engine(model)
        eng.set_problems(cams, gt[:B], conf[:B])
        eng.set_sdf(model['faces'], num_faces=NF, grid_size=G)
        res[B] = _checked_fit(eng, x0[:B], stages)
        _same(_checked_fit(eng, x0[:B], stages), res[B], 'second fit on the engine, B = %d' % B)
        eng.close()
    _same(res[5], tuple(r[:5] for r in res[NSMALL]), '5 against 37')


# ---- B7: the closure with the term beyond one 32-problem chunk ----
B7_SEED = 3          # (checked with the oracle's own vertices: at most 42 of a problem's samples within 1e-3 of a cell face, the cap is 60)


def test_closure_with_the_term_beyond_one_chunk_matches_oracle():
    """37 problems - the golden ones repeated, the repeats perturbed by 0.02 - against the float64 oracle on problems 0, 31, 32 and
    36 (both chunks, their edges, the ragged end); tolerances and the cap on samples near cell faces of
    test_closure_with_sdf_term_matches_oracle."""
    cfg, g, model, vpw, gmm, wts, cams = load_case('l2_s3_v6')
    n = g['x'].shape[0]
    idx = np.arange(NSMALL) % n
    x = np.asarray(g['x'], np.float64)[idx]
    pert = 0.02 * np.random.default_rng(B7_SEED).normal(0, 1, (NSMALL, 86))
    pert[:n] = 0.0
    res = _closure_case(NF, G, 20.0, nprob=NSMALL, problems=(x + pert, g['gt_xy'][idx], g['conf'][idx]), check=(0, 31, 32, 36))
    assert len(res) == 4 and any(r['S'] > 0 for r in res), 'test case does not exercise the term'
    for r in res:
        assert abs(r['L'] - r['Lr']) <= 1e-5 * abs(r['Lr']), (r['L'], r['Lr'])
        assert abs(r['pen'] - r['pen_r']) <= 1e-4 * max(r['pen_r'], 1e-3 * abs(r['Lr'])), (r['pen'], r['pen_r'])
        assert np.abs(r['g'] - r['gr']).max() <= 2e-4 * np.abs(r['gr']).max(), (np.abs(r['g'] - r['gr']).max(), np.abs(r['gr']).max())


# ---- B5 (last): face lists - the per-problem bin counters of a sub-batch ----
def test_service_sub_batches_with_face_lists():
    """512 faces: the term samples through per-round face lists whose bin counters have to be zero between rounds - those of
    the problems of sub-batch [0, 96) as much as those of the last one.  Two fits on one engine, against 37 problems.  (Short
    fits, a few iterations per stage: a round of this term sorts 512 faces into 327,680 bins per problem.)"""
    model, vpw, use_vp, cams, gt, conf, x0 = _term_problems('l2_s3_v6', 165, B2_STAR)
    stages = eng_stage_weights(1536.0, coll_w=[0.0, 0.0, 5.0, 20.0])
    short = dict(max_iter=5, maxiters=2)
    res = {}
    for B in (NSMALL, 165):
        eng = make_engine(model)
        eng.set_problems(cams, gt[:B], conf[:B])
        eng.set_sdf(model['faces'], num_faces=512, grid_size=16)
        res[B] = _checked_fit(eng, x0[:B], stages, **short)
        assert eng.sdf_info()['term'] == 'face_lists', eng.sdf_info()
        if B == 165:
            _same(_checked_fit(eng, x0, stages, **short), res[B], 'second fit on the engine')
        eng.close()
    idx = np.arange(165) % NSMALL
    _same(res[165], tuple(r[idx] for r in res[NSMALL]), '165 against 37')
