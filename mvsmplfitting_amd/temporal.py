"""Temporal smoothing of fitted sequences: the fit with the vertex-target term against the bodies of the neighbouring frames,
frozen at the start of every sweep (include/mvfit.h:mvfit_set_vertex_targets, mvfit_set_vertex_target_term).

The joint energy of a sequence s is the frames' own losses plus a first-order chain over consecutive frames,

    E_s(x) = sum_{j in s} f_j(x_j) + w^2 sum_{pairs (t, t+1) of s} ||V_{t+1}(x) - V_t(x)||^2 .

With the neighbours of frame j frozen, its part of the chain is L_j = sum_{neighbours n} ||V_j - V_n||^2: the vertex-target
loss with the neighbours' vertices as targets, a per-problem term - the shape the batched fit is built around.  The frozen
problems are the exact restrictions of E to one frame; summed over the frames they count every pair twice, so

    E_s(x) = sum_{j in s} (loss_j(x) - 1/2 w^2 L_j(x)),   loss_j = f_j + w^2 L_j, targets frozen at vertices(x).

All frames move at once against neighbours frozen where the sweep started: a Jacobi sweep.  For the chain energy on a
quadratic model it is monotone (2 D - A is positive definite for a path graph's degree and adjacency matrices); the fit
is not quadratic, so every sweep is judged on E with the targets re-frozen at the new bodies, and a sequence whose energy
did not fall keeps its previous parameters: the accept rule is what makes E non-increasing.

Not built: second-order (constant-velocity) smoothing - the term's K <= 4 targets are there for it, this driver offers first
order only -, per-vertex weights, smoothing the parameters instead of the vertices, sharing betas or scale over a sequence."""
import numpy as np
import torch


def neighbour_table(seq_id, frame_idx):
    """seq_id [B], frame_idx [B] (integers) -> (nbr [B,2] int64, a [B,2] float32): nbr[j] = the problems of j's sequence at
    frame_idx[j] - 1 and frame_idx[j] + 1, -1 with weight 0 where there is none, weight 1 where there is.  A duplicate
    (seq_id, frame_idx) raises ValueError."""
    seq = np.asarray(seq_id).reshape(-1)
    frm = np.asarray(frame_idx).reshape(-1)
    if seq.shape != frm.shape:
        raise ValueError('seq_id has %d entries, frame_idx %d' % (seq.size, frm.size))
    where = {}
    for j, key in enumerate(zip(seq.tolist(), frm.tolist())):
        if key in where:
            raise ValueError('problems %d and %d are both frame %r of sequence %r' % (where[key], j, key[1], key[0]))
        where[key] = j
    nbr = np.full((seq.size, 2), -1, np.int64)
    for (s, f), j in where.items():
        nbr[j, 0] = where.get((s, f - 1), -1)
        nbr[j, 1] = where.get((s, f + 1), -1)
    return nbr, (nbr >= 0).astype(np.float32)


def _np(t):
    return np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t)


def smooth_sequences(engine, params, stage, seq_id, frame_idx, *, sweeps=3, **fit_kwargs):
    """params [B,118] of the engine's B problems (set_problems done); problem j is frame ``frame_idx[j]`` of sequence
    ``seq_id[j]``; ``stage``: one weight dict with coll_loss_weight = w > 0, the smoothing weight.

      1. freeze the neighbours at x_0; one closure and sdf_term_read give E(x_0);
      2. per sweep: x' = engine.fit(x_k, [stage]); freeze at vertices(x'); one closure gives E(x'); sequence s is accepted
         iff E_s(x') < E_s(x_k), a rejected sequence's rows revert to x_k exactly;
      3. stop when no sequence was accepted, or after ``sweeps`` sweeps;
      4. the engine is left with the term off and the targets cleared (also when something raises).

    Returns (params, report).  report: dict(sequences [S] = the sorted distinct seq_id, E0 [S], smooth0 [S] = sum over the
    sequence's consecutive pairs of ||V_{t+1} - V_t||^2, params0 [B,118], sweeps = one dict per sweep run with E [S] (after
    the accept rule), accepted [S] bool, smooth [S], params [B,118] kept after the sweep, n_closure [B] of the sweep's fit;
    loss [B] = the per-problem closure loss of the returned params with the neighbours frozen at them)."""
    w = float(stage.get('coll_loss_weight', 0.0))
    if w <= 0.0:
        raise ValueError('smooth_sequences: the stage needs coll_loss_weight > 0 (the smoothing weight)')
    nbr, a = neighbour_table(seq_id, frame_idx)
    if nbr.shape[0] != engine.B:
        raise ValueError('seq_id has %d entries, the engine %d problems' % (nbr.shape[0], engine.B))
    flags = int(stage.get('flags', 0))
    seq = np.asarray(seq_id).reshape(-1)
    names, member = np.unique(seq, return_inverse=True)
    S = len(names)
    x = params if isinstance(params, torch.Tensor) else torch.as_tensor(np.asarray(params, np.float32))
    x = x.to(engine.device).clone()
    rows = torch.as_tensor(np.maximum(nbr, 0), device=engine.device)        # (-1: any row will do, its weight is 0)
    state = dict(term=False)

    def sums(values):
        """Per-sequence sums of a per-problem vector, in float64 on the host, problems in order."""
        return np.array([values[member == s].sum() for s in range(S)], np.float64)

    def freeze(xx):
        v, _ = engine.vertices(xx, flags=flags)
        engine.set_vertex_targets(v[rows], a)
        if not state['term']:
            engine.set_vertex_target_term()
            state['term'] = True

    def objective(xx):
        """(loss [B] tensor, E [S], smooth [S]) with the targets as frozen."""
        loss = engine.closure(xx, stage, want_grad=False)['loss']
        L = _np(engine.sdf_term_read()[1]).astype(np.float64)
        return loss, sums(_np(loss).astype(np.float64) - 0.5 * w * w * L), 0.5 * sums(L)

    try:
        freeze(x)
        loss, E, smooth = objective(x)
        report = dict(sequences=names.copy(), E0=E.copy(), smooth0=smooth.copy(), params0=_np(x).copy(), sweeps=[])
        for k in range(int(sweeps)):
            x_new, st = engine.fit(x, [stage], **fit_kwargs)
            x_new = x_new.to(x.dtype)
            freeze(x_new)
            loss_new, E_new, smooth_new = objective(x_new)
            accepted = E_new < E
            for s in np.flatnonzero(~accepted):
                keep = torch.as_tensor(np.flatnonzero(member == s), device=x.device)
                x_new[keep] = x[keep]
                loss_new[keep] = loss[keep]
            x, loss = x_new, loss_new
            E, smooth = np.where(accepted, E_new, E), np.where(accepted, smooth_new, smooth)
            report['sweeps'].append(dict(E=E.copy(), accepted=accepted.copy(), smooth=smooth.copy(), params=_np(x).copy(),
                                         n_closure=_np(st['n_closure']).copy()))
            if not accepted.any():
                break
            if k + 1 < int(sweeps) and not accepted.all():
                freeze(x)                    # the next sweep starts from the kept bodies of the rejected sequences
        report['loss'] = _np(loss).astype(np.float64)
        return x, report
    finally:
        engine.clear_vertex_target_term()
        engine.clear_vertex_targets()


__all__ = ['neighbour_table', 'smooth_sequences']
