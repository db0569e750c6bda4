"""Joint refinement with several terms in one fit: the scene collision term against the other bodies of the scene, the
silhouette term against the engine's mask set, the vertex-target term against the bodies of the neighbouring frames and the
scan term against the engine's scan set, mixed behind one weight (include/mvfit.h:mvfit_set_term_mix).

Run one after another, the three refinements (scene_fit.refine_scenes, silhouette.refine_fit, temporal.smooth_sequences)
each undo part of what the one before achieved.  Here every sweep is ONE fit of

    loss_j = f_j + w^2 (l_sc S_sc,j^2 + l_sil L_sil,j + l_t L_vt,j + l_scan L_scan,j)

with the obstacles and the neighbours frozen where the sweep started - a Jacobi sweep, as in the two single drivers.  The
frozen problems count every pair of consecutive frames twice (temporal.py), so the joint energy of a set g of problems is

    E_g = sum_{j in g} (loss_j - 1/2 w^2 l_t L_vt,j),

the scene part counted as refine_scenes counts it.  Freezing couples the problems of one scene and the consecutive frames
of one sequence, and nothing else: the accept rule works on the connected components of that graph.  A component keeps a
sweep only if its E fell with everything re-frozen at the new bodies; otherwise its rows revert exactly, which is what makes
E non-increasing.  The scan part is a problem's own, like the silhouette's: it links no problems and needs no correction in E.

Not built: per-problem shares, sequence mode, the one-person SDF term in the mix."""
import numpy as np
import torch

from .temporal import neighbour_table

SHARE_KEYS = ('scene', 'silhouette', 'temporal')
SCAN_KEY = 'scan'                       # the optional fourth share


def _np(t):
    return np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t)


def problem_groups(B, scene_sizes=None, nbr=None):
    """group [B] int64: the connected components of the graph that links the problems of one scene (``scene_sizes``
    consecutive problems each) and consecutive frames of one sequence (``nbr`` of temporal.neighbour_table), numbered in
    order of their first problem."""
    parent = list(range(B))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    def link(i, j):
        i, j = find(i), find(j)
        if i != j:
            parent[max(i, j)] = min(i, j)

    if scene_sizes is not None:
        first = 0
        for n in scene_sizes:
            for j in range(first + 1, first + int(n)):
                link(first, j)
            first += int(n)
    if nbr is not None:
        for j in range(B):
            for n in nbr[j]:
                if n >= 0:
                    link(j, int(n))
    roots = [find(j) for j in range(B)]
    number = {}
    for r in roots:
        number.setdefault(r, len(number))
    return np.array([number[r] for r in roots], np.int64)


def check_shares(shares):
    """shares -> (scene, silhouette, temporal) floats, or (scene, silhouette, temporal, scan) when ``shares`` has the key
    'scan'; ValueError for unknown keys, negative or non-finite values and fewer than two shares > 0."""
    keys = SHARE_KEYS + ((SCAN_KEY,) if SCAN_KEY in shares else ())
    unknown = sorted(set(shares) - set(SHARE_KEYS) - {SCAN_KEY})
    if unknown:
        raise ValueError('refine_joint: unknown shares %r (known: %s)' % (unknown, ', '.join(SHARE_KEYS + (SCAN_KEY,))))
    lam = tuple(float(shares.get(k, 0.0)) for k in keys)
    if any(not np.isfinite(v) or v < 0.0 for v in lam):
        raise ValueError('refine_joint: the shares must be finite and >= 0, got %r' % (dict(zip(keys, lam)),))
    if sum(v > 0.0 for v in lam) < 2:
        raise ValueError('refine_joint: at least two shares must be > 0 (a single term has a driver of its own)')
    return lam


def refine_joint(engine, params, stage, *, shares, scene_sizes=None, seq_id=None, frame_idx=None, sweeps=3, grid_size=32,
                 scale_factor=0.2, robustifier=0.05, w_in=1.0, w_out=1.0, sigma=0.0, scan_w_s2m=1.0, scan_w_m2s=0.0, scan_sigma=0.0,
                 **fit_kwargs):
    """params [B,118] of the engine's B problems (set_problems done); ``stage``: one weight dict with coll_loss_weight = w >
    0; ``shares`` = dict(scene=, silhouette=, temporal=), at least two > 0.  scene > 0 needs ``scene_sizes`` (consecutive
    problems per scene), temporal > 0 needs ``seq_id`` and ``frame_idx`` (temporal.neighbour_table), silhouette > 0 needs the
    mask set on the engine already (set_silhouettes; w_in, w_out, sigma are the term's scalars).  ``shares`` may also name
    scan: scan > 0 needs the scan set of B bodies on the engine already (set_scans; scan_w_s2m, scan_w_m2s, scan_sigma are the
    term's scalars); parts0, parts and parts_problem then have a fourth column, L_scan, and the scan set stays like the masks.

      1. freeze obstacles and neighbour targets at x_0; one closure and term_mix_read give E(x_0);
      2. per sweep: x' = engine.fit(x_k, [stage]); re-freeze at vertices(x'); one closure gives E(x'); group g is accepted
         iff E_g(x') < E_g(x_k), a rejected group's rows revert to x_k exactly;
      3. stop when no group was accepted, or after ``sweeps`` sweeps;
      4. the engine is left with the mix off, the targets and the obstacles cleared (also when something raises); the mask
         set stays - the caller owns it.

    Returns (params, report).  report: dict(group [B] = the group of every problem, shares, E0 [G], parts0 [G,3] = the groups'
    sums of the unweighted (S_sc^2, L_sil, L_vt), params0 [B,118], sweeps = one dict per sweep run with E [G] (after the accept
    rule), accepted [G] bool, parts [G,3], params [B,118] kept after the sweep, n_closure [B] of the sweep's fit; loss [B] and
    parts_problem [B,3] = the closure loss and the unweighted parts of the returned params with everything frozen at them)."""
    w = float(stage.get('coll_loss_weight', 0.0))
    if w <= 0.0:
        raise ValueError('refine_joint: the stage needs coll_loss_weight > 0')
    lam = check_shares(shares)
    lam_sc, lam_sil, lam_t = lam[:3]
    with_scan = len(lam) > 3 and lam[3] > 0.0
    lam_scan = lam[3] if with_scan else 0.0
    B = engine.B
    sizes = None
    if lam_sc > 0.0:
        if scene_sizes is None:
            raise ValueError('refine_joint: a scene share needs scene_sizes')
        sizes = [int(n) for n in scene_sizes]
        if sum(sizes) != B:
            raise ValueError('scene_sizes %r do not add up to the %d problems of the engine' % (sizes, B))
    nbr = a = rows = None
    if lam_t > 0.0:
        if seq_id is None or frame_idx is None:
            raise ValueError('refine_joint: a temporal share needs seq_id and frame_idx')
        nbr, a = neighbour_table(seq_id, frame_idx)
        if nbr.shape[0] != B:
            raise ValueError('seq_id has %d entries, the engine %d problems' % (nbr.shape[0], B))
        rows = torch.as_tensor(np.maximum(nbr, 0), device=engine.device)        # (-1: any row will do, its weight is 0)
    group = problem_groups(B, sizes, nbr)
    G = int(group.max()) + 1
    flags = int(stage.get('flags', 0))
    x = params if isinstance(params, torch.Tensor) else torch.as_tensor(np.asarray(params, np.float32))
    x = x.to(engine.device).clone()
    state = dict(mix=False)

    def sums(values):
        """Per-group sums of a per-problem array ([B] or [B,k]), in float64 on the host, problems in order."""
        v = np.asarray(values, np.float64)
        return np.array([v[group == g].sum(axis=0) for g in range(G)], np.float64)

    def freeze(xx):
        v, _ = engine.vertices(xx, flags=flags)
        if lam_sc > 0.0:
            engine.set_scene_obstacles(v, sizes, grid_size=grid_size, scale_factor=scale_factor, robustifier=robustifier)
        if lam_t > 0.0:
            engine.set_vertex_targets(v[rows], a)
        if not state['mix']:
            if with_scan:
                engine.set_term_mix(scene=lam_sc, silhouette=lam_sil, vertex_targets=lam_t, w_in=w_in, w_out=w_out, sigma=sigma,
                                    scan=lam_scan, scan_w_s2m=scan_w_s2m, scan_w_m2s=scan_w_m2s, scan_sigma=scan_sigma)
            else:                            # (exactly the call of a mix without the share)
                engine.set_term_mix(scene=lam_sc, silhouette=lam_sil, vertex_targets=lam_t, w_in=w_in, w_out=w_out, sigma=sigma)
            state['mix'] = True

    def objective(xx):
        """(loss [B] tensor, parts [B,3], E [G]) with everything as frozen."""
        loss = engine.closure(xx, stage, want_grad=False)['loss']
        parts = _np(engine.term_mix_read(scan=True) if with_scan else engine.term_mix_read()).astype(np.float64)
        return loss, parts, sums(_np(loss).astype(np.float64) - 0.5 * w * w * lam_t * parts[:, 2])

    try:
        freeze(x)
        loss, parts, E = objective(x)
        gparts = sums(parts)
        report = dict(group=group.copy(), shares=dict(zip(SHARE_KEYS + ((SCAN_KEY,) if len(lam) > 3 else ()), lam)), E0=E.copy(),
                      parts0=gparts.copy(), params0=_np(x).copy(), sweeps=[])
        for k in range(int(sweeps)):
            x_new, st = engine.fit(x, [stage], **fit_kwargs)
            x_new = x_new.to(x.dtype)
            freeze(x_new)
            loss_new, parts_new, E_new = objective(x_new)
            gparts_new = sums(parts_new)
            accepted = E_new < E
            for g in np.flatnonzero(~accepted):
                keep = np.flatnonzero(group == g)
                keep_t = torch.as_tensor(keep, device=x.device)
                x_new[keep_t] = x[keep_t]
                loss_new[keep_t] = loss[keep_t]
                parts_new[keep] = parts[keep]
            x, loss, parts = x_new, loss_new, parts_new
            E = np.where(accepted, E_new, E)
            gparts = np.where(accepted[:, None], gparts_new, gparts)
            report['sweeps'].append(dict(E=E.copy(), accepted=accepted.copy(), parts=gparts.copy(), params=_np(x).copy(),
                                         n_closure=_np(st['n_closure']).copy()))
            if not accepted.any():
                break
            if k + 1 < int(sweeps) and not accepted.all():
                freeze(x)                    # the next sweep starts from the kept bodies of the rejected groups
        report['loss'] = _np(loss).astype(np.float64)
        report['parts_problem'] = parts.copy()
        return x, report
    finally:
        engine.clear_term_mix()
        if lam_t > 0.0:
            engine.clear_vertex_targets()
        if lam_sc > 0.0:
            engine.clear_scene_obstacles()


__all__ = ['problem_groups', 'check_shares', 'refine_joint']
