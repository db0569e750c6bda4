"""Identities for multi-person keypoint files: which detections of a frame's views show the same person, and which
person of one frame is which of the next.

A 2-D detector run per view writes each file's ``people`` list in its own order (the reference's keypoint_predict.py
does), so entry k of one view is in general not entry k of another.  The steps, files in, track ids out:

    load_serial_detections   every entry of every file in file order (a ``person_id`` field is ignored)
    MvFit.associate_views    per frame, on the device: ray-distance cost of every cross-view pair of detections and
                             complete-linkage clustering into persons (include/mvfit.h:mvfit_associate_views)
    cluster_centres          one batched triangulation of all clusters -> a 3-D centre per (frame, cluster)
    track_clusters           links the frames' clusters into tracks by nearest centre (host, NumPy)
    associate_serial         the four above -> (ids, kp [F,P,V,17,3], mask [F,P,V]) as batch.load_serial_people returns them

track_clusters runs on the host: it is one pass over the frames in order (a frame's assignment needs the tracks the frame
before left), O(F * C^2) on a [F, C, 3] array with C = persons per frame.  The module imports no device code; the engine
is an argument."""
from __future__ import annotations

import numpy as np

from . import _lib
from . import io_formats as iof

MAX_DET = _lib.ASSOC_MAX_DET          # detections per view and frame (include/mvfit.h: MVFIT_ASSOC_MAX_DET)

# max_cost: largest mean distance (metres) between the rays of two detections of one person; min_joints: joints both
# detections must carry; min_views: detections a person needs; max_move: largest displacement (metres) of a person's
# centre per frame; max_gap: frames a person may be absent and keep their id
DEFAULTS = dict(max_cost=0.05, min_joints=6, min_views=2, max_move=0.5, max_gap=5)


def check_params(params):
    """``associate=`` of batch.fit_folder -> the full parameter dict (True: the defaults); ValueError for an unknown key."""
    if params is True:
        return dict(DEFAULTS)
    if not isinstance(params, dict):
        raise ValueError('associate: True or a dict of %s, not %r' % (sorted(DEFAULTS), params))
    unknown = set(params) - set(DEFAULTS)
    if unknown:
        raise ValueError('associate: unknown keys %s' % sorted(unknown))
    return dict(DEFAULTS, **params)


def load_serial_detections(frames, num_views):
    """(det [F, V, Nmax, 17, 3] float32, count [F, V] int32, slot [F, V, Nmax] int32) of one serial (frames as
    batch.list_frames gives them): the entries of every file's ``people`` list in file order, whatever ``person_id`` they
    carry, without those whose confidences are all zero; slot = the entry's index in its file (-1: no detection).  Nmax
    is the largest count of the serial (at least 1); more than 16 detections in one file: ValueError naming it."""
    found = {}
    for f, (_, paths) in enumerate(frames):
        for v, p in enumerate(paths[:num_views]):
            if p is None:
                continue
            ent = [(k, a) for k, a in enumerate(iof.read_keypoints(p)) if a[:, 2].any()]
            if len(ent) > MAX_DET:
                raise ValueError('%s lists %d detections; the association takes at most %d per view' % (p, len(ent), MAX_DET))
            found[(f, v)] = ent
    nmax = max([len(e) for e in found.values()] + [1])
    det = np.zeros((len(frames), num_views, nmax, 17, 3), np.float32)
    count = np.zeros((len(frames), num_views), np.int32)
    slot = np.full((len(frames), num_views, nmax), -1, np.int32)
    for (f, v), ent in found.items():
        count[f, v] = len(ent)
        for i, (k, a) in enumerate(ent):
            det[f, v, i, :a.shape[0]] = a
            slot[f, v, i] = k
    return det, count, slot


def cluster_keypoints(det, labels, num_clusters):
    """The clusters as persons: (rows [n, 2] = (frame, cluster), kp [n, V, 17, 3] with zeros for the views without a
    member, member [n, V] bool), frame-major in ascending cluster number."""
    det, labels = np.asarray(det, np.float32), np.asarray(labels)
    F, V = det.shape[:2]
    rows = [(f, c) for f in range(F) for c in range(int(num_clusters[f]))]
    kp = np.zeros((len(rows), V, 17, 3), np.float32)
    member = np.zeros((len(rows), V), bool)
    at = {r: n for n, r in enumerate(rows)}
    for f, v, k in zip(*np.nonzero(labels >= 0)):
        n = at[(int(f), int(labels[f, v, k]))]
        kp[n, v] = det[f, v, k]
        member[n, v] = True
    return np.asarray(rows, np.int64).reshape(-1, 2), kp, member


def cluster_centres(engine, det, labels, num_clusters, extris, intris):
    """(centres [F, C, 3] float64, valid [F, C] bool), C = the largest cluster count (at least 1): every cluster
    triangulated from its members in ONE engine.triangulate call, the centre the mean over the joints that at least two
    member views see with confidence > 0; a cluster without such a joint is invalid."""
    num_clusters = np.asarray(num_clusters)
    F, C = len(num_clusters), max(int(num_clusters.max()) if len(num_clusters) else 0, 1)
    centres, valid = np.zeros((F, C, 3)), np.zeros((F, C), bool)
    rows, kp, _ = cluster_keypoints(det, labels, num_clusters)
    if len(rows):
        V = kp.shape[1]
        j3 = engine.triangulate(kp, np.asarray(intris, np.float64)[:V], np.asarray(extris, np.float64)[:V]).cpu().numpy()
        seen = (kp[..., 2] > 0).sum(1) >= 2                                 # [n, 17]
        for n, (f, c) in enumerate(rows):
            if seen[n].any():
                centres[f, c] = j3[n][seen[n]].mean(0)
                valid[f, c] = True
    return centres, valid


def track_clusters(centres, valid, max_move=0.5, max_gap=5):
    """ids [F, C] int64 from centres [F, C, 3] and valid [F, C]: frames in order; a track is live while it has been absent
    for at most ``max_gap`` frames; a (live track, valid cluster) pair is a candidate when their distance is at most
    ``max_move`` * (frames since the track was seen); candidates are taken in ascending distance - ties: lower track id,
    then lower cluster number -, every track and every cluster once; a valid cluster left over opens the next id.  Ids
    count from 0 in order of first appearance; invalid clusters get -1."""
    centres, valid = np.asarray(centres, np.float64), np.asarray(valid, bool)
    F, C = valid.shape
    ids = np.full((F, C), -1, np.int64)
    pos, last = [], []                                   # per track: centre and frame when last seen
    for f in range(F):
        cand = []
        for t in range(len(pos)):
            dt = f - last[t]
            if dt - 1 > max_gap:
                continue
            for c in np.flatnonzero(valid[f]):
                d = float(np.linalg.norm(centres[f, c] - pos[t]))
                if d <= max_move * dt:
                    cand.append((d, t, int(c)))
        used_t, used_c = set(), set()
        for d, t, c in sorted(cand):
            if t in used_t or c in used_c:
                continue
            used_t.add(t)
            used_c.add(c)
            ids[f, c] = t
        for c in np.flatnonzero(valid[f]):
            if ids[f, c] < 0:
                ids[f, c] = len(pos)
                pos.append(None)
                last.append(f)
            pos[ids[f, c]], last[ids[f, c]] = centres[f, c].copy(), f
    return ids


def associate_serial(engine, frames, extris, intris, max_cost=0.05, min_joints=6, min_views=2, max_move=0.5, max_gap=5):
    """One serial's keypoint files -> (ids, kp [F, P, V, 17, 3] float32, mask [F, P, V] bool, report): what
    batch.load_serial_people returns, with ``ids`` the track ids (0 .. P - 1 in order of first appearance) instead of the
    files' own, and report = dict(labels [F, V, Nmax]: the frame's cluster number of every detection or -1, track_ids
    [F, V, Nmax]: its person or -1, slot [F, V, Nmax]: its index in its file, count [F, V], num_clusters [F], unassigned:
    detections without a person, params)."""
    V = len(frames[0][1]) if frames else 0
    if V < 2:
        raise ValueError('associate: a serial needs at least two views, this one has %d' % V)
    det, count, slot = load_serial_detections(frames, V)
    ex, it = np.asarray(extris, np.float64)[:V], np.asarray(intris, np.float64)[:V]
    labels, num = engine.associate_views(det, count, it, ex, max_cost=max_cost, min_joints=min_joints, min_views=min_views)
    labels, num = labels.cpu().numpy(), num.cpu().numpy()
    centres, valid = cluster_centres(engine, det, labels, num, ex, it)
    tracks = track_clusters(centres, valid, max_move=max_move, max_gap=max_gap)
    F, P = len(frames), int(tracks.max()) + 1 if tracks.size else 0
    track_ids = np.full(labels.shape, -1, np.int32)
    kp = np.zeros((F, P, V, 17, 3), np.float32)
    mask = np.zeros((F, P, V), bool)
    for f, v, k in zip(*np.nonzero(labels >= 0)):
        t = int(tracks[f, labels[f, v, k]])
        if t >= 0:
            track_ids[f, v, k] = t
            kp[f, t, v] = det[f, v, k]
            mask[f, t, v] = True
    report = dict(labels=labels, track_ids=track_ids, slot=slot, count=count, num_clusters=num,
                  unassigned=int(count.sum() - (track_ids >= 0).sum()),
                  params=dict(max_cost=max_cost, min_joints=min_joints, min_views=min_views, max_move=max_move, max_gap=max_gap))
    return list(range(P)), kp, mask, report


__all__ = ['DEFAULTS', 'MAX_DET', 'check_params', 'load_serial_detections', 'cluster_keypoints', 'cluster_centres',
           'track_clusters', 'associate_serial']
