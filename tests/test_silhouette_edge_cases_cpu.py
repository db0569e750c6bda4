"""CPU: every case of tests/silhouette_edge_cases.py reaches the edge of the silhouette kernels it is named for, shown on
the NumPy oracles alone (tests/silhouette_oracle.py, tests/silhouette_occlusion_oracle.py).  A case that does not reach its
edge fails here; tests/test_gpu_silhouette_edges.py then runs the kernels on the same cases.

The kernels' constants are restated below by hand: a change there has to be repeated here."""
import functools

import numpy as np
import pytest

from tests import render_oracle as ro
from tests import silhouette_edge_cases as ec
from tests import silhouette_occlusion_oracle as oo
from tests import silhouette_oracle as so

SIL_CHUNK = 512          # mvsmplfitting_amd/csrc/silhouette.hip:43 (SIL_NT * SIL_PPT): contour points per search workgroup
SIL_VT = 3456            # mvsmplfitting_amd/csrc/silhouette.hip:44: vertices per LDS tile of the search
OCC_GROUP = 512          # mvsmplfitting_amd/csrc/silhouette_occlusion.hip:34: instances rasterised per pass
RD_BIG_BOX = 1024        # mvsmplfitting_amd/csrc/render_raster.h:14: pixel boxes above this take the whole-workgroup path
WAVE = 64                # silhouette.hip:sil_ordered_sum strides over the partials by the wave's 64 lanes
NV = SIL_VT + 1


@functools.lru_cache(maxsize=None)
def plain(nv):
    """The untouched world at nv vertices, stride 1: vertices, cameras, the oracle's answer and both kinds of winners."""
    verts, cams, prep = ec.posed(nv, ec.params()), ec.arc_cameras(), ec.prepared(1)
    ref = so.evaluate(prep, verts, ec.IMAGE_BODY, cams, sigma=20.0)
    lo, hi = ec.winners(prep, verts, ec.IMAGE_BODY, cams)
    assert np.array_equal(lo, ref['winner'])                # ec.winners works on the oracle's own matrix
    return dict(verts=verts, cams=cams, prep=prep, ref=ref, last=hi, jw=ec.most_winning(lo, prep['first'], ec.IMAGE_BODY, nv))


def test_kept_points_per_image_and_the_chunks_they_make():
    for stride in (1, 3):
        prep = ec.prepared(stride)
        kept = np.diff(prep['first'])
        assert tuple(kept) == ec.KEPT[stride], kept
        chunks = -(-kept // SIL_CHUNK)
        assert (kept[chunks > 0] - (chunks[chunks > 0] - 1) * SIL_CHUNK).min() == 1          # a last chunk of one point
    kept = np.array(ec.KEPT[1])
    chunks = -(-kept // SIL_CHUNK)
    assert chunks[ec.BIG_IMAGE] == WAVE + 1 and kept[ec.BIG_IMAGE] % SIL_CHUNK == 1          # sil_ordered_sum's second trip
    assert set(kept[[2, 4, 7]] % SIL_CHUNK) == {0} and chunks[4] == 2 and chunks[7] == 3     # full last chunks
    assert kept[6] == 0 and kept[5] > 0 and kept[7] > 0                                      # chunk_first[6] == chunk_first[7]
    assert np.array(ec.KEPT[3])[7] == SIL_CHUNK and np.array(ec.KEPT[3])[8] == SIL_CHUNK + 1
    masks, prep = ec.exact_count_masks(), ec.prepared(1)
    assert masks[10].all() and not prep['fields'][10].any() and not prep['fields'][6].any() and prep['fields'][0].max() > 500
    # interleaved image lists, one body without images
    assert sorted(set(ec.IMAGE_BODY.tolist())) == [0, 2] and ec.N == 3 and ec.IMAGE_BODY[ec.BIG_IMAGE] == ec.BIG_BODY


def test_vertex_counts_and_tiles():
    assert ec.NVS == (701, SIL_VT, SIL_VT + 1, 6890)
    assert 701 % 2 == 1 and 701 < SIL_VT and -(-701 // 256) == 3                   # odd, one tile: the pad; three vertex blocks
    assert 6890 - SIL_VT == 3434                                                  # the full body: two even tiles
    for nv in ec.NVS:
        assert ec.model(nv)['v_template'].shape[0] == nv
    w = plain(NV)
    cams = w['cams']
    for i in range(len(ec.IMAGE_BODY)):                                           # BEHIND is behind every camera, no body is
        assert ro.transform(ec.BEHIND[None], *(a[i] for a in cams))[0][0, 2] < 0
        p, u, v = ro.transform(w['verts'][ec.IMAGE_BODY[i]], *(a[i] for a in cams))
        assert p[:, 2].min() > 1 and u.min() > 0 and u.max() < ec.SIZE and v.min() > 0 and v.max() < ec.SIZE
    assert (w['ref']['winner'] >= SIL_VT).any(), 'no point is won by the vertex of the second tile'
    assert w['ref']['loss'][1] == 0 and not w['ref']['g'][1].any() and (w['ref']['loss'][[0, 2]] > 0).all()


def _check_tie(nv, kind):
    w = plain(nv)
    verts, tied = ec.tie_world(w['verts'], w['jw'], kind)
    lo, hi = ec.winners(w['prep'], verts, ec.IMAGE_BODY, w['cams'])
    for body, (lower, higher) in tied.items():
        first_wins = ec.wins(lo, w['prep']['first'], ec.IMAGE_BODY, body, nv)
        last_wins = ec.wins(hi, w['prep']['first'], ec.IMAGE_BODY, body, nv)
        print('%d %s body %d: lower %d wins %d, higher %s win %s; with the last minimum %d and %s'
              % (nv, kind, body, lower, first_wins[lower], higher, first_wins[higher], last_wins[lower], last_wins[higher]))
        assert first_wins[lower] >= 100 and not first_wins[higher].any()
        # a search that kept the later of two equal distances gives other winners for exactly those points
        assert last_wins[lower] == 0 and last_wins[higher[-1]] == first_wins[lower]
    assert (lo != hi).sum() >= 200
    return verts, tied, lo


@pytest.mark.parametrize('kind', sorted(ec.TIES))
def test_ties_at_3457_vertices(kind):
    verts, tied, lo = _check_tie(NV, kind)
    lower, higher = tied[ec.BIG_BODY]
    where = dict(pair=lambda: lower % 2 == 0 and higher == [lower + 1],
                 next_read=lambda: higher == [(lower | 1) + 1],
                 second_tile=lambda: lower < SIL_VT and higher == [SIL_VT],
                 all_three=lambda: lower % 2 == 0 and higher == [lower + 1, lower + 2, SIL_VT],
                 tile_boundary=lambda: (lower, higher) == (SIL_VT - 1, [SIL_VT]),
                 tile_boundary_even=lambda: (lower, higher) == (SIL_VT - 2, [SIL_VT]),
                 next_read_odd=lambda: lower % 2 == 1 and higher == [lower + 1],
                 next_read_even=lambda: lower % 2 == 0 and higher == [lower + 2],
                 second_tile_odd=lambda: lower % 2 == 1 and lower < SIL_VT and higher == [SIL_VT])
    assert where[kind](), (kind, lower, higher)
    if kind == 'all_three':
        w = plain(NV)
        assert np.array_equal(so.evaluate(w['prep'], verts, ec.IMAGE_BODY, w['cams'])['winner'], lo)


@pytest.mark.parametrize('kind', ec.TIES_701)
def test_ties_at_701_vertices(kind):
    _check_tie(701, kind)


def test_a_body_with_one_valid_vertex():
    w = plain(NV)
    verts = ec.single_valid(w['verts'], SIL_VT)
    r = so.evaluate(w['prep'], verts, ec.IMAGE_BODY, w['cams'], sigma=20.0)
    assert len(r['winner']) == sum(ec.KEPT[1]) and (r['winner'] == SIL_VT).all()
    assert np.isfinite(r['loss']).all() and (r['loss'][[0, 2]] > 0).all() and r['loss'][1] == 0
    gmax = np.abs(r['g']).max()
    assert np.isfinite(gmax) and gmax > 0 and not r['g'][:, :SIL_VT].any()
    print('one valid vertex: loss %s, max |g| %.6g' % (r['loss'], gmax))


def test_an_image_whose_body_lies_behind_its_camera():
    w = plain(NV)
    prep, first = w['prep'], w['prep']['first']
    cams = ec.all_behind(w['cams'], ec.BIG_IMAGE)
    r = so.evaluate(prep, w['verts'], ec.IMAGE_BODY, cams, sigma=20.0)
    assert not r['cells'][ec.BIG_IMAGE][0].any()
    lo, hi = first[ec.BIG_IMAGE], first[ec.BIG_IMAGE + 1]
    assert (r['winner'][lo:hi] == -1).all() and hi - lo == 32769
    assert (np.delete(r['winner'], np.arange(lo, hi)) >= 0).all()
    # exactly 0 from that image: the same numbers without it
    keep = np.array([i for i in range(len(ec.IMAGE_BODY)) if i != ec.BIG_IMAGE])
    rest = so.evaluate(so.prepare(ec.exact_count_masks()[keep], 1), w['verts'], ec.IMAGE_BODY[keep], tuple(a[keep] for a in cams),
                       sigma=20.0)
    assert np.array_equal(r['loss'], rest['loss']) and np.array_equal(r['g'], rest['g']) and r['loss'][ec.BIG_BODY] > 0
    assert r['loss'][ec.BIG_BODY] < w['ref']['loss'][ec.BIG_BODY]


def test_the_occluder_world_leaves_the_first_instance_group():
    inst = ec.instances(ec.OCC_BODY, ec.OCC_SCENE)
    assert len(inst) == 576 and len(inst) > OCC_GROUP and len(inst) - OCC_GROUP < OCC_GROUP        # two passes
    images = [i for i, _, _ in inst]
    assert images == sorted(images) and images[OCC_GROUP - 1] == images[OCC_GROUP] == 42           # image 42 straddles
    assert [k for k, i in enumerate(images) if i == 42] == list(range(504, 516))
    assert inst[504] == (42, 6, 0) and all(m == 1 for _, _, m in inst[505:516])
    assert min(i for i in images[OCC_GROUP:] if i != 42) == ec.OCC_CLOSE_FROM == 43 and (ec.OCC_VIEW[43:] == 3).all()
    for half in (ec.OCC_BODY[:24], ec.OCC_BODY[24:]):
        assert len(ec.instances(half, ec.OCC_SCENE)) == 288 <= OCC_GROUP                           # the halves: one group each
    faces = np.asarray(ec.model(ec.OCC_NV)['faces'])
    verts = ec.posed(ec.OCC_NV, ec.occ_params())
    _, pc = ec.occ_cameras()
    z_occ, z_own = oo.freeze(verts, faces, ec.OCC_BODY, pc, ec.OCC_SCENE, ec.OCC_H, ec.OCC_W)
    # a face on the whole-workgroup path in the second group: its visible pixels alone exceed the box threshold
    largest = 0
    for i in range(ec.OCC_CLOSE_FROM, ec.OCC_M):
        for b in range(ec.OCC_N):
            fid = ro.render(verts[b], faces, tuple(a[i] for a in pc), ec.OCC_H, ec.OCC_W)[1]
            if (fid >= 0).any():
                largest = max(largest, int(np.bincount(fid[fid >= 0].ravel()).max()))
    assert largest > RD_BIG_BOX, largest
    masks = ec.modal_masks(z_occ, z_own)
    prep = so.prepare(masks, 1)
    first = prep['first']
    flags = oo.point_flags(masks, first, prep['xy'], z_occ, z_own)
    hidden = oo.hidden_bytes(verts + ec.OCC_SHIFT, ec.OCC_BODY, pc, z_occ, ec.OCC_MARGIN)
    print('largest visible face in images 43 .. 47: %d px; contour %d points, %d flagged; hidden per image %s'
          % (largest, len(flags), flags.sum(), hidden.sum(1).tolist()))
    assert flags.any() and not flags.all()
    assert first[43] > first[42] and hidden[42].any() and flags[first[42]:first[43]].any()         # the straddling image
    assert hidden[:42].any() and hidden[43:].any() and flags[:first[42]].any() and flags[first[43]:].any()
    assert np.isfinite(z_occ[43:]).any() and np.isfinite(z_own[43:]).any()
    assert ec.OCC_NV % 2 == 1 and ec.OCC_NV < SIL_VT                                       # the OCC = true search pads its tile
