"""CPU: the file side of fit_folder(silhouettes=...) - io_formats.read_mask / downscale_mask, the option's ValueErrors, the
mask file names of both person modes, and the plumbing of batch.refine_serial_silhouettes / silhouette.refine_fit through a
stand-in engine (which images go to which problem, camera scaling, the revert rule)."""
import os

import numpy as np
import pytest
import torch

from mvsmplfitting_amd import batch
from mvsmplfitting_amd import io_formats as iof
from mvsmplfitting_amd.silhouette import refine_fit

Image = pytest.importorskip('PIL.Image')


# ------------------------------------------------------------------------------------------------------------ read_mask
def _pattern():
    m = np.zeros((5, 7), np.uint8)
    m[1:4, 2:6] = 255
    m[0, 0] = 255
    return m


def test_read_mask_grey_rgb_palette(tmp_path):
    m = _pattern()
    Image.fromarray(m, 'L').save(tmp_path / 'grey.png')
    Image.fromarray(np.stack([m, m // 2, m * 0], axis=2), 'RGB').save(tmp_path / 'rgb.png')
    pal = Image.fromarray((m > 0).astype(np.uint8), 'P')
    pal.putpalette([0, 0, 0, 255, 255, 255] + [0] * (254 * 3))
    pal.save(tmp_path / 'pal.png')
    Image.fromarray(m > 0).save(tmp_path / 'bit.png')
    for name in ('grey.png', 'rgb.png', 'pal.png', 'bit.png'):
        got = iof.read_mask(str(tmp_path / name))
        assert got.dtype == np.uint8 and got.shape == (5, 7), name
        assert np.array_equal(got != 0, m != 0), name
    assert np.array_equal(iof.read_mask(str(tmp_path / 'grey.png')), m)


def test_read_mask_applies_the_exif_orientation(tmp_path):
    m = _pattern()
    im = Image.fromarray(m, 'L')
    exif = im.getexif()
    exif[0x0112] = 6                                   # stored rotated: the viewer turns it 90 degrees clockwise
    im.save(tmp_path / 'turned.png', exif=exif)
    got = iof.read_mask(str(tmp_path / 'turned.png'))
    assert got.shape == (7, 5) == iof.image_size(str(tmp_path / 'turned.png'))
    assert np.array_equal(got, np.rot90(m, -1))


# ------------------------------------------------------------------------------------------------------- downscale_mask
def test_downscale_identity_and_half_rule():
    rng = np.random.default_rng(1)
    m = (rng.random((7, 9)) < 0.5).astype(np.uint8) * 200
    assert np.array_equal(iof.downscale_mask(m, 1), m)
    for k in (2, 3, 4):
        got = iof.downscale_mask(m, k)
        h, w = -(-7 // k), -(-9 // k)
        assert got.shape == (h, w) and got.dtype == np.uint8
        for y in range(h):
            for x in range(w):
                blk = m[y * k:(y + 1) * k, x * k:(x + 1) * k] != 0       # edge blocks: the pixels they have
                assert got[y, x] == (1 if 2 * blk.sum() >= blk.size else 0), (k, y, x)


def test_downscale_edge_blocks_count_over_their_own_pixels():
    m = np.zeros((5, 5), np.uint8)
    m[4, 4] = 1                                        # the corner block of k = 2 has ONE pixel: on
    m[0, 4] = 1                                        # the right edge block of row 0 has two pixels, one on: exactly half
    m[0, 0] = 1                                        # a full block with one of four on: off
    got = iof.downscale_mask(m, 2)
    assert got.tolist() == [[0, 0, 1], [0, 0, 0], [0, 0, 1]]
    with pytest.raises(ValueError):
        iof.downscale_mask(m, 0)
    with pytest.raises(ValueError):
        iof.downscale_mask(np.zeros((2, 2, 3), np.uint8), 2)


# ----------------------------------------------------------------------------------------------- the option's ValueErrors
MODEL = dict(kp_regressor=object())                    # (fit_folder reads the model kind before the option; nothing else here)


@pytest.mark.parametrize('kw, match', [
    (dict(silhouettes=dict(weight=1.0)), 'mask_root'),
    (dict(silhouettes=dict(mask_root='m')), 'weight'),
    (dict(silhouettes='masks'), 'mask_root'),
    (dict(silhouettes=dict(mask_root='m', weight=1.0, blur=2)), "unknown keys \\['blur'\\]"),
    (dict(silhouettes=dict(mask_root='m', weight=1.0), is_seq=True), 'is_seq'),
    (dict(silhouettes=dict(mask_root='m', weight=1.0), persons='all', scene_collision=dict(weight=1.0)), 'one term slot'),
    (dict(silhouettes=dict(mask_root='m', weight=1.0, downscale=0)), 'downscale'),
    (dict(silhouettes=dict(mask_root='m', weight=0.0)), 'weight must be > 0'),
])
def test_fit_folder_refuses_a_bad_option_before_it_reads_anything(kw, match, tmp_path):
    with pytest.raises(ValueError, match=match):
        batch.fit_folder(MODEL, str(tmp_path / 'none'), str(tmp_path / 'none.txt'), str(tmp_path / 'out'), engine=object(), **kw)


def test_mask_file_names():
    assert batch.mask_path('/m', 's1', 'Camera00', '00001') == os.path.join('/m', 's1', 'Camera00', '00001.png')
    assert batch.mask_path('/m', 's1', 'Camera00', '00001', 7) == os.path.join('/m', 's1', 'Camera00', '00001_007.png')
    assert batch.mask_path('/m', 's1', 'Camera00', '00001', 0) == os.path.join('/m', 's1', 'Camera00', '00001_000.png')


# ------------------------------------------------------------------------------------------------------------- plumbing
class StubEngine:
    """As far as refine_fit and refine_serial_silhouettes drive an engine.  The "objective" of row j is |x_j - target_j|^2 +
    w^2 L_j with L_j = j + 1; fit() moves row 0 onto its target and every other row AWAY from it."""

    def __init__(self, target, fail_fit=False):
        self.device = torch.device('cpu')
        self.target = torch.as_tensor(target, dtype=torch.float32)
        self.fail_fit = fail_fit
        self.calls, self.set_args, self.term = [], None, None

    def set_silhouettes(self, masks, image_body, cams, contour_stride=1):
        self.set_args = (np.array(masks), np.array(image_body), tuple(np.array(a) for a in cams), contour_stride)
        self.calls.append('set')

    def clear_silhouettes(self):
        self.calls.append('clear')

    def set_silhouette_term(self, w_in=1.0, w_out=1.0, sigma=0.0):
        self.term = (w_in, w_out, sigma)
        self.calls.append('term_on')

    def clear_silhouette_term(self):
        self.term = None
        self.calls.append('term_off')

    def _L(self, x):
        return torch.arange(1, x.shape[0] + 1, dtype=torch.float32)

    def closure(self, x, stage, want_grad=True):
        assert self.term is not None
        self.calls.append('closure')
        self.last = x
        w = float(stage['coll_loss_weight'])
        return dict(loss=((x - self.target) ** 2).sum(dim=1) + w * w * self._L(x))

    def sdf_term_read(self):
        return None, self._L(self.last)

    def fit(self, x, stages, **kw):
        assert self.term is not None and len(stages) == 1
        self.calls.append('fit')
        if self.fail_fit:
            raise RuntimeError('fit failed')
        out = x + 2.0 * (x - self.target)
        out[0] = self.target[0]
        return out, dict(n_closure=torch.full((x.shape[0],), 5, dtype=torch.int32))


def test_refine_fit_keeps_what_fell_and_reverts_the_rest_exactly():
    target = np.zeros((3, 118), np.float32)
    x0 = np.random.default_rng(0).normal(0, 1, (3, 118)).astype(np.float32)
    eng = StubEngine(target)
    out, rep = refine_fit(eng, x0, dict(coll_loss_weight=2.0), sigma=3.0)
    assert eng.calls == ['term_on', 'closure', 'fit', 'closure', 'term_off'] and eng.term is None
    assert rep['accepted'].tolist() == [True, False, False]
    assert torch.equal(out[0], torch.zeros(118)) and torch.equal(out[1:], torch.from_numpy(x0[1:]))
    assert rep['after'][0] < rep['before'][0] and np.array_equal(rep['after'][1:], rep['before'][1:])
    assert np.array_equal(rep['loss'], rep['after']) and rep['silhouette_after'].tolist() == [1.0, 2.0, 3.0]
    assert rep['after'][0] == 4.0 * 1.0                              # w^2 L_0 at the target
    with pytest.raises(ValueError):
        refine_fit(eng, x0, dict(coll_loss_weight=0.0))


def test_refine_fit_clears_the_term_when_the_fit_raises():
    eng = StubEngine(np.zeros((2, 118), np.float32), fail_fit=True)
    with pytest.raises(RuntimeError):
        refine_fit(eng, np.ones((2, 118), np.float32), dict(coll_loss_weight=1.0))
    assert eng.calls[-1] == 'term_off' and eng.term is None


CAMS = ['Camera00', 'Camera01', 'Camera02']
FRAMES = [('00001', [None] * 3), ('00002', [None] * 3)]
RIG = (np.stack([np.eye(3, dtype=np.float32) * (v + 1) for v in range(3)]), np.arange(9, dtype=np.float32).reshape(3, 3),
       np.array([1000.0, 1100.0, 1200.0], np.float32), np.array([[640, 360], [650, 370], [660, 380]], np.float32))


def _write(root, serial, cam, name, shape=(6, 10), on=(slice(1, 5), slice(2, 8))):
    d = os.path.join(root, serial, cam)
    os.makedirs(d, exist_ok=True)
    m = np.zeros(shape, np.uint8)
    m[on] = 255
    Image.fromarray(m, 'L').save(os.path.join(d, name))
    return m


def _cfg(root, **kw):
    return batch.check_silhouettes(dict(mask_root=str(root), weight=2.0, **kw))


def test_images_go_to_their_problem_with_scaled_cameras(tmp_path):
    root = str(tmp_path)
    m = _write(root, 's', 'Camera00', '00001.png')
    _write(root, 's', 'Camera02', '00001.png')
    _write(root, 's', 'Camera01', '00002.png')
    _write(root, 's', 'Camera01', '00002_000.png')                    # (the other mode's name: not this problem's)
    eng = StubEngine(np.zeros((2, 118), np.float32))
    x = torch.ones(2, 118)
    out, rep = batch.refine_serial_silhouettes(eng, x, dict(data_weight=1.0), _cfg(root, downscale=2, contour_stride=3, sigma=5.0),
                                               's', CAMS, FRAMES, [(0, None), (1, None)], RIG, 6890)
    masks, body, cams, stride = eng.set_args
    assert rep['images'] == [(0, 0), (0, 2), (1, 1)] and body.tolist() == [0, 0, 1] and stride == 3
    assert masks.shape == (3, 3, 5) and rep['mask_size'] == (3, 5)
    assert np.array_equal(masks[0], iof.downscale_mask(m, 2))
    view = [0, 2, 1]
    assert np.array_equal(cams[0], RIG[0][view]) and np.array_equal(cams[1], RIG[1][view])
    assert np.array_equal(cams[2], RIG[2][view] / 2) and np.array_equal(cams[3], RIG[3][view] / 2)
    assert eng.calls == ['set', 'term_on', 'closure', 'fit', 'closure', 'term_off', 'clear']
    assert rep['accepted'].tolist() == [True, False] and torch.equal(out[1], x[1])


def test_the_multi_person_names(tmp_path):
    root = str(tmp_path)
    _write(root, 's', 'Camera01', '00001_003.png')
    _write(root, 's', 'Camera00', '00002_012.png')
    _write(root, 's', 'Camera00', '00001.png')                        # (the single-person name: nobody's here)
    eng = StubEngine(np.zeros((3, 118), np.float32))
    _, rep = batch.refine_serial_silhouettes(eng, torch.ones(3, 118), {}, _cfg(root), 's', CAMS, FRAMES,
                                             [(0, 3), (0, 12), (1, 12)], RIG, 6890)
    assert rep['images'] == [(0, 1), (2, 0)]
    assert np.array_equal(eng.set_args[2][2], RIG[2][[1, 0]])         # downscale 1: the rig's own f


def test_serial_without_masks_and_masks_of_two_sizes(tmp_path):
    root = str(tmp_path)
    eng = StubEngine(np.zeros((1, 118), np.float32))
    with pytest.raises(ValueError, match='has no mask file'):
        batch.refine_serial_silhouettes(eng, torch.ones(1, 118), {}, _cfg(root), 's', CAMS, FRAMES, [(0, None)], RIG, 6890)
    _write(root, 's', 'Camera00', '00001.png')
    _write(root, 's', 'Camera01', '00001.png', shape=(6, 12))
    with pytest.raises(ValueError, match='differ in size'):
        batch.refine_serial_silhouettes(eng, torch.ones(1, 118), {}, _cfg(root), 's', CAMS, FRAMES, [(0, None)], RIG, 6890)
    assert eng.calls == []


def test_workspace_over_the_limit_names_the_downscale_that_fits(tmp_path):
    root = str(tmp_path)
    _write(root, 's', 'Camera00', '00001.png', shape=(64, 96), on=(slice(8, 40), slice(8, 60)))
    nv = 100
    need = [batch.silhouette_workspace_bytes(1, -(-64 // k), -(-96 // k), nv) for k in range(1, 9)]
    assert need[0] == 64 * 96 * 5 + 64 * 4 + (16 * nv + 8 * 1 + 92) + 8
    limit = need[2]                                                    # k = 3 just fits, k = 2 does not
    assert need[1] > limit
    eng = StubEngine(np.zeros((1, 118), np.float32))
    with pytest.raises(ValueError, match='smallest downscale that fits is 3'):
        batch.refine_serial_silhouettes(eng, torch.ones(1, 118), {}, _cfg(root, max_mask_bytes=limit), 's', CAMS, FRAMES,
                                        [(0, None)], RIG, nv)
    assert eng.calls == []
    batch.refine_serial_silhouettes(eng, torch.ones(1, 118), {}, _cfg(root, max_mask_bytes=limit, downscale=3), 's', CAMS, FRAMES,
                                    [(0, None)], RIG, nv)
    assert eng.set_args[0].shape == (1, 22, 32)
