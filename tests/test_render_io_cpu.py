"""CPU: the host side of save_images - render_serial_images streams its jobs in bounded chunks (a stand-in engine takes
the GPU's place), and read_image / image_size apply the EXIF orientation like cv2.imread."""
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from mvsmplfitting_amd import batch
from mvsmplfitting_amd import io_formats as iof

pytest.importorskip('PIL')


class _Engine:
    """Records the calls and returns the images inverted."""

    def __init__(self):
        self.calls = []

    def render_overlay(self, verts, joints, images, problems, views):
        assert isinstance(images, np.ndarray) and images.dtype == np.uint8
        self.calls.append((images.shape, list(problems), list(views)))
        return torch.from_numpy(255 - images)


def test_render_serial_images_streams_bounded_chunks(tmp_path, monkeypatch):
    monkeypatch.setattr(batch, 'RENDER_BATCH', 3)
    sizes = [(24, 32)] * 7 + [(16, 20)] * 4            # 11 jobs > RENDER_BATCH, two sizes interleaved below
    order = [0, 7, 1, 2, 8, 3, 4, 9, 5, 10, 6]
    jobs = []
    for n, s in enumerate(order):
        H, W = sizes[s]
        path = str(tmp_path / ('in%02d.png' % n))
        iof.save_image(path, np.full((H, W, 3), 10 * n, np.uint8))
        jobs.append((n // 4, n % 4, path, ('S', 'f%d' % (n // 4), 'Cam%d' % (n % 4))))
    live, peak, lock = [0], [0], threading.Lock()
    read, save = iof.read_image, iof.save_image

    def counted_read(path):
        im = read(path)
        with lock:
            live[0] += 1
            peak[0] = max(peak[0], live[0])
        return im

    def counted_save(path, rgb, quality=95):
        out = save(path, rgb, quality)
        with lock:
            live[0] -= 1
        return out
    monkeypatch.setattr(iof, 'read_image', counted_read)
    monkeypatch.setattr(iof, 'save_image', counted_save)
    eng = _Engine()
    with ThreadPoolExecutor(4) as pool:
        paths = batch.render_serial_images(eng, None, None, jobs, str(tmp_path / 'out'), pool)
    assert live[0] == 0 and peak[0] <= 2 * 3, peak[0]
    # chunks of at most RENDER_BATCH images of one size, every job exactly once, with its own problem and view
    assert all(len(p) <= 3 and shape[0] == len(p) for shape, p, _ in eng.calls)
    assert sorted(zip(sum((c[1] for c in eng.calls), []), sum((c[2] for c in eng.calls), []))) == \
        sorted((j[0], j[1]) for j in jobs)
    assert len(eng.calls) == 5                          # 7 -> 3 + 3 + 1, 4 -> 3 + 1
    for n, (j, p) in enumerate(zip(jobs, paths)):
        assert p == os.path.join(str(tmp_path / 'out'), 'S', j[3][1], j[3][2] + '.jpg')
        got = read(p)
        assert got.shape[:2] == sizes[order[n]]
        assert np.abs(got.astype(int) - (255 - 10 * n)).max() <= 2      # JPEG of a flat image


def test_exif_orientation_is_applied(tmp_path):
    from PIL import Image
    a = np.zeros((20, 30, 3), np.uint8)
    a[:, :10] = 255                                     # white on the left
    im = Image.fromarray(a)
    exif = im.getexif()
    exif[0x0112] = 6                                    # stored rotated: display = a quarter turn clockwise
    path = str(tmp_path / 'rot.jpg')
    im.save(path, exif=exif, quality=95)
    got = iof.read_image(path)
    assert got.shape == (30, 20, 3) and iof.image_size(path) == (30, 20)
    assert got[:10].mean() > 200 and got[-10:].mean() < 50      # the left band is now on top
    plain = str(tmp_path / 'plain.png')
    iof.save_image(plain, a)
    assert iof.image_size(plain) == (20, 30) and np.array_equal(iof.read_image(plain), a)
