"""Baseline JPEG encode on the MI355X (csrc/jpeg_encode.hip) against Pillow / libjpeg-turbo, byte for byte: every quality at a
small size, the size / content grid of the CPU driver, 1 024 ScanNet-shaped frames in one call, long thin shapes, n = 0, a
narrow output pitch, and argument errors."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from jpeg_util import content, encode  # noqa: E402

SCANNET_HW = (968, 1296)
SUBSAMPLINGS = ("4:4:4", "4:2:2", "4:2:0")


def _require_turbo():
    from PIL import features
    assert features.check_feature("libjpeg_turbo"), "the encoder is specified against libjpeg-turbo's output"


def _files(imgs, quality, subsampling, pitch=None):
    import torch
    from mspa import engine
    rgb = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    out = None
    if pitch is not None:
        out = torch.empty((len(imgs), pitch), dtype=torch.uint8, device="cuda")
    out, nbytes = engine.jpeg_encode_device(rgb, quality=quality, subsampling=subsampling, out=out)
    torch.cuda.synchronize()
    nb = nbytes.cpu().numpy()
    o = out[:, :min(int(out.shape[1]), int(nb.max()))].cpu().numpy()
    return [o[k, :min(int(nb[k]), o.shape[1])].tobytes() for k in range(len(imgs))], nb


def _patterns(h, w, seed):
    y, x = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(seed)
    checker = np.where(((x + y) % 2)[..., None] == 0, 255, 0).repeat(3, axis=2).astype(np.uint8)
    grad = np.stack([255 * x // max(w - 1, 1), 255 * y // max(h - 1, 1), (x + y) % 256], axis=-1).astype(np.uint8)
    return {"noise": rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "flat": np.full((h, w, 3), 77, np.uint8),
            "checker": checker, "gradient": grad, "mixed": content(h, w, seed)}


def test_every_quality_small():
    _require_turbo()
    for ss in SUBSAMPLINGS:
        imgs = np.stack([content(37, 45, q) for q in range(1, 101)])
        for q in range(1, 101):
            got, _ = _files(imgs[q - 1:q], q, ss)
            assert got[0] == encode(imgs[q - 1], quality=q, subsampling=ss), (q, ss)


def test_size_and_content_grid():
    _require_turbo()
    sizes = [(h, w) for h in range(17, 33) for w in (17, 24, 31)] + [(h, w) for w in range(17, 33) for h in (18, 29)]
    sizes += [(1, 1), (1, 40), (40, 1), (1, 17), (23, 1)]
    for h, w in sizes:
        pats = _patterns(h, w, h * 100 + w)
        imgs = np.stack(list(pats.values()))
        for q in (1, 50, 95, 100):
            for ss in SUBSAMPLINGS:
                got, _ = _files(imgs, q, ss)
                for name, g, img in zip(pats, got, imgs):
                    assert g == encode(img, quality=q, subsampling=ss), (h, w, q, ss, name)


def test_qualities_of_the_grid_on_one_shape():
    _require_turbo()
    pats = _patterns(35, 51, 9)
    imgs = np.stack(list(pats.values()))
    for q in (1, 2, 10, 50, 75, 90, 95, 99, 100):
        for ss in SUBSAMPLINGS:
            got, _ = _files(imgs, q, ss)
            for name, g, img in zip(pats, got, imgs):
                assert g == encode(img, quality=q, subsampling=ss), (q, ss, name)


def test_scannet_batch_1024_in_one_call():
    _require_turbo()
    base = [content(*SCANNET_HW, s) for s in range(4)]
    imgs = np.stack([base[k % 4] if k % 8 else np.roll(base[k % 4], k, axis=1) for k in range(1024)])
    got, _ = _files(imgs, 95, "4:2:0")
    want = {}
    for k in range(1024):
        key = (k % 4, 0 if k % 8 else k)
        if key not in want:
            want[key] = encode(imgs[k], quality=95, subsampling="4:2:0")
        assert got[k] == want[key], k


@pytest.mark.parametrize("hw", [(4096, 16), (16, 4096)])
def test_long_thin_shapes(hw):
    _require_turbo()
    imgs = np.stack([content(*hw, 3), np.random.default_rng(1).integers(0, 256, hw + (3,), dtype=np.uint8)])
    for ss in SUBSAMPLINGS:
        got, _ = _files(imgs, 90, ss)
        for g, img in zip(got, imgs):
            assert g == encode(img, quality=90, subsampling=ss), (hw, ss)


def test_zero_images():
    import torch
    from mspa import engine
    out, nbytes = engine.jpeg_encode_device(torch.empty((0, 8, 8, 3), dtype=torch.uint8, device="cuda"))
    assert out.shape[0] == 0 and nbytes.shape == (0,)


def test_narrow_pitch_reports_the_length_and_writes_no_further():
    img = np.random.default_rng(5).integers(0, 256, (64, 64, 3), dtype=np.uint8)
    want = encode(img, quality=100, subsampling="4:4:4")
    got, nb = _files(np.stack([img, img]), 100, "4:4:4", pitch=1000)
    assert all(int(n) == len(want) for n in nb) and all(g == want[:1000] for g in got)


def test_argument_errors():
    import torch
    from mspa import engine
    rgb = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
    for kw in ({"quality": 0}, {"quality": 101}, {"subsampling": "4:1:1"}, {"subsampling": 3}):
        with pytest.raises(ValueError):
            engine.jpeg_encode_device(rgb, **kw)
    with pytest.raises(ValueError):
        engine.jpeg_encode_device(torch.zeros((1, 8, 8, 4), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        engine.jpeg_encode_device(torch.zeros((1, 8, 8, 3), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        engine.jpeg_encode_device(rgb.cpu())
    lib = engine._lib.load()
    assert lib.mspa_jpeg_encode_device(None, 1, 8, 8, 95, 2, None, 0, None, None, 0, None) == engine._lib.MSPA_EINVAL
    assert lib.mspa_jpeg_encode_device(rgb.data_ptr(), 1, 8, 8, 95, 2, rgb.data_ptr(), 10, rgb.data_ptr(), rgb.data_ptr(), 16,
                                       None) == engine._lib.MSPA_EINVAL          # workspace too small
