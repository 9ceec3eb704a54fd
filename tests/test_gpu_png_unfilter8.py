"""mspa_png_unfilter8_device behind mspa_inflate_blocks_device: 8-bit greyscale PNG scanlines, deflated, inflated and un-filtered
on the device, every pixel against Pillow's decode of the same scanlines (tests/png8_raw.py).  The CPU matrix of
tests/test_png_unfilter8_cpu.py -- widths around the dword, the wave and two bands, heights around the 64-row band, the ten filter
patterns, random and low-entropy bytes -- with the images of one shape batched in one launch; the device may decline none of them.
Then per-image status, the layouts the C ABI refuses, and one ScanNet-sized label image written by Pillow."""
import os
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from png8_raw import (FILTER_KINDS, HEIGHTS, WIDE, WIDTHS, blocky_labels, matrix_images, pillow_unfilter8, row_filters,  # noqa: E402
                      scanlines8)
import png_raw  # noqa: E402

PAD = 0xA5


def _inflate_and_unfilter(raws, h, w, level=1):
    """The scanline blocks deflated on the host, then both device stages; (images [n, h, w] uint8, status [n])."""
    import torch
    from mspa import engine
    streams = [zlib.compress(r, level) for r in raws]
    offsets, at = [], 0
    for s in streams:
        offsets.append(at)
        at += (len(s) + 15) // 16 * 16 + 16
    buf = np.full(at + 16, PAD, np.uint8)
    for o, s in zip(offsets, streams):
        buf[o:o + len(s)] = np.frombuffer(s, np.uint8)
    src = torch.from_numpy(buf).cuda()
    off = torch.tensor(offsets, dtype=torch.int64, device="cuda")
    nb = torch.tensor([len(s) for s in streams], dtype=torch.int64, device="cuda")
    raw, status = engine.inflate_blocks_device(src, off, nb, h * (w + 1))
    out = engine.png_unfilter8_device(raw, h, w, status)
    torch.cuda.synchronize()
    return out.cpu().numpy(), status.cpu().numpy()


def _device_raw(raws, pitch, offset=0):
    import torch
    n = len(raws)
    buf = np.full(offset + n * pitch + 64, PAD, np.uint8)
    for k, r in enumerate(raws):
        buf[offset + k * pitch:offset + k * pitch + len(r)] = np.frombuffer(r, np.uint8)
    dev = torch.from_numpy(buf).cuda()
    return dev[offset:offset + n * pitch].view(n, pitch)


@pytest.mark.parametrize("w", WIDTHS + (WIDE[1],))
def test_matrix_through_inflate_and_unfilter(w):
    rng = np.random.default_rng(800 + w)                     # the CPU test's images
    for h in (HEIGHTS if w != WIDE[1] else (WIDE[0],)):
        images = matrix_images(h, w, rng)
        got, status = _inflate_and_unfilter([r for _, _, r, _ in images], h, w)
        assert status.tolist() == [0] * len(images), (h, status)
        for k, (kind, content, _, want) in enumerate(images):
            assert np.array_equal(got[k], want), (h, kind, content, np.argwhere(got[k] != want)[:5])


@pytest.mark.parametrize("h,w", [(65, 37), (130, 130), (2, 1)])
def test_status_and_untouched_neighbours(h, w):
    """Filter byte 5 / 255 in the first row, the last row or a row of the second band: status 3 and no byte of that image written;
    a non-zero status on entry is kept and the image skipped; the neighbours are exact; 4-byte aligned pitches and starts."""
    import torch
    from mspa import engine
    rng = np.random.default_rng(h * w)
    specs = []
    for k, kind in enumerate(FILTER_KINDS):
        specs.append((kind, 0, None))
        specs.append((kind, [1, 2, 4][k % 3], None))
        specs.append((kind, 0, [(0, 5), (h - 1, 255), (min(64, h - 1), 5)][k % 3]))
    specs.append(("paeth", 4, (0, 5)))
    raws, wants = [], []
    for kind, _, bad in specs:
        raw = bytearray(scanlines8(row_filters(kind, h, rng), w, "random", rng))
        wants.append(pillow_unfilter8(bytes(raw), h, w))
        if bad is not None:
            raw[bad[0] * (w + 1)] = bad[1]
        raws.append(bytes(raw))
    n, block = len(specs), h * (w + 1)
    for pitch, offset in (((block + 3) // 4 * 4, 0), ((block + 3) // 4 * 4 + 4, 12), ((block + 255) // 256 * 256, 4)):
        raw = _device_raw(raws, pitch, offset)
        status = torch.tensor([st for _, st, _ in specs], dtype=torch.int32, device="cuda")
        out = torch.full((n, h, w), 0x5A, dtype=torch.uint8, device="cuda")
        engine.png_unfilter8_device(raw, h, w, status, out)
        torch.cuda.synchronize()
        st, got = status.cpu().numpy(), out.cpu().numpy()
        for k, (kind, entry, bad) in enumerate(specs):
            if entry:
                assert st[k] == entry and (got[k] == 0x5A).all(), (k, kind)
            elif bad is not None:
                assert st[k] == 3 and (got[k] == 0x5A).all(), (k, kind, bad)
            else:
                assert st[k] == 0 and np.array_equal(got[k], wants[k]), (k, kind, pitch, offset)


def test_unaligned_layouts_are_refused():
    import torch
    from mspa import _lib, engine
    h, w = 5, 6                                              # block 35
    rng = np.random.default_rng(3)
    raws = [scanlines8(row_filters("random", h, rng), w, "random", rng) for _ in range(3)]
    for pitch, offset in ((35, 0), (37, 0), (38, 0), (36, 1), (36, 2), (36, 3)):
        raw = _device_raw(raws, pitch, offset)
        status = torch.zeros(3, dtype=torch.int32, device="cuda")
        out = torch.full((3, h, w), 0x5A, dtype=torch.uint8, device="cuda")
        with pytest.raises(_lib.MspaError):
            engine.png_unfilter8_device(raw, h, w, status, out)
        rc = _lib.load().mspa_png_unfilter8_device(raw.data_ptr(), pitch, 3, h, w, out.data_ptr(), status.data_ptr(),
                                                   torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == _lib.MSPA_EINVAL and (out == 0x5A).all() and (status == 0).all(), (pitch, offset)


def test_scannet_sized_label_image_from_a_file(tmp_path):
    """One 1296 x 968 blocky label map written by Pillow (its adaptive filters, its zlib stream), through the public reader."""
    from PIL import Image
    from mspa import ingest
    rng = np.random.default_rng(968)
    labels = blocky_labels(968, 1296, rng)
    path = str(tmp_path / "0.png")
    Image.fromarray(labels, mode="L").save(path)
    filters = {png_raw.scanlines_of(open(path, "rb").read())[y * 1297] for y in range(968)}
    print("filters Pillow chose:", sorted(filters))
    import torch
    from mspa import engine
    buf, offsets, nbytes, st_host, cap = ingest.pack_mask_pngs([path], 968, 1296)
    assert st_host.tolist() == [0]
    raw, status = engine.inflate_blocks_device(torch.from_numpy(buf[:max(cap, 16)]).cuda(), torch.from_numpy(offsets).cuda(),
                                               torch.from_numpy(nbytes).cuda(), 968 * 1297)
    direct = engine.png_unfilter8_device(raw, 968, 1296, status)
    assert status.cpu().tolist() == [0]                      # decoded by the device, not by the reader's host fallback
    assert np.array_equal(direct[0].cpu().numpy(), labels)
    got = ingest.read_label_frames_device([path, path])
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 968, 1296)
    assert np.array_equal(got[0].cpu().numpy(), labels) and np.array_equal(got[1].cpu().numpy(), labels)
