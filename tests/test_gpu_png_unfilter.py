"""mspa_png_unfilter_device called directly, every pixel against Pillow's decode of the same scanlines (tests/png_raw.py): the
three code paths (rows: None / Sub / Up images of even width <= 1 024 with lanes along the row; pairs: the skewed pixel-pair
pipeline for Average / Paeth images of even width 4 .. 4 096; bytes: everything else) at their width and band edges, every filter
pattern, random and low-entropy bytes; the layouts the C ABI accepts (any 4-byte aligned pitch and start) and the ones it refuses;
per-image status in mixed batches."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from png_raw import (BYTES, FILTER_KINDS, HEIGHTS, PAIRS, ROWS, WIDTHS, pillow_unfilter, row_filters,  # noqa: E402
                     scanlines, unfilter_path)

PAD = 0xA5                       # the bytes between images and around them: a load from the wrong place shows


def _round(x, m):
    return (x + m - 1) // m * m


def _device_raw(raws, pitch, offset=0):
    """[n, pitch] uint8 device view whose image k starts ``offset + k * pitch`` bytes into a larger allocation."""
    import torch
    n = len(raws)
    buf = np.full(offset + n * pitch + 64, PAD, np.uint8)
    for k, r in enumerate(raws):
        buf[offset + k * pitch:offset + k * pitch + len(r)] = np.frombuffer(r, np.uint8)
    dev = torch.from_numpy(buf).cuda()
    view = dev[offset:offset + n * pitch].view(n, pitch)
    assert view.is_contiguous() and view.data_ptr() - dev.data_ptr() == offset
    return view


def _images(h, w, rng, kinds=FILTER_KINDS, contents=("random", "low", "flat")):
    """(path, raw bytes, Pillow's decode) per image: every filter pattern with every content."""
    out = []
    for kind in kinds:
        for content in contents:
            f = row_filters(kind, h, rng)
            raw = scanlines(f, w, content, rng)
            out.append((unfilter_path(w, f), raw, pillow_unfilter(raw, h, w)))
    return out


def _run(images, h, w, pitch, offset=0, out=None):
    import torch
    from mspa import engine
    raw = _device_raw([r for _, r, _ in images], pitch, offset)
    status = torch.zeros(len(images), dtype=torch.int32, device="cuda")
    got = engine.png_unfilter_device(raw, h, w, status, out)
    torch.cuda.synchronize()
    return got.cpu().numpy().view(np.uint16), status.cpu().numpy()


def _path_id(w):
    paths = sorted({unfilter_path(w, [0, 1, 2]), unfilter_path(w, [4])})
    return "+".join(paths) + f"-w{w}"


@pytest.mark.parametrize("w", WIDTHS, ids=[_path_id(w) for w in WIDTHS])
def test_every_path_width_height_and_filter_pattern(w):
    """Per width: the paths its images take are in the test id (rows+pairs for even widths up to 1 024, rows+bytes at 2, pairs
    alone from 1 026 to 4 096 -- nd = 9 leaves the rows path -- bytes for odd widths and beyond 4 096); the widths include all
    eight remainders of the pair loop (tests/test_png_unfilter_cpu.py).  Heights around the 64-row band; one call per height
    holds every filter pattern with random, low-entropy-byte and flat-image contents, at the smallest pitch the ABI accepts."""
    rng = np.random.default_rng(1000 + w)
    heights = HEIGHTS if w <= 1026 else (1, 2, 64, 65, 130)
    seen = set()
    for h in heights:
        images = _images(h, w, rng)
        got, status = _run(images, h, w, _round(h * (2 * w + 1), 4))
        assert status.tolist() == [0] * len(images), (h, status)
        for k, (path, _, want) in enumerate(images):
            assert np.array_equal(got[k], want), (h, k, path, FILTER_KINDS[k // 3], np.argwhere(got[k] != want)[:5])
            seen.add(path)
    assert seen == set(_path_id(w).split("-")[0].split("+"))


@pytest.mark.parametrize("h,w", [(65, 130), (64, 2), (3, 5), (2, 4098), (63, 1026)],
                         ids=["rows+pairs", "rows+bytes", "bytes-odd", "bytes-wide", "pairs-only"])
def test_accepted_layouts_are_exact(h, w):
    """Every 4-byte aligned layout the ABI accepts: the pitch rounded up to 4 (the exact block size when that is a multiple of
    4), 4 more, rounded up to 256 (the in-tree callers'); images starting 0, 4 or 12 bytes into the allocation.  Then an ``out``
    view one int16 in (not 4-byte aligned): every image goes to the bytes path, still exact."""
    import torch
    rng = np.random.default_rng(h * 10 + w)
    images = _images(h, w, rng, kinds=("sub", "none_sub_up", "up_first", "paeth", "random", "average_first"), contents=("random", "low"))
    block = h * (2 * w + 1)
    want = np.stack([x for _, _, x in images])
    for pitch in sorted({_round(block, 4), _round(block, 4) + 4, _round(block, 256)}):
        for offset in (0, 4, 12):
            got, status = _run(images, h, w, pitch, offset)
            assert (status == 0).all() and np.array_equal(got, want), (pitch, offset)
    n = len(images)
    flat = torch.full((n * h * w + 1,), 0x5A5A, dtype=torch.int16, device="cuda")
    out = flat[1:].view(n, h, w)
    assert out.is_contiguous() and out.data_ptr() % 4 == 2
    assert unfilter_path(w, [0], out_aligned=False) == BYTES
    got, status = _run(images, h, w, _round(block, 4), 0, out=out)
    assert (status == 0).all() and np.array_equal(got, want)
    assert int(flat[0]) == 0x5A5A


@pytest.mark.parametrize("h,w", [(2, 2), (65, 130), (3, 5), (1, 1026)])
def test_unaligned_layouts_are_refused(h, w):
    """A pitch that is not a multiple of 4 (the exact block size among them when it is not) or a start 1, 2 or 3 bytes off:
    the fast paths load aligned dwords and clamp them to the image's last one, so such a layout would decode wrong pixels with
    status 0.  The engine raises, the C ABI returns MSPA_EINVAL and leaves ``out`` and ``status`` alone."""
    import torch
    from mspa import _lib, engine
    rng = np.random.default_rng(h + w)
    images = _images(h, w, rng, kinds=("none", "sub", "paeth"), contents=("random",))
    n, block = len(images), h * (2 * w + 1)
    layouts = [(p, 0) for p in sorted({block, _round(block, 4) + 1, _round(block, 4) + 2, _round(block, 4) + 3}) if p % 4]
    layouts += [(_round(block, 4), off) for off in (1, 2, 3)]
    assert any(p == block for p, _ in layouts) == (block % 4 != 0)
    lib = _lib.load()
    for pitch, offset in layouts:
        raw = _device_raw([r for _, r, _ in images], pitch, offset)
        status = torch.zeros(n, dtype=torch.int32, device="cuda")
        out = torch.full((n, h, w), 0x5A5A, dtype=torch.int16, device="cuda")
        with pytest.raises(_lib.MspaError):
            engine.png_unfilter_device(raw, h, w, status, out)
        rc = lib.mspa_png_unfilter_device(raw.data_ptr(), pitch, n, h, w, out.data_ptr(), status.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == _lib.MSPA_EINVAL, (pitch, offset)
        assert (out == 0x5A5A).all() and (status == 0).all(), (pitch, offset)


@pytest.mark.parametrize("h,w", [(130, 130), (65, 2)], ids=["rows+pairs", "rows+bytes"])
def test_status_in_mixed_batches(h, w):
    """One call holds images for the first launch's rows path and for the second launch (via status 0x40000000 between them):
    the pair pipeline at w = 130, the bytes path at w = 2.  (No single call can hold all three paths: rows and pairs need an even
    width and a 4-byte aligned ``out``, which every image of the call then has, and the bytes path takes such an image only when
    w = 2 or w > 4 096 -- and the rows path none with w > 1 024.)  Images whose status is non-zero on entry keep it and their
    output; images with filter byte 5 or 255 in the first row, the last row or a row of the second band get status 3; their
    neighbours are exact; no image is left pending."""
    import torch
    from mspa import engine
    rng = np.random.default_rng(h * w)
    specs = []                   # (kind, status on entry, (row, filter byte) to break or None)
    for k, kind in enumerate(FILTER_KINDS):
        specs.append((kind, 0, None))
        specs.append((kind, [1, 2, 4][k % 3], None))
        specs.append((kind, 0, [(0, 5), (h - 1, 255), (64, 5), (h - 1, 5), (64, 255)][k % 5]))
    specs.append(("paeth", 4, (0, 5)))                                   # skipped: its entry status wins over the bad filter
    raws, wants, paths = [], [], []
    for kind, _, bad in specs:
        f = row_filters(kind, h, rng)
        raw = bytearray(scanlines(f, w, "random", rng))
        wants.append(pillow_unfilter(bytes(raw), h, w))
        paths.append(unfilter_path(w, f))
        if bad is not None:
            raw[bad[0] * (2 * w + 1)] = bad[1]
        raws.append(bytes(raw))
    assert {ROWS, PAIRS if w > 2 else BYTES} <= set(p for p, (_, st, bad) in zip(paths, specs) if st == 0 and bad is None)
    n = len(specs)
    raw = _device_raw(raws, _round(h * (2 * w + 1), 256))
    status = torch.tensor([st for _, st, _ in specs], dtype=torch.int32, device="cuda")
    out = torch.full((n, h, w), 0x5A5A, dtype=torch.int16, device="cuda")
    engine.png_unfilter_device(raw, h, w, status, out)
    torch.cuda.synchronize()
    st, got = status.cpu().numpy(), out.cpu().numpy().view(np.uint16)
    assert not (st == 0x40000000).any()
    for k, (kind, entry, bad) in enumerate(specs):
        if entry:
            assert st[k] == entry and (got[k] == 0x5A5A).all(), (k, kind)
        elif bad is not None:
            assert st[k] == 3, (k, kind, bad)
        else:
            assert st[k] == 0 and np.array_equal(got[k], wants[k]), (k, kind, paths[k])
