"""The 8-bit greyscale PNG path on the CPU: mspa_png_unfilter8_host (the rule of csrc/png_unfilter8_core.h, the one the device
kernel compiles) against Pillow's decode and against PNG 9.2 written out byte by byte (tests/png8_raw.py); the packer
mspa_png_pack_idat8_host on files; and the 16-bit packer, which moved behind a shared function, still returning what it returned."""
import ctypes
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from png8_raw import (CONTENTS, FILTER_KINDS, HEIGHTS, WIDE, WIDTHS, blocky_labels, matrix_images, pillow_unfilter8,  # noqa: E402
                      png8_from_scanlines, row_filters, scanlines8, unfilter8_reference)
import png_raw  # noqa: E402


def _unfilter8_host(raws, h, w, pitch=None, status=None):
    from mspa import _lib
    n, block = len(raws), h * (w + 1)
    pitch = pitch or block
    buf = np.full(n * pitch + 8, 0xA5, np.uint8)
    for k, r in enumerate(raws):
        buf[k * pitch:k * pitch + block] = np.frombuffer(r, np.uint8)
    out = np.full((n, h, w), 0x5A, np.uint8)
    st = np.zeros(n, np.int32) if status is None else np.asarray(status, np.int32).copy()
    _lib.check(_lib.load().mspa_png_unfilter8_host(buf.ctypes.data, pitch, n, h, w, out.ctypes.data, st.ctypes.data))
    return out, st


@pytest.mark.parametrize("w", WIDTHS + (WIDE[1],))
def test_host_unfilter_equals_pillow_and_the_definition(w):
    """Every width with every height, filter pattern and content, against Pillow and against the byte-by-byte restatement."""
    rng = np.random.default_rng(800 + w)
    for h in (HEIGHTS if w != WIDE[1] else (WIDE[0],)):
        images = matrix_images(h, w, rng)
        assert len(images) == len(FILTER_KINDS) * len(CONTENTS)
        got, st = _unfilter8_host([r for _, _, r, _ in images], h, w)
        assert st.tolist() == [0] * len(images)
        for k, (kind, content, raw, want) in enumerate(images):
            assert np.array_equal(got[k], want), (h, kind, content, np.argwhere(got[k] != want)[:5])
            assert np.array_equal(unfilter8_reference(raw, h, w), want), (h, kind, content)


def test_bad_filter_byte_and_entry_status():
    """A filter byte of 5 (or 255) gives status 3 and leaves the image's output alone; a non-zero status on entry is kept and
    the image skipped; the neighbours are exact.  A pitch wider than the block is honoured."""
    h, w = 65, 37
    rng = np.random.default_rng(5)
    raws, wants = [], []
    for kind in ("paeth", "random", "sub", "average_first", "up_first"):
        raw = scanlines8(row_filters(kind, h, rng), w, "random", rng)
        raws.append(bytearray(raw))
        wants.append(pillow_unfilter8(raw, h, w))
    raws[1][0] = 5
    raws[3][(h - 1) * (w + 1)] = 255
    got, st = _unfilter8_host([bytes(r) for r in raws], h, w, pitch=h * (w + 1) + 12, status=[0, 0, 7, 0, 0])
    assert st.tolist() == [0, 3, 7, 3, 0]
    for k in (0, 4):
        assert np.array_equal(got[k], wants[k])
    for k in (1, 2, 3):
        assert (got[k] == 0x5A).all()


def _pack8(paths, h, w, threads=3):
    from mspa import ingest
    return ingest.pack_mask_pngs(paths, h, w, threads)


def test_pack_idat8_on_files(tmp_path):
    """One Pillow-written L file round-trips (the packed bytes inflate to the file's scanlines, which un-filter to the image); a
    16-bit file gets status 2, a truncated one 3, a missing one 1; the size-only first call agrees with the second."""
    from PIL import Image
    from mspa import _lib
    h, w = 121, 162
    rng = np.random.default_rng(11)
    labels = blocky_labels(h, w, rng, block=16)
    good = str(tmp_path / "good.png")
    Image.fromarray(labels, mode="L").save(good)
    deep = str(tmp_path / "deep.png")
    Image.fromarray(labels.astype(np.uint16)).save(deep)
    assert Image.open(deep).mode.startswith("I;16")
    cut = str(tmp_path / "cut.png")
    data = open(good, "rb").read()
    open(cut, "wb").write(data[:len(data) // 2])
    paths = [good, deep, cut, str(tmp_path / "missing.png"), good]
    buf, offsets, nbytes, status, cap = _pack8(paths, h, w)
    assert status.tolist() == [0, 2, 3, 1, 0]
    assert (offsets % 16 == 0).all() and cap <= buf.nbytes
    scan = png_raw.scanlines_of(data)
    for k in (0, 4):
        packed = bytes(buf[offsets[k]:offsets[k] + nbytes[k]])
        assert zlib.decompress(packed) == scan
    got, st = _unfilter8_host([scan], h, w)
    assert st[0] == 0 and np.array_equal(got[0], labels)
    # the size-only call: same capacity and offsets
    lib = _lib.load()
    enc = [p.encode() for p in paths]
    arr = (ctypes.c_char_p * len(enc))(*enc)
    off2, nb2, st2 = np.zeros(5, np.int64), np.zeros(5, np.int64), np.zeros(5, np.int32)
    need = ctypes.c_int64(0)
    _lib.check(lib.mspa_png_pack_idat8_host(arr, 5, h, w, None, 0, off2.ctypes.data, nb2.ctypes.data, st2.ctypes.data, ctypes.byref(need), 1))
    assert need.value == cap and np.array_equal(off2, offsets)
    # another size than asked for: status 2
    assert _pack8([good], h, w + 1)[3].tolist() == [2]


def test_pack_idat16_still_returns_what_it_returned(tmp_path):
    """The 16-bit packer on one file: the packed bytes are the file's IDAT payload (they inflate to png_raw.scanlines_of), and it
    declines an 8-bit file with status 2."""
    from mspa import ingest
    h, w = 33, 47
    rng = np.random.default_rng(16)
    raw = png_raw.scanlines(png_raw.row_filters("random", h, rng), w, "random", rng)
    png = png_raw.png_from_scanlines(raw, h, w, level=6)
    p16, p8 = str(tmp_path / "d.png"), str(tmp_path / "m.png")
    open(p16, "wb").write(png)
    open(p8, "wb").write(png8_from_scanlines(scanlines8(row_filters("random", h, rng), w, "random", rng), h, w))
    buf, offsets, nbytes, status, _cap = ingest.pack_depth_pngs([p16, p8], h, w, 2)
    assert status.tolist() == [0, 2]
    packed = bytes(buf[offsets[0]:offsets[0] + nbytes[0]])
    assert packed == zlib.compress(raw, 6) and zlib.decompress(packed) == png_raw.scanlines_of(png) == raw
