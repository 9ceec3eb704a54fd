"""PNG scanlines as test data for mspa_png_unfilter_device: any byte string of h rows (one filter byte + 2 w sample bytes each)
is the body of a valid 16-bit greyscale PNG once its filter bytes are 0..4, so a test can draw the FILTERED bytes at random, set
each row's filter, and take Pillow's decode of the wrapped file as the reference -- Pillow un-filters with code of its own.

Also here: which of the device un-filter's three code paths an image takes (the dispatch of png_unfilter_kernel /
png_unfilter_hard_kernel in csrc/device_ingest.hip), and the widths the GPU tests run, so that a CPU test can check that the case
lists reach every path and every remainder of the pair pipeline's unrolled loop."""
import io
import struct
import zlib

import numpy as np

ROWS, PAIRS, BYTES = "rows", "pairs", "bytes"


def png_from_scanlines(raw: bytes, h: int, w: int, level: int = 0) -> bytes:
    """A 16-bit greyscale, non-interlaced h x w PNG whose IDAT is ``zlib.compress(raw)``."""
    assert len(raw) == h * (2 * w + 1)

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, 0, 0, 0, 0))
            + chunk(b"IDAT", zlib.compress(bytes(raw), level)) + chunk(b"IEND", b""))


def pillow_unfilter(raw: bytes, h: int, w: int) -> np.ndarray:
    """[h, w] uint16: Pillow's decode of the scanlines ``raw``."""
    from PIL import Image
    im = Image.open(io.BytesIO(png_from_scanlines(raw, h, w)))
    assert im.mode == "I;16" and im.size == (w, h)
    a = np.array(im)
    assert a.dtype == np.uint16 and a.shape == (h, w)
    return a


def scanlines_of(png: bytes) -> bytes:
    """The inflated IDAT payload (the filtered scanlines) of a PNG file's bytes."""
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat = 8, []
    while pos < len(png):
        n, kind = struct.unpack(">I4s", png[pos:pos + 8])
        if kind == b"IDAT":
            idat.append(png[pos + 8:pos + 8 + n])
        pos += 12 + n
    return zlib.decompress(b"".join(idat))


def unfilter_reference(raw: bytes, h: int, w: int) -> np.ndarray:
    """PNG 9.2 written out byte by byte (bytes per pixel = 2): a third opinion for the CPU test of the Pillow reference."""
    stride = 2 * w + 1
    prior = [0] * (2 * w)
    out = np.zeros((h, 2 * w), np.uint8)
    for y in range(h):
        ft, row = raw[y * stride], raw[y * stride + 1:(y + 1) * stride]
        cur = [0] * (2 * w)
        for i in range(2 * w):
            a = cur[i - 2] if i >= 2 else 0
            b = prior[i]
            c = prior[i - 2] if i >= 2 else 0
            if ft == 0:
                p = 0
            elif ft == 1:
                p = a
            elif ft == 2:
                p = b
            elif ft == 3:
                p = (a + b) >> 1
            else:
                pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                p = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            cur[i] = (row[i] + p) & 0xFF
        out[y] = cur
        prior = cur
    return out.view(">u2").astype(np.uint16)


def unfilter_path(w: int, filters, out_aligned: bool = True) -> str:
    """The code path png_unfilter_kernel / png_unfilter_hard_kernel choose for one image of width w whose rows carry
    ``filters`` (all 0..4), when raw and raw_pitch are 4-byte aligned (what the C ABI accepts)."""
    nd = (w + 127) // 128
    easy = all(int(f) <= 2 for f in filters)
    if easy and w % 2 == 0 and nd <= 8 and out_aligned:
        return ROWS
    if w % 2 == 0 and 4 <= w <= 4096 and out_aligned:
        return PAIRS
    return BYTES


def pair_remainder(w: int) -> int:
    """Steps of the pair pipeline's unrolled-by-8 loop that its remainder switch runs, for an even width."""
    return (w // 2 + 63) % 8


# Widths of the un-filter matrix (tests/test_gpu_png_unfilter.py): the rows path's edges (nd = 1 .. 9 dwords per lane), the pair
# pipeline's edges (4 .. 4 096 pixels) and past them; 8 / 10 / 12 and 1 608 / 1 610 / 1 612 give the pair loop's remainders 3, 4
# and 5, which no other width here does.
WIDTHS = (1, 2, 3, 4, 5, 6, 8, 10, 12, 126, 128, 130, 254, 256, 1022, 1024, 1026, 1608, 1610, 1612, 2046, 4094, 4096, 4098, 5001)
HEIGHTS = (1, 2, 63, 64, 65, 130)
EASY_FILTER_KINDS = ("none", "sub", "up", "none_sub_up", "up_first")
HARD_FILTER_KINDS = ("average", "paeth", "paeth_but_one", "random", "average_first")
FILTER_KINDS = EASY_FILTER_KINDS + HARD_FILTER_KINDS


def row_filters(kind: str, h: int, rng) -> np.ndarray:
    """The filter byte of every row of an h-row image, by pattern name."""
    if kind == "none":
        return np.zeros(h, np.uint8)
    if kind == "sub":
        return np.ones(h, np.uint8)
    if kind == "up":
        return np.full(h, 2, np.uint8)
    if kind == "none_sub_up":
        return rng.integers(0, 3, h).astype(np.uint8)
    if kind == "up_first":                                   # Up on the first row: the row above is zeros
        f = rng.integers(0, 3, h).astype(np.uint8)
        f[0] = 2
        return f
    if kind == "average":
        return np.full(h, 3, np.uint8)
    if kind == "paeth":
        return np.full(h, 4, np.uint8)
    if kind == "paeth_but_one":                              # one Sub row inside a band: that band is not all-Paeth
        f = np.full(h, 4, np.uint8)
        f[min(h - 1, 37)] = 1
        return f
    if kind == "random":
        return rng.integers(0, 5, h).astype(np.uint8)
    if kind == "average_first":                              # Average on the first row, then Paeth / Average / Up
        f = rng.choice(np.array([2, 3, 4], np.uint8), h)
        f[0] = 3
        return f
    raise ValueError(kind)


LOW_ENTROPY = np.array([0x00, 0x01, 0x7F, 0x80, 0xFF], np.uint8)


def scanlines(filters: np.ndarray, w: int, content: str, rng) -> bytes:
    """h rows of filtered bytes, the row filters set to ``filters``.  ``content``: "random" (uniform bytes); "low" (bytes from
    LOW_ENTROPY: per-byte wrap in the SWAR adds and the Sub prefix scan); "flat" (an image of a few sample values built from
    LOW_ENTROPY, filtered as an encoder would: the decoded neighbours are mostly equal, so Paeth's three distances tie)."""
    h = len(filters)
    if content == "random":
        body = rng.integers(0, 256, (h, 2 * w), dtype=np.uint8)
    elif content == "low":
        body = rng.choice(LOW_ENTROPY, (h, 2 * w))
    elif content == "flat":
        from test_sweep_cpu import _png_gray16
        values = (LOW_ENTROPY.astype(np.uint16)[:, None] << 8 | LOW_ENTROPY[None, :]).ravel()
        a = np.repeat(rng.choice(values, (h, (w + 3) // 4)), 4, axis=1)[:, :w]
        return scanlines_of(_png_gray16(a, [int(f) for f in filters], 1))
    else:
        raise ValueError(content)
    return np.concatenate([np.asarray(filters, np.uint8)[:, None], body], axis=1).tobytes()
