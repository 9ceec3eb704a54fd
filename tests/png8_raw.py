"""PNG scanlines as test data for mspa_png_unfilter8_device / _host, the 8-bit twin of tests/png_raw.py: any byte string of h rows
(one filter byte + w sample bytes each) is the body of a valid 8-bit greyscale PNG once its filter bytes are 0..4, so a test draws
the FILTERED bytes at random, sets each row's filter (png_raw.row_filters), and takes Pillow's decode of the wrapped file (mode
``L``) as the reference.  ``unfilter8_reference`` restates PNG 9.2 with bytes-per-pixel 1 byte by byte as a third opinion."""
import io
import struct
import zlib

import numpy as np

from png_raw import FILTER_KINDS, LOW_ENTROPY, row_filters  # noqa: F401  (re-exported for the tests)

# the widths and heights of the un-filter matrix: around the dword (4), the wave (64) and two bands; 1100 crosses the 1 024-byte chunk
# in which the kernel stages the row above a band
WIDTHS = (1, 2, 3, 4, 5, 63, 64, 65, 127, 130)
HEIGHTS = (1, 2, 63, 64, 65, 130)
CONTENTS = ("random", "low")
WIDE = (66, 1100)                    # (h, w) of the extra case: two bands, the staged row above refilled once


def png8_from_scanlines(raw: bytes, h: int, w: int, level: int = 0) -> bytes:
    """An 8-bit greyscale, non-interlaced h x w PNG whose IDAT is ``zlib.compress(raw)``."""
    assert len(raw) == h * (w + 1)

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0))
            + chunk(b"IDAT", zlib.compress(bytes(raw), level)) + chunk(b"IEND", b""))


def pillow_unfilter8(raw: bytes, h: int, w: int) -> np.ndarray:
    """[h, w] uint8: Pillow's decode of the scanlines ``raw``."""
    from PIL import Image
    im = Image.open(io.BytesIO(png8_from_scanlines(raw, h, w)))
    assert im.mode == "L" and im.size == (w, h)
    a = np.array(im)
    assert a.dtype == np.uint8 and a.shape == (h, w)
    return a


def unfilter8_reference(raw: bytes, h: int, w: int) -> np.ndarray:
    """PNG 9.2 written out byte by byte with bytes per pixel = 1."""
    stride = w + 1
    prior = [0] * w
    out = np.zeros((h, w), np.uint8)
    for y in range(h):
        ft, row = raw[y * stride], raw[y * stride + 1:(y + 1) * stride]
        cur = [0] * w
        for i in range(w):
            a = cur[i - 1] if i >= 1 else 0
            b = prior[i]
            c = prior[i - 1] if i >= 1 else 0
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
    return out


def scanlines8(filters: np.ndarray, w: int, content: str, rng) -> bytes:
    """h rows of filtered bytes, the row filters set to ``filters``.  ``content``: "random" (uniform bytes) or "low" (bytes from
    png_raw.LOW_ENTROPY: wrap-around sums, Paeth ties)."""
    h = len(filters)
    if content == "random":
        body = rng.integers(0, 256, (h, w), dtype=np.uint8)
    elif content == "low":
        body = rng.choice(LOW_ENTROPY, (h, w))
    else:
        raise ValueError(content)
    return np.concatenate([np.asarray(filters, np.uint8)[:, None], body], axis=1).tobytes()


def matrix_images(h: int, w: int, rng, kinds=FILTER_KINDS, contents=CONTENTS):
    """(filter pattern, content, raw bytes, Pillow's decode) per image: every filter pattern with every content."""
    out = []
    for kind in kinds:
        for content in contents:
            raw = scanlines8(row_filters(kind, h, rng), w, content, rng)
            out.append((kind, content, raw, pillow_unfilter8(raw, h, w)))
    return out


def blocky_labels(h: int, w: int, rng, n_labels: int = 30, block: int = 48) -> np.ndarray:
    """[h, w] uint8 label map of rectangles, as an instance mask looks: long flat runs, label 0 between objects."""
    a = np.zeros((h, w), np.uint8)
    for _ in range(3 * n_labels):
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        a[y:y + int(rng.integers(block // 4, 3 * block)), x:x + int(rng.integers(block // 4, 3 * block))] = int(rng.integers(0, n_labels + 1))
    return a
