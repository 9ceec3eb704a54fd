"""Host-side JPEG header parser (mspa_jpeg_parse_host): the descriptor fields against what Pillow wrote, and the refusal
of everything outside baseline sequential 8-bit Huffman greyscale / YCbCr 4:4:4, 4:2:2, 4:2:0 -- without a crash."""
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from jpeg_util import content, encode, marker_offset, sos_end  # noqa: E402

from mspa import engine  # noqa: E402


def _parse(*payloads):
    desc, status = engine.jpeg_parse_host(list(payloads))
    return engine.jpeg_desc_fields(desc), status


@pytest.mark.parametrize("sub,samp", [(0, (1, 1)), (1, (2, 1)), (2, (2, 2))])
def test_sampling_quant_tables_and_segment(sub, samp):
    from PIL import Image
    data = encode(content(37, 53, 1), quality=80, subsampling=sub)
    f, st = _parse(data)
    assert st[0] == 0 and f["status"][0] == 0
    assert (f["h"][0], f["w"][0], f["ncomp"][0]) == (37, 53, 3)
    assert (f["samp_h"][0, 0], f["samp_v"][0, 0]) == samp
    assert list(f["samp_h"][0, 1:]) == [1, 1] and list(f["samp_v"][0, 1:]) == [1, 1]
    assert f["restart_interval"][0] == 0
    with Image.open(io.BytesIO(data)) as im:
        q = im.quantization
    for c in range(3):
        assert list(f["qt"][0, c]) == list(q[int(f["tq"][0, c])])
    assert f["scan_offset"][0] == sos_end(data)
    assert f["scan_offset"][0] + f["scan_bytes"][0] == len(data) and data[-2:] == b"\xff\xd9"


def test_restart_interval():
    img = content(40, 72, 2)
    f, st = _parse(encode(img, quality=75, subsampling=2, restart_marker_blocks=3),
                   encode(img, quality=75, subsampling=2, restart_marker_rows=1),
                   encode(img, quality=75, subsampling=0, restart_marker_rows=2))
    assert list(st) == [0, 0, 0]
    assert list(f["restart_interval"]) == [3, (72 + 15) // 16, 2 * ((72 + 7) // 8)]


def test_greyscale_optimized_progressive_cmyk():
    from PIL import Image
    img = content(24, 40, 3)
    grey = encode(img[..., 1], quality=90)
    opt = encode(img, quality=90, optimize=True)
    prog = encode(img, quality=90, progressive=True)
    bio = io.BytesIO()
    Image.fromarray(img).convert("CMYK").save(bio, "JPEG", quality=90)
    f, st = _parse(grey, opt, prog, bio.getvalue())
    assert st[0] == 0 and f["ncomp"][0] == 1 and (f["h"][0], f["w"][0]) == (24, 40)
    assert st[1] == 0 and f["ncomp"][1] == 3
    assert st[2] != 0 and st[3] != 0


def _patched(data, at, value):
    b = bytearray(data)
    b[at] = value
    return bytes(b)


def test_declined_variants():
    data = encode(content(16, 24, 4), quality=75, subsampling=2)
    sof = marker_offset(data, 0xC0)
    variants = [_patched(data, sof + 1, 0xC2),          # progressive
                _patched(data, sof + 1, 0xC9),          # arithmetic
                _patched(data, sof + 4, 12)]            # 12-bit precision
    # a 4th component: the component count and the segment length patched, one more component record inserted
    b = bytearray(data)
    n = (b[sof + 2] << 8) | b[sof + 3]
    b[sof + 2:sof + 4] = (n + 3).to_bytes(2, "big")
    b[sof + 9] = 4
    b[sof + 2 + n:sof + 2 + n] = bytes([4, 0x11, 0])
    variants.append(bytes(b))
    f, st = _parse(*variants)
    assert all(s != 0 for s in st), st


def test_truncated_headers():
    data = encode(content(16, 24, 5), quality=75, subsampling=2, restart_marker_blocks=2)
    end = sos_end(data)
    cuts = [data[:n] for n in range(0, end + 2)]
    f, st = _parse(*cuts)
    assert all(s != 0 for s in st)
    f, st = _parse(data)
    assert st[0] == 0


def test_garbage_never_crashes():
    rng = np.random.default_rng(6)
    data = encode(content(16, 24, 6), quality=75)
    end = sos_end(data)
    cases = [b"", b"\xff", b"\xff\xd8", b"\xff\xd8\xff", bytes(rng.integers(0, 256, 300, dtype=np.uint8))]
    for _ in range(300):
        b = bytearray(data)
        for _ in range(3):
            b[int(rng.integers(2, end))] = int(rng.integers(0, 256))
        cases.append(bytes(b))
    _parse(*cases)
