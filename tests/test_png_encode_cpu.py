"""The 16-bit PNG encoder's definition (csrc/png_encode_core.h) on the CPU, from a g++ build of the header: on a size / content
grid, the filtered stream equals zlib.decompress of Pillow's IDAT, the file decodes (Pillow) to the input, it is structurally
strict (chunk CRCs, IHDR, zlib header, Adler-32, back-references within 32 KiB, nothing after IEND) and within the capacity;
and the files are within the size gates against Pillow's."""
import io
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from png_encode_util import KINDS, SIZES, build_driver, chunks, content, encode_core, pillow_png, strict_idat  # noqa: E402


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(str(tmp_path_factory.mktemp("png_core")))


@pytest.fixture(scope="module")
def grid(driver):
    cases = [(k, hw) for hw in SIZES for k in KINDS]
    imgs = [content(k, *hw) for k, hw in cases]
    return cases, imgs, encode_core(driver, imgs)


def _capacity(h, w):
    from mspa import engine
    return engine.png_encode_capacity((h, w))


@pytest.mark.parametrize("i", range(len(SIZES) * len(KINDS)))
def test_grid_case(grid, i):
    from PIL import Image
    cases, imgs, res = grid
    (kind, (h, w)), img, (f, filt) = cases[i], imgs[i], res[i]
    pil = pillow_png(img)
    pil_raw = zlib.decompress(b"".join(b for t, b in chunks(pil) if t == b"IDAT"))
    assert filt == pil_raw, f"{kind} {h}x{w}: filtered stream differs from Pillow's"
    assert strict_idat(f, h, w) == filt
    back = np.array(Image.open(io.BytesIO(f)))
    assert back.dtype == np.uint16 or back.dtype == np.int32
    assert np.array_equal(back.astype(np.int64), img.astype(np.int64))
    assert len(f) <= _capacity(h, w)


def test_capacity_refusals():
    from mspa import _lib
    lib = _lib.load()
    assert lib.mspa_png_encode_capacity(0, 1) == -1 and lib.mspa_png_encode_capacity(1, 8193) == -1
    assert lib.mspa_png_encode_capacity(8192, 8192) > 8192 * 16385
    assert lib.mspa_png_encode_workspace_bytes(1, 480, 640) >= 7 * 480 * 1281


def test_worst_case_is_near_capacity(driver):
    """Incompressible frames come out as stored blocks: within 0.1 % of the stated bound."""
    img = content("noise", 968, 1296, seed=11)
    f, _ = encode_core(driver, [img])[0]
    cap = _capacity(968, 1296)
    assert len(f) <= cap and len(f) > 0.995 * cap


def test_size_gates(grid):
    cases, imgs, res = grid
    mine = {}
    pil = {}
    for (kind, hw), img, (f, _) in zip(cases, imgs, res):
        if hw in ((480, 640), (968, 1296)):
            mine[kind] = mine.get(kind, 0) + len(f)
            pil[kind] = pil.get(kind, 0) + len(pillow_png(img))
    smooth_planar = (mine["smooth"] + mine["planar"]) / (pil["smooth"] + pil["planar"])
    assert smooth_planar <= 1.12, f"smooth + planar: {smooth_planar:.4f} x Pillow"
    assert mine["noise"] <= 1.005 * pil["noise"] + 1024, f"noise: {mine['noise']} vs Pillow {pil['noise']}"
