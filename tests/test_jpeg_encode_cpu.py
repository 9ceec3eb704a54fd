"""The baseline JPEG encoder's arithmetic (csrc/jpeg_encode_core.h) on the CPU, against Pillow / libjpeg-turbo byte for byte:
the header of mspa_jpeg_encode_header_host, the reciprocal quantiser over every int16 value and divisor, whole files from a
g++ build of the header on a size / quality / content grid, and the worst-case capacity."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from jpeg_util import content, encode, sos_end  # noqa: E402

from mspa import engine  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-spatialmllm_amd", "csrc")
SUBSAMPLINGS = (0, 1, 2)

# Reads (mode, h, w, quality, subsampling) as int32 and, for mode 0, h * w * 3 RGB bytes from stdin; writes the file (mode 0)
# or the number of quantiser results that differ from rounding division over every int16 value and divisor q << 3 (mode 1).
DRIVER = r"""
#include "jpeg_encode_core.h"
#include <cstdio>
#include <vector>
using namespace mspa::jpege;
int main() {
    int32_t a[5];
    if (fread(a, 4, 5, stdin) != 5) return 2;
    if (a[0] == 1) {
        long bad = 0;
        for (int q = 1; q <= 255; ++q) {
            uint16_t recip, corr;
            uint8_t shift;
            const int d = q << 3;
            reciprocal(d, recip, corr, shift);
            for (int v = -32768; v <= 32767; ++v) {
                const int m = v < 0 ? -v : v;
                const int want = (v < 0 ? -1 : 1) * ((m + d / 2) / d);
                if (quantize(v, recip, corr, shift) != want) ++bad;
            }
        }
        printf("%ld\n", bad);
        return 0;
    }
    const int h = a[1], w = a[2];
    if (!valid_args(h, w, a[3], a[4])) return 3;
    std::vector<uint8_t> rgb((size_t)h * w * 3);
    if (fread(rgb.data(), 1, rgb.size(), stdin) != rgb.size()) return 4;
    std::vector<uint8_t> out(capacity(geometry(h, w, a[4])));
    const int64_t n = encode_file_host(rgb.data(), h, w, a[3], a[4], out.data(), (int64_t)out.size());
    if (n > (int64_t)out.size()) return 5;
    fwrite(out.data(), 1, n, stdout);
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("jpeg_encode_driver")
    (d / "driver.cpp").write_text(DRIVER)
    exe = str(d / "driver")
    build = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(d / "driver.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


def _encode_cpu(exe, img, quality, subsampling) -> bytes:
    h, w = img.shape[:2]
    run = subprocess.run([exe], input=struct.pack("<5i", 0, h, w, quality, subsampling) + np.ascontiguousarray(img).tobytes(),
                         capture_output=True, timeout=120)
    assert run.returncode == 0, run.returncode
    return run.stdout


def _patterns(h, w, seed):
    y, x = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(seed)
    checker = np.where(((x + y) % 2)[..., None] == 0, 255, 0).repeat(3, axis=2).astype(np.uint8)
    grad = np.stack([255 * x // max(w - 1, 1), 255 * y // max(h - 1, 1), (x + y) % 256], axis=-1).astype(np.uint8)
    return {"noise": rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "flat": np.full((h, w, 3), 200, np.uint8),
            "checker": checker, "gradient": grad}


def test_header_equals_pillow():
    for h, w in [(1, 1), (37, 21), (9, 1000), (968, 1296), (17, 33)]:
        img = np.zeros((h, w, 3), np.uint8)
        for ss in SUBSAMPLINGS:
            for q in range(1, 101):
                data = encode(img, quality=q, subsampling=ss)
                assert engine.jpeg_encode_header_host((h, w), q, ss) == data[:sos_end(data)], (h, w, q, ss)


def test_header_argument_errors():
    for args in [((0, 5), 95, 2), ((5, 65536), 95, 2), ((5, 5), 0, 2), ((5, 5), 101, 2)]:
        with pytest.raises(engine._lib.MspaError):
            engine.jpeg_encode_header_host(*args)
    with pytest.raises(ValueError):
        engine.jpeg_encode_header_host((5, 5), 95, "4:1:1")


def test_quantiser_is_rounding_division_exhaustively(driver):
    run = subprocess.run([driver], input=struct.pack("<5i", 1, 0, 0, 0, 0), capture_output=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip() == b"0", run.stdout


def test_files_equal_pillow_on_the_grid(driver):
    sizes = [(16 + a, 16 + b) for a in range(16) for b in (0, 5, 11)] + [(16 + a, 16 + b) for b in range(16) for a in (3, 14)]
    sizes += [(1, 1), (1, 37), (37, 1), (1, 16), (16, 1)]
    qualities = (1, 2, 10, 50, 75, 90, 95, 99, 100)
    n = 0
    for i, (h, w) in enumerate(sizes):
        for name, img in _patterns(h, w, i).items():
            # every size x pattern x subsampling, the quality cycling through the list; the full quality list on a few sizes
            qs = qualities if i % 13 == 0 else (qualities[(i + len(name)) % len(qualities)],)
            for q in qs:
                for ss in SUBSAMPLINGS:
                    assert _encode_cpu(driver, img, q, ss) == encode(img, quality=q, subsampling=ss), (h, w, name, q, ss)
                    n += 1
    assert n > 1000


def test_capacity_bounds_the_worst_file():
    for h, w in [(1, 1), (8, 8), (33, 47), (128, 96)]:
        noise = np.random.default_rng(h * w).integers(0, 256, (h, w, 3), dtype=np.uint8)
        for ss in SUBSAMPLINGS:
            assert engine.jpeg_encode_capacity((h, w), ss) >= len(encode(noise, quality=100, subsampling=ss))
    assert engine._lib.load().mspa_jpeg_encode_capacity(0, 5, 2) == -1
