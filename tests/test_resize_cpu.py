"""The resampler's arithmetic (csrc/resize_core.h) on the CPU, against Pillow's ``Image.resize`` value for value: a g++ build of
the header over the shape / content grid of resize_util, the tables of mspa_resize_coeffs_host against the header's, the
accumulator bound the header claims, argument errors, and ``resize_tree(backend="pillow")`` against the one-line definition."""
import io
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from jpeg_util import content  # noqa: E402
from resize_util import FILTERS, OUTSIDE, grid_pairs, patterns, pillow_resize  # noqa: E402

from mspa import engine  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-spatialmllm_amd", "csrc")

# Reads records (mode, h, w, H, W, filter) as int32 until the input ends.  Mode 0: h * w * 3 RGB bytes follow, the resized
# image is written.  Mode 1: the tables of the axis h -> H are written (ksize, bounds [H, 2], coeffs [H, ksize], int32).
# Mode 2: the largest sum |k| of a coefficient row over every in <= h and every out with 1/8 <= out / in <= 8, both filters,
# is written as int64 (-1: a table was refused).  Mode 3: mode 0 with the passes in the other order.
DRIVER = r"""
#include "resize_core.h"
#include <cstdio>
#include <vector>
using namespace mspa::resize;
int main() {
    int32_t a[6];
    while (fread(a, 4, 6, stdin) == 6) {
        const int h = a[1], w = a[2], H = a[3], W = a[4], f = a[5];
        if (a[0] == 1) {
            const Axis ax = axis(h, H, f);
            std::vector<int32_t> b(2 * (size_t)H), k((size_t)H * ax.ksize), kr(ax.ksize);
            std::vector<double> s(ax.ksize);
            if (coeffs(ax, b.data(), k.data(), s.data(), kr.data()) < 0) return 6;
            fwrite(&ax.ksize, 4, 1, stdout);
            fwrite(b.data(), 4, b.size(), stdout);
            fwrite(k.data(), 4, k.size(), stdout);
            continue;
        }
        if (a[0] == 2) {
            int64_t worst = 0;
            for (int filt = 2; filt <= 3 && worst >= 0; ++filt)
                for (int in = 1; in <= h && worst >= 0; ++in)
                    for (int out = (in + 7) / 8; out <= 8 * in; ++out) {
                        const Axis ax = axis(in, out, filt);
                        std::vector<int32_t> b(2 * (size_t)out), kr(ax.ksize);
                        std::vector<double> s(ax.ksize);
                        const int64_t m = coeffs(ax, b.data(), nullptr, s.data(), kr.data());
                        if (m < 0) { worst = -1; break; }
                        if (m > worst) worst = m;
                    }
            fwrite(&worst, 8, 1, stdout);
            continue;
        }
        std::vector<uint8_t> src((size_t)h * w * 3), dst((size_t)H * W * 3);
        if (fread(src.data(), 1, src.size(), stdin) != src.size()) return 4;
        if (!resize_host(src.data(), h, w, dst.data(), H, W, f, a[0] == 3)) return 5;
        fwrite(dst.data(), 1, dst.size(), stdout);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("resize_driver")
    (d / "driver.cpp").write_text(DRIVER)
    exe = str(d / "driver")
    build = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, str(d / "driver.cpp"),
                            "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


def _resize_cpu(exe, jobs, mode=0):
    """jobs: [(img [h, w, 3], (H, W), filter)] -> the resized images, one driver run."""
    inp = b"".join(struct.pack("<6i", mode, img.shape[0], img.shape[1], hw[0], hw[1], f) + np.ascontiguousarray(img).tobytes()
                   for img, hw, f in jobs)
    run = subprocess.run([exe], input=inp, capture_output=True, timeout=1200)
    assert run.returncode == 0, run.returncode
    out, o = [], 0
    for _, (H, W), _ in jobs:
        out.append(np.frombuffer(run.stdout[o:o + H * W * 3], np.uint8).reshape(H, W, 3))
        o += H * W * 3
    assert o == len(run.stdout)
    return out


def test_values_equal_pillow_on_the_grid(driver):
    jobs = []
    for i, ((h, w), hw) in enumerate(grid_pairs()):
        for img in patterns(h, w, i):
            for f in FILTERS.values():
                jobs.append((img, hw, f))
    assert len(jobs) > 18000
    differing = []
    for c in range(0, len(jobs), 4096):
        part = jobs[c:c + 4096]
        for (img, hw, f), got in zip(part, _resize_cpu(driver, part)):
            n = int((got != pillow_resize(img, hw, f)).sum())
            if n:
                differing.append((img.shape[:2], hw, f, n))
    assert not differing, differing[:20]


def test_outside_the_range_pillow_runs_the_other_order(driver):
    """Why the device path stops at 8 x: for 3 x 2000 -> 900 x 5 Pillow's values are those of the vertical pass run first."""
    (h, w), hw = OUTSIDE
    img = np.random.default_rng(5).integers(0, 256, (h, w, 3), dtype=np.uint8)
    for f in FILTERS.values():
        want = pillow_resize(img, hw, f)
        assert np.array_equal(_resize_cpu(driver, [(img, hw, f)], mode=3)[0], want)
        assert not np.array_equal(_resize_cpu(driver, [(img, hw, f)], mode=0)[0], want)


def test_coeffs_host_equals_the_header(driver):
    for n_in, n_out in [(512, 1296), (512, 968), (360, 968), (968, 484), (1296, 648), (64, 8), (8, 64), (17, 3), (1, 5), (2, 9),
                        (100, 13), (23, 184), (2000, 5), (3, 900), (7, 7)]:
        for name, f in FILTERS.items():
            run = subprocess.run([driver], input=struct.pack("<6i", 1, n_in, 0, n_out, 0, f), capture_output=True, timeout=120)
            assert run.returncode == 0
            raw = np.frombuffer(run.stdout, np.int32)
            ksize = int(raw[0])
            bounds, coeffs = engine.resize_coeffs_host(n_in, n_out, name)
            assert coeffs.shape == (n_out, ksize) and bounds.shape == (n_out, 2)
            assert np.array_equal(bounds.ravel(), raw[1:1 + 2 * n_out])
            assert np.array_equal(coeffs.ravel(), raw[1 + 2 * n_out:])
            assert bounds[:, 0].min() >= 0 and (bounds[:, 0] + bounds[:, 1]).max() <= n_in and bounds[:, 1].max() <= ksize
            assert abs(int(coeffs.sum(axis=1).min()) - (1 << 22)) <= ksize and abs(int(coeffs.sum(axis=1).max()) - (1 << 22)) <= ksize


def test_accumulator_bound(driver):
    """255 * sum|k| + 2^21 stays inside int32 for every row of every table of the device range (walked up to in = 96; the
    header's comment quotes the result)."""
    run = subprocess.run([driver], input=struct.pack("<6i", 2, 96, 0, 0, 0, 0), capture_output=True, timeout=1200)
    assert run.returncode == 0
    worst = int(np.frombuffer(run.stdout, np.int64)[0])
    print("largest sum|k| / 2^22:", worst / (1 << 22))
    assert 0 < worst and 255 * worst + (1 << 21) <= 2 ** 31 - 1


def test_coeffs_argument_errors():
    import ctypes
    lib = engine._lib.load()
    ksize = ctypes.c_int32(0)
    for n_in, n_out, f in [(0, 5, 3), (5, 0, 3), (65536, 5, 3), (5, 65536, 2), (5, 5, 0), (5, 5, 1), (5, 5, 4)]:
        assert lib.mspa_resize_coeffs_host(n_in, n_out, f, None, None, ctypes.byref(ksize)) == engine._lib.MSPA_EINVAL
    assert lib.mspa_resize_coeffs_host(5, 9, 3, None, None, None) == engine._lib.MSPA_EINVAL
    coeffs = np.zeros((9, 5), np.int32)
    assert lib.mspa_resize_coeffs_host(5, 9, 3, None, coeffs.ctypes.data, ctypes.byref(ksize)) == engine._lib.MSPA_EINVAL
    assert lib.mspa_resize_coeffs_host(5, 9, 3, None, None, ctypes.byref(ksize)) == 0 and ksize.value == 5
    assert lib.mspa_resize_coeffs_host(16, 2, 2, None, None, ctypes.byref(ksize)) == 0 and ksize.value == 17
    assert lib.mspa_resize_workspace_bytes(4, 10, 10, 20, 20) == 4 * 10 * 64
    assert lib.mspa_resize_workspace_bytes(4, 10, 10, 10, 20) == 0 and lib.mspa_resize_workspace_bytes(0, 10, 10, 20, 20) == 0
    assert lib.mspa_resize_workspace_bytes(-1, 10, 10, 20, 20) == -1 and lib.mspa_resize_workspace_bytes(1, 0, 10, 20, 20) == -1
    with pytest.raises(ValueError):
        engine.resize_coeffs_host(5, 9, "lanczos")


def _make_tree(root):
    """A small tree of mixed shapes and kinds; returns the relative paths."""
    from PIL import Image
    files = {"a/sq_0.jpg": (64, 64), "a/sq_1.jpg": (64, 64), "a/wide.jpeg": (36, 64), "b/c/tall.JPG": (50, 30),
             "b/same.jpg": (48, 60), "b/pic.png": (40, 40), "top.jpg": (33, 47)}
    for k, (rel, (h, w)) in enumerate(sorted(files.items())):
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        Image.fromarray(content(h, w, k)).save(path, quality=90)
    with open(os.path.join(root, "notes.txt"), "w") as f:
        f.write("not an image")
    return sorted(files)


def test_resize_tree_pillow_backend_is_the_definition(tmp_path):
    from PIL import Image
    from mspa import resize
    src, dst = str(tmp_path / "src"), str(tmp_path / "dst")
    files = _make_tree(src)
    assert resize.list_images(src) == files
    for name, f in FILTERS.items():
        out = os.path.join(dst, name)
        counts = resize.resize_tree(src, out, (48, 60), resample=name, backend="pillow", n_threads=4)
        assert counts["files"] == len(files) == counts["host_resized"] and counts["device_resized"] == 0 and counts["copied"] == 0
        assert resize.list_images(out) == files
        for rel in files:
            bio = io.BytesIO()
            with Image.open(os.path.join(src, rel)) as im:
                im.convert("RGB").resize((60, 48), f).save(bio, format="PNG" if rel.endswith(".png") else "JPEG", quality=95)
            with open(os.path.join(out, rel), "rb") as fh:
                assert fh.read() == bio.getvalue(), (name, rel)
            with Image.open(os.path.join(out, rel)) as im:
                assert im.size == (60, 48)
    counts = resize.resize_tree(src, os.path.join(dst, "skip"), (48, 60), backend="pillow", skip_same_shape=True, n_threads=2)
    assert counts["copied"] == 1 and counts["host_resized"] == len(files) - 1
    with open(os.path.join(src, "b/same.jpg"), "rb") as a, open(os.path.join(dst, "skip", "b/same.jpg"), "rb") as b:
        assert a.read() == b.read()


def test_resize_tree_command_line(tmp_path, capsys):
    import json
    from PIL import Image
    from mspa import resize
    src, dst = str(tmp_path / "src"), str(tmp_path / "dst")
    files = _make_tree(src)
    assert resize.main([src, dst, "--size", "30x20", "--resample", "bilinear", "--quality", "80", "--backend", "pillow"]) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["files"] == len(files)
    for rel in files:
        with Image.open(os.path.join(dst, rel)) as im:
            assert im.size == (30, 20)


def test_pillow_annotator_output_size(tmp_path):
    from PIL import Image
    from mspa.annotate import Mark, PillowAnnotator
    src = str(tmp_path / "s.jpg")
    Image.fromarray(content(60, 80, 3)).save(src, quality=92)
    marks = [Mark(20, 20, 6, (0, 0, 255), "A"), Mark(50, 30, 6, (0, 255, 0), "B")]
    PillowAnnotator().annotate(src, str(tmp_path / "plain.jpg"), marks)
    PillowAnnotator(output_size=(121, 162)).annotate(src, str(tmp_path / "sized.jpg"), marks)
    with Image.open(str(tmp_path / "plain.jpg")) as im:
        assert im.size == (80, 60)
    # the sized file is the painted canvas through the Pillow line; the painted canvas is not recoverable from plain.jpg
    # (JPEG is lossy), so the check here is the shape; test_gpu_resize.py compares the device annotator's files with these
    with Image.open(str(tmp_path / "sized.jpg")) as im:
        assert im.size == (162, 121) and im.mode == "RGB"
