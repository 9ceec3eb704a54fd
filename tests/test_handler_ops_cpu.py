"""The handler's ops without a GPU: the module exposes upstream's nine functions; the six that are a few flops each against the
imported reference, bit for bit (skipped when the reference tree is absent); the grid search of csrc/knn_grid_core.h through
the library's host twin against scipy's cKDTree, and once more as a stand-alone g++ program under AddressSanitizer + UBSan."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import handler_ops_util as HU  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-spatialmllm_amd", "csrc")

NAMES = ["filter_images_laplacian", "calculate_image_sharpness", "convert_to_corners", "calculate_iou_2d", "calculate_iou_3d",
         "remove_statistical_outliers", "remove_truncated_outliers", "calculate_aabb", "project_mask_to_3d"]


def _ops():
    for name in [m for m in sys.modules if m == "spatial_engine" or m.startswith("spatial_engine.")]:
        if not (getattr(sys.modules[name], "__file__", None) or "").startswith(ROOT):
            del sys.modules[name]                   # the reference's modules of the same names, left by another test
    from spatial_engine.utils.scannet_utils.handler import ops
    assert ops.__file__.startswith(ROOT)
    return ops


def test_the_module_exposes_upstreams_nine_functions():
    ops = _ops()
    for name in NAMES:
        assert callable(getattr(ops, name)), name
    assert sorted(ops.__all__) == sorted(NAMES)


def test_argument_errors_need_no_device():
    ops = _ops()
    pts = HU.cloud("uniform", 30)
    for nb, ratio in ((0, 1.0), (20, 0.0), (20, -2.0)):
        with pytest.raises(RuntimeError):
            ops.remove_statistical_outliers(pts, nb, ratio)
    with pytest.raises(NotImplementedError, match="64"):
        ops.remove_statistical_outliers(pts, 65)
    assert ops.remove_statistical_outliers(np.zeros((0, 4), dtype=np.float32)).shape == (0, 4)
    with pytest.raises(AssertionError):
        ops.remove_truncated_outliers(pts, 0.5, 0.0, 0.0)


# ---- the six small functions against the reference --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def both():
    from oracle import ref_harness
    if not ref_harness.reference_available():
        pytest.skip("reference tree not present")
    ref = ref_harness.import_reference().OPS
    return ref, _ops()


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _clouds():
    rng = np.random.default_rng(21)
    yield rng.normal(size=(257, 3))
    yield rng.normal(size=(100, 6)).astype(np.float32)
    yield rng.integers(0, 4, size=(64, 4)).astype(np.float64)                  # ties on every axis
    yield np.zeros((10, 3))
    yield rng.normal(size=(1, 3))
    yield rng.normal(size=(3, 5))


def test_boxes_and_ious_are_bit_identical(both):
    ref, ops = both
    rng = np.random.default_rng(8)
    for pts in _clouds():
        box = ops.calculate_aabb(pts)
        assert _same(box, ref.calculate_aabb(pts))
        mine, theirs = ops.convert_to_corners([box, box * 3]), ref.convert_to_corners([box, box * 3])
        assert len(mine) == len(theirs) == 2 and all(_same(m, t) for m, t in zip(mine, theirs))
    boxes = [np.array([0, 0, 0, 1, 1, 1.0]), np.array([0.5, 0, 0, 1, 1, 1.0]), np.array([1, 0, 0, 1, 1, 1.0]), np.array([5, 5, 5, 1, 2, 3.0]),
             np.array([0.1, 0.2, -0.3, 2, 0.5, 0.7], dtype=np.float32)] + [rng.random(6) for _ in range(20)] + [rng.random(9)]
    assert _same(ops.convert_to_corners(boxes), ref.convert_to_corners(boxes))
    assert _same(ops.convert_to_corners([list(boxes[3])]), ref.convert_to_corners([list(boxes[3])]))
    for a in boxes[:-1]:
        for b in boxes[:-1]:
            assert _same(ops.calculate_iou_3d(a, b), ref.calculate_iou_3d(a, b))
    masks = [np.zeros((6, 7), dtype=bool), np.ones((6, 7), dtype=bool), rng.random((6, 7)) > 0.5, (rng.random((6, 7)) > 0.3).astype(np.uint8),
             rng.integers(0, 3, size=(6, 7))]
    for a in masks:
        for b in masks:
            got, want = ops.calculate_iou_2d(a, b), ref.calculate_iou_2d(a, b)
            assert type(got) is type(want) and _same(got, want)


def test_truncated_outliers_are_bit_identical(both):
    ref, ops = both
    ratios = [(0.1, 0.1, 0.1), (0.0, 0.0, 0.0), (0.2, 0.0, 0.0), (0.0, 0.3, 0.1), (0.49, 0.49, 0.49), (0.001, 0.2, 0.2), (0.05, 0.25, 0.4)]
    for pts in _clouds():
        for r in ratios:
            try:
                want = ref.remove_truncated_outliers(pts, *r)
            except Exception as e:                                              # upstream's own failure is part of its behaviour
                with pytest.raises(type(e)):
                    ops.remove_truncated_outliers(pts, *r)
                continue
            got = ops.remove_truncated_outliers(pts, *r)
            assert _same(got, want), (pts.shape, r)
            if r == (0.0, 0.0, 0.0):
                assert got is pts
    one = np.arange(12.0).reshape(4, 3)                                         # 2 nx >= n: int(0.49 * 4) = 1 is fine, a 2-row cloud is not
    for pts in (one, one[:2]):
        try:
            want = ref.remove_truncated_outliers(pts, 0.49, 0.49, 0.49)
        except Exception as e:
            with pytest.raises(type(e)):
                ops.remove_truncated_outliers(pts, 0.49, 0.49, 0.49)
        else:
            assert _same(ops.remove_truncated_outliers(pts, 0.49, 0.49, 0.49), want)


# ---- the grid search on the CPU --------------------------------------------------------------------------------------------
KNN_CASES = [("uniform", n, 20) for n in (1, 2, 19, 20, 21, 64, 65, 1000, 20000)] + [("uniform", 1000, 1), ("uniform", 1000, 64)] + \
    [("plane", 1000, 20), ("line", 1000, 20), ("clusters", 1000, 20), ("identical", 200, 20), ("far", 20000, 20)]


def _check_knn(xyz, k, mean, evals, kind):
    want = HU.knn_mean_oracle(xyz, k)
    assert (np.abs(mean - want) <= HU.knn_tolerance(k) * want).all(), (kind, len(xyz), k)
    if kind == "far":
        assert int(np.asarray(evals, dtype=np.int64).sum()) < len(xyz) ** 2 / 8


@pytest.mark.parametrize("kind,n,k", KNN_CASES, ids=[f"{c[0]}-{c[1]}-k{c[2]}" for c in KNN_CASES])
def test_host_twin_against_ckdtree(kind, n, k):
    pytest.importorskip("scipy")
    from mspa import engine
    xyz = HU.cloud(kind, n)
    mean, evals = engine.knn_mean_distance_host(xyz, k, want_evals=True)
    _check_knn(xyz, k, mean, evals, kind)


def test_host_twin_refuses_what_it_cannot_take():
    from mspa import _lib, engine
    pts = HU.cloud("uniform", 10)
    for k in (0, 65):
        with pytest.raises(ValueError):
            engine.knn_mean_distance_host(pts, k)
    bad = pts.copy()
    bad[3, 2] = np.inf
    with pytest.raises(_lib.MspaError):
        engine.knn_mean_distance_host(bad, 5)
    assert len(engine.knn_mean_distance_host(np.zeros((0, 3)), 5)) == 0


# Records until the input ends: int64 n, int64 k, n * 3 float64 -> n float64 means, n int32 evaluation counts.  Every buffer is a
# heap block of exactly its size: a read or a write outside it is the sanitizer's to report.
DRIVER = r"""
#include "knn_grid_core.h"
#include <cstdio>
#include <cstdlib>
int main() {
    int64_t head[2];
    while (fread(head, 8, 2, stdin) == 2) {
        const int64_t n = head[0], k = head[1];
        double *xyz = (double *)malloc((size_t)n * 24), *mean = (double *)malloc((size_t)n * 8);
        int32_t *evals = (int32_t *)malloc((size_t)n * 4);
        if (fread(xyz, 24, (size_t)n, stdin) != (size_t)n) return 4;
        if (!mspa::knn::mean_distance_all(xyz, n, (int32_t)k, mean, evals)) return 5;
        fwrite(mean, 8, (size_t)n, stdout);
        fwrite(evals, 4, (size_t)n, stdout);
        free(xyz);
        free(mean);
        free(evals);
    }
    return 0;
}
"""


def test_the_header_under_sanitizers(tmp_path):
    pytest.importorskip("scipy")
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    (tmp_path / "driver.cpp").write_text(DRIVER)
    exe = str(tmp_path / "driver")
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", CSRC, str(tmp_path / "driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    cases = [("uniform", 1, 20), ("uniform", 21, 20), ("uniform", 65, 64), ("uniform", 3000, 20), ("plane", 500, 20), ("line", 500, 1),
             ("clusters", 600, 20), ("identical", 200, 20), ("far", 3000, 20)]
    clouds = [HU.cloud(kind, n) for kind, n, _k in cases]
    inp = b"".join(struct.pack("<qq", len(x), k) + np.asarray(x, dtype="<f8").tobytes() for x, (_kind, _n, k) in zip(clouds, cases))
    run = subprocess.run([exe], input=inp, capture_output=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:].decode(errors="replace"))
    o = 0
    from mspa import engine
    for x, (kind, _n, k) in zip(clouds, cases):
        mean = np.frombuffer(run.stdout, dtype="<f8", count=len(x), offset=o)
        evals = np.frombuffer(run.stdout, dtype="<i4", count=len(x), offset=o + 8 * len(x))
        o += 12 * len(x)
        _check_knn(x, k, mean, evals, kind if len(x) > 10000 else "")
        lib_mean, lib_evals = engine.knn_mean_distance_host(x, k, want_evals=True)        # the library's build of the same header
        assert np.array_equal(lib_evals, evals) and (np.abs(lib_mean - mean) <= HU.knn_tolerance(k) * mean).all()
    assert o == len(run.stdout)
