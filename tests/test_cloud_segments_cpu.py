"""The ragged-batch cleaning without a GPU (csrc/cloud_segments_core.h through the library's host twins): the search per segment
against the single-cloud host twin, bit for bit, and against scipy's cKDTree; the statistics against a Python restatement of the
header's stated sum order, bit for bit; the kept sets against the sequential-sum oracle behind a guard on the batch; the
regrouping by object on a hand-made InstanceClouds; the C entry points' argument errors; and the two headers once more as a
stand-alone g++ program under AddressSanitizer + UBSan."""
import functools
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_segments_util as U  # noqa: E402
import handler_ops_util as HU  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-spatialmllm_amd", "csrc")


@functools.lru_cache(maxsize=None)
def host_search(k):
    from mspa import cloud_segments as CS
    xyz, offsets, _names = U.batch()
    avg, evals = CS.knn_mean_distance_segments_host(xyz, offsets, k, want_evals=True)
    avg.setflags(write=False)
    return avg, evals


@functools.lru_cache(maxsize=None)
def host_stats(k, ratio):
    from mspa import cloud_segments as CS
    xyz, offsets, _names = U.batch()
    return CS.outlier_stats_segments_host(host_search(k)[0], offsets, ratio, xyz)


@pytest.mark.parametrize("k", U.KS)
def test_the_search_equals_the_single_cloud_twin_per_segment_bit_for_bit(k):
    from mspa import engine
    xyz, offsets, names = U.batch()
    avg, evals = host_search(k)
    for s, name in enumerate(names):
        a, b = offsets[s], offsets[s + 1]
        want, want_evals = engine.knn_mean_distance_host(xyz[a:b], k, want_evals=True)
        assert np.array_equal(U.bits(avg[a:b]), U.bits(want)) and np.array_equal(evals[a:b], want_evals), (name, k)


@pytest.mark.parametrize("k", U.KS)
def test_the_search_against_ckdtree(k):
    pytest.importorskip("scipy")
    xyz, offsets, names = U.batch()
    avg, _evals = host_search(k)
    for s, name in enumerate(names):
        a, b = offsets[s], offsets[s + 1]
        if b > a:
            want = HU.knn_mean_oracle(xyz[a:b], k)
            assert (np.abs(avg[a:b] - want) <= HU.knn_tolerance(k) * want).all(), (name, k)


@pytest.mark.parametrize("k", U.KS)
def test_mean_sd_and_threshold_follow_the_stated_sum_order_bit_for_bit(k):
    _xyz, offsets, names = U.batch()
    avg = host_search(k)[0]
    for ratio in U.RATIOS:
        got = host_stats(k, ratio)
        for s, name in enumerate(names):
            mean, sd, thr = U.stated_statistics(avg[offsets[s]:offsets[s + 1]], ratio)
            for key, want in (("mean", mean), ("sd", sd), ("thr", thr)):
                assert U.bits(got[key][s]) == U.bits(want), (name, k, ratio, key, got[key][s], want)


@pytest.mark.parametrize("k", U.KS)
def test_kept_sets_equal_the_sequential_oracle_behind_the_guard(k):
    xyz, offsets, names = U.batch()
    avg = host_search(k)[0]
    for ratio in U.RATIOS:
        got = host_stats(k, ratio)
        oracle_thr = np.array([HU.outlier_rule_oracle(avg[offsets[s]:offsets[s + 1]], ratio)[1] for s in range(len(names))])
        U.assert_guard(avg, offsets, (got["thr"], oracle_thr), (k, ratio))
        for s, name in enumerate(names):
            a, b = offsets[s], offsets[s + 1]
            want = HU.outlier_rule_oracle(avg[a:b], ratio)[0]
            assert np.array_equal(np.nonzero(got["keep"][a:b])[0], want), (name, k, ratio)
            assert got["kept"][s] == len(want)
            rows = xyz[a:b][want]
            if len(want):
                assert np.array_equal(got["lo"][s], rows.min(axis=0)) and np.array_equal(got["hi"][s], rows.max(axis=0)), name
            else:
                assert (got["lo"][s] == np.inf).all() and (got["hi"][s] == -np.inf).all(), name
    assert host_stats(k, 1.0)["kept"][names.index("identical-200")] == 0
    if k > 1:
        assert host_stats(k, 1.0)["kept"].sum() > 20000                   # the rule is not vacuous on this batch


def test_the_host_form_keeps_columns_dtype_and_order():
    from mspa import cloud_segments as CS
    xyz, offsets, _names = U.batch()
    rows = np.concatenate([xyz, np.arange(len(xyz), dtype=np.float64)[:, None]], axis=1).astype(np.float32)
    kept, kept_offsets, lo, _hi = CS.remove_statistical_outliers_segments_host(rows, offsets, 20, 1.0)
    assert kept.dtype == np.float32 and kept.shape[1] == 4 and kept_offsets[-1] == len(kept) and (np.diff(kept[:, 3]) > 0).all()
    assert lo.shape == (len(offsets) - 1, 3)
    for s in range(len(offsets) - 1):                                        # every kept row stays in its own segment
        tags = kept[kept_offsets[s]:kept_offsets[s + 1], 3]
        assert ((tags >= offsets[s]) & (tags < offsets[s + 1])).all()
    for nb, ratio in ((0, 1.0), (20, 0.0), (20, -2.0)):
        with pytest.raises(RuntimeError):
            CS.remove_statistical_outliers_segments_host(rows, offsets, nb, ratio)
    with pytest.raises(NotImplementedError, match="64"):
        CS.remove_statistical_outliers_segments_host(rows, offsets, 65)
    bad = rows.copy()
    bad[7, 1] = np.nan
    with pytest.raises(ValueError):
        CS.remove_statistical_outliers_segments_host(bad, offsets)


@pytest.mark.parametrize("name", ["S=1", "all-empty", "N=0"])
def test_one_segment_only_empty_segments_and_no_rows(name):
    from mspa import cloud_segments as CS, engine
    xyz, offsets = U.small_batches()[name]
    avg, evals = CS.knn_mean_distance_segments_host(xyz, offsets, 20, want_evals=True)
    assert avg.shape == (len(xyz),) and evals.shape == (len(xyz),)
    if len(xyz):
        want = engine.knn_mean_distance_host(xyz, 20, want_evals=True)
        assert np.array_equal(avg, want[0]) and np.array_equal(evals, want[1])
    st = CS.outlier_stats_segments_host(avg, offsets, 1.0, xyz)
    S = len(offsets) - 1
    assert st["kept"].shape == (S,) and st["lo"].shape == (S, 3) and st["keep"].shape == (len(xyz),)
    if not len(xyz):
        assert not st["kept"].any() and np.isnan(st["mean"]).all() and np.isnan(st["thr"]).all() and (st["lo"] == np.inf).all()
    kept, kept_offsets, _lo, _hi = CS.remove_statistical_outliers_segments_host(xyz, offsets)
    assert kept_offsets.shape == offsets.shape and kept_offsets[-1] == len(kept)


def test_by_object_regroups_the_rows_of_object_cloud():
    import torch
    from mspa.instances import InstanceClouds
    rng = np.random.default_rng(5)
    F, L = 3, 6
    counts = rng.integers(0, 5, size=(F, L))
    counts[:, 2] = 0                                                         # an object no image shows
    counts[1] = 0                                                            # an image that shows nothing
    counts[0, 0] = 3                                                         # label 0 is no object
    total = int(counts.sum())
    rows = torch.from_numpy(np.arange(total * 3, dtype=np.float64).reshape(total, 3))
    clouds = InstanceClouds([10, "11", 12], counts, rows, None, torch.zeros((F, L, 3), dtype=torch.float64), torch.zeros((F, L, 3), dtype=torch.float64))
    got, offsets, object_ids = clouds.by_object()
    want_ids = [v - 1 for v in range(1, L) if counts[:, v].any()]
    assert object_ids.tolist() == want_ids and offsets.dtype == np.int64 and offsets[0] == 0 and offsets[-1] == len(got)
    for j, t in enumerate(want_ids):
        assert torch.equal(got[offsets[j]:offsets[j + 1]], clouds.object_cloud(t)), t
    empty = InstanceClouds([1], np.zeros((1, L), dtype=np.int64), rows[:0], None, torch.zeros((1, L, 3)), torch.zeros((1, L, 3)))
    got, offsets, object_ids = empty.by_object()
    assert got.shape == (0, 3) and offsets.tolist() == [0] and len(object_ids) == 0


def test_the_c_entry_points_refuse_bad_arguments_before_anything_is_enqueued():
    """Every refusal below returns MSPA_EINVAL from the argument checks; none of the pointers is a device pointer, and none is
    ever dereferenced as one (the checks come before the first launch)."""
    from mspa import _lib
    lib = _lib.load()
    xyz = HU.cloud("uniform", 10)
    good = np.array([0, 4, 4, 10], dtype=np.int64)
    S = 3
    base = np.zeros(S + 1, dtype=np.int64)
    assert lib.mspa_knn_segments_tables_host(good.ctypes.data, S, 20, base.ctypes.data) == 0 and base[1] == base[2] < base[3]
    lo, hi = np.zeros((S, 3)), np.ones((S, 3))
    grids = np.zeros((S, _lib.KNN_GRID_BYTES), dtype=np.uint8)
    assert lib.mspa_knn_segments_grids_host(lo.ctypes.data, hi.ctypes.data, good.ctypes.data, S, 20, grids.ctypes.data) == 0
    assert not grids[1].any() and grids[0].any()
    work_bytes = lib.mspa_knn_segments_workspace_bytes(good.ctypes.data, S, 20)
    assert work_bytes > 0 and work_bytes % 16 == 0
    work = np.zeros(work_bytes + 16, dtype=np.uint8)
    aligned = (work.ctypes.data + 15) // 16 * 16
    mean, evals, keys, order = np.zeros(10), np.zeros(10, dtype=np.int32), np.zeros(10, dtype=np.int64), np.arange(10, dtype=np.int64)
    p = lambda a: a.ctypes.data                                              # noqa: E731
    descending = np.array([0, 5, 4, 10], dtype=np.int64)
    not_from_zero = np.array([1, 4, 4, 10], dtype=np.int64)
    too_long = np.array([0, (1 << 30) + 1], dtype=np.int64)
    no_grid = grids.copy()
    no_grid[0, :] = 0                                                        # a record grid_ok rejects for a non-empty segment
    infinite, not_a_number = hi * np.inf, xyz * np.nan

    def cells(off=good, n_seg=S, g=grids, xyz_p=p(xyz), keys_p=p(keys)):
        return lib.mspa_knn_segments_cells_device(xyz_p, p(off), n_seg, p(g), p(off), p(g), p(base), keys_p, None)

    def search(off=good, n_seg=S, k=20, g=grids, w=aligned, w_bytes=work_bytes, order_p=p(order)):
        return lib.mspa_knn_segments_mean_distance_device(p(xyz), p(off), n_seg, k, p(g), p(off), p(g), p(base), order_p, p(mean), p(evals),
                                                          w, w_bytes, None)

    keep, kept, st = np.zeros(10, dtype=np.uint8), np.zeros(S, dtype=np.int64), [np.zeros(S) for _ in range(3)]
    ext = [np.zeros((S, 3)) for _ in range(2)]

    def stats(off=good, n_seg=S, ratio=1.0, avg_p=p(mean)):
        return lib.mspa_outlier_segments_device(avg_p, p(xyz), p(off), n_seg, ratio, p(off), p(keep), p(kept), *(p(a) for a in st + ext), None)

    refused = {
        "cells: descending offsets": cells(off=descending), "cells: offsets[0] != 0": cells(off=not_from_zero),
        "cells: null xyz": cells(xyz_p=None), "cells: null keys": cells(keys_p=None), "cells: a grid grid_ok rejects": cells(g=no_grid),
        "cells: N > 2^30": cells(off=too_long, n_seg=1), "cells: negative S": cells(n_seg=-1),
        "search: descending offsets": search(off=descending), "search: k = 0": search(k=0), "search: k = 65": search(k=65),
        "search: N > 2^30": search(off=too_long, n_seg=1), "search: a grid grid_ok rejects": search(g=no_grid),
        "search: workspace too small": search(w_bytes=work_bytes - 16), "search: workspace misaligned": search(w=aligned + 8),
        "search: null workspace": search(w=None), "search: null order": search(order_p=None),
        "stats: descending offsets": stats(off=descending), "stats: null avg": stats(avg_p=None), "stats: NaN ratio": stats(ratio=float("nan")),
        "stats: N > 2^30": stats(off=too_long, n_seg=1),
        "tables: k = 65": lib.mspa_knn_segments_tables_host(p(good), S, 65, p(base.copy())),
        "tables: descending": lib.mspa_knn_segments_tables_host(p(descending), S, 20, p(base.copy())),
        "grids: lo > hi": lib.mspa_knn_segments_grids_host(p(hi), p(lo), p(good), S, 20, p(grids.copy())),
        "grids: infinite box": lib.mspa_knn_segments_grids_host(p(lo), p(infinite), p(good), S, 20, p(grids.copy())),
        "host search: NaN": lib.mspa_knn_segments_mean_distance_host(p(not_a_number), p(good), S, 20, p(mean), None),
        "host search: k = 0": lib.mspa_knn_segments_mean_distance_host(p(xyz), p(good), S, 0, p(mean), None),
        "host stats: descending": lib.mspa_outlier_segments_host(p(mean), p(xyz), p(descending), S, 1.0, p(keep), p(kept), *(p(a) for a in st + ext)),
    }
    assert {k: v for k, v in refused.items() if v != _lib.MSPA_EINVAL} == {}
    assert lib.mspa_knn_segments_workspace_bytes(p(descending), S, 20) == -1 and lib.mspa_knn_segments_workspace_bytes(p(good), S, 0) == -1
    assert b"offsets must be" in lib.mspa_last_error_string() or b"k outside" in lib.mspa_last_error_string()


# One record: int64 S, int64 k, float64 std_ratio, (S + 1) int64 offsets, N * 3 float64 -> N float64 avg, N int32 evals, N uint8 keep,
# S int64 kept, S float64 mean / sd / thr, S * 3 float64 lo / hi.  Every buffer is a heap block of exactly its size.
DRIVER = r"""
#include "cloud_segments_core.h"
#include <cstdio>
#include <cstdlib>
template <typename T> static T *block(int64_t n) { return (T *)malloc((size_t)(n > 0 ? n : 1) * sizeof(T)); }
int main() {
    int64_t head[2];
    double ratio;
    while (fread(head, 8, 2, stdin) == 2) {
        const int64_t S = head[0], k = head[1];
        if (fread(&ratio, 8, 1, stdin) != 1) return 3;
        int64_t *offsets = (int64_t *)malloc((size_t)(S + 1) * 8);
        if (fread(offsets, 8, (size_t)(S + 1), stdin) != (size_t)(S + 1)) return 4;
        const int64_t N = mspa::segs::batch_rows(offsets, S);
        if (N < 0) return 5;
        double *xyz = (double *)malloc((size_t)N * 24 + 1), *avg = block<double>(N);
        int32_t *evals = block<int32_t>(N);
        uint8_t *keep = block<uint8_t>(N);
        if (fread(xyz, 24, (size_t)N, stdin) != (size_t)N) return 6;
        if (!mspa::segs::mean_distance_segments_all(xyz, offsets, S, (int32_t)k, avg, evals)) return 7;
        int64_t *kept = block<int64_t>(S);
        double *mean = block<double>(S), *sd = block<double>(S), *thr = block<double>(S), *lo = block<double>(3 * S), *hi = block<double>(3 * S);
        mspa::segs::outlier_segments_all(avg, xyz, offsets, S, ratio, keep, kept, mean, sd, thr, lo, hi);
        fwrite(avg, 8, (size_t)N, stdout);
        fwrite(evals, 4, (size_t)N, stdout);
        fwrite(keep, 1, (size_t)N, stdout);
        fwrite(kept, 8, (size_t)S, stdout);
        fwrite(mean, 8, (size_t)S, stdout);
        fwrite(sd, 8, (size_t)S, stdout);
        fwrite(thr, 8, (size_t)S, stdout);
        fwrite(lo, 8, (size_t)(3 * S), stdout);
        fwrite(hi, 8, (size_t)(3 * S), stdout);
        void *all[] = {offsets, xyz, avg, evals, keep, kept, mean, sd, thr, lo, hi};
        for (void *b : all) free(b);
    }
    return 0;
}
"""


def test_the_two_headers_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    from mspa import cloud_segments as CS
    (tmp_path / "driver.cpp").write_text(DRIVER)
    exe = str(tmp_path / "driver")
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", CSRC, str(tmp_path / "driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    xyz, offsets, _names = U.batch()
    cut = int(np.searchsorted(offsets, 12000))                               # the batch without its longest segment: seconds under ASan
    records = [(xyz[:offsets[cut]], offsets[:cut + 1], 20, 1.0), (xyz[:offsets[cut]], offsets[:cut + 1], 64, 0.5)]
    records += [(x, o, 1, 1.0) for x, o in U.small_batches().values()]
    inp = b"".join(struct.pack("<qqd", len(o) - 1, k, r) + np.asarray(o, dtype="<i8").tobytes() + np.asarray(x, dtype="<f8").tobytes()
                   for x, o, k, r in records)
    run = subprocess.run([exe], input=inp, capture_output=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:].decode(errors="replace"))
    at = 0

    def take(dtype, count, shape=None):
        nonlocal at
        a = np.frombuffer(run.stdout, dtype=dtype, count=count, offset=at)
        at += a.nbytes
        return a if shape is None else a.reshape(shape)

    for x, o, k, r in records:
        N, S = len(x), len(o) - 1
        avg, evals = take("<f8", N), take("<i4", N)
        keep = take("u1", N)
        got = {"kept": take("<i8", S), "mean": take("<f8", S), "sd": take("<f8", S), "thr": take("<f8", S), "lo": take("<f8", 3 * S, (S, 3)),
               "hi": take("<f8", 3 * S, (S, 3))}
        want_avg, want_evals = CS.knn_mean_distance_segments_host(x, o, k, want_evals=True)
        assert np.array_equal(U.bits(avg), U.bits(want_avg)) and np.array_equal(evals, want_evals), (N, S, k)
        want = CS.outlier_stats_segments_host(want_avg, o, r, x)
        assert np.array_equal(keep.astype(bool), want["keep"]) and np.array_equal(got["kept"], want["kept"])
        for key in ("mean", "sd", "thr", "lo", "hi"):
            assert np.array_equal(U.bits(got[key]), U.bits(want[key])), (key, N, S, k)
    assert at == len(run.stdout)
