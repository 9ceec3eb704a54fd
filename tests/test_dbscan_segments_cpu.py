"""DBSCAN of a ragged batch without a GPU (csrc/dbscan_core.h through the library's host twin, mspa_dbscan_segments_host): the twin
against ``sklearn.cluster.DBSCAN(eps, min_samples=min_points, algorithm="kd_tree")`` run per segment, labels value for value, on
the batch of tests/dbscan_segments_util.py and on a row permutation of it; the largest-cluster keep against ``np.bincount`` on
scikit-learn's labels; the edge batches; every argument error of the C entry points and of the Python functions; the frozen labels
of tests/golden against a fresh run; and the header once more as a stand-alone g++ program under AddressSanitizer + UBSan, which
also calls the union-find loop with a lowered cap.  scikit-learn is imported plainly: a machine without it fails these tests."""
import inspect
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dbscan_segments_util as D  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-spatialmllm_amd", "csrc")
CASES = [(eps, m) for eps in D.eps_values() for m in D.MIN_POINTS]


def _ops():
    for name in [m for m in sys.modules if m == "spatial_engine" or m.startswith("spatial_engine.")]:
        if not (getattr(sys.modules[name], "__file__", None) or "").startswith(ROOT):
            del sys.modules[name]                   # the reference's modules of the same names, left by another test
    from spatial_engine.utils.scannet_utils.handler import ops
    return ops


def _names_of(rows_at, offsets, names):
    return sorted({names[int(np.searchsorted(offsets, r, side="right")) - 1] for r in rows_at})


@pytest.mark.parametrize("shuffled", [False, True], ids=["input-order", "rows-permuted"])
@pytest.mark.parametrize("eps,min_points", CASES)
def test_the_host_twin_gives_scikit_learns_labels_value_for_value(eps, min_points, shuffled):
    _rows, offsets, names, _eps = D.batch()
    want, want_clusters = D.batch_sklearn(eps, min_points, shuffled)
    got, got_clusters = D.batch_twin(eps, min_points, shuffled)
    assert got.dtype == np.int32 and got_clusters.dtype == np.int64 and got.shape == want.shape
    differ = np.nonzero(got != want)[0]
    assert len(differ) == 0, (eps, min_points, len(differ), _names_of(differ[:20], offsets, names))
    assert np.array_equal(got_clusters, want_clusters)


def test_the_batch_is_what_its_docstring_says():
    rows, offsets, names, eps = D.batch()
    assert len(rows) == offsets[-1] < 25000 and len(names) == len(offsets) - 1 == len(eps)
    lengths = dict(zip(names, np.diff(offsets)))
    assert lengths["front-empty"] == lengths["middle-empty"] == lengths["end-empty"] == 0 and lengths["n=1"] == 1
    assert names[0] == "front-empty" and names[-1] == "end-empty" and lengths["chain-3000"] == 3000 and lengths["dup8"] == 2400
    seg = lambda n: rows[offsets[names.index(n)]:offsets[names.index(n) + 1]]      # noqa: E731
    # the chain: one cluster at its own eps while a point needs at most three near points, noise from four on; thousands of cells
    s = names.index("chain-3000")
    for m, clusters in ((1, 1), (4, 0)):
        labels, count = D.batch_sklearn(D.DEFAULT_EPS, m)
        assert count[s] == clusters and (labels[offsets[s]:offsets[s + 1]] == (0 if clusters else -1)).all()
    assert np.ptp(seg("chain-3000")[:, 0]) / D.DEFAULT_EPS > 1500
    # the lattices: many pairs whose squared distance, formed the rule's way, EQUALS eps * eps
    for name, e, take in (("lattice-eighths", 0.125, 300), ("lattice-tenths", 0.1, 300), ("lattice-3000", 0.125, 1500)):
        p = seg(name)[:take]
        d = p[:, None, :] - p[None, :, :]
        sq = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        assert (sq == e * e).sum() >= 100, name
    # dup8: every point eight times
    assert len(np.unique(seg("dup8"), axis=0)) == 300
    # the shared border point takes cluster 0 in both copies, and cluster 0 is the other group in the second
    labels, count = D.batch_sklearn(D.DEFAULT_EPS, 4)
    for name, border in (("shared-border", 6), ("shared-border-swapped", 6)):
        s = names.index(name)
        assert count[s] == 2 and labels[offsets[s]:offsets[s + 1]].tolist() == [0] * 7 + [1] * 6, name
    assert np.array_equal(seg("shared-border")[:6], seg("shared-border-swapped")[7:])
    s = names.index("noise-only")
    for e in (0.02, 0.05, 0.125):
        assert (D.batch_sklearn(e, 4)[0][offsets[s]:offsets[s + 1]] == -1).all()
    # the parameter grid reaches every regime somewhere: noise, border rows, several clusters in a segment, one cluster that is all
    labels, count = D.batch_sklearn(0.05, 4)
    assert (labels < 0).sum() > 1000 and count.max() > 10
    whole = D.batch_sklearn(100.0, 20)
    for name in ("bridge", "dup8", "uniform-4097", "far"):
        s = names.index(name)
        assert whole[1][s] == 1 and (whole[0][offsets[s]:offsets[s + 1]] == 0).all(), name


@pytest.mark.parametrize("eps,min_points", CASES)
def test_the_largest_cluster_is_bincounts_on_scikit_learns_labels_with_the_tie_rule(eps, min_points):
    from mspa import cloud_segments as CS
    rows, offsets, _names, _eps = D.batch()
    keep, kept = D.largest_keep(D.batch_sklearn(eps, min_points)[0], offsets)
    out, kept_offsets, lo, hi, index = CS.largest_cluster_segments_host(rows, offsets, eps, min_points)
    assert np.array_equal(index, np.nonzero(keep)[0]) and index.dtype == np.int64
    assert np.array_equal(np.diff(kept_offsets), kept) and kept_offsets.dtype == np.int64 and kept_offsets[0] == 0
    assert np.array_equal(out, rows[keep])
    for s in range(len(offsets) - 1):
        part = out[kept_offsets[s]:kept_offsets[s + 1]]
        if len(part):
            assert np.array_equal(lo[s], part.min(axis=0)) and np.array_equal(hi[s], part.max(axis=0))
        else:
            assert (lo[s] == np.inf).all() and (hi[s] == -np.inf).all()


def test_a_tie_between_clusters_goes_to_the_lowest_number():
    from mspa import cloud_segments as CS
    rows, offsets, names, _eps = D.batch()
    s = names.index("shared-border-swapped")
    part = np.delete(rows[offsets[s]:offsets[s + 1]], 6, axis=0)            # without the border point: two clusters of six
    labels, clusters = CS.dbscan_segments_host(part, [0, 12], 0.05, 4)
    assert clusters.tolist() == [2] and labels.tolist() == [0] * 6 + [1] * 6
    _out, kept_offsets, _lo, _hi, index = CS.largest_cluster_segments_host(part, [0, 12], 0.05, 4)
    assert index.tolist() == [0, 1, 2, 3, 4, 5] and kept_offsets.tolist() == [0, 6]


@pytest.mark.parametrize("name", ["S=1", "all-empty", "N=0", "n=1"])
def test_one_segment_only_empty_segments_no_rows_and_one_row(name):
    from mspa import cloud_segments as CS
    xyz, offsets = D.small_batches()[name]
    for eps, m in ((0.1, 1), (0.1, 4), (10.0, 2)):
        labels, clusters = CS.dbscan_segments_host(xyz, offsets, eps, m)
        want, want_clusters = D.sklearn_labels(xyz, offsets, eps, m)
        assert np.array_equal(labels, want) and np.array_equal(clusters, want_clusters) and clusters.shape == (len(offsets) - 1,)
        out, kept_offsets, lo, hi, index = CS.largest_cluster_segments_host(xyz, offsets, eps, m)
        keep, kept = D.largest_keep(want, offsets)
        assert np.array_equal(index, np.nonzero(keep)[0]) and np.array_equal(np.diff(kept_offsets), kept) and lo.shape == (len(offsets) - 1, 3)
    if name == "n=1":
        assert CS.dbscan_segments_host(xyz, offsets, 0.1, 1)[0].tolist() == [0] and CS.dbscan_segments_host(xyz, offsets, 0.1, 2)[0].tolist() == [-1]


def test_the_frozen_labels_are_scikit_learns():
    frozen = D.golden()
    assert sorted(frozen) == sorted(D.GOLDEN_PARAMETERS)
    for (eps, m), labels in frozen.items():
        assert labels.dtype == np.int32 and np.array_equal(labels, D.batch_sklearn(eps, m)[0]), (eps, m)
    assert os.path.getsize(D.GOLDEN) < 1 << 20


def test_the_python_functions_refuse_bad_arguments():
    from mspa import cloud_segments as CS
    ops = _ops()
    rows, offsets, _names, _eps = D.batch()
    bad_parameters = [(0, 4), (0.0, 4), (-1.0, 4), (float("nan"), 4), (float("inf"), 4), (None, 4), ("wide", 4), (1e-200, 4),
                      (0.05, 0), (0.05, -3), (0.05, None), (0.05, 2.5), (0.05, "many")]
    for eps, m in bad_parameters:
        for call in (lambda: CS.dbscan_segments_host(rows, offsets, eps, m), lambda: CS.largest_cluster_segments_host(rows, offsets, eps, m),
                     lambda: ops.cluster_dbscan(rows, eps, m)):
            with pytest.raises(RuntimeError, match="cluster_dbscan: eps must be positive"):
                call()
    for call in (CS.dbscan_segments_host, CS.largest_cluster_segments_host):
        with pytest.raises(ValueError, match="eps 1e-06 is too small"):
            call(rows, offsets, D.TOO_SMALL, 4)
        for value in (np.nan, np.inf, -np.inf):
            bad = rows.copy()
            bad[5000, 1] = value
            with pytest.raises(ValueError, match="non-finite"):
                call(bad, offsets, 0.05, 4)
        with pytest.raises(ValueError):
            call(rows, offsets[:-2], 0.05, 4)                                # offsets that do not end at N
        with pytest.raises(ValueError):
            call(rows, offsets[::-1], 0.05, 4)                               # descending
        with pytest.raises(ValueError):
            call(rows[:, :2], offsets, 0.05, 4)                              # C < 3
        with pytest.raises(ValueError):
            call(rows.reshape(-1), offsets, 0.05, 4)
    bad = rows.copy()
    bad[17, 0] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        ops.cluster_dbscan(bad, 0.05, 4)
    for call in (CS.dbscan_segments, CS.largest_cluster_segments):
        with pytest.raises((ValueError, RuntimeError)):
            call(rows, offsets, 0.05, 4)                                     # NumPy rows have no device: no quiet fallback


def test_the_c_entry_points_refuse_bad_arguments_before_anything_is_enqueued():
    """Every refusal below returns MSPA_EINVAL from the argument checks; none of the pointers is a device pointer, and none is ever
    dereferenced as one (the checks come before the first launch)."""
    from mspa import _lib
    lib = _lib.load()
    rows = np.random.default_rng(1).random((10, 4))
    good = np.array([0, 4, 4, 10], dtype=np.int64)
    S, C = 3, 4
    work_bytes = lib.mspa_dbscan_segments_workspace_bytes(good.ctypes.data, S)
    assert work_bytes > 0 and work_bytes % 16 == 0
    work = np.zeros(work_bytes + 16, dtype=np.uint8)
    aligned = (work.ctypes.data + 15) // 16 * 16
    keys, order = np.zeros(10, dtype=np.int64), np.arange(10, dtype=np.int64)
    labels, seg, keep = np.zeros(10, dtype=np.int32), np.zeros(2 * S + 1, dtype=np.int32), np.zeros(10, dtype=np.uint8)
    clusters, kept, flags = np.zeros(S, dtype=np.int32), np.zeros(S, dtype=np.int32), np.zeros(1, dtype=np.int32)
    lo, hi = np.zeros((S, 3)), np.zeros((S, 3))
    p = lambda a: a.ctypes.data                                              # noqa: E731
    descending = np.array([0, 5, 4, 10], dtype=np.int64)
    not_from_zero = np.array([1, 4, 4, 10], dtype=np.int64)
    too_long = np.array([0, (1 << 30) + 1], dtype=np.int64)
    many = (1 << 24) + 1

    def device_call(off=good, n_seg=S, c=C, eps=0.5, m=3, rows_p=p(rows), off_p=p(good), keys_p=p(keys), order_p=p(order), labels_p=p(labels),
                    keep_p=p(keep), seg_p=p(seg), w=aligned, w_bytes=work_bytes, base_p=p(good), lo_p=p(lo), hi_p=p(hi)):
        return lib.mspa_dbscan_segments_device(rows_p, c, p(off), n_seg, eps, m, off_p, keys_p, order_p, base_p, labels_p, keep_p, lo_p, hi_p, seg_p, w,
                                               w_bytes, None)

    def host_call(off=good, n_seg=S, c=C, eps=0.5, m=3, rows_p=p(rows), labels_p=p(labels), clusters_p=p(clusters), keep_p=p(keep),
                  kept_p=p(kept), flags_p=p(flags)):
        return lib.mspa_dbscan_segments_host(rows_p, c, p(off), n_seg, eps, m, labels_p, clusters_p, keep_p, kept_p, flags_p)

    refused = {}
    for name, call in (("device", device_call), ("host", host_call)):
        refused.update({
            f"{name}: descending offsets": call(off=descending), f"{name}: offsets[0] != 0": call(off=not_from_zero),
            f"{name}: N > 2^30": call(off=too_long, n_seg=1), f"{name}: negative S": call(n_seg=-1), f"{name}: S > 2^24": call(n_seg=many),
            f"{name}: C = 2": call(c=2), f"{name}: eps 0": call(eps=0.0), f"{name}: eps -1": call(eps=-1.0), f"{name}: eps NaN": call(eps=float("nan")),
            f"{name}: eps inf": call(eps=float("inf")), f"{name}: eps whose square is not normal": call(eps=1e-200),
            f"{name}: eps whose square is not finite": call(eps=1e200), f"{name}: min_points 0": call(m=0), f"{name}: min_points -1": call(m=-1),
            f"{name}: null rows": call(rows_p=None), f"{name}: null labels": call(labels_p=None)})
    refused.update({
        "device: null workspace": device_call(w=None), "device: workspace too small": device_call(w_bytes=work_bytes - 16),
        "device: workspace misaligned": device_call(w=aligned + 8), "device: null offsets_dev": device_call(off_p=None),
        "device: null keys": device_call(keys_p=None), "device: null order": device_call(order_p=None), "device: null seg": device_call(seg_p=None),
        "device: keys at 4 mod 8": device_call(keys_p=p(keys) + 4), "device: order at 4 mod 8": device_call(order_p=p(order) + 4),
        "device: rows at 4 mod 8": device_call(rows_p=p(rows) + 4), "device: labels at 2 mod 4": device_call(labels_p=p(labels) + 2),
        "device: seg at 2 mod 4": device_call(seg_p=p(seg) + 2), "device: keep without lo": device_call(lo_p=None),
        "device: keep without hi": device_call(hi_p=None), "device: keep without tile_base": device_call(base_p=None),
        "device: lo at 4 mod 8": device_call(lo_p=p(lo) + 4), "device: tile_base at 4 mod 8": device_call(base_p=p(good) + 4),
        "host: null clusters": host_call(clusters_p=None), "host: null flags": host_call(flags_p=None), "host: keep without kept": host_call(kept_p=None),
    })
    assert {k: v for k, v in refused.items() if v != _lib.MSPA_EINVAL} == {}
    assert lib.mspa_dbscan_segments_workspace_bytes(p(descending), S) == -1 and lib.mspa_dbscan_segments_workspace_bytes(p(too_long), 1) == -1
    assert b"mspa_dbscan_segments" in lib.mspa_last_error_string()
    for eps in (0.0, -1.0, float("nan"), float("inf"), 1e-200, 1e200):
        assert lib.mspa_dbscan_cell_side(eps) == -1.0
    assert lib.mspa_dbscan_cell_side(0.125) == 0.125 * (1.0 + 2.0 ** -20) > 0.125
    assert host_call() == 0 and flags[0] == 0                                # the good arguments are good
    assert host_call(keep_p=None, kept_p=None) == 0
    # the flag word: a NaN row and an eps that is too small, clamped and reported, not refused by the C layer
    nan_rows = rows.copy()
    nan_rows[7, 2] = np.nan
    assert host_call(rows_p=p(nan_rows)) == 0 and flags[0] & 1
    wide = rows.copy()
    wide[0, 0] = 1e6
    assert host_call(rows_p=p(wide), eps=1e-3) == 0 and flags[0] == 2


def test_ops_cluster_dbscan_on_numpy_input_is_the_one_segment_batch():
    import torch
    from mspa import cloud_segments as CS
    ops = _ops()
    fold = lambda text: " ".join(text.split())                               # noqa: E731
    assert "No reference counterpart" in fold(ops.cluster_dbscan.__doc__) and "scikit-learn's" in fold(ops.cluster_dbscan.__doc__)
    assert "cluster_dbscan" not in ops.__all__
    rows, offsets, names, _eps = D.batch()
    s = names.index("bridge")
    cloud = rows[offsets[s]:offsets[s + 1]]
    for eps, m in ((0.05, 4), (0.02, 10)):
        got = ops.cluster_dbscan(cloud, eps, m)
        assert isinstance(got, np.ndarray) and got.dtype == np.int32 and np.array_equal(got, D.batch_sklearn(eps, m)[0][offsets[s]:offsets[s + 1]])
    wide = np.concatenate([cloud, np.arange(len(cloud) * 3, dtype=np.float64).reshape(-1, 3)], axis=1)       # extra columns are not read
    assert np.array_equal(ops.cluster_dbscan(wide, 0.05, 4), ops.cluster_dbscan(cloud, 0.05, 4))
    narrow = cloud.astype(np.float32)                                        # float32 in: widened exactly
    assert np.array_equal(ops.cluster_dbscan(narrow, 0.05, 4), ops.cluster_dbscan(narrow.astype(np.float64), 0.05, 4))
    empty = ops.cluster_dbscan(np.zeros((0, 3), dtype=np.float32), 0.1, 3)
    assert empty.shape == (0,) and empty.dtype == np.int32
    on_host = ops.cluster_dbscan(torch.from_numpy(cloud.copy()), 0.05, 4)    # a host tensor in gives a host tensor out
    assert isinstance(on_host, torch.Tensor) and np.array_equal(on_host.numpy(), ops.cluster_dbscan(cloud, 0.05, 4))
    assert CS.dbscan_segments_host(cloud, [0, len(cloud)], 0.05, 4)[1].tolist() == [int(on_host.max()) + 1]


def test_cluster_is_off_by_default_and_the_docstrings_keep_their_sentences():
    from mspa import cloud_segments as CS
    from mspa.instances import InstanceClouds
    for fn in (InstanceClouds.cleaned, InstanceClouds.cleaned_objects, _handler().instance_boxes):
        assert inspect.signature(fn).parameters["cluster"].default is None, fn
    fold = lambda text: " ".join(text.split())                               # noqa: E731
    assert "One read-back per call, whatever S is: the per-segment cluster counts together with the flag word." in fold(CS.dbscan_segments.__doc__)
    assert "One read-back per call, whatever S is: the kept counts with the flag word." in fold(CS.largest_cluster_segments.__doc__)
    assert "not a fallback" in fold(CS.dbscan_segments_host.__doc__)


def _handler():
    _ops()
    from spatial_engine.utils.scannet_utils.handler.info_handler import SceneInfoHandler
    return SceneInfoHandler


# One record: int64 S, int64 min_points, int64 cap (-1: the rule's), float64 eps, (S + 1) int64 offsets, N * 3 float64 -> int32 flags,
# N int32 labels, S int32 clusters, N uint8 keep, S int32 kept.  Every buffer is a heap block of exactly its size.
DRIVER = r"""
#include "dbscan_core.h"
#include <cstdio>
#include <cstdlib>
template <typename T> static T *block(int64_t n) { return (T *)malloc((size_t)(n > 0 ? n : 1) * sizeof(T)); }
int main() {
    int64_t head[3];
    double eps;
    while (fread(head, 8, 3, stdin) == 3) {
        const int64_t S = head[0], min_points = head[1], cap = head[2];
        if (fread(&eps, 8, 1, stdin) != 1) return 3;
        int64_t *offsets = block<int64_t>(S + 1);
        if (fread(offsets, 8, (size_t)(S + 1), stdin) != (size_t)(S + 1)) return 4;
        const int64_t N = mspa::dbscan::batch_rows(offsets, S);
        if (N < 0 || !mspa::dbscan::eps_ok(eps) || min_points < 1) return 5;
        double *rows = block<double>(N * 3);
        int32_t *labels = block<int32_t>(N), *clusters = block<int32_t>(S), *kept = block<int32_t>(S);
        uint8_t *keep = block<uint8_t>(N);
        if (fread(rows, 8, (size_t)(N * 3), stdin) != (size_t)(N * 3)) return 6;
        const int32_t flags = mspa::dbscan::dbscan_all(rows, 3, offsets, S, eps, min_points, labels, clusters, keep, kept, cap);
        fwrite(&flags, 4, 1, stdout);
        fwrite(labels, 4, (size_t)N, stdout);
        fwrite(clusters, 4, (size_t)S, stdout);
        fwrite(keep, 1, (size_t)N, stdout);
        fwrite(kept, 4, (size_t)S, stdout);
        void *all[] = {offsets, rows, labels, clusters, kept, keep};
        for (void *b : all) free(b);
    }
    return 0;
}
"""


def test_the_header_under_sanitizers_and_the_cap_of_the_union_find(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    (tmp_path / "driver.cpp").write_text(DRIVER)
    exe = str(tmp_path / "driver")
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", CSRC, str(tmp_path / "driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    rows, offsets, names, _eps = D.batch()
    records = [(rows, offsets, eps, m, -1) for eps, m in ((0.05, 1), (0.05, 4), (0.125, 10), (100.0, 20))]
    records += [(x, o, 0.1, 2, -1) for x, o in D.small_batches().values()]
    nan_rows = rows.copy()
    nan_rows[123, 0] = np.nan
    records += [(rows, offsets, D.TOO_SMALL, 4, -1), (nan_rows, offsets, 0.05, 4, -1)]            # the clamped keys index nothing outside a block
    s = names.index("chain-3000")
    chain = (rows[offsets[s]:offsets[s + 1]], np.array([0, 3000], dtype=np.int64))
    records += [(*chain, 0.05, 1, 3000), (*chain, 0.05, 1, 2), (*chain, 0.05, 1, 0)]                # the rule's cap, and two that the chain reaches
    inp = b"".join(struct.pack("<qqqd", len(o) - 1, m, cap, e) + np.asarray(o, dtype="<i8").tobytes() + np.asarray(x, dtype="<f8").tobytes()
                   for x, o, e, m, cap in records)
    run = subprocess.run([exe], input=inp, capture_output=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:].decode(errors="replace"))
    at = 0

    def take(dtype, count):
        nonlocal at
        a = np.frombuffer(run.stdout, dtype=dtype, count=count, offset=at)
        at += a.nbytes
        return a

    from mspa import cloud_segments as CS
    for n, (x, o, e, m, cap) in enumerate(records):
        S, N = len(o) - 1, len(x)
        flags = int(take("<i4", 1)[0])
        labels, clusters, keep, kept = take("<i4", N), take("<i4", S), take("u1", N), take("<i4", S)
        lowered = 0 <= cap < N
        assert flags == (2 if e == D.TOO_SMALL else 1 if np.isnan(x).any() else 4 if lowered else 0), (n, flags)
        if not flags:
            want = CS.dbscan_segments_host(x, o, e, m)
            assert np.array_equal(labels, want[0]) and np.array_equal(clusters, want[1]), n
            index = CS.largest_cluster_segments_host(x, o, e, m)[4]
            assert np.array_equal(np.nonzero(keep)[0], index) and kept.sum() == len(index), n
    assert at == len(run.stdout)
