"""The ragged-batch cleaning on the device (csrc/cloud_segments.hip) on the batch of tests/cloud_segments_util.py: the search
against its host twin and against the single-cloud device op per segment, bit for bit; the statistics against the host twin, bit
for bit; the kept rows against ``ops.remove_statistical_outliers`` per segment behind the guard on the batch; the exceptions; and
a permuted or out-of-range order handed to the C entry point between fences."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_segments_util as U  # noqa: E402

pytestmark = pytest.mark.gpu


def _ops():
    from test_gpu_facade import facade
    return facade().OPS


@functools.lru_cache(maxsize=None)
def device_batch():
    xyz, offsets, names = U.batch()
    return torch.from_numpy(xyz.copy()).cuda(), offsets, names


@functools.lru_cache(maxsize=None)
def host_search(k):
    from mspa import cloud_segments as CS
    xyz, offsets, _names = U.batch()
    return CS.knn_mean_distance_segments_host(xyz, offsets, k, want_evals=True)


@functools.lru_cache(maxsize=None)
def device_search(k):
    from mspa import cloud_segments as CS
    xyz, offsets, _names = device_batch()
    return CS.knn_mean_distance_segments(xyz, offsets, k, want_evals=True)


@pytest.mark.parametrize("k", U.KS)
def test_avg_and_evals_equal_the_host_twin_and_the_single_cloud_op_bit_for_bit(k):
    from mspa import cloud_segments as CS, engine
    xyz, offsets, names = device_batch()
    avg, evals = device_search(k)
    want_avg, want_evals = host_search(k)
    assert np.array_equal(U.bits(avg.cpu().numpy()), U.bits(want_avg)) and np.array_equal(evals.cpu().numpy(), want_evals)
    for s, name in enumerate(names):
        a, b = int(offsets[s]), int(offsets[s + 1])
        if b > a:
            one, one_evals = engine.knn_mean_distance(xyz[a:b].contiguous(), k, want_evals=True)
            assert torch.equal(avg[a:b].view(torch.int64), one.view(torch.int64)) and torch.equal(evals[a:b], one_evals), (name, k)
    assert torch.equal(avg.view(torch.int64), CS.knn_mean_distance_segments(xyz, offsets, k).view(torch.int64))      # without evals: the same avg


@pytest.mark.parametrize("ratio", U.RATIOS)
@pytest.mark.parametrize("k", U.KS)
def test_statistics_equal_the_host_twin_bit_for_bit(k, ratio):
    from mspa import cloud_segments as CS
    xyz, offsets, _names = device_batch()
    got = CS.outlier_stats_segments(device_search(k)[0], offsets, ratio, xyz)
    want = CS.outlier_stats_segments_host(host_search(k)[0], offsets, ratio, U.batch()[0])
    assert got["keep"].dtype == torch.bool and np.array_equal(got["keep"].cpu().numpy(), want["keep"])
    assert np.array_equal(got["kept"].cpu().numpy(), want["kept"])
    for key in ("mean", "sd", "thr", "lo", "hi"):
        assert np.array_equal(U.bits(got[key].cpu().numpy()), U.bits(want[key])), (key, k, ratio)


ROWS = [("float64", 0, 20, 1.0), ("float64", 0, 20, 0.5), ("float64", 2, 64, 1.0), ("float64", 0, 1, 1.0), ("float32", 3, 20, 1.0),
        ("float32", 0, 64, 0.5)]


@pytest.mark.parametrize("dtype,extra,k,ratio", ROWS, ids=[f"{d}-{e}cols-k{k}-r{r}" for d, e, k, r in ROWS])
def test_kept_rows_equal_the_single_cloud_op_per_segment(dtype, extra, k, ratio):
    from mspa import cloud_segments as CS
    ops = _ops()
    xyz, offsets, names = U.batch()
    rng = np.random.default_rng(9)
    rows = torch.from_numpy(np.concatenate([xyz, rng.random((len(xyz), extra))], axis=1)).to(getattr(torch, dtype)).cuda()
    # the guard, first: on the avg of exactly these coordinates (float32 rows are widened, so their avg is their own)
    wide = rows[:, :3].to(torch.float64).contiguous()
    avg = CS.knn_mean_distance_segments(wide, offsets, k)
    stated = CS.outlier_stats_segments(avg, offsets, ratio, wide)["thr"].cpu().numpy()
    U.assert_guard(avg.cpu().numpy(), offsets, (stated, U.torch_sum_thresholds(avg, offsets, ratio)), (dtype, k, ratio))
    kept, kept_offsets, lo, hi = CS.remove_statistical_outliers_segments(rows, offsets, k, ratio)
    assert kept.dtype == rows.dtype and kept.shape[1] == 3 + extra and kept.is_cuda
    assert isinstance(kept_offsets, np.ndarray) and kept_offsets.dtype == np.int64 and kept_offsets[0] == 0 and kept_offsets[-1] == len(kept)
    some = 0
    for s, name in enumerate(names):
        a, b = int(offsets[s]), int(offsets[s + 1])
        want = ops.remove_statistical_outliers(rows[a:b], k, ratio)
        got = kept[int(kept_offsets[s]):int(kept_offsets[s + 1])]
        assert got.shape == want.shape and torch.equal(got, want), (name, dtype, k, ratio)
        if len(want):
            some += 1
            box = ops.calculate_aabb(want.to(torch.float64))
            assert torch.equal(torch.cat([(hi[s] + lo[s]) / 2, hi[s] - lo[s]]), box), name
        else:
            assert bool((lo[s] == float("inf")).all()) and bool((hi[s] == float("-inf")).all()), name
    assert some >= (12 if k > 1 else 0)


@pytest.mark.parametrize("name", ["S=1", "all-empty", "N=0"])
def test_one_segment_only_empty_segments_and_no_rows(name):
    from mspa import cloud_segments as CS
    ops = _ops()
    xyz, offsets = U.small_batches()[name]
    rows = torch.from_numpy(np.ascontiguousarray(xyz)).cuda()
    avg, evals = CS.knn_mean_distance_segments(rows, offsets, 20, want_evals=True)
    want = CS.knn_mean_distance_segments_host(xyz, offsets, 20, want_evals=True)
    assert np.array_equal(avg.cpu().numpy(), want[0]) and np.array_equal(evals.cpu().numpy(), want[1])
    st = CS.outlier_stats_segments(avg, offsets, 1.0, rows)
    st_host = CS.outlier_stats_segments_host(want[0], offsets, 1.0, xyz)
    for key in ("kept", "mean", "sd", "thr", "lo", "hi"):
        got = st[key].cpu().numpy()
        assert got.shape == st_host[key].shape and got.tobytes() == st_host[key].tobytes(), key
    kept, kept_offsets, lo, _hi = CS.remove_statistical_outliers_segments(rows, offsets)
    assert kept_offsets.shape == offsets.shape and kept_offsets[-1] == len(kept) and lo.shape == (len(offsets) - 1, 3)
    if len(xyz):
        U.assert_guard(want[0], offsets, (st_host["thr"], U.torch_sum_thresholds(avg, offsets, 1.0)), name)
        assert torch.equal(kept, ops.remove_statistical_outliers(rows))


def test_the_three_exceptions():
    from mspa import cloud_segments as CS
    xyz, offsets, _names = device_batch()
    for nb, ratio in ((0, 1.0), (20, 0.0), (20, -2.0)):
        with pytest.raises(RuntimeError, match="nb_neighbors must be at least 1"):
            CS.remove_statistical_outliers_segments(xyz, offsets, nb, ratio)
    with pytest.raises(NotImplementedError, match="64"):
        CS.remove_statistical_outliers_segments(xyz, offsets, 65)
    for value in (float("nan"), float("inf")):
        bad = xyz.clone()
        bad[5000, 1] = value                                                 # in the middle of a long segment: no order statistic sees it
        with pytest.raises(ValueError, match="non-finite"):
            CS.remove_statistical_outliers_segments(bad, offsets)
        with pytest.raises(ValueError):
            CS.knn_mean_distance_segments(bad, offsets, 20)
    with pytest.raises(ValueError):
        CS.knn_mean_distance_segments(xyz, offsets[:-1], 20)                 # offsets that do not end at N


ORDERS = ["reversed", "shuffled", "out_of_range", "one_row"]


@pytest.mark.parametrize("kind", ORDERS)
def test_an_order_that_is_no_permutation_of_the_sort_leaves_every_index_inside_the_buffers(kind):
    """mspa_knn_segments_mean_distance_device clamps every order entry into [0, N) and into its slot's segment: whatever order_dev
    holds, the outputs may be wrong, but nothing is written outside them and nothing faults.  Inputs, outputs and workspace sit
    between fences.  (The first 14 segments of the batch: 800 rows, rows of three segments in one wave included.)"""
    from fence_util import fenced_allocations, fenced_copy
    from mspa import _lib, cloud_segments as CS
    from mspa.engine import _ptr, _stream_ptr, _workspace
    lib = _lib.load()
    xyz_all, offsets_all, _names = U.batch()
    S, k = 14, 20
    off = np.ascontiguousarray(offsets_all[:S + 1])
    N = int(off[-1])
    rng = np.random.default_rng(3)
    order = {"reversed": np.arange(N)[::-1], "shuffled": rng.permutation(N),
             "out_of_range": rng.choice(np.array([-1, -(1 << 40), N, N + 1, 1 << 40, 0, N - 1]), size=N),
             "one_row": np.full(N, 7)}[kind].astype(np.int64)
    for mode in ("a", "b"):
        inputs, on_inputs, _snap = fenced_copy({"xyz": torch.from_numpy(xyz_all[:N].copy()).cuda(), "order": torch.from_numpy(order.copy()).cuda()}, mode)
        with fenced_allocations(mode) as fences:
            grids, off_dev, grids_dev, base_dev = CS._search_tables(inputs["xyz"], off, k)
            mean = torch.zeros((N,), dtype=torch.float64, device="cuda")
            evals = torch.zeros((N,), dtype=torch.int32, device="cuda")
            work = _workspace(int(lib.mspa_knn_segments_workspace_bytes(off.ctypes.data, S, k)), "cuda")
            _lib.check(lib.mspa_knn_segments_mean_distance_device(_ptr(inputs["xyz"]), off.ctypes.data, S, k, grids.ctypes.data, _ptr(off_dev),
                                                                  _ptr(grids_dev), _ptr(base_dev), _ptr(inputs["order"]), _ptr(mean), _ptr(evals),
                                                                  _ptr(work), int(work.numel()), _stream_ptr()))
            torch.cuda.synchronize()
        assert len(fences) >= 3
        assert on_inputs.check_fences() + fences.check_fences() == [], (kind, mode)
        assert on_inputs.changed_inputs() == [], (kind, mode)
        assert bool((evals >= 0).all())
