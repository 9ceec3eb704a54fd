"""The voxel down-sampling of a ragged batch on the device (csrc/voxel_segments.hip) on the batch of tests/voxel_segments_util.py:
the device against the host twin, bit for bit, every case twice with equal bits between the runs; clamp-worthy input handed to the C
entry points between fences; the refusals; and ``InstanceClouds.by_object`` / ``cleaned_objects`` / ``instance_boxes`` with a
``voxel_size`` on the golden scene and the four-frame synthetic scene of tests/test_gpu_instance_boxes.py."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_segments_util as V  # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def device_batch(columns):
    rows, offsets, names = V.batch(columns)
    return torch.from_numpy(rows.copy()).cuda(), offsets, names


def _np(result):
    rows, offsets, counts = result
    assert rows.is_cuda and counts.is_cuda and isinstance(offsets, np.ndarray)
    return rows.cpu().numpy(), offsets, counts.cpu().numpy()


@pytest.mark.parametrize("columns", V.COLUMNS)
@pytest.mark.parametrize("size", V.SIZES)
def test_the_device_equals_the_host_twin_bit_for_bit_and_itself_on_a_second_run(size, columns):
    from mspa import cloud_segments as CS
    rows, offsets, _names = device_batch(columns)
    first = _np(CS.voxel_down_sample_segments(rows, offsets, size))
    second = _np(CS.voxel_down_sample_segments(rows, offsets, size))
    V.assert_same(first, V.batch_twin(size, columns), (size, columns))
    assert all(np.array_equal(a, b) for a, b in zip(first, second)) and np.array_equal(V.bits(first[0]), V.bits(second[0]))


def test_more_than_256_compaction_tiles_so_that_the_scan_takes_two_tiles_per_thread():
    """V.scan_batch(): 526 750 slots, 526 400 voxels (five of them runs of 71 rows), so both compactions -- the heads over the slots
    and the long runs over the voxels -- have 258 tiles of 2 048 and the one workgroup's scan gives each thread two."""
    from mspa import cloud_segments as CS
    rows, offsets = V.scan_batch()
    want = CS.voxel_down_sample_segments_host(rows, offsets, 0.5)
    assert len(want[0]) == 526400 > V.SCAN_SLOTS and int((want[2] == 71).sum()) == 5 and int((want[2] == 1).sum()) == 526395
    V.assert_same(_np(CS.voxel_down_sample_segments(torch.from_numpy(rows.copy()).cuda(), offsets, 0.5)), want)


def test_a_float32_origin_input_widened_to_float64():
    from mspa import cloud_segments as CS
    rows, offsets, _names = V.batch(6)
    narrow = rows.astype(np.float32)
    wide = narrow.astype(np.float64)
    want = CS.voxel_down_sample_segments_host(wide, offsets, 0.25)
    for given in (torch.from_numpy(wide).cuda(), torch.from_numpy(narrow).cuda()):      # widened by the caller, and by the function
        first, second = _np(CS.voxel_down_sample_segments(given, offsets, 0.25)), _np(CS.voxel_down_sample_segments(given, offsets, 0.25))
        V.assert_same(first, want)
        assert np.array_equal(V.bits(first[0]), V.bits(second[0])) and np.array_equal(first[2], second[2])


@pytest.mark.parametrize("name", ["S=1", "all-empty", "N=0", "n=1"])
def test_one_segment_only_empty_segments_no_rows_and_one_row(name):
    from mspa import cloud_segments as CS
    xyz, offsets = V.small_batches()[name]
    rows = torch.from_numpy(np.ascontiguousarray(xyz)).cuda()
    for size in (0.05, 10.0):
        V.assert_same(_np(CS.voxel_down_sample_segments(rows, offsets, size)), CS.voxel_down_sample_segments_host(xyz, offsets, size), (name, size))


def test_ops_voxel_down_sample_on_a_device_tensor_is_the_one_segment_batch():
    from test_gpu_facade import facade
    ops = facade().OPS
    rows, offsets, names = device_batch(6)
    s = names.index("near-1e3-20000")
    whole = V.batch_twin(0.25, 6)
    got = ops.voxel_down_sample(rows[offsets[s]:offsets[s + 1]], 0.25)
    assert got.is_cuda and got.dtype == torch.float64
    assert np.array_equal(V.bits(got.cpu().numpy()), V.bits(whole[0][whole[1][s]:whole[1][s + 1]]))
    empty = ops.voxel_down_sample(rows[:0], 0.25)
    assert empty.shape == (0, 6) and empty.is_cuda and empty.dtype == torch.float64


def test_the_refusals():
    from mspa import cloud_segments as CS
    rows, offsets, _names = device_batch(3)
    with pytest.raises(ValueError, match="voxel_size"):                      # from the single read-back
        CS.voxel_down_sample_segments(rows, offsets, V.TOO_SMALL)
    for value in (float("nan"), float("inf")):
        bad = rows.clone()
        bad[5000, 1] = value
        with pytest.raises(ValueError, match="non-finite"):
            CS.voxel_down_sample_segments(bad, offsets, 0.25)
    for size in (0, -1, 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="voxel_size"):
            CS.voxel_down_sample_segments(rows, offsets, size)
    with pytest.raises(ValueError):
        CS.voxel_down_sample_segments(rows, offsets[:-1], 0.25)
    with pytest.raises(ValueError):
        CS.voxel_down_sample_segments(rows[:, :2], offsets, 0.25)


CLAMPED = ["out_of_range_size", "nan_row", "reversed_order", "constant_order"]


@pytest.mark.parametrize("kind", CLAMPED)
def test_clamp_worthy_input_to_the_c_entry_points_leaves_every_index_inside_the_buffers(kind):
    """A size whose indices pass 2^21, a NaN row, and a reversed or a constant permutation in place of the sort's output: keys are
    clamped and order entries are clamped into the slot's segment, so the result may hold wrong values or the flag word is raised,
    but nothing is written outside a buffer and nothing faults.  Inputs, outputs and workspace sit between fences.  (The first 16
    segments of the batch, 4 909 rows, with the far points of far-2005 behind them for the size that is too small.)"""
    from fence_util import fenced_allocations, fenced_copy
    from mspa import _lib, cloud_segments as CS
    from mspa.engine import _ptr, _stream_ptr, _workspace
    lib = _lib.load()
    rows_all, offsets_all, names = V.batch(6)
    far = names.index("far-2005")
    host_rows = np.ascontiguousarray(np.concatenate([rows_all[:offsets_all[16]], rows_all[offsets_all[far]:offsets_all[far + 1]]]))
    off = np.ascontiguousarray(np.concatenate([offsets_all[:17], [offsets_all[16] + offsets_all[far + 1] - offsets_all[far]]]))
    N, S, C = len(host_rows), len(off) - 1, 6
    size = V.TOO_SMALL if kind == "out_of_range_size" else 0.25
    if kind == "nan_row":
        host_rows[4500, 2] = np.nan
    for mode in ("a", "b"):
        inputs, on_inputs, _snap = fenced_copy({"rows": torch.from_numpy(host_rows.copy()).cuda()}, mode)
        with fenced_allocations(mode) as fences:
            tile_base = np.zeros((S + 1,), dtype=np.int64)
            _lib.check(lib.mspa_voxel_segments_tables_host(off.ctypes.data, S, tile_base.ctypes.data))
            off_dev, base_dev = CS._upload(off, tile_base, device="cuda")
            keys = torch.zeros((N,), dtype=torch.int64, device="cuda")
            segment = torch.zeros((N,), dtype=torch.int32, device="cuda")
            seg_voxels = torch.zeros((S + 1,), dtype=torch.int32, device="cuda")
            work = _workspace(int(lib.mspa_voxel_segments_workspace_bytes(off.ctypes.data, S)), "cuda")
            _lib.check(lib.mspa_voxel_segments_keys_device(_ptr(inputs["rows"]), C, off.ctypes.data, S, size, _ptr(off_dev), _ptr(base_dev),
                                                           _ptr(keys), _ptr(segment), _ptr(seg_voxels), _ptr(work), int(work.numel()), _stream_ptr()))
            order = torch.sort(keys, stable=True).indices
            order = order.gather(0, torch.sort(segment.gather(0, order), stable=True).indices)
            if kind == "reversed_order":
                order = order.flip(0).contiguous()
            elif kind == "constant_order":
                order = torch.full_like(order, 7)
            _lib.check(lib.mspa_voxel_segments_heads_device(off.ctypes.data, S, _ptr(off_dev), _ptr(keys), _ptr(order), _ptr(seg_voxels), _ptr(work),
                                                            int(work.numel()), _stream_ptr()))
            back = seg_voxels.cpu().numpy()
            M = int(back[:S].sum())
            out = torch.zeros((M, C), dtype=torch.float64, device="cuda")
            counts = torch.zeros((M,), dtype=torch.int32, device="cuda")
            _lib.check(lib.mspa_voxel_segments_means_device(_ptr(inputs["rows"]), C, off.ctypes.data, S, _ptr(off_dev), _ptr(order), M, _ptr(out),
                                                            _ptr(counts), _ptr(work), int(work.numel()), _stream_ptr()))
            torch.cuda.synchronize()
        assert len(fences) >= 3
        assert on_inputs.check_fences() + fences.check_fences() == [], (kind, mode)
        assert on_inputs.changed_inputs() == [], (kind, mode)
        assert bool((keys >= 0).all()) and bool((segment >= 0).all()) and bool((segment < S).all())
        assert {"out_of_range_size": 2, "nan_row": 1}.get(kind, 0) == int(back[S]), (kind, back[S])
        n = np.diff(off)
        assert (back[:S] >= (n > 0)).all() and (back[:S] <= n).all() and 0 < M <= N
        assert int(counts.sum()) == N and bool((counts >= 1).all())           # the runs tile the slots, whatever the order says


# ---- the scene: by_object, cleaned_objects and instance_boxes with a voxel size ------------------------------------------------

SCENE_SIZES = (0.02, 0.1)
NB, RATIO = 20, 1.0


@pytest.fixture(scope="module", params=["golden", "synth"])
def scene(request, tmp_path_factory):
    import test_gpu_instance_boxes as TB
    from mspa import instances
    root = str(tmp_path_factory.mktemp("voxel_scene_" + request.param))
    ns, h, sid, ids, with_color, n_objects = (TB._golden_scene if request.param == "golden" else TB._synth_scene)(root)
    clouds = h.instance_clouds(sid, with_color=with_color)
    TB._annotate(h, sid, clouds, n_objects)
    assert instances.LAST_INSTANCE_CLOUDS["path"] == "device", instances.LAST_INSTANCE_CLOUDS
    return ns, h, sid, ids, clouds


def _same(a, b):
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


@pytest.mark.parametrize("size", SCENE_SIZES)
def test_by_object_and_cleaned_objects_with_a_voxel_size_equal_the_single_cloud_op_per_object(scene, size):
    from mspa import cloud_segments as CS
    ns, h, sid, ids, clouds = scene
    plain_rows, plain_offsets, object_ids = clouds.by_object()
    rows, offsets, ids_ds = clouds.by_object(size)
    assert np.array_equal(ids_ds, object_ids) and offsets.dtype == np.int64 and offsets[-1] == len(rows) and rows.dtype == torch.float64
    assert rows.shape[1] == clouds.rows.shape[1] and len(rows) <= len(plain_rows) and (np.diff(offsets) >= 1).all()
    for j, t in enumerate(object_ids):
        want = ns.OPS.voxel_down_sample(clouds.object_cloud(int(t)), size)
        assert torch.equal(rows[offsets[j]:offsets[j + 1]].view(torch.int64), want.view(torch.int64)), (t, size)
    again = clouds.by_object(size)
    assert torch.equal(again[0].view(torch.int64), rows.view(torch.int64)) and np.array_equal(again[1], offsets)
    # ... and then the batched cleaning of that
    kept, kept_offsets, kept_ids, boxes = clouds.cleaned_objects(NB, RATIO, voxel_size=size)
    want_kept, want_offsets, lo, hi = CS.remove_statistical_outliers_segments(rows, offsets, NB, RATIO)
    assert np.array_equal(kept_ids, object_ids) and np.array_equal(kept_offsets, want_offsets) and torch.equal(kept, want_kept)
    assert _same(boxes, CS.boxes_of(lo, hi))
    out = h.instance_boxes(sid, nb_neighbors=NB, std_ratio=RATIO, per="object", voxel_size=size)
    assert np.array_equal(out["object_ids"], object_ids) and _same(out["boxes"], boxes) and np.array_equal(out["kept"], np.diff(kept_offsets))
    assert out["iou"].shape == (len(object_ids),)


def test_without_a_voxel_size_everything_is_bit_identical_and_per_image_refuses_one(scene):
    ns, h, sid, ids, clouds = scene
    a, b = clouds.by_object(), clouds.by_object(voxel_size=None)
    assert torch.equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    a, b = clouds.cleaned_objects(NB, RATIO), clouds.cleaned_objects(NB, RATIO, voxel_size=None)
    assert torch.equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and _same(a[3], b[3])
    for per in ("image", "object"):
        a, b = h.instance_boxes(sid, nb_neighbors=NB, std_ratio=RATIO, per=per), h.instance_boxes(sid, nb_neighbors=NB, std_ratio=RATIO, per=per,
                                                                                                  voxel_size=None)
        assert _same(a["boxes"], b["boxes"]) and _same(a["iou"], b["iou"]) and np.array_equal(a["kept"], b["kept"])
    with pytest.raises(ValueError, match="voxel_size"):
        h.instance_boxes(sid, per="image", voxel_size=0.05)
    with pytest.raises(RuntimeError, match="voxel_size"):
        h.instance_boxes(sid, per="object", voxel_size=0.0)
