"""DBSCAN of a ragged batch on the device (csrc/dbscan_segments.hip) on the batch of tests/dbscan_segments_util.py: the device against
the host twin, labels and cluster counts equal, every case twice with equal values between the runs; the device against
scikit-learn's labels frozen in tests/golden/dbscan_labels.npz (no scikit-learn is needed here); the refusals; clamp-worthy input
handed to the C entry point between fences; ``largest_cluster_segments`` against the twin; and ``InstanceClouds.cleaned`` /
``cleaned_objects`` / ``instance_boxes`` with ``cluster=`` on the golden scene and the four-frame synthetic scene of
tests/test_gpu_instance_boxes.py, held against the composition over the single-segment functions."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dbscan_segments_util as D  # noqa: E402
import voxel_segments_util as V  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = [(eps, m) for eps in D.eps_values() for m in D.MIN_POINTS]


@functools.lru_cache(maxsize=None)
def device_batch():
    rows, offsets, names, _eps = D.batch()
    return torch.from_numpy(rows.copy()).cuda(), offsets, names


@pytest.mark.parametrize("eps,min_points", CASES)
def test_the_device_equals_the_host_twin_and_itself_on_a_second_run(eps, min_points):
    from mspa import cloud_segments as CS
    rows, offsets, names = device_batch()
    want, want_clusters = D.batch_twin(eps, min_points)
    first, second = CS.dbscan_segments(rows, offsets, eps, min_points), CS.dbscan_segments(rows, offsets, eps, min_points)
    for labels, clusters in (first, second):
        assert labels.is_cuda and labels.dtype == torch.int32 and isinstance(clusters, np.ndarray) and clusters.dtype == np.int64
        got = labels.cpu().numpy()
        differ = np.nonzero(got != want)[0]
        assert len(differ) == 0, (eps, min_points, len(differ), sorted({names[int(np.searchsorted(offsets, r, side="right")) - 1] for r in differ[:20]}))
        assert np.array_equal(clusters, want_clusters)


def test_the_device_gives_the_frozen_labels_of_scikit_learn():
    from mspa import cloud_segments as CS
    rows, offsets, _names = device_batch()
    frozen = D.golden()
    assert sorted(frozen) == sorted(D.GOLDEN_PARAMETERS)
    for (eps, m), want in frozen.items():
        labels, clusters = CS.dbscan_segments(rows, offsets, eps, m)
        assert np.array_equal(labels.cpu().numpy(), want), (eps, m)
        assert np.array_equal(clusters, [want[a:b].max(initial=-1) + 1 for a, b in zip(offsets[:-1], offsets[1:])])


@pytest.mark.parametrize("eps,min_points", [(0.02, 4), (0.05, 1), (0.05, 4), (0.125, 10), (100.0, 20)])
def test_the_largest_cluster_equals_the_host_twins(eps, min_points):
    from mspa import cloud_segments as CS
    rows, offsets, _names = device_batch()
    want = CS.largest_cluster_segments_host(D.batch()[0], offsets, eps, min_points)
    for _run in range(2):
        kept, kept_offsets, lo, hi, index = CS.largest_cluster_segments(rows, offsets, eps, min_points)
        assert kept.is_cuda and index.dtype == torch.int64 and isinstance(kept_offsets, np.ndarray) and kept_offsets.dtype == np.int64
        assert np.array_equal(index.cpu().numpy(), want[4]) and np.array_equal(kept_offsets, want[1])
        assert np.array_equal(kept.cpu().numpy(), want[0]) and np.array_equal(lo.cpu().numpy(), want[2]) and np.array_equal(hi.cpu().numpy(), want[3])


def test_more_than_256_compaction_tiles_so_that_the_scan_takes_two_tiles_per_thread():
    """tests/voxel_segments_util.scan_batch() at (eps 0.4, min_points 1): every distinct point is its own cluster, so 526 400 of the
    526 750 rows are representatives; the compaction has 258 tiles of 2 048 rows and the one workgroup's scan gives each thread two."""
    from mspa import cloud_segments as CS
    host_rows, offsets = V.scan_batch()
    rows = torch.from_numpy(host_rows.copy()).cuda()
    want_labels, want_clusters = CS.dbscan_segments_host(host_rows, offsets, 0.4, 1)
    assert int(want_clusters.sum()) == 526400 > V.SCAN_SLOTS and want_labels.min() == 0
    labels, clusters = CS.dbscan_segments(rows, offsets, 0.4, 1)
    assert np.array_equal(labels.cpu().numpy(), want_labels) and np.array_equal(clusters, want_clusters) and clusters.dtype == np.int64
    want = CS.largest_cluster_segments_host(host_rows, offsets, 0.4, 1)
    kept, kept_offsets, lo, hi, index = CS.largest_cluster_segments(rows, offsets, 0.4, 1)
    assert np.array_equal(index.cpu().numpy(), want[4]) and np.array_equal(kept_offsets, want[1]) and kept_offsets[-1] == 1 + 1 + 71
    assert np.array_equal(kept.cpu().numpy(), want[0]) and np.array_equal(lo.cpu().numpy(), want[2]) and np.array_equal(hi.cpu().numpy(), want[3])


def test_extra_columns_and_float32_rows_are_carried_and_widened():
    from mspa import cloud_segments as CS
    rows, offsets, _names, _eps = D.batch()
    narrow = np.concatenate([rows, np.arange(len(rows) * 3).reshape(-1, 3) % 251], axis=1).astype(np.float32)
    want = CS.largest_cluster_segments_host(narrow, offsets, 0.05, 4)
    kept, kept_offsets, _lo, _hi, index = CS.largest_cluster_segments(torch.from_numpy(narrow).cuda(), offsets, 0.05, 4)
    assert kept.dtype == torch.float32 and kept.shape[1] == 6 and np.array_equal(kept.cpu().numpy(), want[0]) and np.array_equal(kept_offsets, want[1])
    labels, _clusters = CS.dbscan_segments(torch.from_numpy(narrow).cuda(), offsets, 0.05, 4)
    assert np.array_equal(labels.cpu().numpy(), CS.dbscan_segments_host(narrow, offsets, 0.05, 4)[0])


@pytest.mark.parametrize("name", ["S=1", "all-empty", "N=0", "n=1"])
def test_one_segment_only_empty_segments_no_rows_and_one_row(name):
    from mspa import cloud_segments as CS
    xyz, offsets = D.small_batches()[name]
    rows = torch.from_numpy(np.ascontiguousarray(xyz)).cuda()
    for eps, m in ((0.1, 1), (0.1, 4), (10.0, 2)):
        labels, clusters = CS.dbscan_segments(rows, offsets, eps, m)
        want = CS.dbscan_segments_host(xyz, offsets, eps, m)
        assert np.array_equal(labels.cpu().numpy(), want[0]) and np.array_equal(clusters, want[1]) and clusters.shape == want[1].shape
        got, want = CS.largest_cluster_segments(rows, offsets, eps, m), CS.largest_cluster_segments_host(xyz, offsets, eps, m)
        assert np.array_equal(got[4].cpu().numpy(), want[4]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2].cpu().numpy(), want[2])


def test_ops_cluster_dbscan_on_a_device_tensor_is_the_one_segment_batch():
    from test_gpu_facade import facade
    ops = facade().OPS
    rows, offsets, names = device_batch()
    s = names.index("bridge")
    got = ops.cluster_dbscan(rows[offsets[s]:offsets[s + 1]], 0.05, 4)
    assert got.is_cuda and got.dtype == torch.int32
    assert np.array_equal(got.cpu().numpy(), D.golden()[(0.05, 4)][offsets[s]:offsets[s + 1]])
    empty = ops.cluster_dbscan(rows[:0], 0.05, 4)
    assert empty.shape == (0,) and empty.is_cuda and empty.dtype == torch.int32


def test_the_refusals():
    from mspa import cloud_segments as CS
    rows, offsets, _names = device_batch()
    for call in (CS.dbscan_segments, CS.largest_cluster_segments):
        with pytest.raises(ValueError, match="eps 1e-06 is too small"):      # from the single read-back
            call(rows, offsets, D.TOO_SMALL, 4)
        for value in (float("nan"), float("inf")):
            bad = rows.clone()
            bad[5000, 1] = value
            with pytest.raises(ValueError, match="non-finite"):
                call(bad, offsets, 0.05, 4)
        for eps, m in ((0, 4), (-1.0, 4), (float("nan"), 4), (float("inf"), 4), (1e-200, 4), (0.05, 0), (0.05, -1), (0.05, 2.5)):
            with pytest.raises(RuntimeError, match="cluster_dbscan: eps must be positive"):
                call(rows, offsets, eps, m)
        with pytest.raises(ValueError):
            call(rows, offsets[:-2], 0.05, 4)
        with pytest.raises(ValueError):
            call(rows[:, :2], offsets, 0.05, 4)


CLAMPED = ["eps_too_small", "nan_row", "reversed_order", "constant_order", "negative_keys"]


@pytest.mark.parametrize("kind", CLAMPED)
def test_clamp_worthy_input_to_the_c_entry_point_leaves_every_index_inside_the_buffers(kind):
    """An eps whose cell indices pass 2^21, a NaN row, a reversed or a constant permutation in place of the sort's output, keys that
    are not the keys call's: keys are clamped, order entries are clamped into the slot's segment, rows no slot names stay "not
    core" and "noise", so the result may hold wrong labels or the flag word is raised, but nothing is written outside a buffer.
    Inputs, outputs and both workspaces sit between fences.  (The first 16 segments of the batch with far-2005 behind them.)"""
    from fence_util import fenced_allocations, fenced_copy
    from mspa import _lib, cloud_segments as CS
    from mspa.engine import _ptr, _stream_ptr, _workspace
    lib = _lib.load()
    rows_all, offsets_all, names, _eps = D.batch()
    far = names.index("far-2005")
    host_rows = np.ascontiguousarray(np.concatenate([rows_all[:offsets_all[17]], rows_all[offsets_all[far]:offsets_all[far + 1]]]))
    off = np.ascontiguousarray(np.concatenate([offsets_all[:18], [offsets_all[17] + offsets_all[far + 1] - offsets_all[far]]]))
    N, S = len(host_rows), len(off) - 1
    eps = D.TOO_SMALL if kind == "eps_too_small" else 0.05
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
            seg = torch.zeros((2 * S + 1,), dtype=torch.int32, device="cuda")
            labels = torch.full((N,), 77, dtype=torch.int32, device="cuda")
            keep = torch.full((N,), 77, dtype=torch.uint8, device="cuda")
            cells_work = _workspace(int(lib.mspa_voxel_segments_workspace_bytes(off.ctypes.data, S)), "cuda")
            _lib.check(lib.mspa_voxel_segments_keys_device(_ptr(inputs["rows"]), 3, off.ctypes.data, S, lib.mspa_dbscan_cell_side(eps),
                                                           _ptr(off_dev), _ptr(base_dev), _ptr(keys), _ptr(segment), _ptr(seg[S:]), _ptr(cells_work),
                                                           int(cells_work.numel()), _stream_ptr()))
            order = torch.sort(keys, stable=True).indices
            order = order.gather(0, torch.sort(segment.gather(0, order), stable=True).indices)
            if kind == "reversed_order":
                order = order.flip(0).contiguous()
            elif kind == "constant_order":
                order = torch.full_like(order, 7)
            elif kind == "negative_keys":
                keys = -keys - 1
            work = _workspace(int(lib.mspa_dbscan_segments_workspace_bytes(off.ctypes.data, S)), "cuda")
            lo, hi = torch.zeros((S, 3), dtype=torch.float64, device="cuda"), torch.zeros((S, 3), dtype=torch.float64, device="cuda")
            _lib.check(lib.mspa_dbscan_segments_device(_ptr(inputs["rows"]), 3, off.ctypes.data, S, eps, 4, _ptr(off_dev), _ptr(keys), _ptr(order),
                                                       _ptr(base_dev), _ptr(labels), _ptr(keep), _ptr(lo), _ptr(hi), _ptr(seg), _ptr(work),
                                                       int(work.numel()), _stream_ptr()))
            torch.cuda.synchronize()
        back = seg.cpu().numpy()
        assert len(fences) >= 4
        assert on_inputs.check_fences() + fences.check_fences() == [], (kind, mode)
        assert on_inputs.changed_inputs() == [], (kind, mode)
        assert {"eps_too_small": 2, "nan_row": 1}.get(kind, 0) == int(back[2 * S]) & 3, (kind, back[2 * S])
        n = np.diff(off)
        kept, clusters = back[:S], back[S:2 * S]
        assert (clusters >= 0).all() and (clusters <= n).all() and (kept >= 0).all() and (kept <= n).all()
        got, kept_rows = labels.cpu().numpy(), keep.cpu().numpy()
        assert (got >= -1).all() and (kept_rows <= 1).all()
        for s in range(S):
            assert (got[off[s]:off[s + 1]] < max(clusters[s], 1)).all(), (kind, s)


# ---- the scene: cleaned, cleaned_objects and instance_boxes with cluster= ------------------------------------------------------

NB, RATIO = 20, 1.0
CLUSTERS = ((0.05, 10), (0.1, 4))


@pytest.fixture(scope="module", params=["golden", "synth"])
def scene(request, tmp_path_factory):
    import test_gpu_instance_boxes as TB
    from mspa import instances
    root = str(tmp_path_factory.mktemp("dbscan_scene_" + request.param))
    ns, h, sid, ids, with_color, n_objects = (TB._golden_scene if request.param == "golden" else TB._synth_scene)(root)
    clouds = h.instance_clouds(sid, with_color=with_color)
    TB._annotate(h, sid, clouds, n_objects)
    assert instances.LAST_INSTANCE_CLOUDS["path"] == "device", instances.LAST_INSTANCE_CLOUDS
    return ns, h, sid, ids, clouds


def _same(a, b):
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def _largest_of_one(ns, cloud, eps, min_points):
    """The rows of one cloud's largest cluster over the single-segment functions: ``ops.cluster_dbscan``, then ``torch.bincount``."""
    labels = ns.OPS.cluster_dbscan(cloud, eps, min_points)
    if not bool((labels >= 0).any()):
        return cloud[:0], labels[:0].to(torch.int64)
    best = int(torch.bincount(labels[labels >= 0].to(torch.int64)).argmax())        # (the first maximum, checked against np below)
    assert best == int(np.bincount(labels[labels >= 0].cpu().numpy()).argmax())
    index = torch.nonzero(labels == best).flatten()
    return cloud.index_select(0, index), index


def _box(ns, rows):
    return ns.OPS.calculate_aabb(rows[:, :3]) if len(rows) else torch.full((6,), float("nan"), dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("cluster", CLUSTERS)
def test_cleaned_objects_and_instance_boxes_with_a_cluster_equal_the_composition_per_object(scene, cluster):
    from mspa import cloud_segments as CS
    ns, h, sid, ids, clouds = scene
    for size in (None, 0.02):
        base, base_offsets, object_ids, _boxes = clouds.cleaned_objects(NB, RATIO, voxel_size=size)
        kept, kept_offsets, kept_ids, boxes = clouds.cleaned_objects(NB, RATIO, voxel_size=size, cluster=cluster)
        assert np.array_equal(kept_ids, object_ids) and kept_offsets.dtype == np.int64 and kept_offsets[-1] == len(kept) and kept.dtype == base.dtype
        for j, t in enumerate(object_ids):
            want, _index = _largest_of_one(ns, base[base_offsets[j]:base_offsets[j + 1]], *cluster)
            assert torch.equal(kept[kept_offsets[j]:kept_offsets[j + 1]], want), (t, cluster, size)
            assert _same(boxes[j], _box(ns, want).to(torch.float64)), (t, cluster, size)
        assert len(kept) > 0
        out = h.instance_boxes(sid, nb_neighbors=NB, std_ratio=RATIO, per="object", voxel_size=size, cluster=cluster)
        assert np.array_equal(out["object_ids"], object_ids) and _same(out["boxes"], boxes) and np.array_equal(out["kept"], np.diff(kept_offsets))
        assert _same(out["iou"], CS.iou_3d(boxes, _gt(h, sid, object_ids, boxes.device)))


def _gt(h, sid, object_ids, device):
    gt = np.full((len(object_ids), 6), np.nan)
    for j, t in enumerate(object_ids):
        if 0 <= t < h.get_num_objects(sid):
            gt[j] = np.asarray(h.get_object_gt_bbox(sid, int(t), axis_aligned=True), dtype=np.float64)[:6]
    return torch.from_numpy(gt).to(device)


@pytest.mark.parametrize("cluster", CLUSTERS)
def test_cleaned_with_a_cluster_equals_the_composition_per_image_and_object(scene, cluster):
    ns, h, sid, ids, clouds = scene
    base = clouds.cleaned(NB, RATIO)
    got = clouds.cleaned(NB, RATIO, cluster=cluster)
    assert got.counts.shape == clouds.counts.shape and got.offsets[-1] == len(got.rows) and got.image_ids == clouds.image_ids
    assert (got.pixel is None) == (clouds.pixel is None) and (got.rgb is None) == (clouds.rgb is None)
    boxes = got.boxes()
    seen = 0
    for k, image in enumerate(clouds.image_ids):
        for t in base.present(image):
            a = base._segment(image, t)[2]
            want, index = _largest_of_one(ns, base.cloud(image, t), *cluster)
            assert torch.equal(got.cloud(image, t), want), (image, t, cluster)
            assert _same(boxes[k, t + 1], _box(ns, want).to(torch.float64)), (image, t)
            ga, gb = got._segment(image, t)[2:]
            if got.pixel is not None:
                assert torch.equal(got.pixel[ga:gb], base.pixel[a + index])
            if got.rgb is not None:
                assert torch.equal(got.rgb[ga:gb], base.rgb[a + index])
            seen += len(want) > 0
    assert seen > 0 and int(got.counts.sum()) == len(got.rows) <= len(base.rows)
    out = h.instance_boxes(sid, nb_neighbors=NB, std_ratio=RATIO, per="image", cluster=cluster)
    assert _same(out["boxes"], boxes) and np.array_equal(out["kept"], got.counts)


def test_without_a_cluster_everything_is_what_the_functions_in_front_of_it_give(scene):
    """``cluster=None`` is the code path of before: ``cleaned`` is ``clean_segments`` and ``cleaned_objects`` is
    ``remove_statistical_outliers_segments`` over ``by_object``, value for value."""
    from mspa import cloud_segments as CS
    ns, h, sid, ids, clouds = scene
    rows, offsets, lo, hi, index = CS.clean_segments(clouds.rows, clouds.offsets, NB, RATIO)
    for got in (clouds.cleaned(NB, RATIO), clouds.cleaned(NB, RATIO, cluster=None)):
        assert torch.equal(got.rows, rows) and np.array_equal(got.offsets, offsets) and _same(got.lo.reshape(-1, 3), lo) and _same(got.hi.reshape(-1, 3), hi)
        if clouds.pixel is not None:
            assert torch.equal(got.pixel, clouds.pixel.index_select(0, index))
    for size in (None, 0.02):
        by_rows, by_offsets, object_ids = clouds.by_object(size)
        want = CS.remove_statistical_outliers_segments(by_rows, by_offsets, NB, RATIO)
        for got in (clouds.cleaned_objects(NB, RATIO, voxel_size=size), clouds.cleaned_objects(NB, RATIO, voxel_size=size, cluster=None)):
            assert torch.equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], object_ids)
            assert _same(got[3], CS.boxes_of(want[2], want[3]))
    for per in ("image", "object"):
        a, b = h.instance_boxes(sid, nb_neighbors=NB, std_ratio=RATIO, per=per), h.instance_boxes(sid, nb_neighbors=NB, std_ratio=RATIO, per=per,
                                                                                                  cluster=None)
        assert _same(a["boxes"], b["boxes"]) and _same(a["iou"], b["iou"]) and np.array_equal(a["kept"], b["kept"])
    with pytest.raises(RuntimeError, match="cluster_dbscan"):
        h.instance_boxes(sid, per="object", cluster=(0.0, 4))
