"""The upright minimal boxes of a ragged batch on the device (csrc/upright_segments.hip) on the batch of tests/upright_box_util.py: the
device against the host twin BIT FOR BIT -- hull indices, hull offsets, chosen edges and all eight box values -- twice, and once
more with the rows permuted (the hull as coordinates and the boxes are then identical); the device against the frozen results of
tests/golden/upright_boxes.npz; float32 rows with extra columns; the refusals and every MSPA_EINVAL of the C entry points; the
survivor counts, which keep the filter honest; and ``InstanceClouds.upright_boxes`` / ``cleaned_objects(upright=True)`` /
``instance_boxes(upright=True)`` on the synthetic scene of tests/test_gpu_instance_boxes.py against the composition over the
one-segment op ``ops.calculate_upright_box``."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import upright_box_util as B  # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def device_batch(shuffled=False):
    rows, off = (B.permuted() if shuffled else B.batch())[:2]
    return torch.from_numpy(rows.copy()).cuda(), off


def _run(rows, off):
    from mspa import cloud_segments as CS
    boxes, index, hull_offsets, edges, survivors = CS.upright_boxes_segments(rows, off, want_hull=True, want_edges=True, want_survivors=True)
    assert boxes.is_cuda and boxes.dtype == torch.float64 and index.is_cuda and index.dtype == torch.int64 and edges.dtype == torch.int32
    assert isinstance(hull_offsets, np.ndarray) and hull_offsets.dtype == np.int64 and survivors.dtype == np.int64
    return boxes.cpu().numpy(), index.cpu().numpy(), hull_offsets, edges.cpu().numpy(), survivors


def _assert_equal(got, want, names, what):
    boxes, index, hull_offsets, edges = got[:4]
    assert np.array_equal(hull_offsets, want[2]), what
    assert np.array_equal(index, want[1]), what
    assert np.array_equal(edges, want[3]), (what, [n for n, a, b in zip(names, edges, want[3]) if a != b])
    differ = [n for n, a, b in zip(names, boxes, want[0]) if a.tobytes() != b.tobytes()]
    assert differ == [], (what, differ)


def test_the_device_equals_the_host_twin_bit_for_bit_twice_and_with_the_rows_permuted():
    _rows, _off, names = B.batch()
    rows, off = device_batch()
    want = B.batch_twin()
    first, second = _run(rows, off), _run(rows, off)
    _assert_equal(first, want, names, "first run")
    _assert_equal(second, want, names, "second run")
    shuffled_rows, _off2 = device_batch(True)
    third = _run(shuffled_rows, off)
    _assert_equal(third, B.batch_twin(True), names, "rows permuted")
    assert np.array_equal(B.batch()[0][first[1], :2], B.permuted()[0][third[1], :2])      # the hull as coordinates
    assert first[0].tobytes() == third[0].tobytes() and np.array_equal(first[3], third[3])
    from mspa import cloud_segments as CS
    index, hull_offsets = CS.footprint_hull_segments(rows, off)
    assert np.array_equal(index.cpu().numpy(), want[1]) and np.array_equal(hull_offsets, want[2])


def test_the_device_gives_the_frozen_results():
    _rows, _off, names = B.batch()
    frozen = B.golden()
    _assert_equal(_run(*device_batch()), (frozen["boxes"], frozen["hull_index"], frozen["hull_offsets"], frozen["edges"]), names, "frozen")


def test_float32_rows_with_extra_columns_are_widened_and_the_extra_columns_are_not_read():
    from mspa import cloud_segments as CS
    narrow, off = B.float32_segment()
    want = CS.upright_boxes_segments_host(narrow, off, want_hull=True, want_edges=True)
    got = _run(torch.from_numpy(narrow).cuda(), off)
    _assert_equal(got, want, ["float32"], "float32, C = 6")
    assert np.array_equal(want[0], CS.upright_boxes_segments_host(narrow[:, :3].astype(np.float64), off))


@pytest.mark.parametrize("name", ["S=1", "N=0", "all-empty"])
def test_one_segment_no_rows_and_only_empty_segments(name):
    from mspa import cloud_segments as CS
    host_rows, off = B.small_batches()[name]
    got = _run(torch.from_numpy(np.ascontiguousarray(host_rows)).cuda(), off)
    want = CS.upright_boxes_segments_host(host_rows, off, want_hull=True, want_edges=True)
    _assert_equal(got, want, [name] * (len(off) - 1), name)
    assert got[0].shape == (len(off) - 1, 8) and got[4].shape == (len(off) - 1,)


def test_the_refusals():
    from mspa import cloud_segments as CS
    rows, off = device_batch()
    for call in (CS.upright_boxes_segments, CS.footprint_hull_segments):
        for value in (float("nan"), float("inf")):
            for column in (0, 2):
                bad = rows.clone()
                bad[20000, column] = value
                with pytest.raises(ValueError, match="non-finite"):
                    call(bad, off)
        for value in (1e300, 1e-300):
            bad = rows.clone()
            bad[20000, 1] = value
            with pytest.raises(ValueError, match="outside"):
                call(bad, off)
        with pytest.raises(ValueError):
            call(rows, off[:-2])
        with pytest.raises(ValueError):
            call(rows[:, :2], off)


def test_the_c_entry_points_answer_einval_for_every_bad_argument():
    """The argument checks come before the first launch: the same refusals as on a machine without a GPU, now with real device
    pointers around the bad one."""
    from mspa import _lib
    from mspa.engine import _ptr
    lib = _lib.load()
    good = np.array([0, 4, 4, 10], dtype=np.int64)
    hull_good = np.array([0, 3, 3, 8], dtype=np.int64)
    S = 3
    p = lambda a: a.ctypes.data                                              # noqa: E731
    dev = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device="cuda")      # noqa: E731
    rows, off_dev, rows_list, ext, seg = dev(10, 3), dev(S + 1, dtype=torch.int64), dev(10, dtype=torch.int64), dev(S, 10), dev(2 * S + 1, dtype=torch.int32)
    pts, row, stack = dev(10, 2), dev(10, dtype=torch.int64), dev(2, 10, dtype=torch.int32)
    hull_index, edges, boxes = dev(10, dtype=torch.int64), dev(S, dtype=torch.int32), dev(S, 8)
    filter_bytes, boxes_bytes = lib.mspa_upright_filter_workspace_bytes(p(good), S), lib.mspa_upright_boxes_workspace_bytes(p(hull_good), S)
    work = dev(max(filter_bytes, boxes_bytes), dtype=torch.uint8)
    descending = np.array([0, 5, 4, 10], dtype=np.int64)
    too_many_vertices = np.array([0, 5, 5, 10], dtype=np.int64)

    def filter_call(off=good, c=3, rows_p=_ptr(rows), list_p=_ptr(rows_list), ext_p=_ptr(ext), seg_p=_ptr(seg), w=_ptr(work), w_bytes=filter_bytes):
        return lib.mspa_upright_filter_device(rows_p, c, p(off), S, _ptr(off_dev), _ptr(off_dev), list_p, ext_p, seg_p, w, w_bytes, None)

    def hull_call(off=good, pts_p=_ptr(pts), stack_p=_ptr(stack), seg_p=_ptr(seg)):
        return lib.mspa_upright_hull_device(pts_p, p(off), S, _ptr(off_dev), stack_p, seg_p, None)

    def boxes_call(off=good, hull=hull_good, pts_p=_ptr(pts), index_p=_ptr(hull_index), boxes_p=_ptr(boxes), w=_ptr(work), w_bytes=boxes_bytes):
        return lib.mspa_upright_boxes_device(pts_p, _ptr(row), p(off), p(hull), S, _ptr(off_dev), _ptr(off_dev), _ptr(off_dev), _ptr(stack), _ptr(seg),
                                             _ptr(ext), index_p, _ptr(edges), boxes_p, w, w_bytes, None)

    refused = {
        "filter: descending offsets": filter_call(off=descending), "filter: C = 2": filter_call(c=2), "filter: null rows": filter_call(rows_p=None),
        "filter: null list": filter_call(list_p=None), "filter: null ext": filter_call(ext_p=None), "filter: null seg": filter_call(seg_p=None),
        "filter: null workspace": filter_call(w=None), "filter: workspace too small": filter_call(w_bytes=filter_bytes - 16),
        "filter: workspace misaligned": filter_call(w=_ptr(work) + 8), "filter: rows at 4 mod 8": filter_call(rows_p=_ptr(rows) + 4),
        "hull: descending offsets": hull_call(off=descending), "hull: null pts": hull_call(pts_p=None), "hull: null stack": hull_call(stack_p=None),
        "hull: null seg": hull_call(seg_p=None), "hull: stack at 2 mod 4": hull_call(stack_p=_ptr(stack) + 2),
        "boxes: descending offsets": boxes_call(off=descending), "boxes: descending hull offsets": boxes_call(hull=descending),
        "boxes: more vertices than survivors": boxes_call(hull=too_many_vertices), "boxes: null pts": boxes_call(pts_p=None),
        "boxes: null hull_index": boxes_call(index_p=None), "boxes: null boxes": boxes_call(boxes_p=None), "boxes: null workspace": boxes_call(w=None),
        "boxes: workspace too small": boxes_call(w_bytes=boxes_bytes - 16), "boxes: workspace misaligned": boxes_call(w=_ptr(work) + 8),
        "boxes: boxes at 4 mod 8": boxes_call(boxes_p=_ptr(boxes) + 4),
    }
    assert {k: v for k, v in refused.items() if v != _lib.MSPA_EINVAL} == {}
    torch.cuda.synchronize()
    assert float(boxes.abs().sum()) == 0 and int(seg.abs().sum()) == 0       # nothing was enqueued


def test_the_filter_leaves_few_rows_of_a_rectangle_and_may_keep_a_whole_circle():
    """The four corners of a turned rectangle are rows and are the extreme rows in the axis directions, so every row strictly inside
    is provably inside: at most a tenth of the rows may reach the hull stage.  On a circle every row is a hull vertex, and none may
    be dropped."""
    _rows, off, names = B.batch()
    rows, _off = device_batch()
    survivors = _run(rows, off)[4]
    lengths = np.diff(off)
    assert (survivors <= lengths).all() and ((survivors > 0) == (lengths > 0)).all()
    for name in B.RECT_CENTRES:
        s = names.index(name)
        print(name, "survivors", survivors[s], "of", lengths[s])
        assert 4 <= survivors[s] <= lengths[s] // 10, (name, survivors[s])
    for name in ("circle-5000", "ellipse-thin"):
        assert survivors[names.index(name)] == lengths[names.index(name)], name
    assert survivors[names.index("circle-5000")] > 2048                      # more than one compaction tile
    assert survivors[names.index("gauss-10000")] <= 1000
    print("survivor share of the batch", survivors.sum() / lengths.sum())


# ---- the scene: InstanceClouds.upright_boxes, cleaned_objects(upright=True) and instance_boxes(upright=True) ---------------------

NB, RATIO = 20, 1.0


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    import test_gpu_instance_boxes as TB
    from mspa import instances
    root = str(tmp_path_factory.mktemp("upright_scene"))
    ns, h, sid, ids, with_color, n_objects = TB._synth_scene(root)
    clouds = h.instance_clouds(sid, with_color=with_color)
    TB._annotate(h, sid, clouds, n_objects)
    assert instances.LAST_INSTANCE_CLOUDS["path"] == "device", instances.LAST_INSTANCE_CLOUDS
    return ns, h, sid, ids, clouds


def _same(a, b):
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def test_the_scenes_upright_boxes_equal_the_composition_over_the_one_segment_op(scene):
    ns, h, sid, ids, clouds = scene
    boxes = clouds.upright_boxes()
    assert boxes.shape == clouds.counts.shape + (8,) and boxes.is_cuda and boxes.dtype == torch.float64
    seen = 0
    for k, image in enumerate(clouds.image_ids):
        for t in clouds.present(image):
            want = ns.OPS.calculate_upright_box(clouds.cloud(image, t))
            assert want.is_cuda and want.shape == (8,) and _same(boxes[k, t + 1], want), (image, t)
            seen += 1
    assert seen > 0 and bool(torch.isnan(boxes[torch.from_numpy(clouds.counts == 0).cuda()]).all())
    empty = ns.OPS.calculate_upright_box(clouds.rows[:0])
    assert empty.is_cuda and empty.shape == (8,) and bool(torch.isnan(empty).all())
    # z is calculate_aabb's
    plain = clouds.boxes()
    assert _same(boxes[..., 2], plain[..., 2]) and _same(boxes[..., 5], plain[..., 5])


def test_cleaned_objects_and_instance_boxes_with_upright_equal_the_composition_and_the_defaults_are_todays(scene):
    ns, h, sid, ids, clouds = scene
    for size in (None, 0.02):
        plain = clouds.cleaned_objects(NB, RATIO, voxel_size=size)
        kept, kept_offsets, object_ids, boxes, upright = clouds.cleaned_objects(NB, RATIO, voxel_size=size, upright=True)
        assert len(plain) == 4 and torch.equal(kept, plain[0]) and np.array_equal(kept_offsets, plain[1]) and _same(boxes, plain[3])
        assert upright.shape == (len(object_ids), 8)
        for j, t in enumerate(object_ids):
            assert _same(upright[j], ns.OPS.calculate_upright_box(kept[kept_offsets[j]:kept_offsets[j + 1]])), (t, size)
        out = h.instance_boxes(sid, nb_neighbors=NB, std_ratio=RATIO, per="object", voxel_size=size, upright=True)
        today = h.instance_boxes(sid, nb_neighbors=NB, std_ratio=RATIO, per="object", voxel_size=size)
        assert _same(out["upright"], upright) and "upright" not in today and sorted(out) == sorted(list(today) + ["upright"])
        assert _same(out["boxes"], today["boxes"]) and _same(out["iou"], today["iou"]) and np.array_equal(out["kept"], today["kept"])
    cleaned = clouds.cleaned(NB, RATIO)
    out = h.instance_boxes(sid, nb_neighbors=NB, std_ratio=RATIO, per="image", upright=True)
    today = h.instance_boxes(sid, nb_neighbors=NB, std_ratio=RATIO, per="image", upright=False)
    assert _same(out["upright"], cleaned.upright_boxes()) and out["upright"].shape == cleaned.counts.shape + (8,) and "upright" not in today
    assert _same(out["boxes"], today["boxes"]) and _same(out["iou"], today["iou"]) and np.array_equal(out["kept"], today["kept"])
    for image in cleaned.image_ids[:2]:
        for t in cleaned.present(image):
            k = cleaned._frame[cleaned._key(image)]
            assert _same(out["upright"][k, t + 1], ns.OPS.calculate_upright_box(cleaned.cloud(image, t))), (image, t)


def test_the_corners_and_the_yaw_enqueue_only(scene):
    import warnings
    from mspa import cloud_segments as CS
    _ns, _h, _sid, _ids, clouds = scene
    boxes = clouds.upright_boxes()
    torch.cuda.synchronize()
    previous = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            corners, yaw = CS.upright_corners(boxes), CS.upright_yaw(boxes)
    finally:
        torch.cuda.set_sync_debug_mode(previous)
    assert [str(w.message) for w in seen if "synchroniz" in str(w.message)] == []
    assert corners.shape == boxes.shape[:-1] + (8, 3) and yaw.shape == boxes.shape[:-1]
    live = ~torch.isnan(boxes[..., 0])
    centre = corners[live].mean(dim=1)
    assert float((centre - boxes[live][:, :3]).abs().max()) < 1e-9
    assert float(yaw[live].abs().max()) <= np.pi / 2 + 1e-12
