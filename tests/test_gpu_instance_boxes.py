"""Cleaned clouds, boxes and IoU of every object of a scene at once (``InstanceClouds.cleaned`` / ``boxes`` / ``by_object`` /
``cleaned_objects``, ``SceneInfoHandler.instance_boxes``) against the loop a user writes with the single-cloud functions of
handler/ops.py -- on the three-frame scene of tests/golden/instance_clouds.npz and on a synthetic scene of four frames.  Every
comparison of kept rows stands behind the guard of tests/cloud_segments_util.py on the scene's own clouds."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_segments_util as U  # noqa: E402
from test_gpu_facade import facade  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "instance_clouds.npz")
NB, RATIO = 20, 1.0


def _annotate(h, sid, clouds, n_objects):
    """Ground-truth boxes [cx, cy, cz, dx, dy, dz, class] for objects 0 .. n_objects - 1: near the object's own points where the
    masks show it (shifted and shrunk, so the IoU is strictly between 0 and 1), far away for every third one (IoU 0)."""
    h.infos[sid]["num_objects"] = n_objects
    for t in range(n_objects):
        pts = clouds.object_cloud(t)[:, :3].cpu().numpy()
        if len(pts) and t % 3 != 2:
            lo, hi = pts.min(axis=0), pts.max(axis=0)
            box = np.concatenate([(lo + hi) / 2 + 0.07 * (hi - lo), 0.8 * (hi - lo) + 0.05, [1.0]])
        else:
            box = np.array([50.0 + t, -40.0, 30.0, 1.0, 2.0, 3.0, 1.0])
        h.infos[sid][t] = {"aligned_bbox": box}


def _golden_scene(root):
    from test_gpu_instance_clouds import SID, _layout
    ns = facade()
    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    h, ids = _layout(ns, g, root)
    return ns, h, SID, ids, True, 7                                         # target 7 is shown by the masks but is no annotated object


def _synth_scene(root):
    import pickle
    from PIL import Image
    from mspa import synth
    ns = facade()
    sc = synth.make_scene(41, n_points=256, n_frames=4, color_hw=(240, 320), depth_hw=(120, 160), invalid_pose_frac=0.0, with_color=False,
                          scene_id="scene0941_00")
    where = synth.write_scannet_layout([sc], root, jpeg_for_every_image=True)
    scans = os.path.join(root, "scans")
    os.makedirs(os.path.join(scans, sc.scene_id, "instance-filt"))
    rng = np.random.default_rng(6)
    for i in sc.image_ids:
        m = np.zeros((240, 320), np.uint8)
        for v in rng.permutation(np.arange(1, 7)):
            y, x = int(rng.integers(0, 200)), int(rng.integers(0, 280))
            m[y:y + int(rng.integers(20, 110)), x:x + int(rng.integers(20, 140))] = v
        Image.fromarray(m, mode="L").save(os.path.join(scans, sc.scene_id, "instance-filt", f"{int(i)}.png"))
    infos = pickle.load(open(where["info_path"], "rb"))
    h = ns.IH.SceneInfoHandler(infos, posed_images_root=where["posed_images_root"], instance_data_root=where["instance_data_root"],
                               mask_image_root=scans)
    return ns, h, sc.scene_id, list(sc.image_ids), False, 5                # label 6 (target 5) is shown but not annotated


@pytest.fixture(scope="module", params=["golden", "synth"])
def scene(request, tmp_path_factory):
    """(façade, handler, scene id, image ids, clouds, cleaned): built once per scene; the guard is asserted here, first."""
    from mspa import instances
    root = str(tmp_path_factory.mktemp("instance_boxes_" + request.param))
    ns, h, sid, ids, with_color, n_objects = (_golden_scene if request.param == "golden" else _synth_scene)(root)
    clouds = h.instance_clouds(sid, with_color=with_color)
    _annotate(h, sid, clouds, n_objects)
    assert instances.LAST_INSTANCE_CLOUDS["path"] == "device", instances.LAST_INSTANCE_CLOUDS
    U.assert_guard_on_device(clouds.rows, clouds.offsets, NB, RATIO, request.param)
    return ns, h, sid, ids, clouds, clouds.cleaned(NB, RATIO)


def _same(a, b):
    """Equal shapes and equal float64 values, NaN equal to NaN."""
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def test_cleaned_clouds_boxes_and_pixels_equal_the_single_cloud_loop(scene):
    from mspa.instances import InstanceClouds
    ns, h, sid, ids, clouds, cleaned = scene
    assert isinstance(cleaned, InstanceClouds) and cleaned.image_ids == clouds.image_ids and cleaned.counts.shape == clouds.counts.shape
    assert cleaned.with_color == clouds.with_color and cleaned.rows.dtype == torch.float64 and len(cleaned.rows) == cleaned.offsets[-1]
    boxes = cleaned.boxes()
    assert boxes.shape == clouds.counts.shape + (6,) and boxes.is_cuda and boxes.dtype == torch.float64
    seen = np.zeros(clouds.counts.shape, dtype=bool)
    n_boxes = 0
    for k, i in enumerate(ids):
        assert clouds.present(i), i
        for t in clouds.present(i):
            want = ns.OPS.remove_statistical_outliers(clouds.cloud(i, t), NB, RATIO)
            got = cleaned.cloud(i, t)
            assert got.shape == want.shape and torch.equal(got, want), (i, t)
            assert cleaned.count(i, t) == len(want) and (t in cleaned.present(i)) == (len(want) > 0)
            seen[k, t + 1] = True
            if len(want):
                n_boxes += 1
                box = ns.OPS.calculate_aabb(want)
                assert torch.equal(cleaned.aabb(i, t), box) and torch.equal(boxes[k, t + 1], box), (i, t)
            else:
                assert bool(torch.isnan(boxes[k, t + 1]).all())
                with pytest.raises(ValueError):
                    cleaned.aabb(i, t)
            # the pixel indices (and the colours) went through the same selection
            _k, _v, a, b = clouds._segment(i, t)
            _k, _v, ca, cb = cleaned._segment(i, t)
            at = torch.searchsorted(clouds.pixel[a:b].contiguous(), cleaned.pixel[ca:cb].contiguous())
            assert torch.equal(clouds.pixel[a:b][at], cleaned.pixel[ca:cb]) and torch.equal(clouds.rows[a:b][at], got), (i, t)
            if clouds.rgb is not None:
                assert torch.equal(cleaned.rgb[ca:cb], clouds.rgb[a:b][at]) and torch.equal(cleaned.rgb[ca:cb].to(torch.float64), got[:, 3:6])
    assert n_boxes >= 8
    label0 = np.zeros_like(seen)
    label0[:, 0] = True
    assert bool(torch.isnan(boxes[torch.from_numpy(~seen & ~label0).cuda()]).all())        # no rows, no box
    assert not cleaned.counts[~seen & ~label0].any()
    for t in clouds.present(ids[0])[:2]:                                                     # object_cloud works on the cleaned object unchanged
        assert torch.equal(cleaned.object_cloud(t), torch.cat([cleaned.cloud(i, t) for i in ids]))


def test_cleaned_objects_equal_the_fused_single_cloud_loop(scene):
    ns, h, sid, ids, clouds, _cleaned = scene
    rows, offsets, object_ids = clouds.by_object()
    assert object_ids.tolist() == sorted({t for i in ids for t in clouds.present(i)})
    for j, t in enumerate(object_ids):
        assert torch.equal(rows[offsets[j]:offsets[j + 1]], clouds.object_cloud(int(t))), t
    U.assert_guard_on_device(rows, offsets, NB, RATIO, "by_object")
    kept, kept_offsets, kept_ids, boxes = clouds.cleaned_objects(NB, RATIO)
    assert np.array_equal(kept_ids, object_ids) and boxes.shape == (len(object_ids), 6) and kept_offsets[-1] == len(kept)
    for j, t in enumerate(object_ids):
        want = ns.OPS.remove_statistical_outliers(clouds.object_cloud(int(t)), NB, RATIO)
        got = kept[int(kept_offsets[j]):int(kept_offsets[j + 1])]
        assert got.shape == want.shape and torch.equal(got, want), t
        if len(want):
            assert torch.equal(boxes[j], ns.OPS.calculate_aabb(want)), t
        else:
            assert bool(torch.isnan(boxes[j]).all())


def test_instance_boxes_per_image_and_per_object(scene):
    ns, h, sid, ids, clouds, cleaned = scene
    n_objects = h.get_num_objects(sid)
    out = h.instance_boxes(sid, nb_neighbors=NB, std_ratio=RATIO, per="image")
    assert out["image_ids"] == ids and _same(out["boxes"], cleaned.boxes()) and np.array_equal(out["kept"], cleaned.counts)
    assert out["iou"].shape == cleaned.counts.shape and out["iou"].dtype == torch.float64 and out["iou"].is_cuda
    some, positive = 0, 0
    for k, i in enumerate(ids):
        for v in range(cleaned.n_labels):
            t = v - 1
            if cleaned.counts[k, v] and 0 <= t < n_objects:
                gt = np.asarray(h.get_object_gt_bbox(sid, t, axis_aligned=True), dtype=np.float64)[:6]
                want = ns.OPS.calculate_iou_3d(out["boxes"][k, v], gt)
                assert torch.equal(out["iou"][k, v], want), (i, t, float(out["iou"][k, v]), float(want))
                some += 1
                positive += float(want) > 0
            else:                                                               # no box, label 0, or no such object in the annotation
                assert bool(torch.isnan(out["iou"][k, v])), (i, t)
    assert some >= 8 and positive >= 1
    per_object = h.instance_boxes(sid, nb_neighbors=NB, std_ratio=RATIO, per="object")
    _rows, offsets, object_ids, boxes = clouds.cleaned_objects(NB, RATIO)
    assert np.array_equal(per_object["object_ids"], object_ids) and _same(per_object["boxes"], boxes)
    assert np.array_equal(per_object["kept"], np.diff(offsets)) and per_object["iou"].shape == (len(object_ids),)
    for j, t in enumerate(object_ids):
        if per_object["kept"][j] and t < n_objects:
            gt = np.asarray(h.get_object_gt_bbox(sid, int(t), axis_aligned=True), dtype=np.float64)[:6]
            assert torch.equal(per_object["iou"][j], ns.OPS.calculate_iou_3d(boxes[j], gt)), t
        else:
            assert bool(torch.isnan(per_object["iou"][j])), t
    with pytest.raises(ValueError):
        h.instance_boxes(sid, per="frame")
    sub = h.instance_boxes(sid, image_ids=[ids[1]], per="image")
    assert sub["image_ids"] == [ids[1]] and _same(sub["boxes"][0], out["boxes"][1]) and _same(sub["iou"][0], out["iou"][1])


def test_the_host_composition_path_gives_the_same_boxes(scene):
    """A mask registered in memory sends ``instance_clouds`` through the per-object composition; the boxes, the kept counts and the
    IoU are the device path's."""
    from mspa import instances
    ns, h, sid, ids, _clouds, _cleaned = scene
    device = {per: h.instance_boxes(sid, per=per) for per in ("image", "object")}
    path = os.path.join(h.mask_image_root, sid, "instance-filt", f"{int(ids[0])}.png")
    ns.IMG.register(path, np.asarray(ns.IMG.read_depth(path)).copy())
    try:
        for per in ("image", "object"):
            host = h.instance_boxes(sid, per=per)
            assert instances.LAST_INSTANCE_CLOUDS["path"] == "host", instances.LAST_INSTANCE_CLOUDS
            cut = slice(1, None) if per == "image" else slice(None)           # (label 0 is no object: its column is not compared)
            assert np.array_equal(host["kept"][..., cut], device[per]["kept"][..., cut]), per
            if per == "image":
                assert _same(host["boxes"][:, 1:], device[per]["boxes"][:, 1:]) and _same(host["iou"][:, 1:], device[per]["iou"][:, 1:])
            else:
                assert _same(host["boxes"], device[per]["boxes"]) and _same(host["iou"], device[per]["iou"])
            if per == "object":
                assert np.array_equal(host["object_ids"], device[per]["object_ids"])
    finally:
        del ns.IMG.MEMORY[path]
