"""The dot heads with DeviceAnnotator against PillowAnnotator on the MI355X: the same seed gives the same JSONL / records and
byte-identical image trees.  Covers VC_D's dataset build and its single-row entry point (which renames the files right after
the records are built), and the object-movement dot engine on a scene whose frames recur, so that ``needs()`` answers from the
annotator's pending jobs."""
import importlib
import io
import json
import os
import pickle
import random
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from jpeg_util import content  # noqa: E402

from mspa import synth  # noqa: E402
from mspa.annotate import DeviceAnnotator, PillowAnnotator  # noqa: E402
from mspa.scene import SceneOnDevice  # noqa: E402

DEV = "cuda"


def _tree(d):
    files = {}
    for root, _, names in os.walk(d):
        for n in names:
            with open(os.path.join(root, n), "rb") as f:
                files[os.path.relpath(os.path.join(root, n), d)] = f.read()
    return files


def _scannet_like(tmp_path):
    """Two synthetic scenes with real colour JPEGs on disk, their pair table and visibility index (as test_gpu_heads.py's
    correspondence facade test builds them)."""
    from PIL import Image
    pd = pytest.importorskip("pandas")
    pytest.importorskip("pyarrow")
    IMG = importlib.import_module("spatial_engine.utils.scannet_utils.handler._images")
    IH = importlib.import_module("spatial_engine.utils.scannet_utils.handler.info_handler")
    scenes = [synth.make_scene(7600 + k, n_points=3000, n_frames=9, color_hw=(96, 128), depth_hw=(96, 128),
                               invalid_pose_frac=0.1, with_color=False) for k in range(2)]
    posed, inst = str(tmp_path / "posed_images"), str(tmp_path / "inst")
    infos, vis_all, table_rows = {}, {}, []
    for n, sc in enumerate(scenes):
        os.makedirs(os.path.join(inst, sc.scene_id), exist_ok=True)
        os.makedirs(os.path.join(posed, sc.scene_id), exist_ok=True)
        np.save(os.path.join(inst, sc.scene_id, "aligned_points.npy"), sc.points)
        for k, i in enumerate(sc.image_ids):
            jpg = os.path.join(posed, sc.scene_id, f"{i}.jpg")
            Image.fromarray(content(*sc.color_hw, 10 * n + k)).save(jpg, quality=90)
            IMG.register(os.path.join(posed, sc.scene_id, f"{i}.png"), sc.depth[i])
        infos[sc.scene_id] = sc.info_dict()
        resident = SceneOnDevice(sc.K, sc.A, sc.E, sc.depth, sc.color_hw, sc.points, DEV)
        vis_all[sc.scene_id] = resident.visibility_index()
        for (a, b), v in resident.frames_relations().items():
            table_rows.append({"scene_id": sc.scene_id, "image_id1": a, "image_id2": b, "overlap": float(v["overlap"]),
                               "distance": float(v["distance"]), "yaw": float(v["yaw"]), "pitch": float(v["pitch"])})
    info_path, vis_path, table_path = str(tmp_path / "infos.pkl"), str(tmp_path / "vis.pkl"), str(tmp_path / "pairs.parquet")
    with open(info_path, "wb") as f:
        pickle.dump(infos, f)
    with open(vis_path, "wb") as f:
        pickle.dump(vis_all, f)
    pd.DataFrame(table_rows).to_parquet(table_path)
    return IH.SceneInfoHandler(info_path, posed_images_root=posed, instance_data_root=inst), vis_path, table_path, vis_all


def test_visual_correspondence_dot_build_device_equals_pillow(tmp_path, monkeypatch):
    import pandas as pd
    VD = importlib.import_module("spatial_engine.visual_correspondence.visual_correspondence_qa_engine_dot_2_multichoice")
    h, vis_path, table_path, vis_all = _scannet_like(tmp_path)
    results = {}
    for name, annotator in (("pillow", PillowAnnotator()), ("device", DeviceAnnotator())):
        monkeypatch.setattr(VD, "ANNOTATOR", annotator)
        out = str(tmp_path / name)
        os.makedirs(out)
        warn = str(tmp_path / f"{name}_w.txt")
        open(warn, "w").close()
        random.seed(61); np.random.seed(61)
        VD.build_train_dataset(table_path, out, h, 24, 1, 60, 1, vis_path, warn)
        with open(os.path.join(out, "train_visual_correspondence_dot_2_multichoice.jsonl")) as f:
            text = f.read().replace(out, "<out>")
        # the single-row entry point renames its two files as soon as the records are built
        random.seed(62)
        sampled = VD.sample_dataframe(pd.read_parquet(table_path), all_overlap_samples=24, non_overlap_samples=0, overlap_min=1,
                                      overlap_max=60, interval=1)
        one = None
        for k in range(len(sampled)):
            one = VD.build_training_sample(h, sampled.iloc[k], 37 + k, vis_all, warn, image_output_dir=os.path.join(out, "dbg"))
            if one is not None:
                break
        assert one is not None
        if isinstance(annotator, DeviceAnnotator):
            assert not annotator._jobs, "a record function returned with jobs still queued"
        results[name] = (text, json.dumps(one).replace(out, "<out>"), _tree(out))
    (pt, po, ptree), (dt, do, dtree) = results["pillow"], results["device"]
    assert pt == dt and po == do
    records = [json.loads(line) for line in pt.splitlines()]
    assert len(records) >= 8
    assert sorted(ptree) == sorted(dtree) and sum(k.endswith(".jpg") for k in ptree) >= 2 * len(records) + 2
    for k in ptree:
        assert dtree[k] == ptree[k], k


class _CountingDevice(DeviceAnnotator):
    """Counts the ``pending()`` answers that were True: the draws that relied on a queued, not yet written, file."""
    hits = 0

    def pending(self, dst):
        p = super().pending(dst)
        self.hits += bool(p)
        return p


def test_object_movement_dot_device_equals_pillow(tmp_path):
    from PIL import Image
    OMD = importlib.import_module("spatial_engine.object_movement.single_object_movement_engine_dot")
    tr = synth.make_tracks(33, T=150, P=64, n_groups=4)
    H, W = tr.image_hw
    payloads = []
    for t in range(tr.tracks_XYZ.shape[0]):
        b = io.BytesIO()
        Image.fromarray(content(H, W, t % 7)).save(b, "JPEG", quality=85)
        payloads.append(b.getvalue())
    (tmp_path / "src").mkdir()
    path = str(tmp_path / "src" / f"{tr.scene_id}.npz")
    np.savez(path, images_jpeg_bytes=np.array(payloads, dtype=object), tracks_XYZ=tr.tracks_XYZ, visibility=tr.visibility,
             fx_fy_cx_cy=tr.fx_fy_cx_cy, extrinsics_w2c=tr.extrinsics_w2c)
    results = {}
    for name, annotator in (("pillow", PillowAnnotator()), ("device", _CountingDevice())):
        eng = OMD.TwoFrameVideoQAEngineDot("tapvid3d_total_distance", "adt")
        eng.annotator = annotator
        img = str(tmp_path / name / "img")
        random.seed(71)
        recs = eng.generate_qa_training_single_scene(path, str(tmp_path / name / "base"), 6, 5, img, True, 0.5)
        after = random.random()                   # the generator's state after the build: equal only if every draw was
        results[name] = (json.dumps(recs).replace(str(tmp_path / name), "<dir>"), after, _tree(img))
        if name == "device":
            assert annotator.hits > 0, "no frame recurred: needs() never answered from a pending job"
            assert not annotator._jobs
    (pr, pa, ptree), (dr, da, dtree) = results["pillow"], results["device"]
    assert pr == dr and pa == da
    assert len(json.loads(pr)) > 20
    assert sorted(ptree) == sorted(dtree) and len(ptree) > 10
    for k in ptree:
        assert dtree[k] == ptree[k], k
