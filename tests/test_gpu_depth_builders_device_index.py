"""The four depth builders with ``MSPA_VISINDEX_DECODE=device``: the visibility index comes from the parquet file's pages as lists on
the GPU (``SceneRowGroups.scene_lists``) instead of ``VisibilityInfoHandler``'s dict of the whole file -- and the JSONL, the
warning files and the annotated JPEGs are byte for byte those of the switch unset.  The split is the one of
tests/test_gpu_visindex_decode.py (``_small_split``), restated."""
import json
import os
import pickle
import random
import shutil
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "multi-spatialmllm_amd")
for p in (PKG, ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

INFO = "data/scannet/scannet_instance_data/scenes_info.pkl"
ENGINES = {"estimation_coor": ("depth_estimation_coor_engine", "DepthEstimationCoorQAEngine"),
           "estimation_dot": ("depth_estimation_dot_engine", "DepthEstimationDotQAEngine"),
           "comparison_coor": ("depth_comparison_coor_engine", "DepthComparisonCoorQAEngine"),
           "comparison_dot": ("depth_comparison_dot_engine", "DepthComparisonDotQAEngine")}
ALL_MAX_SAMPLES = 40            # 40 // 3 + 1 = 14 draws a scene: more than its 5 - 9 images, so every image is drawn


def _small_split(root):
    """Three small scenes on disk in the reference's layout (3 scenes, 96 x 128 frames, 5 - 9 frames, 3 000 - 4 400 points), the
    furniture boxes as labelled objects."""
    from mspa import synth
    scenes = [synth.make_scene(9400 + k, n_points=3000 + 700 * k, n_frames=5 + 2 * k, color_hw=(96, 128), depth_hw=(96, 128),
                               invalid_pose_frac=0.0, with_color=False, scene_id=f"scene{9400 + k:04d}_00") for k in range(3)]
    paths = synth.write_scannet_layout(scenes, os.path.join(root, "data", "scannet"), jpeg_for_every_image=True)
    with open(paths["info_path"], "rb") as f:
        infos = pickle.load(f)
    for sc in scenes:
        idx, bbox, cat = sc.objects()
        mask = np.zeros(sc.points.shape[0], dtype=np.int64)
        for o, pts in idx.items():
            mask[pts] = o + 1
        np.save(os.path.join(paths["instance_data_root"], sc.scene_id, "instance_mask.npy"), mask)
        infos[sc.scene_id]["num_objects"] = 8
        for o in range(8):
            infos[sc.scene_id][o] = {"raw_category": "wall" if o == 7 else cat.get(o, f"thing{o}")}
            if o in bbox:
                infos[sc.scene_id][o]["aligned_bbox"] = np.append(np.asarray(bbox[o], dtype=np.float64), 0.0)
    with open(paths["info_path"], "wb") as f:
        pickle.dump(infos, f)
    return scenes


def _own_spatial_engine():
    for name in [m for m in sys.modules if m == "spatial_engine" or m.startswith("spatial_engine.")]:
        if not (getattr(sys.modules[name], "__file__", None) or "").startswith(PKG):
            del sys.modules[name]


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    """(root, scenes): the split and its index -- ``vis.parquet`` by ``make_visibility_info.run_split``, ``vis.pkl`` the same as a
    nested dict, ``vis_defaults.parquet`` rewritten with pyarrow's defaults (dictionary-coded), ``vis_duplicate.parquet`` with one
    image row's list holding one element twice, ``vis_gap.parquet`` with one image row removed."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    root = str(tmp_path_factory.mktemp("depth_split"))
    scenes = _small_split(root)
    here = os.getcwd()
    was = {k: os.environ.pop(k, None) for k in ("MSPA_VISINDEX_DECODE", "MSPA_VISINDEX_ENCODE")}
    os.chdir(root)
    try:
        _own_spatial_engine()
        import spatial_engine.utils.scannet_utils.make_visibility_info as MVI
        MVI.run_split(INFO, "vis.parquet", "mvi_warn.txt", num_workers=2)
        MVI.run_split(INFO, "vis.pkl", "mvi_warn_pkl.txt", num_workers=2)
        t = pq.read_table("vis.parquet")
        pq.write_table(t, "vis_defaults.parquet")
        keys, values = t.column("key").to_pylist(), t.column("values").to_pylist()
        at = keys.index(f"{scenes[0].scene_id}:image_to_points:{scenes[0].valid_image_ids[1]}")
        seen = json.loads(values[at])
        assert len(seen) > 10
        values[at] = json.dumps(seen[:4] + [seen[3]] + seen[4:])              # one vertex twice: a list still, no bitset's row
        pq.write_table(pa.table({"key": pa.array(keys, pa.string()), "values": pa.array(values, pa.string())}), "vis_duplicate.parquet",
                       use_dictionary=False, data_page_size=1 << 16)
        gone = f"{scenes[1].scene_id}:image_to_points:{scenes[1].valid_image_ids[2]}"
        pq.write_table(t.filter(pa.array([k != gone for k in keys])), "vis_gap.parquet", use_dictionary=False, data_page_size=1 << 16)
    finally:
        os.chdir(here)
        os.environ.update({k: v for k, v in was.items() if v is not None})
    return root, scenes


def _engine(which, index_file, out):
    import importlib
    _own_spatial_engine()
    module, cls = ENGINES[which]
    mod = importlib.import_module(f"spatial_engine.depth_perception.{module}")
    return getattr(mod, cls)(INFO, "v1_0", ALL_MAX_SAMPLES, os.path.join(out, "images"), index_file, warning_file=os.path.join(out, "warn.txt"))


def _tree(directory):
    """{relative path: bytes} of every file under ``directory``."""
    out = {}
    for base, _dirs, names in os.walk(directory):
        for n in names:
            with open(os.path.join(base, n), "rb") as f:
                out[os.path.relpath(os.path.join(base, n), directory)] = f.read()
    return out


def _build(which, index_file, out, mode, monkeypatch):
    """Eval and training data of engine ``which`` into ``out`` (emptied first: both modes write the same names) -> every file
    written, the generator's end state, the engine."""
    import pandas as pd
    shutil.rmtree(out, ignore_errors=True)
    os.makedirs(out)
    with monkeypatch.context() as m:
        if mode == "device":
            m.setenv("MSPA_VISINDEX_DECODE", "device")

            def never(*a, **k):
                raise AssertionError("pandas.read_parquet in device mode")
            m.setattr(pd, "read_parquet", never)
        else:
            m.delenv("MSPA_VISINDEX_DECODE", raising=False)
        eng = _engine(which, index_file, out)
        random.seed(17)
        np.random.seed(17)
        eng.generate_qa_eval_data(os.path.join(out, "val"))
        eng.generate_qa_training_data(os.path.join(out, "train"))
    return _tree(out), random.getstate(), eng


@pytest.mark.parametrize("index_file", ["vis.parquet", "vis_defaults.parquet", "vis_duplicate.parquet"])
@pytest.mark.parametrize("which", list(ENGINES))
def test_builders_write_the_same_bytes_with_the_switch_set_and_unset(split, monkeypatch, which, index_file):
    from mspa import visindex
    root, _ = split
    monkeypatch.chdir(root)
    out = os.path.join(root, f"out_{which}")
    host, host_state, eng = _build(which, index_file, out, "host", monkeypatch)
    assert eng.index_lists is None and eng.visibility_info is not None
    device, device_state, eng = _build(which, index_file, out, "device", monkeypatch)
    assert isinstance(eng.index_lists, visindex.SceneRowGroups) and eng.visibility_info is None and eng.index_lists.page_kinds == "any"
    stats = eng.index_lists.decode_stats
    assert stats["scenes"] > 0 and stats["scenes_declined"] == 0 and stats["rows_declined"] == 0, (stats, eng.index_lists.last_decline)
    assert (stats["dict_pages"] > 0) == (index_file == "vis_defaults.parquet")
    assert len(eng._scene_lists_cache) <= 2
    name = eng.task_name
    assert sorted(host) == sorted(device) and f"val/{name}.jsonl" in host and f"train/{name}.jsonl" in host
    for path in host:                                                         # JSONL, warning file, annotated JPEGs
        assert host[path] == device[path], path
    assert host_state == device_state
    assert host[f"train/{name}.jsonl"].count(b"\n") >= 10
    assert any(p.endswith("_annotated.jpg") for p in host) == which.endswith("dot")


def test_a_missing_key_raises_at_the_same_draw(split, monkeypatch):
    root, scenes = split
    monkeypatch.chdir(root)
    message = f"Key {scenes[1].scene_id}:image_to_points:{scenes[1].valid_image_ids[2]} not found in visibility info."
    for which in ENGINES:
        states = {}
        for mode in ("host", "device"):
            with pytest.raises(ValueError) as e:
                _build(which, "vis_gap.parquet", os.path.join(root, f"gap_{which}"), mode, monkeypatch)
            assert str(e.value) == message
            states[mode] = random.getstate()
        assert states["host"] == states["device"], which


def test_sharded_builds_in_process_give_the_unsharded_host_lines(split, monkeypatch):
    import socket
    import torch
    from mspa import shard
    root, _ = split
    monkeypatch.chdir(root)
    monkeypatch.delenv("MSPA_VISINDEX_DECODE", raising=False)
    want = {}
    for which in ("estimation_coor", "comparison_dot"):                      # the unsharded host run, scene after scene
        out = os.path.join(root, f"shard_host_{which}")
        shutil.rmtree(out, ignore_errors=True)
        eng = _engine(which, "vis.parquet", out)
        eng.max_samples = 6
        random.seed(23)
        records = [r for s in eng.scene_info.get_sorted_keys() for r in eng.generate_qa_training_single_scene(s)]
        want[which] = ([json.dumps(r).encode() for r in records], random.getstate(), _tree(out))
        assert len(records) >= 10
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    for k, v in dict(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port)).items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("MSPA_VISINDEX_DECODE", "device")
    ctx = shard.init_distributed(torch.device("cuda", 0), backend="gloo")     # a world of one: no process is spawned
    try:
        assert ctx.world == 1
        for which, sharded in (("estimation_coor", "_sharded_scene_records"), ("comparison_dot", "_chained_scene_records")):
            out = os.path.join(root, f"shard_host_{which}")                   # the same names: the records carry them
            shutil.rmtree(out, ignore_errors=True)
            eng = _engine(which, "vis.parquet", out)
            assert eng.index_lists is not None
            eng.max_samples = 6
            random.seed(23)
            lines = getattr(eng, sharded)(eng.scene_info.get_sorted_keys(), ctx, num_workers=2)
            assert [bytes(line) for line in lines] == want[which][0], which
            assert random.getstate() == want[which][1] and _tree(out) == want[which][2]
            assert eng.index_lists.decode_stats["scenes"] > 0 and eng.index_lists.decode_stats["scenes_declined"] == 0
    finally:
        ctx.close()


def test_the_switch(split, monkeypatch):
    root, _ = split
    monkeypatch.chdir(root)
    monkeypatch.setenv("MSPA_VISINDEX_DECODE", "device")
    eng = _engine("estimation_coor", "vis.pkl", os.path.join(root, "switch"))  # a .pkl index: the handler, whatever the switch says
    assert eng.index_lists is None and type(eng.visibility_info).__name__ == "VisibilityInfoHandler"
    random.seed(5)
    assert len(eng.generate_qa_training_data(os.path.join(root, "switch", "train"), save_file=False)) >= 10
    monkeypatch.setenv("MSPA_VISINDEX_DECODE", "gpu")
    for index_file in ("vis.parquet", "vis.pkl"):
        with pytest.raises(ValueError, match="MSPA_VISINDEX_DECODE"):
            _engine("comparison_coor", index_file, os.path.join(root, "switch"))
