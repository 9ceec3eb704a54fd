"""The visibility index's way back on the MI355X: the device Snappy decoder against mspa_snappy_decompress_host,
``visindex.SceneRowGroups.scene_bits`` against ``pack_index_lists([json.loads(...)])`` on every file of the CPU page test, the
edge rows, and the two consumers with ``MSPA_VISINDEX_DECODE=device`` against the switch unset.

The corrupt streams reach the GPU only behind tests/test_snappy_decode_cpu.py's sanitizer run of the same rules on the CPU."""
import json
import os
import pickle
import random
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "multi-spatialmllm_amd")
for p in (PKG, ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import visindex_decode_util as VU  # noqa: E402

SENTINEL, GAP = 0xAB, 32


def _decode_batch(cases):
    """cases: [(stream, expected size)] -> (status [n], outputs [n] (bytes), the gaps between the spans all still SENTINEL) by ONE
    mspa_snappy_decompress_device launch.  Streams lie back to back in src, except that every third one shares its bytes with
    a second table entry that reads them again (overlapping streams) -- the caller sees the entries of ``cases`` only."""
    import torch
    from mspa import _lib
    lib = _lib.load()
    src = np.frombuffer(b"".join(s for s, _ in cases) or b"\0", dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(s) for s, _ in cases])]).astype(np.int64)
    entries = [(int(offs[k]), len(s), e) for k, (s, e) in enumerate(cases)]
    again = [entries[k] for k in range(0, len(entries), 3)]
    table = entries + again
    out_off, pos = [], GAP
    for _o, _n, e in table:
        out_off.append(pos)
        pos += e + GAP
    dev = "cuda"
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int64)).to(dev)
    src_dev = torch.from_numpy(src.copy()).to(dev)
    out = torch.full((pos,), SENTINEL, dtype=torch.uint8, device=dev)
    status = torch.full((len(table),), 99, dtype=torch.int32, device=dev)
    o, n, sz, oo = t([e[0] for e in table]), t([e[1] for e in table]), t([e[2] for e in table]), t(out_off)
    rc = lib.mspa_snappy_decompress_device(src_dev.data_ptr(), len(b"".join(s for s, _ in cases)), o.data_ptr(), n.data_ptr(), len(table),
                                           out.data_ptr(), pos, oo.data_ptr(), sz.data_ptr(), status.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    host, st = out.cpu().numpy(), status.cpu().numpy()
    keep = np.ones(pos, dtype=bool)
    outs = []
    for at, (_o, _n, e) in zip(out_off, table):
        keep[at:at + e] = False
        outs.append(host[at:at + e].tobytes())
    gaps_intact = bool((host[keep] == SENTINEL).all())
    for k, j in enumerate(range(0, len(entries), 3)):                          # the second reading of a stream gives the same
        assert st[len(entries) + k] == st[j] and (st[j] != 0 or outs[len(entries) + k] == outs[j])
    return st[:len(entries)], outs[:len(entries)], gaps_intact


def test_device_decoder_equals_the_host_on_the_whole_stream_set_in_one_launch():
    from mspa import _lib
    lib = _lib.load()
    valid = VU.valid_streams()
    assert max(len(d) for _, _, d in valid) == 131079 and any(len(d) == 0 for _, _, d in valid)
    assert any(n.startswith("pa_") for n, _, _ in valid) and any(n.startswith("own_") for n, _, _ in valid)
    status, outs, gaps_intact = _decode_batch([(s, len(d)) for _, s, d in valid])
    assert gaps_intact
    for (name, stream, data), st, got in zip(valid, status, outs):
        rc, want = VU.decompress_host(lib, stream, len(data))
        assert rc == len(data) and want == data
        if name == VU.FAR_NAME:                                                # reaches back more than 64 KiB: equal, or declined
            assert st != 0 or got == want, name
        else:
            assert st == 0 and got == want, (name, int(st))


def test_corrupt_streams_are_declined_with_the_hosts_code_and_their_neighbours_stay_intact():
    from mspa import _lib
    lib = _lib.load()
    corrupt = VU.corrupt_streams()
    good = [(s, d) for n, s, d in VU.valid_streams() if n in ("own_json", "pa_json", "hand_copy4", "pa_p7_65537", "hand_empty")]
    assert len(good) == 5
    cases, kinds = [], []
    for k, (name, stream, expected, code) in enumerate(corrupt):
        s, d = good[k % len(good)]
        cases += [(s, len(d)), (stream, expected)]
        kinds += [("good", d), ("bad", (name, stream, expected, code))]
    cases.append((good[0][0], len(good[0][1])))
    kinds.append(("good", good[0][1]))
    status, outs, gaps_intact = _decode_batch(cases)
    assert gaps_intact                                                        # nothing outside any stream's own span
    for (kind, what), st, got in zip(kinds, status, outs):
        if kind == "good":
            assert st == 0 and got == what
        else:
            name, stream, expected, code = what
            assert VU.decompress_host(lib, stream, expected)[0] == code and st == code, (name, int(st), code)


def test_engine_wrapper_tables_and_wrong_arguments():
    import torch
    from mspa import _lib, engine
    lib = _lib.load()
    pick = [(s, d) for n, s, d in VU.valid_streams() if n in ("own_json", "hand_empty", "pa_noise65537", "hand_ring_edges")]
    src = torch.from_numpy(np.frombuffer(b"".join(s for s, _ in pick), dtype=np.uint8).copy()).cuda()
    lens = [len(s) for s, _ in pick]
    offs = torch.tensor(np.concatenate([[0], np.cumsum(lens)[:-1]]), dtype=torch.int64, device="cuda")
    nbytes = torch.tensor(lens, dtype=torch.int64, device="cuda")
    sizes = torch.tensor([len(d) for _, d in pick], dtype=torch.int64, device="cuda")
    out, out_off, status = engine.snappy_decompress_device(src, offs, nbytes, sizes)
    assert status.tolist() == [0] * len(pick) and out.cpu().numpy().tobytes() == b"".join(d for _, d in pick)
    assert out_off.tolist() == np.concatenate([[0], np.cumsum([len(d) for _, d in pick])]).tolist()
    # a table entry outside src: that stream alone is refused, nothing of it is touched
    bad_n = nbytes.clone()
    bad_n[0] = src.numel() + 1
    _, _, status = engine.snappy_decompress_device(src, offs, bad_n, sizes)
    assert status.tolist() == [_lib.MSPA_EINVAL, 0, 0, 0]
    with pytest.raises(ValueError):
        engine.snappy_decompress_device(src.cpu(), offs, nbytes, sizes)
    with pytest.raises(ValueError):
        engine.snappy_decompress_device(src, offs, nbytes, sizes[:2])
    st = torch.zeros(4, dtype=torch.int32, device="cuda")
    assert lib.mspa_snappy_decompress_device(src.data_ptr(), src.numel(), None, nbytes.data_ptr(), 4, out.data_ptr(), out.numel(), out_off.data_ptr(),
                                             sizes.data_ptr(), st.data_ptr(), None) == _lib.MSPA_EINVAL
    assert lib.mspa_snappy_decompress_device(src.data_ptr(), -1, offs.data_ptr(), nbytes.data_ptr(), 4, out.data_ptr(), out.numel(),
                                             out_off.data_ptr(), sizes.data_ptr(), st.data_ptr(), None) == _lib.MSPA_EINVAL


# ------------------------------------------------------------------------------------------------------------------- scene_bits
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return VU.index_files(tmp_path_factory.mktemp("index_files"))


NAMES = ("many_pages", "page_per_row", "uncompressed", "defaults", "v2", "two_scenes", "two_groups", "split_images", "assembled")


@pytest.mark.parametrize("name", NAMES)
def test_scene_bits_equals_json_loads_and_pack_index_lists(files, name):
    from mspa import visindex
    path, scenes, device_takes = files[name]
    index = visindex.SceneRowGroups(path)
    asked = 0
    for scene_id in scenes:
        ids, texts = VU.image_ids_of(path, scene_id)
        n_points = 5000 if scene_id == "scene0000_00" else 3000
        request = [ids[-1], "99999"] + ids[:-1]                               # not in file order, one image the index lacks
        present, bits = index.scene_bits(scene_id, request, n_points)
        assert present == [ids[-1]] + ids[:-1] and bits.is_cuda and str(bits.dtype) == "torch.int64"
        assert np.array_equal(bits.cpu().numpy(), VU.expected_bits(texts, present, n_points))
        present, bits = index.scene_bits(scene_id, ids[:3])                   # the width from the lists themselves
        top = max(max(json.loads(texts[i])) for i in ids[:3])
        assert present == ids[:3] and np.array_equal(bits.cpu().numpy(), VU.expected_bits(texts, present, top + 1))
        asked += 2
    assert index.decode_stats["scenes"] == asked
    assert index.decode_stats["scenes_declined"] == (0 if device_takes else asked), index.last_decline
    assert index.decode_stats["rows_declined"] == 0
    assert (index.decode_stats["h2d_bytes"] > 0) == device_takes
    present, bits = index.scene_bits("scene0000_00", ["99999"], 5000)         # nothing of the request is there
    assert present == [] and tuple(bits.shape) == (0, 79)
    present, bits = index.scene_bits("scene4040_00", ["00000"], 5000)         # a scene the index lacks
    assert present == []


EDGE_ROWS = {
    "empty": "[]",
    "duplicate": "[1, 1, 5, 5, 5, 700]",
    "descending": "[5, 3]",
    "bit63": "[0, 63, 64, 127, 128, 65471]",
    "spaces": " [ 1,2 ,\n3,\t64 ] ",
    "negative": "[-1]",
    "one": "[7]",
    "long": json.dumps(list(range(1, 60001, 2))),                             # 190 KB of text behind 4 KiB pages
}


def _edge_file(directory, n_points):
    import pyarrow as pa
    import pyarrow.parquet as pq
    rows = dict(EDGE_ROWS)
    rows["last"] = json.dumps([0, n_points - 1])                              # the last vertex
    if n_points % 64:
        rows["beyond"] = json.dumps([3, n_points])                            # >= n_points, still inside the row's last word
    keys = [f"sceneE:image_to_points:{k}" for k in rows] + [f"sceneE:point_to_images:{v}" for v in range(40)]
    values = list(rows.values()) + ['["empty"]'] * 40
    path = os.path.join(str(directory), f"edge_{n_points}.parquet")
    pq.write_table(pa.table({"key": pa.array(keys, pa.string()), "values": pa.array(values, pa.string())}), path, use_dictionary=False,
                   data_page_size=4096, write_batch_size=1)
    return path, rows


@pytest.mark.parametrize("n_points", [65535, 65536, 65537])
def test_edge_rows_decline_alone_and_the_result_is_the_host_paths(tmp_path, n_points):
    from mspa import visindex
    from mspa.scene import pack_index_lists
    path, rows = _edge_file(tmp_path, n_points)
    index = visindex.SceneRowGroups(path)
    request = ["long", "absent"] + [k for k in rows if k != "long"]
    present, bits = index.scene_bits("sceneE", request, n_points)
    assert present == [k for k in request if k != "absent"]
    want = pack_index_lists([json.loads(rows[k]) for k in present], n_points)
    got = bits.cpu().numpy()
    for r, k in enumerate(present):
        assert np.array_equal(got[r], want[r]), k
    assert want[present.index("bit63"), 0] == np.int64(-(2 ** 63) + 1) and want.shape[1] == (n_points + 63) // 64
    declined = {"descending", "negative"} | ({"beyond"} if "beyond" in rows else set())
    assert index.decode_stats["scenes_declined"] == 0 and index.decode_stats["rows_declined"] == len(declined), index.decode_stats
    assert index.decode_stats["rows"] == len(present)
    # without a width: 1 + the largest index of these lists, the declined rows' included
    sub = ["descending", "one", "empty"]
    present, bits = index.scene_bits("sceneE", sub)
    assert np.array_equal(bits.cpu().numpy(), pack_index_lists([json.loads(rows[k]) for k in sub], 8))
    present, bits = index.scene_bits("sceneE", ["empty"])
    assert tuple(bits.shape) == (1, 1) and int(bits.sum()) == 0
    present, bits = index.scene_bits("sceneE", ["one"])                       # one page, one row, one value: tables of one entry
    assert np.array_equal(bits.cpu().numpy(), pack_index_lists([[7]], 8)) and index.decode_stats["rows_declined"] == len(declined) + 1
    # (in the file an empty row stands in front of a non-empty one: "empty", "duplicate")
    assert list(rows)[:2] == ["empty", "duplicate"]


# ------------------------------------------------------------------------------------------------------------------- end to end
def _small_split(root):
    """Three small scenes on disk the way tests/test_gpu_sweep.py writes its split: the reference's layout, the furniture boxes
    as labelled objects; then the index by ``make_visibility_info.run_split``."""
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


def _read(path, mode="rb"):
    with open(path, mode) as f:
        return f.read()


def test_consumers_write_the_same_files_with_the_switch_set_and_unset(tmp_path, monkeypatch):
    import pyarrow as pa
    import pyarrow.parquet as pq
    root = str(tmp_path)
    scenes = _small_split(root)
    monkeypatch.chdir(root)
    monkeypatch.delenv("MSPA_VISINDEX_DECODE", raising=False)
    monkeypatch.delenv("MSPA_VISINDEX_ENCODE", raising=False)
    for name in [m for m in sys.modules if m == "spatial_engine" or m.startswith("spatial_engine.")]:
        if not (getattr(sys.modules[name], "__file__", None) or "").startswith(PKG):
            del sys.modules[name]
    import spatial_engine.utils.scannet_utils.make_visibility_info as MVI
    import spatial_engine.object_perception.compute_object_visibility as COV
    import spatial_engine.object_perception.single_object_coverage_finder as SOC
    from spatial_engine.utils.scannet_utils.handler.info_handler import SceneInfoHandler
    from mspa import visindex
    info = "data/scannet/scannet_instance_data/scenes_info.pkl"
    MVI.run_split(info, "vis.parquet", "mvi_warn.txt", num_workers=2)
    # the same index with one image of the second scene missing, as ONE row group that mixes the scenes
    t = pq.read_table("vis.parquet")
    gone = f"{scenes[1].scene_id}:image_to_points:{scenes[1].valid_image_ids[2]}"
    keep = [k != gone for k in t.column("key").to_pylist()]
    pq.write_table(t.filter(pa.array(keep)), "vis_gap.parquet", use_dictionary=False, data_page_size=1 << 16)
    handler = SceneInfoHandler(info)
    for index_file in ("vis.parquet", "vis_gap.parquet"):
        outs = {}
        for mode in ("host", "device"):
            if mode == "device":
                monkeypatch.setenv("MSPA_VISINDEX_DECODE", "device")
            else:
                monkeypatch.delenv("MSPA_VISINDEX_DECODE", raising=False)
            out = os.path.join(root, f"covis_{index_file}_{mode}")
            COV.process_split("val", info, index_file, out)
            with open(os.path.join(out, "object_visibility.pkl"), "rb") as f:
                obj_vis = pickle.load(f)
            handler_m, index, _ = SOC._load_inputs(info, index_file, os.path.join(out, "object_visibility.pkl"))
            assert isinstance(index, visindex.SceneRowGroups) == (mode == "device")
            random.seed(0)
            tables = SOC._run_scenes(handler.get_all_scene_ids(), handler_m, index, obj_vis)
            random.seed(0)
            one = SOC.process_object(scenes[0].scene_id, next(iter(obj_vis[scenes[0].scene_id]["object_to_images"])), handler_m,
                                     scenes[0].valid_image_ids[:4] + ["absent"], index)
            outs[mode] = (_read(os.path.join(out, "object_visibility.pkl")), _read(os.path.join(out, "warning.txt")), tables, one)
            if mode == "device":
                assert index.decode_stats["scenes"] > 0 and index.decode_stats["scenes_declined"] == 0, index.last_decline
        assert outs["host"][0] == outs["device"][0] and outs["host"][1] == outs["device"][1]
        assert outs["host"][2] == outs["device"][2] and outs["host"][3] == outs["device"][3]
        assert any(outs["host"][2][dim] for dim in outs["host"][2])
        assert (b"not found in visibility dict" in outs["host"][1]) == (index_file == "vis_gap.parquet")
    monkeypatch.setenv("MSPA_VISINDEX_DECODE", "gpu")
    with pytest.raises(ValueError, match="MSPA_VISINDEX_DECODE"):
        COV.process_split("val", info, "vis.parquet", os.path.join(root, "never"))
    with pytest.raises(ValueError, match="MSPA_VISINDEX_DECODE"):
        SOC._load_inputs(info, "vis.parquet", os.path.join(root, "covis_vis.parquet_host", "object_visibility.pkl"))
