"""Dictionary-coded and v2 pages of the visibility index on the MI355X: ``SceneRowGroups.scene_bits`` with ``page_kinds = "any"``
against ``pack_index_lists([json.loads(...)])`` on every layout of tests/rle_hybrid_util.py, mspa_parquet_dict_spans_device on
crafted pages (every page status, a good page beside each bad one), rows that share a dictionary entry, a corrupt dictionary
page, and the two consumers on an index written the reference's way (``DataFrame.to_parquet(index=False)``).

The crafted run streams reach the GPU only behind tests/test_rle_hybrid_cpu.py's sanitizer run of the same rules on the CPU."""
import json
import os
import pickle
import random
import struct
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "multi-spatialmllm_amd")
for p in (PKG, ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import rle_hybrid_util as RU  # noqa: E402
import visindex_decode_util as VU  # noqa: E402

NAMES = tuple(RU.LAYOUTS)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return RU.index_files(tmp_path_factory.mktemp("encoded_pages"))


# ------------------------------------------------------------------------------------------------------------------ whole files
@pytest.mark.parametrize("name", NAMES)
def test_scene_bits_takes_every_layout_and_equals_the_host_path(files, name):
    from mspa import visindex
    path = files[name]
    ids, texts = VU.image_ids_of(path, RU.SCENE)
    request = [ids[-1], "99999"] + ids[:-1]                                   # not in file order, one image the index lacks
    want = VU.expected_bits(texts, [ids[-1]] + ids[:-1], RU.N_POINTS)
    index = visindex.SceneRowGroups(path)
    index.page_kinds = "any"
    present, bits = index.scene_bits(RU.SCENE, request, RU.N_POINTS)
    assert present == [ids[-1]] + ids[:-1] and bits.is_cuda and str(bits.dtype) == "torch.int64"
    assert np.array_equal(bits.cpu().numpy(), want)
    present, bits = index.scene_bits(RU.SCENE, ids[:3])                       # the width from the lists themselves
    top = max(max(json.loads(texts[i])) for i in ids[:3])
    assert present == ids[:3] and np.array_equal(bits.cpu().numpy(), VU.expected_bits(texts, present, top + 1))
    stats = index.decode_stats
    assert stats["scenes"] == 2 and stats["scenes_declined"] == 0, index.last_decline
    assert stats["rows_declined"] == 0 and stats["rows"] == 11 and stats["h2d_bytes"] > 0
    walk = RU.walk(path)
    image_pages = [w for w in walk if w["type"] != 2 and w["first_row"] < 8]
    assert (stats["dict_pages"] > 0) == any(w["encoding"] in (2, 8) for w in image_pages)
    assert (stats["v2_pages"] > 0) == any(w["type"] == 3 for w in image_pages)
    assert stats["dict_pages"] > 0 or stats["v2_pages"] > 0                   # every layout here is one "plain" does not take
    # a default-constructed reader, and this one set back to "plain": declined as a whole, the same bits
    index.page_kinds = "plain"
    for plain in (visindex.SceneRowGroups(path), index):
        before = plain.decode_stats["scenes_declined"]
        present, bits = plain.scene_bits(RU.SCENE, request, RU.N_POINTS)
        assert plain.decode_stats["scenes_declined"] == before + 1 and np.array_equal(bits.cpu().numpy(), want)


# --------------------------------------------------------------------------------------------------------------- crafted pages
ENTRIES = [json.dumps(list(range(k, 300 + 7 * k, k + 1))).encode() for k in range(5)]


def _levels(nv, ones=True):
    run = RU.uleb(nv << 1) + (b"\x01" if ones else b"\x00")
    return struct.pack("<I", len(run)) + run


def _crafted():
    """(buffer, page table rows, expectations): a dictionary page of ENTRIES, then data pages of 20 values each -- a good one
    beside every bad one."""
    dictionary = b"".join(struct.pack("<I", len(e)) + e for e in ENTRIES)
    good_runs, flat, _ = RU.encode([("rle", 9, 4), ("packed", [0, 1, 2, 3, 4, 3, 2, 1]), ("rle", 3, 2)], 3)
    rows = [0, 8, 9, 13, 16, 17, 19]

    def page(bw, runs, levels=None):
        return (levels if levels is not None else _levels(20)) + bytes([bw & 255]) + runs

    past_end, _, _ = RU.encode([("rle", 9, 4), ("packed", [0, 1, 2, 3, 4, 3, 2, 1])], 3)
    pages = [
        ("good", page(3, good_runs), 0, 0),
        ("index_equals_dictionary_size", page(3, RU.encode([("rle", 9, 4), ("packed", [0, 1, 2, 3, 5, 3, 2, 1]), ("rle", 3, 2)], 3)[0]), 4, 0),
        ("good", page(3, good_runs), 0, 0),
        ("run_past_the_pages_end", page(3, past_end[:-1]), 3, RU.E_TRUNCATED),
        ("good", page(3, good_runs), 0, 0),
        ("bit_width_33", page(33, good_runs), 3, RU.E_BITWIDTH),
        ("good", page(3, good_runs), 0, 0),
        ("levels_with_a_zero", page(3, good_runs, _levels(20, ones=False)), 2, 0),
        ("good", page(3, good_runs), 0, 0),
        ("runs_end_early", page(3, RU.rle_run(17, 1, 3)), 3, RU.E_SHORT),
        ("good_rle_only", page(3, RU.rle_run(20, 1, 3)), 0, 0),
    ]
    buf, offs = dictionary, []
    for _, body, _, _ in pages:
        offs.append(len(buf))
        buf += body + b"\xee" * 3                                             # a gap: a page's walk must not leave its page
    return buf, dictionary, offs, pages, rows, flat


def test_dict_spans_statuses_codes_and_the_good_pages_beside_the_bad_ones():
    import torch
    from mspa import _lib, engine
    from mspa.scene import pack_index_lists
    lib = _lib.load()
    buf, dictionary, offs, pages, rows, flat = _crafted()
    dev = "cuda"
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int64)).to(dev)
    payload = torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).copy()).to(dev)
    n = len(pages)
    # the dictionary's span table, by the PLAIN kernel: no levels, every entry a row
    d_start, d_len, d_status = engine.parquet_plain_spans_device(payload, t([0]), t([len(dictionary)]), t([len(ENTRIES)]), t([0, len(ENTRIES)]),
                                                                 t(range(len(ENTRIES))), has_levels=False)
    assert d_status.tolist() == [0] and d_len.tolist() == [len(e) for e in ENTRIES]
    entry_at = d_start.tolist()
    sizes = [len(body) for _, body, _, _ in pages]
    args = (payload, t(offs), t(sizes), t([20] * n), t(np.arange(n + 1) * len(rows)), t(rows * n), t([0] * n), t([len(ENTRIES)] * n), d_start, d_len)
    index, start, length, status, code = engine.parquet_dict_spans_device(*args, has_levels=True)
    torch.cuda.synchronize()
    index, start, length = (x.cpu().numpy().reshape(n, len(rows)) for x in (index, start, length))
    assert status.tolist() == [s for _, _, s, _ in pages] and code.tolist() == [c for _, _, _, c in pages]
    for k, (name, body, st, c) in enumerate(pages):
        if st == 3:                                                           # the host's code for the same runs
            head = len(_levels(20))
            assert RU.take_host(lib, body[head + 1:], body[head], 20, rows)[0] == c, name
        if st:
            assert index[k].tolist() == [-1] * len(rows) and not start[k].any() and not length[k].any(), name
            continue
        want = [1] * len(rows) if name == "good_rle_only" else [flat[r] for r in rows]
        assert index[k].tolist() == want, name
        assert start[k].tolist() == [entry_at[i] for i in want] and length[k].tolist() == [len(ENTRIES[i]) for i in want]
    # the good pages' rows go on to bits
    good = [k for k, p in enumerate(pages) if p[2] == 0]
    got = engine.index_spans_to_bits(payload, t(start[good].reshape(-1)), t(length[good].reshape(-1)), 400)
    assert not got["row_status"].any()
    lists = [json.loads(ENTRIES[i]) for k in good for i in index[k]]
    assert np.array_equal(got["bits"].cpu().numpy(), pack_index_lists(lists, 400))
    # table entries outside: the page, its rows, its dictionary
    for which, value in ((1, len(buf)), (6, len(ENTRIES)), (7, len(ENTRIES) + 1)):
        bad = list(args)
        bad[which] = bad[which].clone()
        bad[which][0] = value
        _, _, _, status, code = engine.parquet_dict_spans_device(*bad, has_levels=True)
        assert status.tolist()[0] == 1 and status.tolist()[1:] == [s for _, _, s, _ in pages][1:] and code.tolist()[0] == 0
    bad = list(args)
    bad[5] = t([8, 0] + (rows * n)[2:])                                       # rows that do not ascend
    assert engine.parquet_dict_spans_device(*bad, has_levels=True)[3].tolist()[0] == 1
    # without levels: the same pages behind no head
    bare = torch.from_numpy(np.frombuffer(dictionary + pages[0][1][len(_levels(20)):], dtype=np.uint8).copy()).to(dev)
    one = engine.parquet_dict_spans_device(bare, t([len(dictionary)]), t([len(pages[0][1]) - len(_levels(20))]), t([20]), t([0, len(rows)]), t(rows),
                                           t([0]), t([len(ENTRIES)]), d_start, d_len, has_levels=False)
    assert one[3].tolist() == [0] and one[0].tolist() == [flat[r] for r in rows]


def test_dict_spans_wrong_arguments():
    import torch
    from mspa import _lib, engine
    lib = _lib.load()
    t = lambda a: torch.tensor(a, dtype=torch.int64, device="cuda")
    payload = torch.zeros(64, dtype=torch.uint8, device="cuda")
    ok = [payload, t([0]), t([8]), t([1]), t([0, 1]), t([0]), t([0]), t([1]), t([0]), t([2])]
    for k, wrong in ((0, payload.cpu()), (1, t([0, 0])), (4, t([0])), (6, t([0, 0])), (8, t([0]).to(torch.int32)), (9, t([0, 0]))):
        args = list(ok)
        args[k] = wrong
        with pytest.raises(ValueError):
            engine.parquet_dict_spans_device(*args)
    out32, out64 = torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
    p = [payload.data_ptr(), 64, ok[1].data_ptr(), ok[2].data_ptr(), ok[3].data_ptr(), 1, 1, ok[4].data_ptr(), ok[5].data_ptr(), 1,
         ok[6].data_ptr(), ok[7].data_ptr(), ok[8].data_ptr(), ok[9].data_ptr(), 1, out32.data_ptr(), out64.data_ptr(), out64.data_ptr(),
         out32.data_ptr(), out32.data_ptr(), None]
    for k, wrong in ((1, -1), (2, None), (6, 2), (10, None), (12, None), (15, None), (19, None), (14, -1)):
        args = list(p)
        args[k] = wrong
        assert lib.mspa_parquet_dict_spans_device(*args) == _lib.MSPA_EINVAL, k
    args = list(p)
    args[5] = 0                                                               # rows without pages
    assert lib.mspa_parquet_dict_spans_device(*args) == _lib.MSPA_EINVAL


# ------------------------------------------------------------------------------------------------- rows that share an entry
def test_two_identical_image_rows_share_one_dictionary_entry_and_give_equal_bitsets(tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    from mspa import visindex
    one = RU.SU.index_table()
    values = one.column("values").to_pylist()
    values[5] = values[2]
    path = str(tmp_path / "twins.parquet")
    pq.write_table(pa.table({"key": one.column("key"), "values": pa.array(values, pa.string())}), path)
    walk = RU.walk(path)
    assert walk[1]["encoding"] == 8 and walk[1]["indices"][5] == walk[1]["indices"][2] and len(set(walk[1]["indices"][:8])) == 7
    ids, texts = VU.image_ids_of(path, RU.SCENE)
    index = visindex.SceneRowGroups(path)
    index.page_kinds = "any"
    present, bits = index.scene_bits(RU.SCENE, ids, RU.N_POINTS)
    got = bits.cpu().numpy()
    assert present == ids and index.decode_stats["scenes_declined"] == 0 and index.decode_stats["rows"] == 8
    assert np.array_equal(got, VU.expected_bits(texts, ids, RU.N_POINTS)) and np.array_equal(got[5], got[2]) and got[2].any()


# ------------------------------------------------------------------------------------------------ a corrupt dictionary page
def test_a_dictionary_entry_longer_than_its_page_declines_the_scene_to_the_host_path(tmp_path):
    from mspa import visindex
    path = RU._write(RU.SU.index_table(), str(tmp_path / "corrupt.parquet"), compression="none")
    ids, texts = VU.image_ids_of(path, RU.SCENE)
    index = visindex.SceneRowGroups(path)
    index.page_kinds = "any"
    present, bits = index.scene_bits(RU.SCENE, ids, RU.N_POINTS)              # intact: taken
    assert index.decode_stats["scenes_declined"] == 0 and np.array_equal(bits.cpu().numpy(), VU.expected_bits(texts, ids, RU.N_POINTS))
    table = index.values_pages(0)
    assert table["type"][0] == 2 and table["codec"] == "UNCOMPRESSED"
    at = int(table["start"] + table["pos"][0])
    with open(path, "r+b") as f:                                              # the first entry's length: beyond the page
        f.seek(at)
        (first,) = struct.unpack("<I", f.read(4))
        assert first == len(texts[ids[0]])
        f.seek(at)
        f.write(struct.pack("<I", int(table["uncompressed"][0])))
    index = visindex.SceneRowGroups(path)
    index.page_kinds = "any"
    calls = []
    index._scene_bits_host = lambda *a: calls.append(a) or ("host path", None)
    assert index.scene_bits(RU.SCENE, ids, RU.N_POINTS) == ("host path", None)
    assert len(calls) == 1 and index.decode_stats["scenes_declined"] == 1 and index.last_decline == "the device declined a page"


# ------------------------------------------------------------------------------------------------------------------- end to end
def _small_split(root):
    """Three small scenes on disk in the reference's layout (as tests/test_gpu_visindex_decode.py writes them), the furniture boxes as
    labelled objects."""
    from mspa import synth
    scenes = [synth.make_scene(9500 + k, n_points=3000 + 700 * k, n_frames=5 + 2 * k, color_hw=(96, 128), depth_hw=(96, 128),
                               invalid_pose_frac=0.0, with_color=False, scene_id=f"scene{9500 + k:04d}_00") for k in range(3)]
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


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def test_consumers_take_an_index_written_with_pandas_defaults(tmp_path, monkeypatch):
    """Both readers on the index as the reference writes it -- ``df.to_parquet(output_file, index=False)``: dictionary-coded pages
    -- give the same files with the switch set and unset, and with it set no scene is declined."""
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
    pq.read_table("vis.parquet").to_pandas().to_parquet("vis_defaults.parquet", index=False)
    probe = visindex.SceneRowGroups("vis_defaults.parquet")
    table = probe.values_pages(0)
    assert table["type"][0] == 2 and table["encoding"][1] == 8               # a dictionary page, dictionary-coded data pages
    handler = SceneInfoHandler(info)
    outs = {}
    for mode in ("host", "device"):
        if mode == "device":
            monkeypatch.setenv("MSPA_VISINDEX_DECODE", "device")
        out = os.path.join(root, f"covis_{mode}")
        COV.process_split("val", info, "vis_defaults.parquet", out)
        with open(os.path.join(out, "object_visibility.pkl"), "rb") as f:
            obj_vis = pickle.load(f)
        handler_m, index, _ = SOC._load_inputs(info, "vis_defaults.parquet", os.path.join(out, "object_visibility.pkl"))
        assert isinstance(index, visindex.SceneRowGroups) == (mode == "device")
        random.seed(0)
        tables = SOC._run_scenes(handler.get_all_scene_ids(), handler_m, index, obj_vis)
        outs[mode] = (_read(os.path.join(out, "object_visibility.pkl")), _read(os.path.join(out, "warning.txt")), tables)
        if mode == "device":
            assert index.page_kinds == "any"
            stats = index.decode_stats
            assert stats["scenes"] > 0 and stats["scenes_declined"] == 0 and stats["dict_pages"] > 0, (stats, index.last_decline)
    assert outs["host"] == outs["device"]
    assert any(outs["host"][2][dim] for dim in outs["host"][2])
    assert len(scenes) == 3
