"""``MSPA_PAIRTABLE=device`` on the MI355X: the pair table's DOUBLE columns decoded from the file's pages (csrc/pair_table.hip),
the bin codes, counts and per-class row lists against the NumPy restatement, and ``PairTable.sample`` against the host line --
frame, floats' bits, printed text, generator state -- over the layouts of four writers; declined files; the three builder
families byte for byte with the switch unset and set."""
import contextlib
import importlib
import io
import os
import pickle
import random
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pairtable_util as PU  # noqa: E402
import rle_hybrid_util as RU  # noqa: E402

pd = pytest.importorskip("pandas")
pa = pytest.importorskip("pyarrow")
import pyarrow.parquet as pq  # noqa: E402

from mspa import _lib, engine, pairtable  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---------------------------------------------------------------------------------------------------- tables
@pytest.fixture(scope="module")
def frames():
    """Three row groups: 25 000 rows, 1 row, 30 011 rows (no multiple of a tile, a wave or a workgroup's share)."""
    return [PU.frame(25000, 21, scene="scene0000_00"), PU.frame(1, 22, scene="scene0001_00"), PU.frame(30011, 23, scene="scene0002_00")]


@pytest.fixture(scope="module")
def files(frames, tmp_path_factory):
    d = tmp_path_factory.mktemp("pairtables_gpu")
    paths = {k: str(d / f"{k}.parquet") for k in ("project", "pandas", "v2", "block", "rows63", "zeros")}
    PU.write_project(paths["project"], frames)                                                     # (a)
    PU.write_pandas(paths["pandas"], frames, row_group_size=30000, dictionary_pagesize_limit=4096, data_page_size=8192)   # (b)
    PU.write_pandas(paths["v2"], frames, row_group_size=30000, data_page_version="2.0", compression="none", data_page_size=8192,
                    dictionary_pagesize_limit=4096)                                                # (c)
    PU.write_pandas(paths["block"], frames, row_group_size=40000, use_dictionary=False, data_page_size=1 << 20)          # (d)
    PU.write_pandas(paths["rows63"], [PU.frame(63, 24)])
    PU.write_project(paths["zeros"], [PU.frame(5000, 25, overlap=np.where(np.arange(5000) % 3, 0.0, -0.0))])
    return paths


@pytest.fixture(scope="module")
def tables(files):
    return {k: pairtable.PairTable(p, DEV) for k, p in files.items()}


def _reference_columns(path):
    t = pq.read_table(path, columns=list(pairtable.DOUBLE_COLUMNS))
    return np.stack([t.column(c).to_pandas().to_numpy(dtype=np.float64) for c in pairtable.DOUBLE_COLUMNS])


# ---------------------------------------------------------------------------------------------------- the kernels
def test_hybrid_streams_expand_as_the_host_reference_takes_them():
    cases = {(bytes(c[1]), c[2], c[3]) for c in RU.valid_cases() + RU.corrupt_cases() + RU.truncation_cases()}
    cases = sorted(cases, key=lambda c: (c[1], c[2], c[0]))
    cases += [(b"", 1, 0), (RU.rle_run(70000, 1, 1), 1, 70000), (RU.rle_run(5, 1, 1) + RU.packed_run([1, 0, 1, 1, 0, 0, 1, 0] * 300, 1)[0], 1, 2405)]
    blob = b"".join(c[0] for c in cases)
    offs = np.concatenate([[0], np.cumsum([len(c[0]) for c in cases])]).astype(np.int64)
    src = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(DEV)

    def dev(a):
        return torch.from_numpy(np.asarray(a, dtype=np.int64)).to(DEV)

    runs = engine.rle_hybrid_runs_device(src, dev(offs[:-1]), dev(np.diff(offs)), dev([c[1] for c in cases]), dev([c[2] for c in cases]))
    values = engine.rle_hybrid_expand_device(src, runs).cpu().numpy()
    begin, status, const = runs["out_begin"].cpu().numpy(), runs["status"].cpu().numpy(), runs["const_value"].cpu().numpy()
    assert runs["total"] == sum(c[2] for c in cases) == len(values)
    declined = 0
    for k, (stream, bw, n) in enumerate(cases):
        rc, want = engine.rle_hybrid_take_host(stream, bw, n, np.arange(n))
        assert status[k] == rc, (k, bw, n, status[k], rc)
        assert np.array_equal(values[begin[k]:begin[k + 1]], want), (k, bw, n)
        if const[k] != -1:                                     # one RLE run over every value
            assert rc == 0 and n > 0 and (want == const[k]).all() and stream[0] & 1 == 0
        declined += rc != 0
    assert declined > 50 and const[-2] == 1 and const[-1] == -1
    # a table entry outside the buffer declines the stream and writes nothing of it
    runs = engine.rle_hybrid_runs_device(src, dev([len(blob) - 1, -4]), dev([2, 2]), dev([1, 1]), dev([3, 3]))
    assert runs["status"].tolist() == [_lib.MSPA_EINVAL] * 2 and engine.rle_hybrid_expand_device(src, runs).tolist() == [-1] * 6


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2048, 2049, 8192, 8193, 30011])
def test_codes_counts_and_row_lists_at_the_tile_seams(n):
    x = PU.overlap_column(n, 100 + n)
    overlap = torch.from_numpy(x).to(DEV)
    for lo, hi, step in PU.EDGE_SETS:
        edges = PU.edges_of(lo, hi, step).astype(np.float64)
        want = PU.classify_numpy(x, edges)
        codes, tile_counts = engine.pair_bin_codes(overlap, torch.from_numpy(edges).to(DEV))
        assert np.array_equal(codes.cpu().numpy(), want)
        rows = int(_lib.load().mspa_pair_tile_rows())
        per_tile = np.stack([np.bincount(want[t:t + rows], minlength=256) for t in range(0, n, rows)])
        assert np.array_equal(tile_counts.cpu().numpy(), per_tile)
        order, begin = engine.pair_partition(codes, tile_counts)
        assert np.array_equal(begin.cpu().numpy(), np.concatenate([[0], np.cumsum(np.bincount(want, minlength=256))]))
        assert np.array_equal(order.cpu().numpy(), np.argsort(want, kind="stable"))
    host_codes, host_counts = engine.pair_bin_codes_host(x, edges)
    assert np.array_equal(host_codes, want) and np.array_equal(host_counts, np.bincount(want, minlength=256))


def test_the_engine_wrappers_check_their_tensors():
    x = torch.zeros(8, dtype=torch.float64, device=DEV)
    e = torch.tensor([0.0, 1.0], dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="overlap"):
        engine.pair_bin_codes(x.float(), e)
    with pytest.raises(ValueError, match="edges"):
        engine.pair_bin_codes(x, e.cpu())
    with pytest.raises(ValueError):
        engine.pair_bin_codes(x, e[:1])
    codes, tile_counts = engine.pair_bin_codes(x, e)
    with pytest.raises(ValueError, match="tile_counts"):
        engine.pair_partition(codes, tile_counts[:, :10].contiguous())
    with pytest.raises(ValueError, match="bit_widths"):
        engine.rle_hybrid_runs_device(codes, *(torch.zeros(1, dtype=torch.int64, device=DEV),) * 2, torch.zeros(1, dtype=torch.int32, device=DEV),
                                      torch.zeros(1, dtype=torch.int64, device=DEV))


# ---------------------------------------------------------------------------------------------------- files
@pytest.mark.parametrize("name", ["project", "pandas", "v2", "block", "rows63", "zeros"])
def test_columns_are_pyarrows_bit_for_bit(files, tables, name):
    t = tables[name]
    cols = t.columns()
    assert not isinstance(cols, str), cols
    want = _reference_columns(files[name])
    assert cols.shape == want.shape and np.array_equal(cols.cpu().numpy().view(np.int64), want.view(np.int64))
    s = t.stats
    assert s["decodes"] == 1 and s["samples_declined"] == 0 and t.last_decline is None
    nulls = int(np.isnan(want).sum())
    if name == "project":
        assert s["dict_pages"] == 0 and s["null_pages"] == 0 and s["v2_pages"] == 0 and nulls > 0       # NaN values, no nulls
    if name == "pandas":    # dictionary-coded pages followed by PLAIN ones in one chunk, several pages with nulls
        assert 0 < s["dict_pages"] < s["pages"] and s["null_pages"] >= 3 and s["v2_pages"] == 0 and nulls > 0
    if name == "v2":
        assert s["v2_pages"] == s["pages"] and s["null_pages"] >= 3 and s["blocks"] == 0 and s["dict_pages"] > 0
    if name == "block":
        assert s["blocks"] >= 8 and s["dict_pages"] == 0                                                # a page above 64 KiB, by blocks
    assert t.columns() is cols                                                                          # decoded once


@pytest.mark.parametrize("name", ["project", "pandas", "v2", "block"])
def test_codes_counts_and_row_lists_of_the_files(files, tables, name):
    t = tables[name]
    x = _reference_columns(files[name])[0]
    assert not isinstance(t.columns(), str)
    for lo, hi, step in PU.EDGE_SETS:
        want = PU.cut_reference(x, PU.edges_of(lo, hi, step))
        counts, order, begin = t.partition(lo, hi, step)
        assert np.array_equal(counts, np.bincount(want, minlength=256))
        assert np.array_equal(order.cpu().numpy(), np.argsort(want, kind="stable"))
        assert np.array_equal(begin.cpu().numpy(), np.concatenate([[0], np.cumsum(counts)]))


@pytest.mark.parametrize("args", PU.PARAMETER_SETS, ids=[str(a) for a in PU.PARAMETER_SETS])
@pytest.mark.parametrize("name", ["project", "pandas", "v2", "block", "rows63", "zeros"])
def test_samples_are_the_host_lines(files, tables, name, args):
    t = tables[name]
    before = t.stats["samples"]
    PU.assert_same_sample(files[name], args, t.sample)
    assert t.stats["samples"] == before + 1 and t.stats["samples_declined"] == 0 and t.last_decline is None and t.stats["decodes"] == 1


def test_the_entry_routes_on_the_switch_and_caches_the_table(files, monkeypatch):
    monkeypatch.setattr(pairtable, "_TABLES", type(pairtable._TABLES)())
    monkeypatch.setenv("MSPA_PAIRTABLE", "device")
    seen = []
    for args in PU.PARAMETER_SETS[:2]:
        PU.assert_same_sample(files["pandas"], args, lambda *a: pairtable.sampled_rows(files["pandas"], *a, on_loaded=seen.append, device=DEV))
    (t,) = pairtable._TABLES.values()
    assert seen == [55012, 55012] and t.stats["samples"] == 2 and t.stats["decodes"] == 1 and t.stats["partitions"] == 1
    assert t.stats["samples_declined"] == 0


def test_declined_files_give_the_host_lines_frame(frames, tmp_path):
    df = pd.concat([f[:3000] for f in frames], ignore_index=True)
    cases = {"gzip": (dict(index=False, compression="gzip"), "codec GZIP"),
             "split": (dict(index=False, use_dictionary=False, column_encoding={c: "BYTE_STREAM_SPLIT" for c in PU.COLUMNS[3:]}),
                       "a data page with encoding 9"),
             "index": (dict(index=True), "a pandas index column")}
    for name, (options, want) in cases.items():
        path = str(tmp_path / f"{name}.parquet")
        (df.set_index(pd.Index(np.arange(len(df)) + 5)) if name == "index" else df).to_parquet(path, **options)
        t = pairtable.PairTable(path, DEV)
        np.random.seed(3)
        host, text, state = PU.host_line(path, PU.PARAMETER_SETS[0])
        np.random.seed(3)
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            got = t.sample(*PU.PARAMETER_SETS[0])
        pd.testing.assert_frame_equal(got, host, check_exact=True)
        assert out.getvalue() == text and PU.same_state(np.random.get_state(), state)
        assert t.last_decline.endswith(want) and t.stats["samples_declined"] == 1 and t.stats["decodes"] == 0
    # a page whose Snappy stream is damaged: the device declines it, the host line raises as it always did
    path = str(tmp_path / "damaged.parquet")
    PU.write_project(path, [frames[0][:4000]])
    from mspa import visindex
    table, _chunk = visindex.column_chunk_pages(path, pq.ParquetFile(path).metadata.row_group(0).column(3))
    raw = bytearray(open(path, "rb").read())
    raw[table["start"] + int(table["pos"][0])] ^= 0x15        # the stream's preamble: the length it says it decodes to
    open(path, "wb").write(raw)
    t = pairtable.PairTable(path, DEV)
    with pytest.raises(Exception):
        t.sample(*PU.PARAMETER_SETS[0])
    assert t.stats["samples_declined"] == 1 and "declined" in t.last_decline


# ---------------------------------------------------------------------------------------------------- the builders
@pytest.fixture(scope="module")
def split(tmp_path_factory):
    """The small synthetic split of tests/test_gpu_heads.py's dataset-level tests: two scenes of 9 and 10 frames on disk, their
    visibility index as a pickle, their pair table as pandas writes it."""
    from mspa import synth
    from mspa.scene import SceneOnDevice
    from test_gpu_heads import _write_scene_files
    root = tmp_path_factory.mktemp("pairtable_split")
    scenes = [synth.make_scene(7400 + k, n_points=3000, n_frames=9 + k, color_hw=(96, 128), depth_hw=(96, 128), invalid_pose_frac=0.1,
                               with_color=False) for k in range(2)]
    info_path, posed, inst = _write_scene_files(root, scenes, False)
    vis_all, rows = {}, []
    for sc in scenes:
        resident = SceneOnDevice(sc.K, sc.A, sc.E, sc.depth, sc.color_hw, sc.points, DEV)
        vis_all[sc.scene_id] = resident.visibility_index()
        for (a, b), v in resident.frames_relations().items():
            rows.append({"scene_id": sc.scene_id, "image_id1": a, "image_id2": b, "overlap": float(v["overlap"]),
                         "distance": float(v["distance"]), "yaw": float(v["yaw"]), "pitch": float(v["pitch"])})
    vis_path, table_path = str(root / "vis.pkl"), str(root / "pairs.parquet")
    with open(vis_path, "wb") as f:
        pickle.dump(vis_all, f)
    pd.DataFrame(rows).to_parquet(table_path)
    IH = importlib.import_module("spatial_engine.utils.scannet_utils.handler.info_handler")
    return {"root": root, "handler": IH.SceneInfoHandler(info_path, posed_images_root=posed, instance_data_root=inst), "vis": vis_path,
            "table": table_path}


def _tree(directory):
    out = {}
    for base, _dirs, names in os.walk(directory):
        for n in names:
            with open(os.path.join(base, n), "rb") as f:
                out[os.path.relpath(os.path.join(base, n), directory)] = f.read()
    return out


def _both_modes(split, monkeypatch, name, build):
    """``build(out directory)`` with the switch unset and set, the same seeds -> both trees, printed texts and end states."""
    got = {}
    out = str(split["root"] / name)
    for mode in ("host", "device"):
        shutil.rmtree(out, ignore_errors=True)                 # both modes write the same names into the same place
        os.makedirs(out)
        with monkeypatch.context() as m:
            m.setattr(pairtable, "_TABLES", type(pairtable._TABLES)())
            if mode == "device":
                m.setenv("MSPA_PAIRTABLE", "device")
            else:
                m.delenv("MSPA_PAIRTABLE", raising=False)
            random.seed(40)
            np.random.seed(40)
            text = io.StringIO()
            with contextlib.redirect_stdout(text):
                extra = build(out)
            tables = list(pairtable._TABLES.values())
            if mode == "device":                               # a condition: the device path ran, nothing fell back
                assert len(tables) == 1 and tables[0].stats["samples"] >= 1 and tables[0].stats["samples_declined"] == 0
                assert tables[0].stats["decodes"] == 1
            else:
                assert not tables
            got[mode] = (_tree(out), text.getvalue().replace(out, "OUT"), random.getstate(), np.random.get_state(), extra)
    (tree_h, text_h, r_h, n_h, x_h), (tree_d, text_d, r_d, n_d, x_d) = got["host"], got["device"]
    assert tree_h == tree_d and text_h == text_d and r_h == r_d and PU.same_state(n_h, n_d) and x_h == x_d
    return tree_h


def test_camera_movement_builder_is_unchanged_by_the_switch(split, monkeypatch):
    CME = importlib.import_module("spatial_engine.camera_movement.camera_movement_engine_train_val")

    def build(out):
        CME.build_train_dataset(split["table"], out, split["handler"], "displacement_vector", 30, 1, 60, 1)
        CME.build_val_dataset(split["table"], out, split["handler"], "yaw_movement", 12, 1, 60, 1)

    tree = _both_modes(split, monkeypatch, "cme", build)
    assert tree["displacement_vector_train.jsonl"].count(b"\n") >= 10 and tree["yaw_movement_val.jsonl"]


def test_correspondence_coor_builder_is_unchanged_by_the_switch(split, monkeypatch):
    VC = importlib.import_module("spatial_engine.visual_correspondence.visual_correspondence_qa_engine_coor_2_coor")

    def build(out):
        warn = os.path.join(out, "warn.txt")
        open(warn, "w").close()
        VC.build_train_dataset(split["table"], out, split["handler"], 30, 1, 60, 1, split["vis"], warn)
        VC.build_val_dataset(split["table"], out, split["handler"], 8, 1, 60, 1, split["vis"], warn)

    tree = _both_modes(split, monkeypatch, "vcc", build)
    assert tree["train_visual_correspondence_coor_2_coor.jsonl"].count(b"\n") >= 10


def test_correspondence_dot_builder_is_unchanged_by_the_switch(split, monkeypatch):
    from mspa.annotate import RecordingAnnotator
    VD = importlib.import_module("spatial_engine.visual_correspondence.visual_correspondence_qa_engine_dot_2_multichoice")

    def build(out):
        warn = os.path.join(out, "warn.txt")
        open(warn, "w").close()
        rec = RecordingAnnotator()
        with monkeypatch.context() as m:
            m.setattr(VD, "ANNOTATOR", rec)
            VD.build_train_dataset(split["table"], out, split["handler"], 24, 1, 60, 1, split["vis"], warn)
        return [repr(j).replace(out, "OUT") for j in rec.jobs]

    tree = _both_modes(split, monkeypatch, "vcd", build)
    assert tree["train_visual_correspondence_dot_2_multichoice.jsonl"].count(b"\n") >= 8
