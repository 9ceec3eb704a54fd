"""mspa/pairtable.py without a GPU: the switch, page planning over the writers' layouts, every decline reason, the lifted page
walk on a visibility-index file, and the host half of the sampler -- draw order, the ``size = 0`` draw, carry, the leftover
warning -- with the device calls stubbed by NumPy, frames and generator state against ``sample_dataframe``."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pairtable_util as PU  # noqa: E402

pd = pytest.importorskip("pandas")
pa = pytest.importorskip("pyarrow")
import pyarrow.parquet as pq  # noqa: E402

from mspa import _lib, pairtable, visindex  # noqa: E402


@pytest.fixture(scope="module")
def frames():
    return [PU.frame(2500, 11, scene="scene0000_00"), PU.frame(1, 12, scene="scene0001_00"), PU.frame(1700, 13, scene="scene0002_00")]


@pytest.fixture(scope="module")
def files(frames, tmp_path_factory):
    d = tmp_path_factory.mktemp("pairtables")
    paths = {k: str(d / f"{k}.parquet") for k in ("project", "pandas", "v2", "plain_big")}
    PU.write_project(paths["project"], frames)
    PU.write_pandas(paths["pandas"], frames, row_group_size=2000, dictionary_pagesize_limit=2048, data_page_size=4096)
    PU.write_pandas(paths["v2"], frames, data_page_version="2.0", compression="none", data_page_size=4096)
    PU.write_pandas(paths["plain_big"], frames + [PU.frame(9000, 14, scene="scene0003_00")], use_dictionary=False, data_page_size=1 << 20)
    return paths


# ---------------------------------------------------------------------------------------------------- the switch
def test_the_switch(monkeypatch):
    monkeypatch.delenv("MSPA_PAIRTABLE", raising=False)
    assert pairtable.mode() == "host"
    monkeypatch.setenv("MSPA_PAIRTABLE", " Device ")
    assert pairtable.mode() == "device"
    monkeypatch.setenv("MSPA_PAIRTABLE", "gpu")
    with pytest.raises(ValueError, match="MSPA_PAIRTABLE"):
        pairtable.mode()
    with pytest.raises(ValueError, match="MSPA_PAIRTABLE"):
        pairtable.sampled_rows("nowhere.parquet", 1, 0)


def test_unset_the_entry_is_the_host_line(files, monkeypatch):
    monkeypatch.delenv("MSPA_PAIRTABLE", raising=False)
    seen = []
    PU.assert_same_sample(files["pandas"], PU.PARAMETER_SETS[0], lambda *a: pairtable.sampled_rows(files["pandas"], *a, on_loaded=seen.append))
    assert seen == [4201]


# ---------------------------------------------------------------------------------------------------- planning
def _plan(path):
    t = pairtable.PairTable(path, device="cpu")
    plan, why = t.plan()
    return t, plan, why


def test_plans_of_the_writers_layouts(files, frames):
    for name, path in files.items():
        n = sum(len(f) for f in frames) + (9000 if name == "plain_big" else 0)
        t, plan, why = _plan(path)
        assert why is None and len(t) == n, (name, why)
        pages = np.array(plan["pages"], dtype=np.int64)
        # the data pages tile the [4, rows] output in order
        assert np.array_equal(pages[:, 4], np.concatenate([[0], np.cumsum(pages[:, 3])])[:-1]) and int(pages[:, 3].sum()) == 4 * n
        coded, v2, v1 = (pages[:, 5] & flag != 0 for flag in (_lib.PAGE_DICT_CODED, _lib.PAGE_LEVELS_GIVEN, _lib.PAGE_LEVELS_INLINE))
        assert np.array_equal(pages[:, 2] >= 0, coded) and np.array_equal(pages[:, 1] >= 0, v2)
        if name == "project":
            assert not coded.any() and v1.all() and len(pages) == 4 * 3
        if name == "pandas":        # one chunk holds dictionary-coded pages followed by PLAIN ones
            assert coded.any() and not coded.all() and v1.all()
            first_chunk = pages[pages[:, 4] < 2000]
            assert (first_chunk[:, 5] & _lib.PAGE_DICT_CODED != 0).any() and (first_chunk[:, 5] & _lib.PAGE_DICT_CODED == 0).any()
        if name == "v2":
            assert v2.all() and not v1.any() and all(not s for _b, _u, s in plan["pieces"])
        if name == "plain_big":
            assert not coded.any() and max(u for _b, u, _s in plan["pieces"]) > 65536
        if name != "v2":
            assert all(s for _b, _u, s in plan["pieces"])


def test_every_decline_reason(frames, tmp_path):
    df = pd.concat(frames, ignore_index=True)
    cases = {}
    df.to_parquet(tmp_path / "gzip.parquet", index=False, compression="gzip")
    cases["gzip"] = "codec GZIP"
    df.assign(overlap=np.arange(len(df))).to_parquet(tmp_path / "int64.parquet", index=False)
    cases["int64"] = "column overlap is INT64, not DOUBLE"
    df.assign(extra=1.0).to_parquet(tmp_path / "extra.parquet", index=False)
    cases["extra"] = "an extra column: extra"
    df.set_index(pd.Index(np.arange(len(df)) * 2)).to_parquet(tmp_path / "index.parquet")
    cases["index"] = "a pandas index column"
    df[PU.COLUMNS[:6]].to_parquet(tmp_path / "missing.parquet", index=False)
    cases["missing"] = "a missing column: pitch"
    df[PU.COLUMNS[::-1]].to_parquet(tmp_path / "order.parquet", index=False)
    cases["order"] = "columns that are not the seven of the pair table, in its order"
    df.to_parquet(tmp_path / "split.parquet", index=False, use_dictionary=False, column_encoding={c: "BYTE_STREAM_SPLIT" for c in PU.COLUMNS[3:]})
    cases["split"] = "a data page with encoding 9"
    for name, want in cases.items():
        _t, plan, why = _plan(str(tmp_path / f"{name}.parquet"))
        assert plan is None and why is not None and why.endswith(want), (name, why)


def test_a_damaged_page_header_declines(files, tmp_path):
    raw = bytearray(open(files["project"], "rb").read())
    md = pq.ParquetFile(files["project"]).metadata
    at = md.row_group(0).column(3).data_page_offset
    raw[at + 1:at + 4] = b"\xff\xff\xff"                      # the first page header of `overlap`
    path = str(tmp_path / "damaged.parquet")
    open(path, "wb").write(raw)
    _t, plan, why = _plan(path)
    assert plan is None and "row group 0, overlap" in why


def test_arguments_the_device_path_leaves_to_the_host():
    ok = pairtable.arguments_reason
    assert ok(10, 0, 6, 35, 1) is None and ok(10, 3, 0, 100, 0.5) is None and ok(np.int64(3), 0, 0.0, 1.0, 1.0) is None
    assert ok(10, 0, 0, 250, 1) is None and ok(10, 0, 0, 251, 1) == "more than 250 bins"
    assert ok(-1, 0, 6, 35, 1) and ok(10, -1, 6, 35, 1) and ok(1.5, 0, 6, 35, 1) and ok(True, 0, 6, 35, 1)
    assert ok(10, 0, 6, 35, 0) == "interval is not positive" and ok(10, 0, 6, 35, -1) and ok(10, 0, 6, float("nan"), 1)
    assert ok(10, 0, 35, 6, 1) == "fewer than one bin" and ok(10, 0, 0, 1e9, 1) == "more than 250 bins"


# ---------------------------------------------------------------------------------------------------- the lifted page walk
def test_the_lifted_walk_serves_values_pages(tmp_path):
    rows = [{"key": f"scene0000_00:image_to_points:{k}", "values": str(list(range(k % 7, 300 + 40 * k, 3)))} for k in range(60)]
    path = str(tmp_path / "vis.parquet")
    pq.write_table(pa.Table.from_pylist(rows), path, data_page_size=4096, row_group_size=40, write_batch_size=8, use_dictionary=["key"])
    reader = visindex.SceneRowGroups(path)
    keys = {"start", "bytes", "codec", "pos", "compressed", "uncompressed", "num_values", "type", "encoding", "levels", "first_row",
            "dict_values", "def_bytes", "rep_bytes", "num_nulls", "is_compressed", "chunk"}
    for g in range(2):
        col = reader.file.metadata.row_group(g).column(1)
        first = reader.values_pages(g)
        table, chunk = visindex.column_chunk_pages(path, col)
        assert set(first) == keys == set(table) and first["chunk"] == chunk and table["chunk"] is None
        assert reader.values_pages(g)["chunk"] is None           # the cache keeps numbers only
        for k in keys - {"chunk"}:
            assert np.array_equal(first[k], table[k]), k
        # against pyarrow's own account of the chunk
        assert table["bytes"] == col.total_compressed_size == len(chunk) and table["codec"] == col.compression == "SNAPPY"
        assert int(table["num_values"].sum()) == col.num_values and table["first_row"][-1] == col.num_values
        assert int(table["pos"][-1] + table["compressed"][-1]) == len(chunk) and len(table["pos"]) >= 3
        text = b"".join(bytes(pa.Codec("snappy").decompress(chunk[p:p + c], int(u))) for p, c, u, t in
                        zip(table["pos"], table["compressed"], table["uncompressed"], table["type"]) if t == 0)
        assert rows[40 * g]["values"].encode() in text
    with pytest.raises(ValueError, match="visindex: the values chunk ends beyond the file"):
        short = str(tmp_path / "short.parquet")
        open(short, "wb").write(open(path, "rb").read()[:200])
        r2 = visindex.SceneRowGroups(path)
        r2._path = short
        r2.values_pages(0)


# ---------------------------------------------------------------------------------------------------- the host half
def test_draw_order_carry_and_the_leftover_warning():
    counts = np.zeros(256, dtype=np.int64)
    counts[[0, 1, 2, 3]] = [5, 0, 50, 5]
    counts[_lib.PAIR_CLASS_ZERO] = 9
    calls, lines = [], []

    def draw(length, want):
        calls.append((length, want))
        return np.arange(want)[::-1]

    picks = pairtable.plan_draws(counts, 4, 40, 0, draw=draw, out=lines.append)
    # the zero part is drawn first (size 0 still draws), the bins from the smallest: 1 (0 rows), 0 and 3 (5 each, bin order), 2
    assert calls == [(9, 0), (50, 30)]
    assert [c for c, _p in picks] == [1, 0, 3, 2, _lib.PAIR_CLASS_ZERO]
    assert picks[0][1] is None and picks[1][1] is None and picks[2][1] is None and list(picks[3][1]) == list(range(30))[::-1] and len(picks[4][1]) == 0
    assert lines == [f"[sample_dataframe] current_quota v.s. group_df: {w} v.s. {n}" for w, n in ((10, 0), (20, 5), (25, 5), (30, 50))]
    # nothing to draw from: every group whole, the zero part kept, the shortfall reported
    calls.clear(), lines.clear()
    picks = pairtable.plan_draws(counts, 4, 1000, 9, draw=draw, out=lines.append)
    assert calls == [] and all(p is None for _c, p in picks)
    assert lines[-1] == "[sample_dataframe] Warning: bins not enough to reach 1000; leftover 940"
    begin = np.concatenate([[0], np.cumsum(counts)])
    assert list(pairtable.pick_positions([(3, None), (2, np.array([4, 0]))], begin)) == [55, 56, 57, 58, 59, 9, 5]


def test_draw_positions_are_dataframe_sample(frames):
    df = frames[0]
    for want in (0, 1, 17, len(df)):
        np.random.seed(5)
        a = df.sample(n=want).index.to_numpy()
        s1 = np.random.get_state()
        np.random.seed(5)
        b = pairtable.draw_positions(len(df), want)
        assert np.array_equal(a, b) and PU.same_state(s1, np.random.get_state())


@pytest.fixture()
def numpy_device(monkeypatch):
    """The device calls of ``PairTable.sample`` by NumPy on CPU tensors: columns from pyarrow, codes by the restatement, the
    partition by a stable sort."""
    import torch
    from mspa import engine

    def columns(self):
        if self._columns is None:
            t = pq.read_table(self.path, columns=list(pairtable.DOUBLE_COLUMNS))
            self._columns = torch.from_numpy(np.stack([t.column(c).to_pandas().to_numpy(dtype=np.float64) for c in pairtable.DOUBLE_COLUMNS]))
        return self._columns

    def pair_bin_codes(overlap, edges):
        codes = PU.classify_numpy(overlap.numpy(), edges.numpy())
        return torch.from_numpy(codes), torch.from_numpy(np.bincount(codes, minlength=256).astype(np.int32)[None])

    def pair_partition(codes, tile_counts):
        begin = np.concatenate([[0], np.cumsum(tile_counts.numpy().sum(axis=0))]).astype(np.int64)
        return torch.from_numpy(np.argsort(codes.numpy(), kind="stable").astype(np.int32)), torch.from_numpy(begin)

    monkeypatch.setattr(pairtable.PairTable, "columns", columns)
    monkeypatch.setattr(engine, "pair_bin_codes", pair_bin_codes)
    monkeypatch.setattr(engine, "pair_partition", pair_partition)


@pytest.mark.parametrize("args", PU.PARAMETER_SETS, ids=[str(a) for a in PU.PARAMETER_SETS])
def test_the_host_half_gives_the_host_lines_sample(files, numpy_device, args):
    for name in ("project", "pandas"):
        t = pairtable.PairTable(files[name], device="cpu")
        got = PU.assert_same_sample(files[name], args, t.sample)
        assert t.stats["samples_declined"] == 0 and t.last_decline is None and len(got) > 0
    assert t.stats["partitions"] == 1


def test_partitions_are_cached_per_parameter_set(files, numpy_device):
    t = pairtable.PairTable(files["project"], device="cpu")
    for args in (PU.PARAMETER_SETS[0], PU.PARAMETER_SETS[1], PU.PARAMETER_SETS[0], PU.PARAMETER_SETS[3]):
        PU.assert_same_sample(files["project"], args, t.sample)
    assert t.stats["partitions"] == 2 and t.stats["samples"] == 4


def test_a_table_without_a_nonzero_row_and_host_arguments(numpy_device, tmp_path):
    path = str(tmp_path / "zeros.parquet")
    PU.write_pandas(path, [PU.frame(40, 3, overlap=np.where(np.arange(40) % 2, 0.0, -0.0))])
    t = pairtable.PairTable(path, device="cpu")
    for args in ((30, 0, 6, 35, 1), (30, 7, 6, 35, 1), (30, 100, 6, 35, 1)):
        got = PU.assert_same_sample(path, args, t.sample)
        assert len(got) == min(args[1], 40)
    assert t.stats["samples_declined"] == 0
    # arguments for which the host function raises go to it, with the reason: the caller sees the host line's exception
    with pytest.raises(IndexError):
        PU.host_line(path, (30, 0, 35, 6, 1))
    with pytest.raises(IndexError):
        t.sample(30, 0, 35, 6, 1)
    assert t.last_decline == "fewer than one bin" and t.stats["samples_declined"] == 1


def test_the_module_cache_keeps_two_files(files, monkeypatch):
    monkeypatch.setattr(pairtable, "_TABLES", type(pairtable._TABLES)())
    a = pairtable.open_table(files["project"], "cpu")
    assert pairtable.open_table(files["project"], "cpu") is a
    pairtable.open_table(files["pandas"], "cpu")
    pairtable.open_table(files["v2"], "cpu")
    assert len(pairtable._TABLES) == 2 and pairtable.open_table(files["project"], "cpu") is not a
    os.utime(files["v2"], ns=(1, 1))
    assert len(pairtable.open_table(files["v2"], "cpu")) == len(a)
