"""The host half of the index's way back over dictionary-coded and v2 pages, without a GPU: the page table's new columns, the
plan ``SceneRowGroups._plan_pages`` makes with ``page_kinds = "any"`` -- against a pure-Python walk of the chunk
(tests/rle_hybrid_util.py) -- over the layouts pyarrow gives, the reasons ``page_kinds = "plain"`` keeps, and the layouts that
still decline."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rle_hybrid_util as RU  # noqa: E402

from mspa import visindex  # noqa: E402

SU = RU.SU
NAMES = tuple(RU.LAYOUTS)
IDS = [f"{k * 10:05d}" for k in range(8)]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return RU.index_files(tmp_path_factory.mktemp("encoded_pages"))


def _plan(path, kinds):
    index = visindex.SceneRowGroups(path)
    index.page_kinds = kinds
    distinct = sorted(set(index.image_rows(RU.SCENE, IDS).values()))
    assert distinct == [(0, r) for r in range(8)]
    return index, index._plan_pages(distinct)


def test_default_is_plain_and_the_reasons_are_todays(files):
    assert visindex.SceneRowGroups.page_kinds == "plain" and "page_kinds" not in vars(visindex.SceneRowGroups(files["defaults"]))
    v2 = "row group 0: a data page that is not v1"
    not_plain = "row group 0: a data page that is not PLAIN"
    want = {"defaults": not_plain, "version_1_0": not_plain, "small_dictionary": not_plain, "small_dictionary_v2": v2, "v2_plain": v2,
            "v2_uncompressed": v2, "straddle": not_plain}
    for name in NAMES:
        assert _plan(files[name], "plain")[1] == (None, want[name]), name
    index = visindex.SceneRowGroups(files["defaults"])
    index.page_kinds = "every"
    with pytest.raises(ValueError, match="page_kinds"):
        index.needed_pages(0, [0])


def test_the_files_have_the_shapes_the_cases_are_about(files):
    def table(name):
        return visindex.SceneRowGroups(files[name]).values_pages(0)

    for name in ("defaults", "version_1_0"):                                   # a dictionary page, then dictionary-coded pages
        t = table(name)
        code = 2 if name == "version_1_0" else 8
        assert t["type"].tolist()[:2] == [2, 0] and t["encoding"].tolist()[:2] == [0 if code == 8 else 2, code], name
        assert t["num_values"][0] == 0 and t["dict_values"][0] > 8 and t["first_row"].tolist()[:2] == [0, 0]
        assert t["dict_values"][1:].tolist() == [0] * (len(t["pos"]) - 1) and t["is_compressed"].tolist() == [1] * len(t["pos"])
    for name in ("small_dictionary", "small_dictionary_v2"):                   # a dictionary page, ONE page of 8 indices, then PLAIN pages
        t = table(name)
        data = 3 if name.endswith("v2") else 0
        assert t["type"].tolist()[:3] == [2, data, data] and t["encoding"].tolist()[:3] == [0, 8, 0], name
        assert t["num_values"].tolist()[:2] == [0, 8] and t["dict_values"][0] == 8 and set(t["encoding"][2:].tolist()) == {0}
    t = table("small_dictionary_v2")
    assert t["def_bytes"].tolist()[:3] == [0, 2, 3] and not t["rep_bytes"].any() and not t["num_nulls"].any()
    assert t["is_compressed"][1] == 0 and t["is_compressed"][2] == 1           # pyarrow leaves the 5-byte stream as it is
    t = table("v2_plain")
    assert t["type"].tolist() == [3] and t["encoding"].tolist() == [0] and t["def_bytes"].tolist() == [3]
    t = table("v2_uncompressed")
    assert t["codec"] == "UNCOMPRESSED" and t["type"].tolist() == [2, 3] and t["encoding"].tolist() == [0, 8]
    # the straddling file: the first six image rows are dictionary-coded, the last two PLAIN, in ONE chunk
    t = table("straddle")
    assert t["type"].tolist()[:3] == [2, 0, 0] and t["encoding"].tolist()[:3] == [0, 8, 0]
    assert t["first_row"].tolist()[:4] == [0, 0, 6, 9] and t["dict_values"][0] == 6
    index, (pages, why) = _plan(files["straddle"], "any")
    assert why is None and [(p.kind, p.rows.tolist()) for p in pages] == [(1, [0, 1, 2, 3, 4, 5]), (0, [0, 1]), (2, [])]


@pytest.mark.parametrize("name", NAMES)
def test_the_plan_names_the_pages_a_python_walk_finds_the_rows_in(files, name):
    import pyarrow as pa
    import pyarrow.parquet as pq
    path = files[name]
    walk = RU.walk(path)
    index, (pages, why) = _plan(path, "any")
    assert why is None, why
    rows_of = {}                                                               # data page -> the wanted rows, counted from its first
    for r in range(8):
        k = max(k for k, w in enumerate(walk) if w["type"] != 2 and w["first_row"] <= r)
        rows_of.setdefault(k, []).append(r - walk[k]["first_row"])
    data = sorted(rows_of)
    coded = any(walk[k]["encoding"] in (2, 8) for k in data)
    want = data + ([0] if coded else [])                                       # the dictionary page behind the data pages
    assert [p.index for p in pages] == want
    at = 0
    for p, k in zip(pages, want):
        w = walk[k]
        assert (p.group, p.src, p.compressed, p.uncompressed, p.snappy) == (0, at, w["stream_bytes"], w["stream_uncompressed"], w["compressed"]), k
        assert p.v2 == (w["type"] == 3) and p.kind == (2 if w["type"] == 2 else 1 if w["encoding"] in (2, 8) else 0)
        assert p.num_values == len(w["values"]) and p.rows.tolist() == (rows_of[k] if w["type"] != 2 else [])
        assert p.dictionary == (len(data) if p.kind == 1 else -1)
        # the bytes are that stream's: decompressed, they are what the walk decoded
        body = pa.Codec("snappy").decompress(p.data.tobytes(), decompressed_size=p.uncompressed).to_pybytes() if p.snappy else p.data.tobytes()
        assert len(body) == p.uncompressed
        if p.kind != 1:
            for r in (rows_of[k] if w["type"] != 2 else range(len(w["values"])))[:8]:
                assert w["values"][r] in body
        at += p.compressed
    # and the rows' texts are the image rows'
    table = pq.read_table(path)
    for r in range(8):
        k = max(k for k in data if walk[k]["first_row"] <= r)
        assert walk[k]["values"][r - walk[k]["first_row"]].decode() == table.column("values")[r].as_py()


def test_other_layouts_decline_with_a_reason(tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    one = SU.index_table()

    def reason(path):
        index = visindex.SceneRowGroups(path)
        index.page_kinds = "any"
        return index._plan_pages(sorted(set(index.image_rows(RU.SCENE, IDS).values())))

    gz = RU._write(one, str(tmp_path / "gzip.parquet"), compression="gzip")
    assert reason(gz) == (None, "row group 0: codec GZIP")
    delta = RU._write(one, str(tmp_path / "delta.parquet"), use_dictionary=False, column_encoding={"values": "DELTA_LENGTH_BYTE_ARRAY"})
    assert reason(delta) == (None, "row group 0: a data page with encoding 6")
    values = one.column("values").to_pylist()
    values[3] = None
    holes = pa.table({"key": one.column("key"), "values": pa.array(values, pa.string())})
    nulls = RU._write(holes, str(tmp_path / "nulls.parquet"), use_dictionary=False, data_page_version="2.0")
    assert reason(nulls) == (None, "row group 0: a v2 page with nulls")
    nulls_dict = RU._write(holes, str(tmp_path / "nulls_dict.parquet"), data_page_version="2.0")
    assert reason(nulls_dict) == (None, "row group 0: a v2 page with nulls")
    # v1 pages with levels in one row group, v2 pages in the next: one scene whose needed pages mix both
    with pq.ParquetWriter(str(tmp_path / "a.parquet"), one.schema) as w:
        w.write_table(one.slice(0, 4))
    with pq.ParquetWriter(str(tmp_path / "b.parquet"), one.schema, data_page_version="2.0") as w:
        w.write_table(one.slice(4))
    from mspa import parquet_splice
    mixed = str(tmp_path / "mixed.parquet")
    with open(mixed, "wb") as f:
        f.write(parquet_splice.splice([open(str(tmp_path / "a.parquet"), "rb").read(), open(str(tmp_path / "b.parquet"), "rb").read()]))
    assert pq.read_table(mixed).equals(one)
    assert reason(mixed) == (None, "v1 pages with levels and v2 pages in one scene")
    index = visindex.SceneRowGroups(mixed)
    assert index._plan_pages(sorted(set(index.image_rows(RU.SCENE, IDS).values())))[1] == "row group 0: a data page that is not PLAIN"


def test_decode_stats_have_the_new_counters(files):
    stats = visindex.SceneRowGroups(files["defaults"]).decode_stats
    assert stats["dict_pages"] == 0 and stats["v2_pages"] == 0
