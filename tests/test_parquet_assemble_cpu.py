"""``parquet_splice.assemble_row_group`` on the CPU: the values pages come from the library's host reference
(mspa_snappy_compress_host over the page payloads of csrc/snappy_core.h), the file must read like pyarrow's own encode of the
same table, splice with pyarrow-encoded row groups on either side and keep the key statistics the scene reader needs."""
import io
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import snappy_util as SU  # noqa: E402

from mspa import _lib, parquet_splice, visindex  # noqa: E402

PAGE_BYTES = 4096


@pytest.fixture(scope="module")
def files():
    lib = _lib.load()
    table = SU.index_table()
    offsets, data = SU.string_buffers(table.column("values"))
    pages = SU.host_pages(lib, offsets, data, PAGE_BYTES)
    assert len(pages["compressed"]) > 20 and pages["num_values"][0] == 1          # an image row alone fills its page
    ours = parquet_splice.assemble_row_group(table.select(["key"]), "values", pages["chunk"], pages["compressed"],
                                             pages["uncompressed"], pages["num_values"], use_dictionary=False)
    theirs = bytes(parquet_splice.encode_row_group(table, use_dictionary=False))
    # the same rows in pages of the default size, pyarrow's own geometry: what the size cap compares (a page is compressed on
    # its own, so forty 4 KiB pages cost any Snappy a quarter more than one page of 130 KB -- Google's included)
    big = SU.host_pages(lib, offsets, data, 1 << 20)
    ours_default = parquet_splice.assemble_row_group(table.select(["key"]), "values", big["chunk"], big["compressed"],
                                                     big["uncompressed"], big["num_values"], use_dictionary=False)
    return table, ours, theirs, ours_default


def test_reads_equal_to_the_host_encoded_file_schema_metadata_included(files):
    import pandas as pd
    import pyarrow.parquet as pq
    table, ours, theirs, _ = files
    a, b = pq.read_table(io.BytesIO(ours)), pq.read_table(io.BytesIO(theirs))
    assert a.equals(b) and a.equals(table) and a.schema.equals(b.schema, check_metadata=True)
    fa, fb = pq.ParquetFile(io.BytesIO(ours)), pq.ParquetFile(io.BytesIO(theirs))
    assert fa.schema.equals(fb.schema) and fa.metadata.metadata == fb.metadata.metadata
    assert fa.metadata.created_by == fb.metadata.created_by and fa.metadata.num_rows == table.num_rows
    pd.testing.assert_frame_equal(pd.read_parquet(io.BytesIO(ours)), pd.read_parquet(io.BytesIO(theirs)))
    col = fa.metadata.row_group(0).column(1)
    assert col.compression == "SNAPPY" and col.physical_type == "BYTE_ARRAY" and set(col.encodings) == {"PLAIN", "RLE"}
    assert col.num_values == table.num_rows and not col.is_stats_set
    assert col.data_page_offset == 4 + fa.metadata.row_group(0).column(0).total_compressed_size


def test_key_statistics_survive_and_the_values_chunk_is_no_larger_than_1_10_of_pyarrows(files):
    import pyarrow.parquet as pq
    table, ours, theirs, ours_default = files
    ma, mb = pq.ParquetFile(io.BytesIO(ours)).metadata.row_group(0), pq.ParquetFile(io.BytesIO(theirs)).metadata.row_group(0)
    sa, sb = ma.column(0).statistics, mb.column(0).statistics
    assert sa.has_min_max and (sa.min, sa.max) == (sb.min, sb.max)
    assert pq.read_table(io.BytesIO(ours_default)).equals(table)
    md = pq.ParquetFile(io.BytesIO(ours_default)).metadata.row_group(0)
    ours_size, theirs_size = md.column(1).total_compressed_size, mb.column(1).total_compressed_size
    print(f"values chunk: {ours_size} bytes, pyarrow's {theirs_size} ({ours_size / theirs_size:.3f} x)")
    assert ours_size <= 1.10 * theirs_size
    assert ma.total_byte_size == ma.column(0).total_uncompressed_size + ma.column(1).total_uncompressed_size


def test_splices_before_and_after_a_pyarrow_row_group_and_the_scene_reader_finds_the_scene(files, tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    table, ours, _theirs, _ = files
    other = SU.index_table("scene0001_00", n_images=3, n_points=40, seed=9)
    other_file = parquet_splice.encode_row_group(other, use_dictionary=False)
    for order, name in (((ours, other_file), "ours_first"), ((other_file, ours), "ours_last")):
        path = str(tmp_path / f"{name}.parquet")
        parquet_splice.splice(list(order), open(path, "wb"))
        want = pa.concat_tables([table, other] if order[0] is ours else [other, table])
        got = pq.read_table(path)
        assert got.equals(want) and pq.ParquetFile(path).metadata.num_row_groups == 2
        groups = visindex.SceneRowGroups(path)
        assert groups.scene_dict("scene0000_00") == dict(zip(table.column("key").to_pylist(), table.column("values").to_pylist()))
        assert len(groups.scene_dict("scene0001_00")) == other.num_rows and groups._mixed == []


def test_pages_that_do_not_hold_the_rows_are_refused(files):
    table, _ours, _theirs, _ = files
    with pytest.raises(ValueError):
        parquet_splice.assemble_row_group(table.select(["key"]), "values", b"abc", [3], [3], [table.num_rows - 1])
    with pytest.raises(ValueError):
        parquet_splice.assemble_row_group(table.select(["key"]), "values", b"abc", [4], [3], [table.num_rows])
