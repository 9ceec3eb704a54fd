"""The host half of the index's way back, without a GPU: the page table ``visindex.SceneRowGroups`` reads off the thrift page
headers, the rows the ``key`` column gives, the pages those rows need and which files the device path takes -- against a
pure-Python walk of the decompressed pages (tests/visindex_decode_util.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import visindex_decode_util as VU  # noqa: E402

from mspa import visindex  # noqa: E402


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return VU.index_files(tmp_path_factory.mktemp("index_files"))


NAMES = ("many_pages", "page_per_row", "uncompressed", "defaults", "v2", "two_scenes", "two_groups", "split_images", "assembled")


def test_the_file_set_is_the_one_the_tests_name(files):
    assert tuple(files) == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_page_table_rows_and_needed_pages_equal_a_python_walk(files, name):
    path, scenes, device_takes = files[name]
    index = visindex.SceneRowGroups(path)
    for scene_id in scenes:
        ids, texts = VU.image_ids_of(path, scene_id)
        request = [ids[-1], "99999"] + ids[:-1]                               # not in file order, and one image the index lacks
        found = index.image_rows(scene_id, request)
        assert sorted(found) == [0] + list(range(2, len(request)))
        for g in sorted({g for g, _ in found.values()}):
            walk = VU.python_page_walk(path, g)
            table = index.values_pages(g)
            assert len(table["pos"]) == len(walk)
            assert table["type"].tolist() == [w[0] for w in walk]
            assert [e for e, w in zip(table["encoding"].tolist(), walk) if w[0] == 0] == [w[1] for w in walk if w[0] == 0]
            where = {row: (k, text) for k, w in enumerate(walk) for row, text in w[2]}      # row -> (page, text) for PLAIN v1 pages
            rows = [r for gg, r in found.values() if gg == g]
            _, page, reason = index.needed_pages(g, rows)
            assert (reason is None) == device_takes, (name, reason)
            if not device_takes:
                continue
            assert page.tolist() == [where[r][0] for r in rows]
            for k, (gg, r) in found.items():
                if gg == g:
                    assert where[r][1].decode() == texts[request[k]]
            for k in np.unique(page):                                          # the table's numbers describe these pages
                first = int(table["first_row"][k])
                assert [row for row, _ in walk[k][2]] == list(range(first, first + int(table["num_values"][k])))


def test_the_files_have_the_shapes_the_cases_are_about(files):
    def pages_of(name, scene="scene0000_00"):
        path = files[name][0]
        index = visindex.SceneRowGroups(path)
        ids, _ = VU.image_ids_of(path, scene)
        found = index.image_rows(scene, ids)
        out = {}
        for g in sorted({g for g, _ in found.values()}):
            out[g] = index.needed_pages(g, [r for gg, r in found.values() if gg == g])
        return index, out

    index, per = pages_of("page_per_row")
    table, page, _ = per[0]
    assert len(set(page.tolist())) == 8 and int(table["uncompressed"][page].min()) > 4096      # image rows larger than a page
    assert len(pages_of("many_pages")[1][0][0]["pos"]) > 1
    assert pages_of("uncompressed")[1][0][0]["codec"] == "UNCOMPRESSED"
    table, _, reason = pages_of("defaults")[1][0]
    assert table["type"][0] == 2 and "PLAIN" in reason                                          # the dictionary page in front
    assert "v1" in pages_of("v2")[1][0][2]
    index, per = pages_of("two_scenes", "scene0001_00")
    assert index._mixed and not index._by_scene and int(per[0][1].min()) > 0                    # one group, scene 1 not on its first page
    assert sorted(pages_of("split_images")[1]) == [0, 1]
    assert len(visindex.SceneRowGroups(files["two_groups"][0])._by_scene["scene0000_00"]) == 2
    assert len(set(pages_of("assembled")[1][0][1].tolist())) > 1


def test_the_plan_of_scene_bits_names_the_pages_a_python_walk_finds_the_rows_in(files, tmp_path):
    """Step 1 of ``scene_bits`` (``_plan_pages``: host code, no device): for scenes whose rows span several pages -- and, in
    split_images, two row groups -- the plan holds exactly the pages of the walk that hold those rows, in file order, with the
    headers' sizes, the rows counted from each page's first row and the pages' bytes back to back; for a file the device path
    does not take it gives ``needed_pages``' reason behind the row group."""
    import pyarrow as pa
    for name in ("page_per_row", "assembled", "split_images"):
        path = files[name][0]
        index = visindex.SceneRowGroups(path)
        ids, texts = VU.image_ids_of(path, "scene0000_00")
        distinct = sorted(set(index.image_rows("scene0000_00", ids).values()))
        pages, why = index._plan_pages(distinct)
        assert why is None and len(pages) > 1, name
        want = []
        for g in sorted({g for g, _ in distinct}):
            walk = VU.python_page_walk(path, g)
            where = {row: k for k, w in enumerate(walk) for row, _ in w[2]}
            rows = [r for gg, r in distinct if gg == g]
            for k in sorted({where[r] for r in rows}):
                first = walk[k][2][0][0]
                want.append((g, k, walk[k][3][0], walk[k][3][1], len(walk[k][2]), [r - first for r in rows if where[r] == k]))
        assert [(p.group, p.index, p.compressed, p.uncompressed, p.num_values, p.rows.tolist()) for p in pages] == want, name
        assert [p.src for p in pages] == np.concatenate([[0], np.cumsum([p.compressed for p in pages])])[:-1].tolist()
        assert all(p.snappy and len(p.data) == p.compressed for p in pages)
        seen = []
        for p in pages:                                                          # the bytes are those pages': the wanted texts are in them
            body = pa.Codec("snappy").decompress(p.data.tobytes(), decompressed_size=p.uncompressed).to_pybytes()
            seen += [i for i in ids if texts[i].encode() in body]
        assert sorted(seen) == sorted(ids), name
    gz = VU._write(VU.SU.index_table(), str(tmp_path / "gzip.parquet"), use_dictionary=False, compression="gzip")
    for path, reason in ((files["defaults"][0], "row group 0: a data page that is not PLAIN"),
                         (files["v2"][0], "row group 0: a data page that is not v1"), (gz, "row group 0: codec GZIP")):
        index = visindex.SceneRowGroups(path)
        ids, _ = VU.image_ids_of(path, "scene0000_00")
        assert index._plan_pages(sorted(set(index.image_rows("scene0000_00", ids).values()))) == (None, reason)


def test_decode_mode_reads_the_switch(monkeypatch):
    monkeypatch.delenv("MSPA_VISINDEX_DECODE", raising=False)
    assert visindex.decode_mode() == "host"
    monkeypatch.setenv("MSPA_VISINDEX_DECODE", " Device ")
    assert visindex.decode_mode() == "device"
    monkeypatch.setenv("MSPA_VISINDEX_DECODE", "")
    assert visindex.decode_mode() == "host"
    monkeypatch.setenv("MSPA_VISINDEX_DECODE", "gpu")
    with pytest.raises(ValueError, match="MSPA_VISINDEX_DECODE"):
        visindex.decode_mode()
