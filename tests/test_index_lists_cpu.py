"""The visibility index read as LISTS, without a GPU: ``SceneRowGroups.scene_lists(..., device="cpu")`` gives the host form of
``IndexLists`` -- the interface the depth builders use with ``MSPA_VISINDEX_DECODE=device`` -- checked against ``json.loads`` on
the files of the page tests and on the edge rows; the reader route and the pick constants import without a GPU."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import index_lists_util as LU  # noqa: E402
import visindex_decode_util as VU  # noqa: E402

from mspa import visindex  # noqa: E402


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return VU.index_files(tmp_path_factory.mktemp("index_files"))


NAMES = ("many_pages", "page_per_row", "uncompressed", "defaults", "v2", "two_scenes", "two_groups", "split_images", "assembled")


@pytest.mark.parametrize("name", NAMES)
def test_host_form_equals_json_loads(files, name):
    path, scenes, _ = files[name]
    index = visindex.SceneRowGroups(path)
    for scene_id in scenes:
        ids, texts = VU.image_ids_of(path, scene_id)
        n_points = 5000 if scene_id == "scene0000_00" else 3000
        request = [ids[-1], "99999"] + ids[:-1]                               # not in file order, one image the index lacks
        lists = index.scene_lists(scene_id, request, device="cpu")
        assert isinstance(lists, visindex.IndexLists) and lists.present == [ids[-1]] + ids[:-1]
        want = {i: json.loads(texts[i]) for i in ids}
        assert lists.counts.dtype.name == "int64" and lists.counts.tolist() == [len(want[i]) for i in lists.present]
        samples = [(i, j) for i in lists.present for j in range(len(want[i]))]
        got = lists.pick(samples, n_points)
        assert str(got.dtype) == "torch.int32" and str(got.device) == "cpu" and got.tolist() == [want[i][j] for i, j in samples]
        some = lists.present[1]
        assert lists.count(some) == len(want[some])
        with pytest.raises(ValueError) as e:
            lists.count("99999")
        assert str(e.value) == LU.key_message(scene_id, "99999")
        with pytest.raises(IndexError):
            lists.pick([(some, len(want[some]))], n_points)                   # position == count
        top = max(want[some])
        with pytest.raises(ValueError, match=f"{scene_id}.*{some}.*{top}"):
            lists.pick([(some, want[some].index(top))], top)                  # a vertex >= n_points
    assert index.decode_stats["scenes"] == len(scenes) and index.decode_stats["scenes_declined"] == 0     # asked for, not declined
    assert index.scene_lists("scene4040_00", ["00000"], device="cpu").present == []                          # a scene the index lacks


def test_host_form_on_the_edge_rows(tmp_path):
    index = visindex.SceneRowGroups(LU.edge_file(tmp_path))
    LU.check_edge_lists(index.scene_lists(LU.SCENE, LU.edge_request(), device="cpu"))


def test_a_row_that_is_no_json_raises_where_the_handler_raises(tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    path = os.path.join(str(tmp_path), "broken.parquet")
    pq.write_table(pa.table({"key": pa.array(["s:image_to_points:a", "s:image_to_points:b"]), "values": pa.array(["[1, 2", "[1.5, 2]"])}), path)
    lists = visindex.SceneRowGroups(path).scene_lists("s", ["a", "b"], device="cpu")            # reading the scene raises nothing
    with pytest.raises(json.JSONDecodeError):
        lists.count("a")
    assert lists.count("b") == 2 and lists.pick([("b", 0), ("b", 1)], 10).tolist() == [1, 2]    # int(), as list_point_numerics


def test_route_and_constants_import_without_a_gpu(monkeypatch):
    from mspa import _lib
    assert (_lib.PICK_OK, _lib.PICK_EROW, _lib.PICK_EPOSITION, _lib.PICK_ERANGE, _lib.PICK_EOFFSETS) == (0, 1, 2, 4, 8)
    assert _lib.PICK_BLOCK == 256 and "mspa_index_lists_pick_device" in _lib.exported_symbols()
    monkeypatch.delenv("MSPA_VISINDEX_DECODE", raising=False)
    assert visindex.index_reader_route("a/vis.parquet") == "handler" and visindex.index_reader_route("a/vis.pkl") == "handler"
    monkeypatch.setenv("MSPA_VISINDEX_DECODE", "device")
    assert visindex.index_reader_route("a/vis.parquet") == "lists" and visindex.index_reader_route("a/vis.pkl") == "handler"
    monkeypatch.setenv("MSPA_VISINDEX_DECODE", "gpu")
    for path in ("a/vis.parquet", "a/vis.pkl"):
        with pytest.raises(ValueError, match="MSPA_VISINDEX_DECODE"):
            visindex.index_reader_route(path)
