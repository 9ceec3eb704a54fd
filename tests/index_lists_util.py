"""What tests/test_index_lists_cpu.py and tests/test_gpu_index_lists.py share: the edge file of the index read as LISTS (the rows of
tests/test_gpu_visindex_decode.py's EDGE_ROWS restated, one page per row) and the check of an ``IndexLists`` against ``json.loads``."""
import json
import os

import pytest

N_POINTS = 65536

EDGE_ROWS = {
    "empty": "[]",
    "duplicate": "[1, 1, 5, 5, 5, 700]",
    "descending": "[5, 3]",
    "bit63": "[0, 63, 64, 127, 128, 65471]",
    "spaces": " [ 1,2 ,\n3,\t64 ] ",
    "negative": "[-1]",
    "one": "[7]",
    "long": json.dumps(list(range(1, 60001, 2))),                             # 30 000 values, 190 KB of text behind 4 KiB pages
    "last": json.dumps([0, N_POINTS - 1]),                                    # the last vertex
    "beyond": json.dumps([3, N_POINTS]),                                      # the first one that is none
    "float": "[2.0, 9]",                                                      # no list for the device; int() of it on the host
}
# the rows K11's parser declines (a '-'); order and duplicates are the bits kernel's rules, not the lists'
PARSER_DECLINES = ("negative", "float")
SCENE = "sceneE"


def edge_file(directory):
    import pyarrow as pa
    import pyarrow.parquet as pq
    keys = [f"{SCENE}:image_to_points:{k}" for k in EDGE_ROWS] + [f"{SCENE}:point_to_images:{v}" for v in range(40)]
    values = list(EDGE_ROWS.values()) + ['["empty"]'] * 40
    path = os.path.join(str(directory), "edge_lists.parquet")
    pq.write_table(pa.table({"key": pa.array(keys, pa.string()), "values": pa.array(values, pa.string())}), path, use_dictionary=False,
                   data_page_size=4096, write_batch_size=1)
    return path


def key_message(scene_id, image_id):
    """VisibilityInfoHandler._get's message for a key the parquet index lacks."""
    return f"Key {scene_id}:image_to_points:{image_id} not found in visibility info."


def check_edge_lists(lists):
    """The edge file's rows through ``lists`` (requested: "long", "absent", every other row, "one" again), either form."""
    request = edge_request()
    assert lists.present == [k for k in request if k != "absent"]                       # request order, the repeat kept
    want = {k: json.loads(v) for k, v in EDGE_ROWS.items()}
    assert lists.counts.dtype.name == "int64" and lists.counts.tolist() == [len(want[k]) for k in lists.present]
    assert lists.count("empty") == 0 and lists.count("duplicate") == 6 and lists.count("long") == 30000
    # duplicates and order are the text's: what no bitset keeps
    got = lists.pick([("duplicate", 3), ("descending", 0), ("descending", 1), ("duplicate", 5), ("one", 0)], N_POINTS)
    assert str(got.dtype) == "torch.int32" and got.tolist() == [5, 5, 3, 700, 7]
    assert lists.pick([("long", 0), ("long", 14999), ("long", 29999)], N_POINTS).tolist() == [1, 29999, 59999]
    assert lists.pick([("last", 1), ("bit63", 5), ("spaces", 3), ("beyond", 0)], N_POINTS).tolist() == [N_POINTS - 1, 65471, 64, 3]
    every = [(k, j) for k in want for j in range(len(want[k])) if k not in ("negative", "beyond")]
    assert lists.pick(every, N_POINTS).tolist() == [want[k][j] for k, j in every]
    mixed = lists.pick([("one", 0), ("float", 0), ("spaces", 2), ("float", 1)], N_POINTS)           # rows of both kinds in one call
    assert str(mixed.dtype) == "torch.int32" and mixed.tolist() == [7, 2, 3, 9]
    with pytest.raises(ValueError, match=f"{SCENE}.*beyond.*{N_POINTS}"):
        lists.pick([("one", 0), ("beyond", 1)], N_POINTS)
    assert lists.count("negative") == 1
    with pytest.raises(ValueError, match=f"{SCENE}.*negative.*-1"):                      # served from its text as [-1]
        lists.pick([("negative", 0)], N_POINTS)
    with pytest.raises(ValueError, match="700"):                                         # the width is the call's
        lists.pick([("duplicate", 5)], 700)
    assert lists.pick([("duplicate", 5)], 701).tolist() == [700]
    for image, position in (("empty", 0), ("one", 1), ("duplicate", 6), ("long", 30000), ("one", -1), ("negative", 1)):
        with pytest.raises(IndexError):
            lists.pick([("one", 0), (image, position)], N_POINTS)
    for call in (lambda: lists.count("absent"), lambda: lists.pick([("one", 0), ("absent", 0)], N_POINTS)):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == key_message(SCENE, "absent")
    with pytest.raises(IndexError):                                                      # the first bad sample decides
        lists.pick([("one", 1), ("absent", 0), ("beyond", 1)], N_POINTS)
    assert lists.pick([], N_POINTS).tolist() == []


def edge_request():
    return ["long", "absent"] + [k for k in EDGE_ROWS if k != "long"] + ["one"]
