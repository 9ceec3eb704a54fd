"""The visibility index read as LISTS on the MI355X: mspa_index_lists_pick_device alone (through ``engine.index_lists_pick``) on a
hand-made CSR with every status provoked as data, ``SceneRowGroups.scene_lists`` against ``json.loads`` on every file of the page
tests with ``page_kinds = "any"``, and the edge rows -- duplicates and a descending row are lists like any other here."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "multi-spatialmllm_amd")
for p in (PKG, ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import index_lists_util as LU  # noqa: E402
import visindex_decode_util as VU  # noqa: E402

# ------------------------------------------------------------------------------------------------------------------- the kernel alone
ROWS = [[], [7], [1, 1, 5, 5, 5, 700]]
SENTINEL = -77


def _csr():
    import torch
    values = torch.tensor([v for r in ROWS for v in r], dtype=torch.int32, device="cuda")
    offsets = torch.tensor(np.concatenate([[0], np.cumsum([len(r) for r in ROWS])]), dtype=torch.int64, device="cuda")
    return values, offsets


def _expected(row, position, n_points, rows=ROWS):
    from mspa import _lib
    if not 0 <= row < len(rows):
        return -1, _lib.PICK_EROW
    if not 0 <= position < len(rows[row]):
        return -1, _lib.PICK_EPOSITION
    v = rows[row][position]
    return (v, 0) if 0 <= v < n_points else (-1, _lib.PICK_ERANGE)


# a bad sample of every kind between good ones: row -1 and n_rows, position -1 and count, a position on the empty row
MIXED = [(2, 3), (-1, 0), (1, 0), (3, 0), (2, 0), (2, -1), (2, 5), (2, 6), (1, 1), (0, 0), (1, 0), (0, -1), (2, 4), (1 << 40, 0), (2, 1 << 40)]


@pytest.mark.parametrize("blocks, extra", [(1, -1), (1, 0), (1, 1), (0, 0), (3, 5)])      # one below, at, one above the block size; none; several
@pytest.mark.parametrize("n_points", [701, 700])
def test_pick_kernel_on_a_hand_made_csr(blocks, extra, n_points):
    import torch
    from mspa import _lib, engine
    n = blocks * _lib.PICK_BLOCK + extra
    values, offsets = _csr()
    samples = [MIXED[k % len(MIXED)] for k in range(n)]
    table = torch.tensor(samples, dtype=torch.int64, device="cuda").reshape(n, 2)
    vertex, status = engine.index_lists_pick(values, offsets, table, n_points)
    assert vertex.is_cuda and status.is_cuda and str(vertex.dtype) == str(status.dtype) == "torch.int32" and tuple(vertex.shape) == tuple(status.shape) == (n,)
    want = [_expected(r, p, n_points) for r, p in samples]
    assert vertex.tolist() == [w[0] for w in want] and status.tolist() == [w[1] for w in want]
    if n:                                                                      # value 700 with n_points = 700 is declined, 701 takes it
        assert (int(vertex[6]), int(status[6])) == ((700, 0) if n_points == 701 else (-1, _lib.PICK_ERANGE))
        assert (int(vertex[0]), int(status[0])) == (5, 0) and (int(vertex[12]), int(status[12])) == (5, 0)      # list[3] and list[4] of the duplicates


def test_pick_kernel_offsets_that_leave_the_values_and_untouched_neighbours():
    import torch
    from mspa import _lib, engine
    values, offsets = _csr()
    bad = offsets.clone()
    bad[-1] = values.numel() + 1                                               # the last row would end behind the values
    table = torch.tensor([(2, 0), (1, 0), (0, 0), (2, 6)], dtype=torch.int64, device="cuda")
    vertex, status = engine.index_lists_pick(values, bad, table, 701)
    assert status.tolist() == [_lib.PICK_EOFFSETS, 0, _lib.PICK_EPOSITION, _lib.PICK_EOFFSETS] and vertex.tolist() == [-1, 7, -1, -1]
    descending = torch.tensor([0, 1, 0, 7], dtype=torch.int64, device="cuda")  # row 1 ends in front of its start; rows 0 and 2 are lists (of other values)
    vertex, status = engine.index_lists_pick(values, descending, table, 701)
    assert status.tolist() == [0, _lib.PICK_EOFFSETS, 0, 0] and vertex.tolist() == [7, -1, 7, 700]
    negative = torch.tensor([-1, 1, 1, 7], dtype=torch.int64, device="cuda")
    assert engine.index_lists_pick(values, negative, table, 701)[1].tolist() == [0, _lib.PICK_EPOSITION, _lib.PICK_EOFFSETS, _lib.PICK_EPOSITION]
    # no values at all: every row is empty, nothing is read
    none = torch.zeros((0,), dtype=torch.int32, device="cuda")
    vertex, status = engine.index_lists_pick(none, torch.zeros((4,), dtype=torch.int64, device="cuda"), table, 701)
    assert status.tolist() == [_lib.PICK_EPOSITION] * 4 and vertex.tolist() == [-1] * 4
    assert engine.index_lists_pick(none, torch.zeros((1,), dtype=torch.int64, device="cuda"), table, 701)[1].tolist() == [_lib.PICK_EROW] * 4
    # the C ABI writes entries [0, n_samples) of its outputs and nothing behind them
    lib = _lib.load()
    n = _lib.PICK_BLOCK + 1
    table = torch.tensor([MIXED[k % len(MIXED)] for k in range(n + 8)], dtype=torch.int64, device="cuda")
    out = torch.full((2, n + 8), SENTINEL, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    assert lib.mspa_index_lists_pick_device(values.data_ptr(), values.numel(), offsets.data_ptr(), 3, table.data_ptr(), n, 701, out[0].data_ptr(),
                                            out[1].data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert out[:, n:].eq(SENTINEL).all() and out[1, :n].tolist() == [_expected(*MIXED[k % len(MIXED)], 701)[1] for k in range(n)]


def test_pick_wrapper_and_c_abi_refuse_wrong_arguments():
    import torch
    from mspa import _lib, engine
    lib = _lib.load()
    values, offsets = _csr()
    table = torch.tensor([(2, 0)], dtype=torch.int64, device="cuda")
    for bad in (lambda: engine.index_lists_pick(values.to(torch.int64), offsets, table, 701),          # dtype
                lambda: engine.index_lists_pick(values, offsets.to(torch.int32), table, 701),
                lambda: engine.index_lists_pick(values, offsets, table.to(torch.int32), 701),
                lambda: engine.index_lists_pick(values, offsets, table.reshape(2), 701),               # shape
                lambda: engine.index_lists_pick(values, offsets, table.reshape(2, 1), 701),
                lambda: engine.index_lists_pick(values, offsets[:0], table, 701),
                lambda: engine.index_lists_pick(values.reshape(1, -1), offsets, table, 701),
                lambda: engine.index_lists_pick(values.cpu(), offsets, table, 701),                    # device
                lambda: engine.index_lists_pick(values, offsets.cpu(), table, 701),
                lambda: engine.index_lists_pick(values, offsets, table.cpu(), 701),
                lambda: engine.index_lists_pick(values, offsets, [(2, 0)], 701),
                lambda: engine.index_lists_pick(values, offsets, table, -1),                           # n_points
                lambda: engine.index_lists_pick(values, offsets, table, 1 << 31)):
        with pytest.raises(ValueError, match="mspa.engine"):
            bad()
    out = torch.full((2, 1), SENTINEL, dtype=torch.int32, device="cuda")
    v, o, t, a, b = values.data_ptr(), offsets.data_ptr(), table.data_ptr(), out[0].data_ptr(), out[1].data_ptr()
    for args in ((None, 7, o, 3, t, 1, 701, a, b), (v, 7, None, 3, t, 1, 701, a, b), (v, 7, o, 3, None, 1, 701, a, b), (v, 7, o, 3, t, 1, 701, None, b),
                 (v, 7, o, 3, t, 1, 701, a, None), (v, -1, o, 3, t, 1, 701, a, b), (v, 7, o, -1, t, 1, 701, a, b), (v, 7, o, 3, t, -1, 701, a, b),
                 (v, 7, o, 3, t, 1, -1, a, b), (v, 7, o, 3, t, 1, 1 << 31, a, b), (v, 7, o, 3, t, (0x7fffffff * _lib.PICK_BLOCK) + 1, 701, a, b)):
        assert lib.mspa_index_lists_pick_device(*args, None) == _lib.MSPA_EINVAL, args
        assert b"mspa_index_lists_pick_device" in lib.mspa_last_error_string()
    assert lib.mspa_index_lists_pick_device(None, 0, None, 0, None, 0, 701, None, None, None) == 0     # no samples: no launch, nothing read
    torch.cuda.synchronize()
    assert out.eq(SENTINEL).all()


# ------------------------------------------------------------------------------------------------------------------- scene_lists
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return VU.index_files(tmp_path_factory.mktemp("index_files"))


NAMES = ("many_pages", "page_per_row", "uncompressed", "defaults", "v2", "two_scenes", "two_groups", "split_images", "assembled")


@pytest.mark.parametrize("name", NAMES)
def test_scene_lists_equals_json_loads(files, name):
    from mspa import visindex
    path, scenes, _ = files[name]
    index = visindex.SceneRowGroups(path)
    index.page_kinds = "any"
    for scene_id in scenes:
        ids, texts = VU.image_ids_of(path, scene_id)
        n_points = 5000 if scene_id == "scene0000_00" else 3000
        request = [ids[-1], "99999"] + ids[:-1]                               # not in file order, one image the index lacks
        lists = index.scene_lists(scene_id, request)
        assert lists.present == [ids[-1]] + ids[:-1] and lists.values.is_cuda and str(lists.values.dtype) == "torch.int32"
        want = {i: json.loads(texts[i]) for i in ids}
        assert lists.counts.tolist() == [len(want[i]) for i in lists.present]
        samples = [(i, j) for i in lists.present for j in range(len(want[i]))]
        got = lists.pick(samples, n_points)                                   # ONE pick of every (image, position) pair
        assert got.is_cuda and str(got.dtype) == "torch.int32" and got.tolist() == [want[i][j] for i, j in samples]
        with pytest.raises(ValueError) as e:
            lists.count("99999")
        assert str(e.value) == LU.key_message(scene_id, "99999")
    assert index.decode_stats["scenes"] == len(scenes) and index.decode_stats["scenes_declined"] == 0, index.last_decline
    assert index.decode_stats["rows_declined"] == 0 and index.decode_stats["h2d_bytes"] > 0
    if name in ("defaults", "v2"):
        assert index.decode_stats["dict_pages" if name == "defaults" else "v2_pages"] > 0
    assert index.scene_lists("scene0000_00", ["99999"]).present == []         # nothing of the request is there
    assert index.scene_lists("scene4040_00", ["00000"]).present == []         # a scene the index lacks


def test_scene_lists_on_the_edge_rows(tmp_path):
    from mspa import visindex
    index = visindex.SceneRowGroups(LU.edge_file(tmp_path))
    index.page_kinds = "any"
    lists = index.scene_lists(LU.SCENE, LU.edge_request())
    assert lists.values.is_cuda and index.decode_stats["scenes_declined"] == 0, index.last_decline
    # the device takes the duplicates and the descending row: only the row K11's parser declines goes to the host
    assert index.decode_stats["rows_declined"] == len(LU.PARSER_DECLINES) and index.decode_stats["rows"] == len(LU.EDGE_ROWS)
    assert sorted(lists._texts) == sorted(LU.PARSER_DECLINES) and json.loads(lists._texts["negative"]) == [-1]
    LU.check_edge_lists(lists)
    assert lists.pick([("duplicate", 3), ("long", 29999)], LU.N_POINTS).is_cuda
    assert lists.pick([("one", 0), ("float", 1)], LU.N_POINTS).is_cuda


def test_a_scene_the_device_does_not_take_comes_in_the_host_form(tmp_path):
    import pyarrow.parquet as pq
    from mspa import visindex
    path = os.path.join(str(tmp_path), "gzip.parquet")
    pq.write_table(pq.read_table(LU.edge_file(tmp_path)), path, compression="gzip")
    index = visindex.SceneRowGroups(path)
    index.page_kinds = "any"
    lists = index.scene_lists(LU.SCENE, LU.edge_request())
    assert lists.values is None and index.decode_stats["scenes_declined"] == 1 and "GZIP" in index.last_decline
    LU.check_edge_lists(lists)
    assert lists.pick([("one", 0)], LU.N_POINTS).is_cuda                      # the same interface: vertices on the device
