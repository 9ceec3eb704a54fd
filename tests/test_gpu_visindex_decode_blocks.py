"""``visindex.SceneRowGroups.scene_bits`` through the Snappy decoder's block route on the MI355X: a scene whose image rows share
ONE page of pyarrow's (the layout every index written on the host has), the same rows in K12's layout with small pages, and a
page with a damaged byte -- against the host path's bitsets, with the ``decode_stats`` counters that say which route ran."""
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

import snappy_blocks_util as BU  # noqa: E402

SCENE, N_IMAGES, N_POINTS = "scene0000_00", 8, 40000
IDS = [f"{k * 10:05d}" for k in range(N_IMAGES)]


@pytest.fixture(scope="module")
def seen():
    return np.random.default_rng(3).random((N_IMAGES, N_POINTS)) < 0.3


@pytest.fixture(scope="module")
def want(seen):
    from mspa.scene import pack_index_lists
    return pack_index_lists([np.nonzero(row)[0].tolist() for row in seen], N_POINTS)


@pytest.fixture(scope="module")
def pyarrow_file(tmp_path_factory, seen):
    """pyarrow's layout: image rows first, then the point rows; the eight image rows (about 650 KB of text) share the first page."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    keys = [f"{SCENE}:image_to_points:{i}" for i in IDS] + [f"{SCENE}:point_to_images:{v}" for v in range(N_POINTS)]
    values = [json.dumps(np.nonzero(seen[k])[0].tolist()) for k in range(N_IMAGES)]
    values += [json.dumps([IDS[k] for k in np.nonzero(seen[:, v])[0]]) for v in range(N_POINTS)]
    path = str(tmp_path_factory.mktemp("blocks_index") / "pyarrow.parquet")
    pq.write_table(pa.table({"key": pa.array(keys, type=pa.string()), "values": pa.array(values, type=pa.string())}), path, use_dictionary=False)
    return path


@pytest.fixture(scope="module")
def k12_file(tmp_path_factory, want):
    """K12's layout: the values chunk written on the device, pages of 128 KiB of PLAIN bytes (two image rows, three blocks each)."""
    import torch
    from mspa import parquet_splice, visindex
    path = str(tmp_path_factory.mktemp("blocks_index_k12") / "k12.parquet")
    csr = visindex.from_bits(torch.from_numpy(want).cuda(), IDS, N_POINTS, text=True, indices=False, pages=True, page_bytes=1 << 17)
    assert csr.values_pages is not None
    with parquet_splice.SplicedParquetWriter(path) as w:
        w.append(csr.to_row_group(SCENE))
    return path


def _first_page(index):
    """(position in the file, compressed size, uncompressed size) of the page that holds the first image row."""
    found = index.image_rows(SCENE, IDS[:1])
    g, row = found[0]
    table, page, reason = index.needed_pages(g, [row])
    assert reason is None and table["codec"] == "SNAPPY"
    pg = int(page[0])
    return table["start"] + int(table["pos"][pg]), int(table["compressed"][pg]), int(table["uncompressed"][pg])


def _check(path, want, min_pages):
    from mspa import visindex
    index = visindex.SceneRowGroups(path)
    _, comp, unc = _first_page(index)
    present, bits = index.scene_bits(SCENE, IDS, N_POINTS)
    host_present, host_bits = index._scene_bits_host(SCENE, IDS, N_POINTS, "cuda")
    assert present == host_present == IDS
    assert np.array_equal(bits.cpu().numpy(), host_bits.cpu().numpy()) and np.array_equal(bits.cpu().numpy(), want)
    stats = index.decode_stats
    assert stats["scenes_declined"] == 0 and stats["rows_declined"] == 0, index.last_decline
    assert stats["blocks"] >= 8 and stats["serial_streams"] == 0, stats
    assert stats["blocks"] >= 2 * min_pages and BU.block_count(unc) >= 2      # every needed page has two blocks or more
    # the one-wave route gives the same, and says so
    old = visindex.SceneRowGroups(path)
    old.decode_by_blocks = False
    _, old_bits = old.scene_bits(SCENE, IDS, N_POINTS)
    assert np.array_equal(old_bits.cpu().numpy(), want) and old.decode_stats["blocks"] == 0 and old.decode_stats["serial_streams"] >= min_pages
    return unc


def test_pyarrows_layout_one_page_of_many_blocks(pyarrow_file, want):
    unc = _check(pyarrow_file, want, 1)
    assert BU.block_count(unc) >= 8                                            # the image rows share one page of >= 8 blocks


def test_k12s_layout_small_pages(k12_file, want):
    _check(k12_file, want, 4)


@pytest.mark.parametrize("where", ["preamble", "block_start"])
def test_a_damaged_page_sends_the_scene_to_the_host_path(pyarrow_file, tmp_path, where):
    from mspa import _lib, visindex
    lib = _lib.load()
    at, comp, unc = _first_page(visindex.SceneRowGroups(pyarrow_file))
    raw = bytearray(open(pyarrow_file, "rb").read())
    stream = bytes(raw[at:at + comp])
    rc, starts = BU.block_starts_host(lib, stream, unc)
    assert rc == BU.block_count(unc) >= 8
    if where == "preamble":
        k, value = 0, stream[0] ^ 0x01                                         # the preamble no longer says the page's size
    else:
        k, value = starts[3], 0xFF                                             # a copy-4 of 64 bytes whose offset is four bytes of text
    raw[at + k] = value
    damaged = bytes(raw[at:at + comp])
    dst = np.empty(unc, dtype=np.uint8)
    assert lib.mspa_snappy_decompress_host(np.frombuffer(damaged, dtype=np.uint8).ctypes.data, comp, dst.ctypes.data, unc) < 0
    path = str(tmp_path / "damaged.parquet")
    with open(path, "wb") as f:
        f.write(raw)
    index = visindex.SceneRowGroups(path)
    calls = []
    index._scene_bits_host = lambda *a: calls.append(a) or ("host path", None)
    assert index.scene_bits(SCENE, IDS, N_POINTS) == ("host path", None)       # declined as a whole, as with the one-wave kernel
    assert len(calls) == 1 and index.decode_stats["scenes_declined"] == 1 and index.last_decline == "the device declined a page"
