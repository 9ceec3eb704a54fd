"""K12 (csrc/parquet_pages.hip) on the MI355X: the batched Snappy compressor and the page kernels against the host reference of
csrc/snappy_core.h byte for byte, and ``make_visibility_info.run_split`` with ``MSPA_VISINDEX_ENCODE=device`` against the host
path -- equal frames, equal key statistics, equal warnings; byte-identical to itself across runs and world sizes."""
import hashlib
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
import snappy_util as SU  # noqa: E402

INFO = "data/scannet/scannet_instance_data/scenes_info.pkl"


def test_batched_streams_equal_the_host_reference_and_round_trip():
    import torch
    from mspa import _lib, engine
    lib = _lib.load()
    cases = SU.streams()
    assert any(len(d) == 0 for _, d in cases[1:-1])                         # zero-length streams in the middle of the batch
    assert any(len(a) == 0 and len(b) > 0 for (_, a), (_, b) in zip(cases, cases[1:]))      # ... one right in front of a stream with a block
    junk = b"\xEE" * 5                                                      # gaps between the streams: offsets, not a running sum
    blob, offsets = bytearray(), []
    for _, d in cases:
        blob += junk
        offsets.append(len(blob))
        blob += d
    src = torch.from_numpy(np.frombuffer(bytes(blob), dtype=np.uint8).copy()).cuda()
    off = torch.tensor(offsets, dtype=torch.int64, device="cuda")
    nb = torch.tensor([len(d) for _, d in cases], dtype=torch.int64, device="cuda")
    out, starts = engine.snappy_compress_device(src, off, nb)
    out, starts = out.cpu().numpy().tobytes(), starts.cpu().numpy()
    assert starts[0] == 0 and starts[-1] == len(out)
    for k, (name, d) in enumerate(cases):
        got = out[starts[k]:starts[k + 1]]
        assert got == SU.compress_host(lib, d), name
        SU.check_stream(name, d, got, lib.mspa_snappy_capacity(len(d)))
    # argument checks come before any launch
    with pytest.raises(ValueError):
        engine.snappy_compress_device(src, off, nb[:-1])
    with pytest.raises(ValueError):
        engine.snappy_compress_device(src, off, nb + len(blob))             # streams that run past src
    with pytest.raises(ValueError):
        engine.snappy_compress_device(src.cpu(), off, nb)
    e, e64 = torch.empty((0,), dtype=torch.uint8, device="cuda"), torch.empty((0,), dtype=torch.int64, device="cuda")
    assert engine.snappy_compress_device(e, e64, e64)[1].tolist() == [0]
    assert lib.mspa_snappy_compress_device(None, 0, None, None, 1, None, 1, None, 0, None, None) == _lib.MSPA_EINVAL


@pytest.fixture(scope="module")
def scene_text():
    """K10's text of a synthetic scene (F = 8, N = 20 000, ~30 % visible) as ONE string column on the device, image rows first."""
    import torch
    from mspa import engine, visindex
    rng = np.random.default_rng(21)
    F, N = 8, 20000
    seen = rng.random((F, N)) < 0.3
    seen[:, 777] = False                                                    # a vertex nobody sees: "[]"
    ids = [f"{k * 10:05d}" for k in range(F)]

    def csr(m):
        offs = np.concatenate([[0], np.cumsum(m.sum(1))]).astype(np.int64)
        return torch.from_numpy(offs).cuda(), torch.from_numpy(np.nonzero(m)[1].astype(np.int32)).cuda()
    t1 = engine.format_lists_device(*csr(seen))
    t2 = engine.format_lists_device(*csr(seen.T), visindex.VisibilityCSR(ids, N, None, None, None, None).quoted_image_ids())
    offsets = torch.cat([t1[1][:-1], t2[1] + t1[0].numel()])
    data = torch.cat([t1[0], t2[0]])
    assert data.numel() > 2 * SU.BLOCK and offsets.numel() == F + N + 1
    return offsets, data


@pytest.mark.parametrize("page_bytes", [4096, 1 << 20])
def test_string_pages_equal_the_host_reference(scene_text, page_bytes):
    from mspa import _lib, engine
    offsets, data = scene_text
    got = engine.parquet_string_pages_device(offsets, data, page_bytes, return_payload=True)
    want = SU.host_pages(_lib.load(), offsets.cpu().numpy(), data.cpu().numpy(), page_bytes)
    assert got["num_values"].tolist() == want["num_values"] and got["uncompressed"].tolist() == want["uncompressed"]
    assert got["payload"].cpu().numpy().tobytes() == want["payload"]
    assert got["compressed"].tolist() == want["compressed"]
    assert got["chunk"].cpu().numpy().tobytes() == want["chunk"]
    if page_bytes == 4096:
        assert len(want["compressed"]) > 50 and want["num_values"][0] == 1                 # an image row fills a page by itself
    else:
        assert len(want["compressed"]) == 1 and want["uncompressed"][0] > 2 * SU.BLOCK      # one page, a stream of many blocks


@pytest.mark.parametrize("rows", [1, 5])
def test_pages_that_end_on_a_threads_first_byte(rows):
    """Every value is 22 bytes and fills a page: a payload of 4 + 2 + 4 + 22 = 32 bytes, so pages start at multiples of the 16 bytes
    a thread packs -- the thread at 32 searches for the page of page 2's first byte.  One row: a page table of one entry."""
    import torch
    from mspa import _lib, engine
    text = b"".join(b"[%020d]" % (7 ** k) for k in range(rows))
    offsets = torch.arange(0, 22 * rows + 1, 22, dtype=torch.int32).cuda()
    data = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    got = engine.parquet_string_pages_device(offsets, data, 26, return_payload=True)
    want = SU.host_pages(_lib.load(), offsets.cpu().numpy(), data.cpu().numpy(), 26)
    assert want["uncompressed"] == [32] * rows and want["num_values"] == [1] * rows
    assert got["num_values"].tolist() == want["num_values"] and got["uncompressed"].tolist() == want["uncompressed"]
    assert got["payload"].cpu().numpy().tobytes() == want["payload"]
    assert got["compressed"].tolist() == want["compressed"] and got["chunk"].cpu().numpy().tobytes() == want["chunk"]


def _scenes():
    from mspa import synth
    out = []
    for k in range(3):
        sc = synth.make_scene(9700 + k, n_points=3000 + 700 * k, n_frames=5 + 2 * k, color_hw=(96, 128), depth_hw=(96, 128),
                              invalid_pose_frac=0.0, with_color=False, scene_id=f"scene{9700 + k:04d}_00")
        if k == 1:
            for image_id in sc.valid_image_ids[:2]:                          # two frames that see nothing: warnings, "[]" rows
                sc.depth[image_id] = np.zeros_like(sc.depth[image_id])
        out.append(sc)
    return out


def _run_split(out_dir):
    for name in [m for m in sys.modules if m == "spatial_engine" or m.startswith("spatial_engine.")]:
        if not (getattr(sys.modules[name], "__file__", None) or "").startswith(PKG):
            del sys.modules[name]
    if sys.path[0] != PKG:
        sys.path.insert(0, PKG)
    import spatial_engine.utils.scannet_utils.make_visibility_info as MVI
    os.makedirs(out_dir, exist_ok=True)
    return MVI.run_split(INFO, os.path.join(out_dir, "vis.parquet"), os.path.join(out_dir, "warn.txt"), num_workers=2)


def _rank_main(rank, world, port, root, out_dir):
    os.chdir(root)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      MSPA_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", MSPA_VISINDEX_ENCODE="device")
    for p in (PKG, ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    from mspa import shard
    _run_split(out_dir)
    ctx = shard.context_from_env()
    ctx.barrier()
    ctx.close()


def _sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def test_run_split_with_the_switch_reads_equal_to_the_host_path_and_is_identical_to_itself(tmp_path, monkeypatch):
    import pandas as pd
    import pyarrow.parquet as pq
    from mspa import synth
    root = str(tmp_path)
    synth.write_scannet_layout(_scenes(), os.path.join(root, "data", "scannet"))
    monkeypatch.chdir(root)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.delenv("MSPA_VISINDEX_ENCODE", raising=False)
    host_dict = _run_split(os.path.join(root, "host"))
    monkeypatch.setenv("MSPA_VISINDEX_ENCODE", "device")
    dev_dict = _run_split(os.path.join(root, "dev"))
    _run_split(os.path.join(root, "dev2"))
    assert dev_dict == host_dict and len(host_dict) == 3                     # keep=True: the nested dicts come back as before
    host, dev = os.path.join(root, "host", "vis.parquet"), os.path.join(root, "dev", "vis.parquet")
    pd.testing.assert_frame_equal(pd.read_parquet(dev), pd.read_parquet(host))
    assert pq.read_schema(dev).equals(pq.read_schema(host), check_metadata=True)
    mh, md = pq.ParquetFile(host).metadata, pq.ParquetFile(dev).metadata
    assert mh.num_row_groups == md.num_row_groups == 3
    for g in range(3):
        sh, sd = mh.row_group(g).column(0).statistics, md.row_group(g).column(0).statistics
        assert sd.has_min_max and (sd.min, sd.max) == (sh.min, sh.max) and mh.row_group(g).num_rows == md.row_group(g).num_rows
        assert md.row_group(g).column(1).compression == "SNAPPY" and not md.row_group(g).column(1).is_stats_set
    warn = open(os.path.join(root, "host", "warn.txt")).read()
    assert warn.count("has no in-bound points") == 2 and open(os.path.join(root, "dev", "warn.txt")).read() == warn
    assert _sha(dev) == _sha(os.path.join(root, "dev2", "vis.parquet")) and _sha(dev) != _sha(host)
    # one rank and two gloo ranks on the one GPU: the same bytes
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    mpc = mp.get_context("spawn")
    procs = [mpc.Process(target=_rank_main, args=(r, 2, port, root, os.path.join(root, "two"))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    assert _sha(os.path.join(root, "two", "vis.parquet")) == _sha(dev)
    assert open(os.path.join(root, "two", "warn.txt")).read() == warn


def test_unsorted_image_ids_fall_back_to_the_host_path_and_still_splice():
    import io
    import pyarrow as pa
    import pyarrow.parquet as pq
    import torch
    from mspa import parquet_splice, visindex
    rng = np.random.default_rng(2)
    F, N = 5, 300
    words = rng.integers(-2 ** 63, 2 ** 63 - 1, size=(F, (N + 63) // 64), dtype=np.int64)
    words[:, -1] &= (1 << (N % 64)) - 1                                      # no bits beyond vertex N - 1
    bits = torch.from_numpy(words).cuda()
    ids_sorted, ids_mixed = ["00000", "00010", "00020", "00030", "00040"], ["00030", "00000", "00040", "00010", "00020"]
    a = visindex.from_bits(bits, ids_sorted, N, text=True, indices=False, pages=True, page_bytes=4096)
    b = visindex.from_bits(bits, ids_mixed, N, text=True, indices=True, pages=True, page_bytes=4096)
    assert a.values_pages is not None and a.i2p_text is None and len(a.values_pages["compressed"]) > 1
    assert b.values_pages is None and b.i2p_text is None                      # host formatters, pyarrow's encode
    fa, fb = a.to_row_group("scene0000_00"), b.to_row_group("scene0001_00")
    c = visindex.from_bits(bits, ids_sorted, N, text=True, indices=True)
    assert pq.read_table(io.BytesIO(fa)).equals(c.to_arrow("scene0000_00"))
    assert bytes(fb) == bytes(parquet_splice.encode_row_group(b.to_arrow("scene0001_00"), use_dictionary=False))
    both = pq.read_table(io.BytesIO(parquet_splice.splice([fa, fb])))
    assert both.equals(pa.concat_tables([c.to_arrow("scene0000_00"), b.to_arrow("scene0001_00")]))


def test_a_bad_switch_value_raises(tmp_path, monkeypatch):
    from mspa import visindex
    monkeypatch.setenv("MSPA_VISINDEX_ENCODE", "gpu")
    with pytest.raises(ValueError, match="MSPA_VISINDEX_ENCODE"):
        visindex.encode_mode()
    for name in [m for m in sys.modules if m == "spatial_engine" or m.startswith("spatial_engine.")]:
        if not (getattr(sys.modules[name], "__file__", None) or "").startswith(PKG):
            del sys.modules[name]
    import spatial_engine.utils.scannet_utils.make_visibility_info as MVI
    with pytest.raises(ValueError, match="MSPA_VISINDEX_ENCODE"):
        MVI.run_split(str(tmp_path / "none.pkl"), str(tmp_path / "vis.parquet"), str(tmp_path / "warn.txt"))
    monkeypatch.setenv("MSPA_VISINDEX_ENCODE", " Device ")
    assert visindex.encode_mode() == "device"
    monkeypatch.delenv("MSPA_VISINDEX_ENCODE")
    assert visindex.encode_mode() == "host"
