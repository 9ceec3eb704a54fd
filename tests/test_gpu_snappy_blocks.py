"""The Snappy decoder's block route on the MI355X: the block-start scan against mspa_snappy_block_starts_host and the decode (scan,
one wave per block, then the one-wave kernel) against mspa_snappy_decompress_host, over both writers' streams, hand-built ones
that are and are not blockwise, the shapes at which a scan by 2 KiB segments can go wrong and the corrupt set
(tests/snappy_blocks_util.py) -- ONE batch, streams at every alignment 0 - 3 with gaps between them.

The corrupt streams reach the GPU only behind tests/test_snappy_blocks_cpu.py's sanitizer run of the same rules on the CPU."""
import functools
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
import visindex_decode_util as VU  # noqa: E402

SENTINEL, GAP = 0xAB, 32


@functools.lru_cache(maxsize=None)
def _cases():
    """[(name, stream, expected size, kind)] -- kind "writer" (either writer's: blockwise), "valid" (hand-built) or "corrupt".  Every
    corrupt stream stands between two good ones."""
    out = [(n, s, len(d), "writer") for n, s, d in BU.writer_streams()]
    out += [(n, s, len(d), "valid") for n, s, d, _ in BU.hand_streams()]
    out += [(n, s, len(d), "valid") for n, s, d in BU.segment_streams()]
    out += [(n, s, len(d), "valid") for n, s, d in VU.valid_streams() if n.startswith("hand_") or n == VU.FAR_NAME]
    good = [c for c in out if c[0] in ("own_json", "pa_lists5", "bw_copy4_literal_heads", "pa_p7_65537", "own_mix3")]
    assert len(good) == 5
    for k, (n, s, e) in enumerate(BU.corrupt_streams()):
        out += [(n, s, e, "corrupt"), good[k % 5][:3] + ("neighbour",)]
    return out


@functools.lru_cache(maxsize=None)
def _host():
    """Per case: (decompress rc, bytes, block_starts rc, starts) by the library's host reference."""
    from mspa import _lib
    lib = _lib.load()
    out = []
    for _n, s, e, _k in _cases():
        rc, data = VU.decompress_host(lib, s, e)
        brc, starts = BU.block_starts_host(lib, s, e)
        out.append((rc, data, brc, starts))
    return out


@functools.lru_cache(maxsize=None)
def _device():
    """The batch through mspa_snappy_block_starts_device and mspa_snappy_decompress_blocks_device, one call each."""
    import torch
    from mspa import _lib
    lib = _lib.load()
    cases = _cases()
    buf, offs = bytearray(), []
    for k, (_n, s, _e, _kind) in enumerate(cases):
        buf += b"\x5a" * ((k % 4 - len(buf)) % 4 + 4 * (k % 3))                # stream k at an offset = k mod 4, gaps of 0 .. 11 bytes
        offs.append(len(buf))
        buf += s
    assert {o % 4 for o in offs} == {0, 1, 2, 3}
    n = len(cases)
    sizes = np.array([e for _, _, e, _ in cases], dtype=np.int64)
    lens = np.array([len(s) for _, s, _, _ in cases], dtype=np.int64)
    block_prefix = np.concatenate([[0], np.cumsum((sizes + BU.BLOCK - 1) // BU.BLOCK)]).astype(np.int64)
    n_blocks = int(block_prefix[-1])
    out_off, pos = [], GAP
    for e in sizes:
        out_off.append(pos)
        pos += int(e) + GAP
    dev = "cuda"
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int64)).to(dev)
    src = torch.from_numpy(np.frombuffer(bytes(buf), dtype=np.uint8).copy()).to(dev)
    o_dev, n_dev, sz_dev, oo_dev, bp_dev = t(offs), t(lens), t(sizes), t(out_off), t(block_prefix)
    ws_bytes = lib.mspa_snappy_blocks_workspace_bytes(int(lens.sum()), n, n_blocks)
    assert ws_bytes >= 8 * int(lens.sum())
    ws = torch.empty(((ws_bytes + 15) // 16 * 2,), dtype=torch.int64, device=dev)
    starts = torch.full((n_blocks + n,), -5, dtype=torch.int64, device=dev)
    route = torch.full((n,), 99, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    rc = lib.mspa_snappy_block_starts_device(src.data_ptr(), src.numel(), o_dev.data_ptr(), n_dev.data_ptr(), n, sz_dev.data_ptr(), bp_dev.data_ptr(),
                                             n_blocks, int(lens.sum()), ws.data_ptr(), ws.numel() * 8, starts.data_ptr(), route.data_ptr(), st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    scan = (starts.cpu().numpy(), route.cpu().numpy())
    out = torch.full((pos,), SENTINEL, dtype=torch.uint8, device=dev)
    status = torch.full((n,), 99, dtype=torch.int32, device=dev)
    route2 = torch.full((n,), 99, dtype=torch.int32, device=dev)
    rc = lib.mspa_snappy_decompress_blocks_device(src.data_ptr(), src.numel(), o_dev.data_ptr(), n_dev.data_ptr(), n, out.data_ptr(), pos,
                                                  oo_dev.data_ptr(), sz_dev.data_ptr(), bp_dev.data_ptr(), n_blocks, int(lens.sum()), ws.data_ptr(),
                                                  ws.numel() * 8, status.data_ptr(), route2.data_ptr(), st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    keep = np.ones(pos, dtype=bool)
    outs = []
    for at, e in zip(out_off, sizes):
        keep[at:at + e] = False
        outs.append(host[at:at + e].tobytes())
    return {"scan": scan, "block_prefix": block_prefix, "status": status.cpu().numpy(), "route": route2.cpu().numpy(), "outs": outs,
            "gaps_intact": bool((host[keep] == SENTINEL).all())}


def test_scan_finds_the_hosts_starts_and_routes():
    cases, host, got = _cases(), _host(), _device()
    starts, route = got["scan"]
    bp = got["block_prefix"]
    sizes = {e for _, _, e, _ in cases}
    assert {0, 1, 65535, 65536, 65537, 3 * 65536} <= sizes
    taken = 0
    for k, ((name, _s, e, _kind), (_rc, _data, brc, want)) in enumerate(zip(cases, host)):
        if brc > 0:
            assert route[k] == brc == BU.block_count(e), (name, int(route[k]), brc)
            assert starts[bp[k] + k:bp[k + 1] + k + 1].tolist() == want, name
            taken += 1
        else:
            assert route[k] == 0, (name, int(route[k]), brc)
    assert taken >= 2 * 62 and any(n.startswith("seg_") for n, *_ in cases)
    # what the kernels' searches for a block's and a segment's stream meet: a stream without blocks in front of one with blocks
    # (they share a block_prefix entry), and a taken stream shorter than a segment in front of a longer one
    lens, pairs = [len(s) for _, s, _, _ in cases], range(len(cases) - 1)
    assert any(cases[k][2] == 0 and host[k + 1][2] > 0 for k in pairs)
    assert any(0 < lens[k] < BU.SEG < lens[k + 1] and host[k][2] > 0 and host[k + 1][2] > 0 for k in pairs)


def test_decode_equals_the_host_and_no_writers_stream_takes_the_fallback():
    cases, host, got = _cases(), _host(), _device()
    assert got["gaps_intact"]                                                 # nothing outside any stream's own span
    for k, ((name, _s, e, kind), (rc, data, brc, _starts)) in enumerate(zip(cases, host)):
        st, route = int(got["status"][k]), int(got["route"][k])
        if rc < 0:
            assert kind == "corrupt" and st == rc and route == 0, (name, st, rc, route)
            continue
        assert kind != "corrupt" and rc == e and st == 0 and got["outs"][k] == data, (name, st)
        blocks = BU.block_count(e)
        if brc == BU.NOT_BLOCKWISE or blocks < 2:
            assert route == 0, (name, route)                                 # the right bytes, by the one-wave kernel
        elif kind in ("writer", "neighbour") or brc == blocks:
            assert route == blocks, (name, route, blocks)
    multi = [k for k, c in enumerate(cases) if c[3] == "writer" and BU.block_count(c[2]) >= 2]
    assert len(multi) >= 20 and all(got["route"][k] == BU.block_count(cases[k][2]) for k in multi)
    assert sum(1 for k, c in enumerate(cases) if host[k][2] == BU.NOT_BLOCKWISE) >= 4


def test_a_damaged_streams_neighbours_decode_intact():
    cases, host, got = _cases(), _host(), _device()
    seen = 0
    for k, c in enumerate(cases):
        if c[3] == "corrupt":
            assert got["status"][k] == host[k][0] < 0
            for j in (k - 1, k + 1):
                if cases[j][3] != "corrupt":
                    assert got["status"][j] == 0 and got["outs"][j] == host[j][1], (c[0], cases[j][0])
                    seen += 1
    assert seen >= len(BU.corrupt_streams())


def test_engine_wrappers_and_wrong_arguments():
    import torch
    from mspa import _lib, engine
    lib = _lib.load()
    by_name = {n: (s, d) for n, s, d in BU.writer_streams()}
    pick = [by_name[n] for n in ("own_json", "pa_lists5", "own_mix3", "pa_zeros0")]
    pick.append(next((s, d) for n, s, d, _ in BU.hand_streams() if n == "nb_copy2_crosses"))
    assert len(pick) == 5
    src = torch.from_numpy(np.frombuffer(b"".join(s for s, _ in pick), dtype=np.uint8).copy()).cuda()
    lens = [len(s) for s, _ in pick]
    offs = torch.tensor(np.concatenate([[0], np.cumsum(lens)[:-1]]), dtype=torch.int64, device="cuda")
    nbytes = torch.tensor(lens, dtype=torch.int64, device="cuda")
    sizes = torch.tensor([len(d) for _, d in pick], dtype=torch.int64, device="cuda")
    blocks = [BU.block_count(len(d)) for _, d in pick]
    out, out_off, status, route = engine.snappy_decompress_blocks_device(src, offs, nbytes, sizes)
    assert status.tolist() == [0] * 5 and out.cpu().numpy().tobytes() == b"".join(d for _, d in pick)
    assert route.tolist() == [0, blocks[1], blocks[2], 0, 0] and blocks[1] >= 5
    old, old_off, old_status = engine.snappy_decompress_device(src, offs, nbytes, sizes)
    assert torch.equal(old, out) and torch.equal(old_off, out_off) and torch.equal(old_status, status)
    starts, block_prefix, scan_route = engine.snappy_block_starts_device(src, offs, nbytes, sizes)
    assert block_prefix.tolist() == np.concatenate([[0], np.cumsum(blocks)]).tolist()
    assert scan_route.tolist() == [blocks[0], blocks[1], blocks[2], 0, 0]
    bp = block_prefix.tolist()
    for k, (s, d) in enumerate(pick[:3]):
        assert starts[bp[k] + k:bp[k + 1] + k + 1].tolist() == BU.block_starts_host(lib, s, len(d))[1]
    # a table entry outside src: that stream alone is refused
    bad_n = nbytes.clone()
    bad_n[1] = src.numel() + 1
    _, _, status, route = engine.snappy_decompress_blocks_device(src, offs, bad_n, sizes)
    assert status.tolist() == [0, _lib.MSPA_EINVAL, 0, 0, 0] and route.tolist() == [0, 0, blocks[2], 0, 0]
    with pytest.raises(ValueError):
        engine.snappy_decompress_blocks_device(src.cpu(), offs, nbytes, sizes)
    with pytest.raises(ValueError):
        engine.snappy_block_starts_device(src, offs, nbytes, sizes[:2])
    # a workspace smaller than the size function says: refused before anything is enqueued
    ws = torch.empty((2,), dtype=torch.int64, device="cuda")
    st = torch.zeros(5, dtype=torch.int32, device="cuda")
    assert lib.mspa_snappy_decompress_blocks_device(src.data_ptr(), src.numel(), offs.data_ptr(), nbytes.data_ptr(), 5, out.data_ptr(), out.numel(),
                                                    out_off.data_ptr(), sizes.data_ptr(), block_prefix.data_ptr(), sum(blocks), src.numel(),
                                                    ws.data_ptr(), 16, st.data_ptr(), st.data_ptr(), None) == _lib.MSPA_EINVAL
