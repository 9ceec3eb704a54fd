"""16-bit depth PNG encode on the MI355X (csrc/png_encode.hip) against the g++ build of csrc/png_encode_core.h, byte for byte:
the size / content grid of the CPU test, 1 024 ScanNet-shaped frames in one call, n = 0, the round trip through the project's
own depth readers, and the argument checks of the C ABI."""
import ctypes
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from png_encode_util import KINDS, SIZES, build_driver, content, encode_core  # noqa: E402


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(str(tmp_path_factory.mktemp("png_core")))


def _device_files(frames):
    import torch
    from mspa import engine
    d = torch.from_numpy(np.ascontiguousarray(frames, dtype=np.uint16).view(np.int16)).cuda()
    out, nbytes = engine.png_encode_device(d)
    torch.cuda.synchronize()
    nb = nbytes.cpu().numpy()
    o = out.cpu().numpy()
    return [o[k, :int(nb[k])].tobytes() for k in range(len(frames))]


def _core_files(driver, frames, workers=16):
    parts = [frames[i::workers] for i in range(workers)]
    with ThreadPoolExecutor(workers) as ex:
        res = list(ex.map(lambda p: [f for f, _ in encode_core(driver, list(p))] if len(p) else [], parts))
    out = [None] * len(frames)
    for i in range(workers):
        out[i::workers] = res[i]
    return out


def scannet_frames(n, seed=0):
    """n 480 x 640 frames: the grid's depth-like kinds, shifted and offset per frame."""
    base = [content(k, 480, 640, seed) for k in ("smooth", "planar", "ramp", "runs", "smooth", "planar", "noise", "zeros")]
    out = np.empty((n, 480, 640), dtype=np.uint16)
    for i in range(n):
        b = base[i % len(base)]
        out[i] = np.roll(b, (i * 7) % 480, axis=0) + np.uint16((i // 8) % 5) * (b > 0)
    return out


@pytest.mark.parametrize("hw", SIZES)
def test_grid_matches_core(driver, hw):
    frames = np.stack([content(k, *hw, seed=3) for k in KINDS])
    assert _device_files(frames) == [f for f, _ in encode_core(driver, list(frames))]


def test_scannet_batch_matches_core(driver):
    frames = scannet_frames(1024)
    dev = _device_files(frames)
    core = _core_files(driver, list(frames))
    bad = [k for k in range(len(frames)) if dev[k] != core[k]]
    assert not bad, f"{len(bad)} of 1024 files differ, first {bad[:5]}"


def test_zero_frames():
    import torch
    from mspa import engine
    out, nbytes = engine.png_encode_device(torch.zeros((0, 480, 640), dtype=torch.int16, device="cuda"))
    assert out.shape[0] == 0 and nbytes.shape[0] == 0


def test_round_trip_through_readers(tmp_path):
    import torch
    from mspa import ingest
    frames = scannet_frames(40, seed=5)
    files = _device_files(frames)
    paths = []
    for k, f in enumerate(files):
        p = str(tmp_path / f"{k}.png")
        with open(p, "wb") as fh:
            fh.write(f)
        paths.append(p)
    host = ingest.read_depth_frames(paths)
    assert np.array_equal(host, frames)
    dev = ingest.read_depth_frames_device(paths)
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy().view(np.uint16), frames)
    # every frame decodes on the device (status 0): the packer and the device inflate accept the stream as it is
    from mspa import engine
    h, w = frames.shape[1:]
    buf, offsets, nbytes, st_host, cap = ingest.pack_depth_pngs(paths, h, w, 4)
    assert not np.any(st_host)
    src = torch.from_numpy(buf[:max(cap, 16)]).cuda()
    raw, status = engine.inflate_blocks_device(src, torch.from_numpy(offsets).cuda(), torch.from_numpy(nbytes).cuda(),
                                               h * (2 * w + 1))
    torch.cuda.synchronize()
    assert not np.any(status.cpu().numpy())


def test_abi_refusals():
    import torch
    from mspa import _lib, engine
    lib = _lib.load()
    h, w, n = 48, 64, 2
    cap = int(lib.mspa_png_encode_capacity(h, w))
    assert cap == engine.png_encode_capacity((h, w)) > 0
    assert lib.mspa_png_encode_capacity(0, 5) == -1 and lib.mspa_png_encode_capacity(5, 8193) == -1
    assert lib.mspa_png_encode_workspace_bytes(-1, h, w) == -1 and lib.mspa_png_encode_workspace_bytes(65536, h, w) == -1
    ws_bytes = int(lib.mspa_png_encode_workspace_bytes(n, h, w))
    depth = torch.zeros((n + 1, h, w), dtype=torch.int16, device="cuda")
    pitch = (cap + 3) // 4 * 4
    out = torch.full((n, pitch + 16), 0xA5, dtype=torch.uint8, device="cuda")
    nb = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    ws = torch.empty((ws_bytes // 8 + 4,), dtype=torch.int64, device="cuda")
    st = engine._stream_ptr()
    d, o, b, wp = depth.data_ptr(), out.data_ptr(), nb.data_ptr(), ws.data_ptr()
    good = dict(d=d, n=n, h=h, w=w, o=o, pitch=pitch + 16, b=b, ws=wp, wsb=ws_bytes)   # out's own row pitch

    def call(**kw):
        a = dict(good, **kw)
        return lib.mspa_png_encode_device(a["d"], a["n"], a["h"], a["w"], a["o"], a["pitch"], a["b"], a["ws"], a["wsb"], st)

    bad = [dict(d=None), dict(o=None), dict(b=None), dict(ws=None), dict(h=0), dict(w=8193), dict(n=-1), dict(n=65536),
           dict(d=d + 1), dict(o=o + 2), dict(b=b + 4), dict(ws=wp + 8), dict(pitch=pitch - 4), dict(pitch=pitch + 2),
           dict(wsb=ws_bytes - 1)]
    for kw in bad:
        assert call(**kw) == _lib.MSPA_EINVAL, kw
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and bool((nb == -7).all()), "a refused call wrote its outputs"
    assert call(n=0, d=None, o=None, b=None, ws=None) == 0
    with pytest.raises(ValueError):
        engine.png_encode_device(depth.transpose(1, 2))
    with pytest.raises(_lib.MspaError):
        engine.png_encode_device(depth, out=torch.empty((n + 1, cap // 2), dtype=torch.uint8, device="cuda"))
    assert call() == 0
    torch.cuda.synchronize()
    assert int(nb[n]) == -7 and bool((out[:, pitch:] == 0xA5).all()), "wrote past frame n - 1 or past the file"
