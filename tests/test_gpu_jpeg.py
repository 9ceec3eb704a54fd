"""Colour-frame decode on the MI355X (csrc/jpeg_decode.hip) against libjpeg-turbo through Pillow, bit for bit: the sampling /
quality / Huffman-table / restart / size matrix, a batch of ScanNet-shaped frames in one call, damaged streams, the file and
.sens readers with their host fallback, and the coloured point cloud of K3 fed from device-decoded colour."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from jpeg_util import content, encode, pillow_rgb, sos_end  # noqa: E402

SCANNET_HW = (968, 1296)


def _require_turbo():
    from PIL import features
    assert features.check_feature("libjpeg_turbo"), \
        "Pillow is not linked against libjpeg-turbo: the device decoder is specified against libjpeg-turbo's output"


def _decode(payloads, hw):
    """One mspa_jpeg_decode_device call over ``payloads``; returns (rgb [n, H, W, 3] numpy, status numpy)."""
    import torch
    from mspa import engine
    offs, pos = [], 0
    for p in payloads:
        offs.append(pos)
        pos += (len(p) + 15) // 16 * 16
    buf = np.zeros(pos + 16, dtype=np.uint8)
    for o, p in zip(offs, payloads):
        buf[o:o + len(p)] = np.frombuffer(p, dtype=np.uint8)
    desc, _ = engine.jpeg_parse_host(payloads)
    out, status = engine.jpeg_decode_device(torch.from_numpy(buf).cuda(), torch.tensor(offs, dtype=torch.int64).cuda(),
                                            torch.tensor([len(p) for p in payloads], dtype=torch.int64).cuda(),
                                            torch.from_numpy(desc).cuda(), hw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), status.cpu().numpy()


SIZES = [(1, 1), (2, 3), (3, 5), (8, 8), (17, 33), (480, 640), (967, 1295), (968, 1296), (16, 4096)]
RESTARTS = [{}, {"restart_marker_blocks": 1}, {"restart_marker_blocks": 3}, {"restart_marker_rows": 1}]


@pytest.mark.parametrize("hw", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_matrix_bit_identical(hw):
    _require_turbo()
    h, w = hw
    big = h * w > 100000
    payloads, names = [], []
    for sub in (0, 1, 2, "L"):
        for q in (5, 50, 75, 95, 100):
            for opt in (False, True):
                for rs in RESTARTS:
                    if big and (q in (5, 50) or (opt and rs)):
                        continue                     # the large frames take a thinner slice of the same matrix
                    for kind in (("mixed", "saturated") if q >= 95 else ("mixed",)):
                        img = content(h, w, 1000 * q + len(payloads), kind)
                        kw = dict(quality=q, optimize=opt, **rs)
                        if sub == "L":
                            img = img[..., 0]
                        else:
                            kw["subsampling"] = sub
                        payloads.append(encode(img, **kw))
                        names.append((sub, q, opt, tuple(rs.items()), kind))
    rgb, st = _decode(payloads, hw)
    for k, p in enumerate(payloads):
        assert st[k] == 0, f"{hw} {names[k]}: status {st[k]}"
        assert np.array_equal(rgb[k], pillow_rgb(p)), f"{hw} {names[k]}: differs from Pillow"


def _scannet_batch(n):
    base = [content(*SCANNET_HW, s) for s in range(4)]
    out = []
    for k in range(n):
        img = np.roll(base[k % 4], (k * 7) % 61, axis=k % 2)
        kw = dict(quality=(75, 90, 95)[k % 3], subsampling=(2, 0)[k % 2])
        if k % 5 == 0:
            kw["restart_marker_rows"] = 1
        out.append(encode(img, **kw))
    return out


def test_scannet_batch_one_call():
    _require_turbo()
    payloads = _scannet_batch(1024)
    rgb, st = _decode(payloads, SCANNET_HW)
    assert (st == 0).all(), np.unique(st, return_counts=True)
    for k in range(len(payloads)):
        assert np.array_equal(rgb[k], pillow_rgb(payloads[k])), f"frame {k} differs from Pillow"


def _pillow_or_none(data):
    try:
        return pillow_rgb(data)
    except Exception:
        return None


def test_damaged_streams():
    _require_turbo()
    rng = np.random.default_rng(11)
    good, damaged = [], []
    for sub in (0, 2, "L"):
        for rs in ({}, {"restart_marker_blocks": 3}):
            img = content(64, 96, len(good))
            kw = dict(quality=75, **rs)
            if sub == "L":
                img = img[..., 0]
            else:
                kw["subsampling"] = sub
            data = encode(img, **kw)
            good.append(data)
            start = sos_end(data)
            for _ in range(12):
                b = bytearray(data)
                b[int(rng.integers(start, len(data) - 2))] ^= 1 << int(rng.integers(0, 8))
                damaged.append(bytes(b))
            for _ in range(4):
                damaged.append(data[:int(rng.integers(start, len(data)))])
            if rs:
                rst = [i for i in range(start, len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]
                b = bytearray(data)
                b[rst[0] + 1], b[rst[1] + 1] = b[rst[1] + 1], b[rst[0] + 1]
                damaged.append(bytes(b))
                damaged.append(data[:rst[2]] + data[rst[2] + 2:])
    # every damaged stream sits between two intact ones in the same call
    payloads = []
    for k, d in enumerate(damaged):
        payloads += [good[k % len(good)], d]
    payloads.append(good[0])
    rgb, st = _decode(payloads, (64, 96))
    for k, p in enumerate(payloads):
        if k % 2 == 0:
            assert st[k] == 0 and np.array_equal(rgb[k], pillow_rgb(p)), f"intact neighbour {k} disturbed"
        elif st[k] == 0:
            ref = _pillow_or_none(p)
            assert ref is not None and np.array_equal(rgb[k], ref), f"damaged stream {k} accepted with another output"
    assert (st[1::2] != 0).sum() > len(damaged) // 2


def test_read_color_frames_device(tmp_path):
    _require_turbo()
    import torch
    from mspa import ingest
    from PIL import Image
    paths, expect = [], []
    for k in range(6):
        img = content(120, 160, 50 + k)
        if k == 4:                                   # undecodable on the device: a CMYK (Adobe) JPEG
            import io
            bio = io.BytesIO()
            Image.fromarray(img).convert("CMYK").save(bio, "JPEG", quality=85)
            data = bio.getvalue()
        else:
            data = encode(img, quality=85, subsampling=(0, 1, 2)[k % 3], progressive=(k == 2))
        p = tmp_path / f"{k:05d}.jpg"
        p.write_bytes(data)
        paths.append(str(p))
        expect.append(pillow_rgb(data))
    got = ingest.read_color_frames_device(paths, "cuda:0", n_threads=3)
    torch.cuda.synchronize()
    assert got.shape == (6, 120, 160, 3) and got.dtype == torch.uint8
    for k in range(6):
        assert np.array_equal(got[k].cpu().numpy(), expect[k]), f"file {k}"


def test_read_sens_color_to_device(tmp_path):
    _require_turbo()
    import torch
    from mspa import sens
    rng = np.random.default_rng(3)
    F, hw = 5, (96, 128)
    payloads = [encode(content(*hw, 70 + k), quality=80, subsampling=2) for k in range(F)]
    b = bytearray(payloads[3])
    b[(sos_end(payloads[3]) + len(b)) // 2] ^= 0x04
    payloads[3] = bytes(b)
    depth = [rng.integers(0, 4000, (48, 64)).astype(np.uint16) for _ in range(F)]
    K = np.eye(4)
    path = str(tmp_path / "scene.sens")
    sens.write_sens(path, K, [np.eye(4)] * F, depth, color_hw=hw, color_payloads=payloads)
    sc = sens.read_sens(path, color_to_device="cuda:0")
    assert sc.color_device is not None and tuple(sc.color_device.shape) == (F,) + hw + (3,)
    got = sc.color_device.cpu().numpy()
    for k in range(F):
        ref = _pillow_or_none(payloads[k])
        if ref is None:
            continue
        assert np.array_equal(got[k], ref), f"frame {k}"


def test_coloured_point_cloud_from_device_colour():
    _require_turbo()
    import torch
    from mspa import engine, ingest, synth
    sc = synth.make_scene(77, n_points=4096, n_frames=4, color_hw=SCANNET_HW, depth_hw=(480, 640), invalid_pose_frac=0.0,
                          with_color=True)
    ids = sc.valid_image_ids
    payloads = [encode(np.ascontiguousarray(sc.color[i]), quality=90) for i in ids]
    stage = torch.empty(sum((len(p) + 15) // 16 * 16 for p in payloads) + 16, dtype=torch.uint8)
    host = stage.numpy()
    offs, pos = [], 0
    for p in payloads:
        offs.append(pos)
        host[pos:pos + len(p)] = np.frombuffer(p, dtype=np.uint8)
        pos += (len(p) + 15) // 16 * 16
    dev = "cuda:0"
    rgb_dev = ingest.decode_jpegs_device(stage, np.array(offs), np.array([len(p) for p in payloads]), dev,
                                         lambda k: pillow_rgb(payloads[k]))
    rgb_host = torch.from_numpy(np.stack([pillow_rgb(p) for p in payloads])).to(dev)
    depth = engine.depth_to_device(np.stack([sc.depth[i] for i in ids]), dev)
    mats = torch.from_numpy(engine.frame_matrices(sc.K, sc.A, [sc.E[i] for i in ids])).to(dev)
    pairs = torch.tensor([[0, 1], [1, 2], [2, 3], [3, 0]], dtype=torch.int32, device=dev)
    outs = []
    for rgb in (rgb_dev, rgb_host):
        out = engine.alloc_pair_outputs(4, SCANNET_HW, ("vis_u8", "counts", "rgba"), dev)
        engine.pair_reproject(depth, mats, pairs, SCANNET_HW, out, rgb=rgb)
        outs.append(out)
    torch.cuda.synchronize()
    assert int(outs[0]["counts"][:, 1].sum()) > 0
    assert torch.equal(outs[0]["rgba"], outs[1]["rgba"])
    assert torch.equal(rgb_dev, rgb_host)
