"""Image resizing on the MI355X (csrc/resize.hip) against Pillow's ``Image.resize`` bit for bit, and the tree tool and the
annotator built on it against their Pillow backends byte for byte.  Every GPU step runs in a child process of its own under a
time limit (this file run as a script with the step's name); the child compares and exits non-zero on a difference."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "multi-spatialmllm_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
from jpeg_util import content  # noqa: E402
from resize_util import FILTERS, OUTSIDE, grid_pairs, patterns, pillow_resize  # noqa: E402

TRAINING_HW = (968, 1296)


def _step(name, tmp_path, limit):
    flags = ["-s"] if sys.flags.no_user_site else []
    run = subprocess.run([sys.executable, *flags, os.path.abspath(__file__), name, str(tmp_path)], capture_output=True, text=True,
                         timeout=limit)
    print(run.stdout[-4000:])
    assert run.returncode == 0, (run.returncode, run.stderr[-4000:])


def _resize(imgs, hw, resample, **kw):
    import torch
    from mspa import engine
    out = engine.resize_rgb_device(torch.from_numpy(np.ascontiguousarray(imgs)).cuda(), hw, resample, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# -- the steps (child process) ------------------------------------------------------------------------------------------------
def step_grid(tmp):
    n = 0
    for i, ((h, w), hw) in enumerate(grid_pairs()):
        imgs = patterns(h, w, i)
        for name, f in FILTERS.items():
            got = _resize(imgs, hw, name)
            for k in range(len(imgs)):
                want = pillow_resize(imgs[k], hw, f)
                assert np.array_equal(got[k], want), ((h, w), hw, name, k, int((got[k] != want).sum()))
                n += 1
    print("grid: images compared", n)
    assert n > 18000


def step_batches(tmp):
    for (h, w), hw, n in [((512, 512), TRAINING_HW, 64), ((360, 640), TRAINING_HW, 64), ((968, 1296), (484, 648), 16)]:
        imgs = np.stack([content(h, w, s) if s % 3 else np.random.default_rng(s).integers(0, 256, (h, w, 3), dtype=np.uint8)
                         for s in range(n)])
        for name, f in FILTERS.items():
            got = _resize(imgs, hw, name)
            for k in range(n):
                assert np.array_equal(got[k], pillow_resize(imgs[k], hw, f)), ((h, w), hw, name, k)
    print("batches ok")


def step_edges(tmp):
    import ctypes
    import torch
    from mspa import engine
    lib, L = engine._lib.load(), engine._lib
    # n = 0
    out = engine.resize_rgb_device(torch.zeros((0, 20, 30, 3), dtype=torch.uint8, device="cuda"), (40, 50))
    assert tuple(out.shape) == (0, 40, 50, 3)
    # padded rows and images, odd pitches (rows that start on any byte), both passes and each pass alone
    rng = np.random.default_rng(11)
    for (h, w), hw in [((37, 45), (80, 101)), ((37, 45), (37, 99)), ((37, 45), (90, 45)), ((37, 45), (20, 21)), ((37, 45), (37, 45)),
                       ((64, 48), (33, 48)), ((64, 48), (64, 20))]:
        for pad_w, pad_h in [(0, 0), (3, 0), (0, 2), (5, 3), (1, 1)]:
            big = torch.from_numpy(rng.integers(0, 256, (5, h + pad_h, w + pad_w, 3), dtype=np.uint8)).cuda()
            view = big[:, :h, :w, :]
            assert view.is_contiguous() == (pad_w == 0 and pad_h == 0)
            for name, f in FILTERS.items():
                got = engine.resize_rgb_device(view, hw, name)
                torch.cuda.synchronize()
                host = view.cpu().numpy()
                for k in range(5):
                    assert np.array_equal(got[k].cpu().numpy(), pillow_resize(host[k], hw, f)), ((h, w), hw, pad_w, pad_h, name, k)
    # a view the kernels cannot address (reversed channels) is copied first
    img = torch.from_numpy(rng.integers(0, 256, (2, 30, 40, 3), dtype=np.uint8)).cuda()
    got = engine.resize_rgb_device(img.flip(3), (50, 60))
    torch.cuda.synchronize()
    assert np.array_equal(got[1].cpu().numpy(), pillow_resize(img[1].cpu().numpy()[..., ::-1], (50, 60), 3))
    # outside the range: MSPA_EUNSUPPORTED from C, Pillow's pixels through the Python layer
    (h, w), hw = OUTSIDE
    far = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    dev = torch.from_numpy(far).cuda()
    with pytest.raises(L.MspaError) as err:
        engine.resize_rgb_device(dev, hw, fallback=False)
    assert err.value.code == L.MSPA_EUNSUPPORTED
    got = engine.resize_rgb_device(dev, hw).cpu().numpy()
    for k in range(2):
        assert np.array_equal(got[k], pillow_resize(far[k], hw, 3))
    # status codes of the C entry point
    src = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device="cuda")
    dst = torch.zeros((2, 16, 16, 3), dtype=torch.uint8, device="cuda")
    bx, kx = engine._resize_tables(8, 16, 3, src.device)
    work = torch.zeros((lib.mspa_resize_workspace_bytes(2, 8, 8, 16, 16) // 8 + 2,), dtype=torch.int64, device="cuda")
    ws, wsn = work.data_ptr(), work.numel() * 8

    def call(src_p, n, h, w, dst_p, H, W, f=3, tab=(bx, kx, bx, kx), ws_p=ws, ws_n=wsn):
        t = [x.data_ptr() if x is not None else None for x in tab]
        return lib.mspa_resize_rgb_device(src_p, n, h, w, w * 3, h * w * 3, dst_p, H, W, f, t[0], t[1], t[2], t[3], ws_p, ws_n, None)
    s, d = src.data_ptr(), dst.data_ptr()
    assert call(s, 2, 8, 8, d, 16, 16) == L.MSPA_OK
    assert call(None, 0, 8, 8, None, 16, 16) == L.MSPA_OK                     # n = 0: nothing is looked at
    assert call(s, 2, 0, 8, d, 16, 16) == L.MSPA_EINVAL and call(s, 2, 8, 8, d, 16, 0) == L.MSPA_EINVAL
    assert call(None, 2, 8, 8, d, 16, 16) == L.MSPA_EINVAL and call(s, 2, 8, 8, None, 16, 16) == L.MSPA_EINVAL
    assert call(s, 2, 8, 8, d, 16, 16, tab=(None, kx, bx, kx)) == L.MSPA_EINVAL
    assert call(s, 2, 8, 8, d, 16, 16, ws_p=None) == L.MSPA_EINVAL and call(s, 2, 8, 8, d, 16, 16, ws_n=16) == L.MSPA_EINVAL
    assert call(s, 2, 8, 8, d, 16, 16, f=1) == L.MSPA_EINVAL and call(s, -1, 8, 8, d, 16, 16) == L.MSPA_EINVAL
    assert call(s, 2, 8, 8, d, 65, 16) == L.MSPA_EUNSUPPORTED and call(s, 2, 8, 8, d, 16, 65) == L.MSPA_EUNSUPPORTED
    assert lib.mspa_resize_rgb_device(s, 2, 8, 8, 23, 8 * 24, d, 16, 16, 3, bx.data_ptr(), kx.data_ptr(), bx.data_ptr(), kx.data_ptr(),
                                      ws, wsn, None) == L.MSPA_EINVAL        # a pitch below a row
    torch.cuda.synchronize()
    assert ctypes.c_char_p(lib.mspa_last_error_string()).value
    print("edges ok")


def _make_tree(root):
    """26 files of mixed shapes: 24 baseline JPEGs written by Pillow, one progressive JPEG, one PNG."""
    from PIL import Image
    shapes = [(512, 512), (360, 640), (968, 1296), (480, 640), (300, 200)]
    rels = []
    for k in range(24):
        h, w = shapes[k % len(shapes)]
        rel = f"seq_{k % 3}/frames/{k:03d}.{'jpeg' if k % 7 == 0 else 'jpg'}"
        os.makedirs(os.path.dirname(os.path.join(root, rel)), exist_ok=True)
        Image.fromarray(content(h, w, k)).save(os.path.join(root, rel), quality=(75, 90, 95)[k % 3], subsampling=(2, 0, 1)[k % 3])
        rels.append(rel)
    Image.fromarray(content(360, 640, 100)).save(os.path.join(root, "seq_0/progressive.jpg"), quality=90, progressive=True)
    Image.fromarray(content(512, 512, 101)).save(os.path.join(root, "seq_1/frames/still.png"))
    return sorted(rels + ["seq_0/progressive.jpg", "seq_1/frames/still.png"])


def _read_tree(root, rels):
    out = {}
    for rel in rels:
        with open(os.path.join(root, rel), "rb") as f:
            out[rel] = f.read()
    return out


def step_tree(tmp):
    from PIL import Image
    from mspa import resize
    src = os.path.join(tmp, "src")
    rels = _make_tree(src)
    want_counts = resize.resize_tree(src, os.path.join(tmp, "pillow"), backend="pillow")
    counts = resize.resize_tree(src, os.path.join(tmp, "device"), backend="device")
    print("tree counts", counts)
    assert resize.list_images(os.path.join(tmp, "device")) == rels == resize.list_images(os.path.join(tmp, "pillow"))
    want, got = _read_tree(os.path.join(tmp, "pillow"), rels), _read_tree(os.path.join(tmp, "device"), rels)
    for rel in rels:
        assert got[rel] == want[rel], rel
        with Image.open(os.path.join(tmp, "device", rel)) as im:
            assert im.size == (1296, 968)
    n = counts["files"]
    assert n == len(rels) == want_counts["files"] and n >= 24
    # the cap: at most one file in ten through Pillow's decoder, none through its resampler
    assert counts["host_decoded"] <= n // 10 and counts["host_resized"] == 0 and counts["device_resized"] == n
    assert counts["device_decoded"] == n - counts["host_decoded"] and counts["device_encoded"] == n - 1 and counts["host_encoded"] == 1
    # another target and filter, and the switch that copies a file of the target shape
    c2 = resize.resize_tree(src, os.path.join(tmp, "device2"), (484, 648), resample="bilinear", quality=80, backend="device")
    resize.resize_tree(src, os.path.join(tmp, "pillow2"), (484, 648), resample="bilinear", quality=80, backend="pillow")
    assert _read_tree(os.path.join(tmp, "device2"), rels) == _read_tree(os.path.join(tmp, "pillow2"), rels)
    assert c2["host_resized"] == 0
    c3 = resize.resize_tree(src, os.path.join(tmp, "device3"), backend="device", skip_same_shape=True)
    assert c3["copied"] == sum(1 for r in rels if Image.open(os.path.join(src, r)).size == (1296, 968)) > 0
    resize.resize_tree(src, os.path.join(tmp, "pillow3"), backend="pillow", skip_same_shape=True)
    assert _read_tree(os.path.join(tmp, "device3"), rels) == _read_tree(os.path.join(tmp, "pillow3"), rels)
    print("tree ok")


def step_annotator(tmp):
    """A VC_D-style batch: pairs of frames, one colour per correspondence, a disc on each and letter labels on the second."""
    from PIL import Image
    from mspa.annotate import DeviceAnnotator, Mark, PillowAnnotator
    srcs = []
    for k, (h, w) in enumerate([(512, 512), (360, 640), (968, 1296), (512, 512)]):
        path = os.path.join(tmp, f"frame_{k}.jpg")
        Image.fromarray(content(h, w, 40 + k)).save(path, quality=92)
        srcs.append((path, h, w))
    jobs = []
    for k, (path, h, w) in enumerate(srcs):
        colors = [(0, 0, 255), (0, 255, 0), (255, 0, 0), (20, 200, 240)]
        first = [Mark(w // 4, h // 3, 10, colors[0])]
        second = [Mark((w * (j + 1)) // 5, (h * (j + 2)) // 7, 10, colors[j], "ABCD"[j]) for j in range(4)]
        jobs += [(path, f"vc_{k}_1.jpg", first), (path, f"vc_{k}_2.jpg", second), (path, f"vc_{k}_edge.jpg",
                                                                                   [Mark(w - 2, h - 2, 10, colors[3], "D"), Mark(1, 1, 10, colors[2], "C")])]
    jobs.append((srcs[0][0], "vc_host.png", [Mark(30, 30, 10, (0, 255, 0), "A")]))
    for name, ann in (("pillow", PillowAnnotator(output_size=TRAINING_HW)), ("device", DeviceAnnotator(output_size=TRAINING_HW))):
        for src, dst, marks in jobs:
            ann.annotate(src, os.path.join(tmp, name, dst), marks)
        ann.copy(srcs[1][0], os.path.join(tmp, name, "copied.jpg"))
        flush = getattr(ann, "flush", None)
        if flush:
            flush()
    names = [dst for _, dst, _ in jobs] + ["copied.jpg"]
    want, got = _read_tree(os.path.join(tmp, "pillow"), names), _read_tree(os.path.join(tmp, "device"), names)
    for dst in names:
        assert got[dst] == want[dst], dst
    for dst in names[:-1]:
        with Image.open(os.path.join(tmp, "device", dst)) as im:
            assert im.size == (1296, 968)
    with Image.open(os.path.join(tmp, "device", "copied.jpg")) as im:
        assert im.size == (640, 360)                       # a copy stays a copy
    print("annotator ok")


# -- the tests (parent) ---------------------------------------------------------------------------------------------------------
def test_resize_equals_pillow_on_the_grid(tmp_path):
    _step("grid", tmp_path, 900)


def test_resize_equals_pillow_on_batches_of_frames(tmp_path):
    _step("batches", tmp_path, 600)


def test_empty_batch_pitches_declined_shapes_and_status_codes(tmp_path):
    _step("edges", tmp_path, 600)


def test_resize_tree_device_equals_pillow_backend(tmp_path):
    _step("tree", tmp_path, 600)


def test_device_annotator_output_size_equals_pillow_annotator(tmp_path):
    _step("annotator", tmp_path, 600)


if __name__ == "__main__":
    {"grid": step_grid, "batches": step_batches, "edges": step_edges, "tree": step_tree,
     "annotator": step_annotator}[sys.argv[1]](sys.argv[2])
