"""The posed-image export with its depth PNGs encoded on the MI355X (depth_png="device"): from host depth and from frames
inflated on the device, and through the extract_posed_images mirror.  Against the Pillow export of the same .sens: the same
file names, byte-identical non-PNG files, PNGs that decode to the same arrays."""
import importlib
import io
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from png_encode_util import content  # noqa: E402

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multi-spatialmllm_amd")


def _write_scene(path, n=37, hw=(480, 640)):
    from mspa import sens
    kinds = ("smooth", "planar", "ramp", "runs", "noise", "zeros")
    depth = [np.roll(content(kinds[k % len(kinds)], *hw, seed=k), 3 * k, axis=1) for k in range(n)]
    poses = [np.eye(4, dtype=np.float32) + np.float32(0.01 * k) for k in range(n)]
    K = np.array([[577.6, 0, 319.5, 0], [0, 578.7, 239.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)
    sens.write_sens(path, K, poses, depth, color_hw=(968, 1296), color_payloads=[b"\xff\xd8jpeg%d\xff\xd9" % k for k in range(n)])
    return depth


def _same_folders(a, b):
    from PIL import Image
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and names
    for name in names:
        x = open(os.path.join(a, name), "rb").read()
        y = open(os.path.join(b, name), "rb").read()
        if name.endswith(".png"):
            assert np.array_equal(np.array(Image.open(io.BytesIO(x))), np.array(Image.open(io.BytesIO(y)))), name
        else:
            assert x == y, name


def test_export_device_matches_pillow(tmp_path):
    from mspa import sens
    path = str(tmp_path / "s.sens")
    _write_scene(path)
    host = sens.read_sens(path, 1, want_color=True)
    sens.export_posed_images(host, str(tmp_path / "pillow"))
    sens.export_posed_images(host, str(tmp_path / "dev_host"), depth_png="device")
    ondev = sens.read_sens(path, 1, want_color=True, depth_to_device="cuda")
    assert ondev.depth_device is not None
    sens.export_posed_images(ondev, str(tmp_path / "dev_dev"), depth_png="device")
    _same_folders(str(tmp_path / "pillow"), str(tmp_path / "dev_host"))
    _same_folders(str(tmp_path / "pillow"), str(tmp_path / "dev_dev"))
    # the device files are the same bytes whichever copy of the frames they were encoded from
    for name in os.listdir(str(tmp_path / "dev_host")):
        assert open(str(tmp_path / "dev_host" / name), "rb").read() == open(str(tmp_path / "dev_dev" / name), "rb").read()


def test_export_device_small_batches(tmp_path):
    from PIL import Image
    from mspa import sens
    path = str(tmp_path / "s.sens")
    depth = _write_scene(path, n=11, hw=(24, 32))
    s = sens.read_sens(path, 1, want_color=False, depth_to_device="cuda")
    paths = [str(tmp_path / f"{k}.png") for k in range(11)]
    sens.write_depth_pngs_device(s.depth_device, paths, batch=4)
    for k, p in enumerate(paths):
        assert np.array_equal(np.array(Image.open(p)), depth[k])


def test_mirror_process_scene_device(tmp_path, monkeypatch):
    for name in [m for m in sys.modules if m == "spatial_engine" or m.startswith("spatial_engine.")]:
        if not (getattr(sys.modules[name], "__file__", None) or "").startswith(PKG):
            del sys.modules[name]
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    EPI = importlib.import_module("spatial_engine.utils.scannet_utils.extract_posed_images")
    for root in ("a", "b"):
        scans = tmp_path / root / "scans" / "scene0007_00"
        scans.mkdir(parents=True)
        _write_scene(str(scans / "scene0007_00.sens"), n=9)
    monkeypatch.chdir(tmp_path / "a")
    EPI.process_directory("scans", 1, nproc=1)
    monkeypatch.chdir(tmp_path / "b")
    EPI.process_directory("scans", 1, nproc=4, depth_png="device")
    _same_folders(str(tmp_path / "a" / "posed_images" / "scene0007_00"), str(tmp_path / "b" / "posed_images" / "scene0007_00"))
