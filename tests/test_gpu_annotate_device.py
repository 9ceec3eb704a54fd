"""mspa.annotate.DeviceAnnotator on the MI355X against PillowAnnotator, file for file: discs and labels off every border,
overlapping marks, radii 0 / 1 / 10 / W // 100, progressive and PNG sources (host decode), a .png destination, the same
destination twice, copies, and batches that span shapes and the flush threshold."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from jpeg_util import content  # noqa: E402

from mspa.annotate import DeviceAnnotator, Mark, PillowAnnotator  # noqa: E402


def _sources(d):
    from PIL import Image
    os.makedirs(d, exist_ok=True)
    srcs = {}
    for name, hw, kw in [("a.jpg", (96, 128), {"quality": 90}), ("b.jpg", (96, 128), {"quality": 75, "subsampling": 0}),
                         ("c.jpg", (61, 83), {"quality": 95}), ("p.jpg", (96, 128), {"quality": 80, "progressive": True}),
                         ("g.png", (96, 128), {})]:
        path = os.path.join(d, name)
        Image.fromarray(content(*hw, len(srcs))).save(path, **kw)
        srcs[name] = (path, hw)
    return srcs


def _jobs(srcs):
    jobs = []
    for name, (path, (h, w)) in srcs.items():
        r1 = w // 100
        edge = [Mark(0, 0, 10, (0, 0, 255), "A"), Mark(w - 1, h - 1, 10, (0, 255, 0), "B"), Mark(-5, h // 2, 10, (255, 0, 0), "C"),
                Mark(w + 3, 4, 10, (255, 255, 255), "D", (-40, 0)), Mark(w // 2, -8, 1, (0, 0, 0), "A", (0, 30)),
                Mark(w // 2, h + 6, 10, (12, 200, 77), "B")]
        overlap = [Mark(40, 40, 10, (10, 20, 30), "A"), Mark(45, 42, 10, (200, 100, 0), "B"), Mark(47, 40, 0, (1, 2, 3), "C"),
                   Mark(30, 30, r1, (9, 9, 250), "D", (15, 0)), Mark(50, 41, 1, (250, 250, 0), "12")]
        jobs.append(("annotate", path, name + "_edge.jpg", edge))
        jobs.append(("annotate", path, name + "_overlap.jpg", overlap))
        jobs.append(("annotate", path, name + "_plain.jpeg", [Mark(w // 3, h // 3, 10, (0, 0, 255))]))
    a = srcs["a.jpg"][0]
    jobs.append(("annotate", a, "dest.png", [Mark(20, 20, 10, (0, 255, 0), "A")]))
    jobs.append(("annotate", a, "twice.jpg", [Mark(20, 20, 10, (0, 255, 0), "A")]))
    jobs.append(("copy", srcs["b.jpg"][0], "copied.jpg"))
    jobs.append(("annotate", a, "twice.jpg", [Mark(60, 50, 10, (255, 0, 0), "B")]))       # the later job wins
    return jobs


def _run(annotator, jobs, out):
    for kind, src, dst, *marks in jobs:
        if kind == "copy":
            annotator.copy(src, os.path.join(out, "sub", dst))
        else:
            annotator.annotate(src, os.path.join(out, "sub", dst), marks[0])


def _tree(d):
    files = {}
    for root, _, names in os.walk(d):
        for n in names:
            with open(os.path.join(root, n), "rb") as f:
                files[os.path.relpath(os.path.join(root, n), d)] = f.read()
    return files


@pytest.mark.parametrize("batch_size", [1024, 3])
def test_device_files_equal_pillow_files(tmp_path, batch_size):
    srcs = _sources(str(tmp_path / "src"))
    jobs = _jobs(srcs)
    _run(PillowAnnotator(), jobs, str(tmp_path / "host"))
    with DeviceAnnotator(batch_size=batch_size, cache_frames=2) as dev:
        _run(dev, jobs, str(tmp_path / "dev"))
        assert batch_size != 1024 or dev.pending(str(tmp_path / "dev" / "sub" / "twice.jpg"))
    want, got = _tree(str(tmp_path / "host")), _tree(str(tmp_path / "dev"))
    assert sorted(want) == sorted(got) and len(want) == 3 * len(srcs) + 3
    for k in want:
        assert got[k] == want[k], k


def test_flush_makes_files_exist_and_errors_raise(tmp_path):
    srcs = _sources(str(tmp_path / "src"))
    dev = DeviceAnnotator()
    dst = str(tmp_path / "o" / "x.jpg")
    dev.annotate(srcs["a.jpg"][0], dst, [Mark(5, 5, 3, (1, 2, 3))])
    assert dev.pending(dst) and not os.path.exists(dst)
    dev.flush()
    assert os.path.exists(dst) and not dev.pending(dst)
    dev.annotate(str(tmp_path / "missing.jpg"), str(tmp_path / "o" / "y.jpg"), [])
    with pytest.raises(Exception):
        dev.flush()


def test_cached_frames_own_their_storage(tmp_path):
    srcs = _sources(str(tmp_path / "src"))
    dev = DeviceAnnotator(cache_frames=8)
    for name in ("a.jpg", "b.jpg", "c.jpg"):
        dev.annotate(srcs[name][0], str(tmp_path / "o" / name), [Mark(5, 5, 3, (1, 2, 3))])
    dev.flush()
    assert len(dev._frames) == 3
    for f in dev._frames.values():           # a view into the decode batch would keep the whole batch alive
        assert f.untyped_storage().nbytes() == f.shape[0] * f.shape[1] * 3


def test_writes_over_sources_keep_call_order(tmp_path):
    """Jobs that overwrite the source of a pending or cached read: the files equal those of the same calls on Pillow."""
    results = {}
    for name, make in (("pillow", PillowAnnotator), ("device", lambda: DeviceAnnotator(cache_frames=4))):
        d = str(tmp_path / name)
        srcs = _sources(os.path.join(d, "src"))
        a, b, g = srcs["a.jpg"][0], srcs["b.jpg"][0], srcs["g.png"][0]
        ann = make()
        ann.annotate(a, os.path.join(d, "o", "1.jpg"), [Mark(10, 10, 5, (0, 0, 255), "A")])     # reads a (cached after)
        ann.copy(b, a)                                                                           # overwrites a
        ann.annotate(a, os.path.join(d, "o", "2.jpg"), [Mark(20, 20, 5, (0, 255, 0))])         # must read the new a
        ann.annotate(b, os.path.join(d, "o", "3.jpg"), [])                                       # reads b ...
        ann.annotate(g, b, [Mark(30, 30, 5, (255, 0, 0), "B")])                                 # ... before b is overwritten
        ann.annotate(b, os.path.join(d, "o", "4.jpg"), [])
        ann.annotate(a, os.path.join(d, "o", "5.png"), [Mark(5, 5, 5, (9, 9, 9))])               # host path reads the new a
        ann.annotate(os.path.join(d, "o", "5.png"), os.path.join(d, "o", "6.jpg"), [])
        ann.annotate(os.path.join(d, "o", "1.jpg"), a, [])                                       # reads a pending output
        getattr(ann, "flush", lambda: None)()
        results[name] = _tree(d)
    want, got = results["pillow"], results["device"]
    assert sorted(want) == sorted(got)
    for k in want:
        assert got[k] == want[k], k
