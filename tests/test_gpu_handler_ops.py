"""The handler's object-cloud and frame-filter ops on the MI355X: the grey JPEG decode (csrc/image_ops.hip) against Pillow's
draft-L, the Laplacian's moments against integer arithmetic in NumPy, the exact k-nearest mean distance (csrc/cloud_ops.hip)
against scipy's cKDTree, and the mirror's functions (spatial_engine/utils/scannet_utils/handler/ops.py) built on them."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import handler_ops_util as HU  # noqa: E402

pytest.importorskip("scipy")


def _ops():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name in [m for m in sys.modules if m == "spatial_engine" or m.startswith("spatial_engine.")]:
        if not (getattr(sys.modules[name], "__file__", None) or "").startswith(root):
            del sys.modules[name]                   # never the reference's package of the same name
    from spatial_engine.utils.scannet_utils.handler import ops
    return ops


# ---- grey decode -----------------------------------------------------------------------------------------------------------
def _decode_luma(payloads, hw):
    import torch
    from mspa import engine
    offs, pos = [], 0
    for p in payloads:
        offs.append(pos)
        pos += (len(p) + 15) // 16 * 16
    buf = np.zeros(pos + 16, dtype=np.uint8)
    for o, p in zip(offs, payloads):
        buf[o:o + len(p)] = np.frombuffer(p, dtype=np.uint8)
    desc, parsed = engine.jpeg_parse_host(payloads)
    out, status = engine.jpeg_decode_luma_device(torch.from_numpy(buf).cuda(), torch.tensor(offs, dtype=torch.int64).cuda(),
                                                 torch.tensor([len(p) for p in payloads], dtype=torch.int64).cuda(),
                                                 torch.from_numpy(desc).cuda(), hw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), status.cpu().numpy(), parsed


LUMA_SIZES = [(1, 1), (16, 16), (17, 33), (100, 75)]


@pytest.mark.parametrize("hw", LUMA_SIZES, ids=[f"{h}x{w}" for h, w in LUMA_SIZES])
def test_luma_equals_pillow_draft_l(hw):
    h, w = hw
    payloads, names = [], []
    for sub in ("L", "4:4:4", "4:2:2", "4:2:0"):
        for restart in (0, 2):
            img = HU.smooth_image(h, w, 17 * len(payloads) + h, channels=1 if sub == "L" else 3)
            payloads.append(HU.jpeg_bytes(img, None if sub == "L" else sub, restart_blocks=restart))
            names.append((sub, restart))
    luma, st, parsed = _decode_luma(payloads, hw)
    assert luma.shape == (len(payloads), h, w) and luma.dtype == np.uint8
    for k, p in enumerate(payloads):
        assert parsed[k] == 0 and st[k] == 0, (hw, names[k], parsed[k], st[k])
        assert np.array_equal(luma[k], HU.pillow_luma(p)), f"{hw} {names[k]}: differs from Pillow's draft-L"


def test_progressive_file_is_declined_and_scores_the_same(tmp_path):
    from mspa import engine, ingest
    img = HU.smooth_image(100, 75, 3)
    base, prog = HU.jpeg_bytes(img, "4:2:0"), HU.jpeg_bytes(img, "4:2:0", progressive=True)
    _desc, parsed = engine.jpeg_parse_host([base, prog])
    assert parsed[0] == 0 and parsed[1] != 0
    paths = []
    for name, data in (("base.jpg", base), ("prog.jpg", prog)):
        paths.append(str(tmp_path / name))
        with open(paths[-1], "wb") as f:
            f.write(data)
    got = ingest.image_sharpness(paths)
    for g, data in zip(got, (base, prog)):
        s1, s2 = HU.moments(HU.pillow_luma(data))
        n = 100 * 75
        assert g == (n * s2 - s1 * s1) / (n * n)


# ---- Laplacian moments ---------------------------------------------------------------------------------------------------
def _moments(img):
    import torch
    from mspa import engine
    part = engine.laplacian_moments(torch.from_numpy(np.ascontiguousarray(img[None])).cuda())
    var = engine.laplacian_variance(part, img.size)[0]
    s = part.cpu().numpy()[0].sum(axis=0)
    return int(s[0]), int(s[1]), var


@pytest.mark.parametrize("img", HU.small_images(), ids=lambda a: f"{a.shape[0]}x{a.shape[1]}")
def test_moments_equal_the_integers(img):
    s1, s2, var = _moments(img)
    assert (s1, s2) == HU.moments(img)
    want = HU.variance_numpy(img)
    print(f"{img.shape}: var {var!r} numpy {want!r}")
    assert abs(var - want) <= 1e-12 * abs(want)


def test_moments_of_a_full_frame_checkerboard_do_not_overflow():
    img = HU.checkerboard()
    s1, s2, var = _moments(img)
    want = HU.moments(img)
    print(f"checkerboard: S1 {s1} S2 {s2} var {var!r} numpy {HU.variance_numpy(img)!r}")
    assert want[1] > 1e12 and (s1, s2) == want
    assert abs(var - HU.variance_numpy(img)) <= 1e-12 * HU.variance_numpy(img)


def test_moments_of_a_batch_are_per_image():
    import torch
    from mspa import engine
    rng = np.random.default_rng(2)
    batch = rng.integers(0, 256, size=(5, 19, 23), dtype=np.uint8)
    part = engine.laplacian_moments(torch.from_numpy(batch).cuda()).cpu().numpy()
    for k in range(5):
        assert tuple(int(v) for v in part[k].sum(axis=0)) == HU.moments(batch[k])


def test_filter_images_laplacian_keeps_order_and_its_own_threshold(tmp_path):
    from PIL import Image
    ops = _ops()
    rng = np.random.default_rng(9)
    paths = []
    for k, (hw, noise) in enumerate([((40, 56), 40), ((40, 56), 2), ((33, 17), 25), ((40, 56), 10), ((24, 24), 60)]):
        img = np.clip(128 + rng.normal(0, noise, size=hw + (3,)), 0, 255).astype(np.uint8)
        paths.append(str(tmp_path / f"{k}.jpg"))
        Image.fromarray(img).save(paths[-1], quality=92)
    paths.append(str(tmp_path / "grey.png"))                                   # not a JPEG: Pillow's grey rule on the host
    Image.fromarray(np.clip(128 + rng.normal(0, 30, size=(20, 31)), 0, 255).astype(np.uint8)).save(paths[-1])
    scores = [float(ops.calculate_image_sharpness(p)) for p in paths]
    for p, s in zip(paths[:5], scores):
        with open(p, "rb") as f:
            luma = HU.pillow_luma(f.read())
        assert abs(s - HU.variance_numpy(luma)) <= 1e-12 * HU.variance_numpy(luma)
    assert abs(scores[5] - HU.variance_numpy(np.asarray(Image.open(paths[5]).convert("L")))) <= 1e-12 * scores[5]
    assert len(set(scores)) == len(scores)
    for k, s in enumerate(scores):                                             # a threshold equal to an image's own score keeps it
        kept = ops.filter_images_laplacian(paths, threshold=s)
        assert kept == [p for p, t in zip(paths, scores) if t >= s] and paths[k] in kept
    assert ops.filter_images_laplacian(paths, threshold=max(scores) * 2) == []
    with pytest.raises(ValueError, match="Unable to read image from"):
        ops.calculate_image_sharpness(str(tmp_path / "missing.jpg"))
    with open(tmp_path / "junk.jpg", "wb") as f:
        f.write(b"not an image at all")
    with pytest.raises(ValueError, match="Unable to read image from"):
        ops.calculate_image_sharpness(str(tmp_path / "junk.jpg"))


# ---- k-nearest mean distance -------------------------------------------------------------------------------------------------
KNN_CASES = [("uniform", n, 20) for n in (1, 2, 19, 20, 21, 64, 65, 1000, 20000)] + [("uniform", 1000, 1), ("uniform", 1000, 64)] + \
    [("plane", 1000, 20), ("line", 1000, 20), ("clusters", 1000, 20), ("identical", 200, 20), ("far", 20000, 20)]


def _knn(xyz, k):
    import torch
    from mspa import engine
    mean, evals = engine.knn_mean_distance(torch.from_numpy(xyz).cuda(), k, want_evals=True)
    return mean.cpu().numpy(), evals.cpu().numpy()


@pytest.mark.parametrize("kind,n,k", KNN_CASES, ids=[f"{c[0]}-{c[1]}-k{c[2]}" for c in KNN_CASES])
def test_knn_mean_distance_against_ckdtree(kind, n, k):
    xyz = HU.cloud(kind, n)
    mean, evals = _knn(xyz, k)
    want = HU.knn_mean_oracle(xyz, k)
    err = np.abs(mean - want)
    print(f"{kind} n={len(xyz)} k={k}: max error {float((err / np.where(want > 0, want, 1)).max()) / 2.0 ** -53:.2f} x 2^-53, "
          f"evaluations per point {evals.sum() / len(xyz):.1f}")
    assert (err <= HU.knn_tolerance(k) * want).all()
    if kind == "identical":
        assert (mean == 0).all()
    if kind == "far":                     # the far points did not stretch the grid into one cell: no all-pairs search
        assert int(evals.astype(np.int64).sum()) < len(xyz) ** 2 / 8


def test_knn_host_twin_gives_the_same_bits():
    from mspa import engine
    for kind, n, k in (("uniform", 1000, 20), ("far", 20000, 20), ("clusters", 1000, 20)):
        xyz = HU.cloud(kind, n)
        mean, evals = _knn(xyz, k)
        host_mean, host_evals = engine.knn_mean_distance_host(xyz, k, want_evals=True)
        assert np.array_equal(mean, host_mean) and np.array_equal(evals, host_evals)


def test_wrappers_refuse_tensors_they_cannot_take():
    import torch
    from mspa import engine
    pts = torch.from_numpy(HU.cloud("uniform", 30)).cuda()
    for bad in (pts.float(), pts.cpu(), pts[:, :2], pts.t().contiguous().t(), pts.cpu().numpy()):
        with pytest.raises(ValueError, match="mspa.engine: xyz"):
            engine.knn_mean_distance(bad, 5)
    for k in (0, 65):
        with pytest.raises(ValueError, match="mspa.engine"):
            engine.knn_mean_distance(pts, k)
    assert engine.knn_mean_distance(pts[:0], 5).shape == (0,)
    img = torch.zeros((2, 5, 7), dtype=torch.uint8, device="cuda")
    for bad in (img.int(), img.cpu(), img[0], img[:, :, ::2]):
        with pytest.raises(ValueError, match="mspa.engine: luma"):
            engine.laplacian_moments(bad)
    assert engine.laplacian_moments(img[:0]).shape == (0, 1, 2)


# ---- remove_statistical_outliers -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def far_cloud():
    xyz = HU.cloud("far", 20000)
    avg = HU.knn_mean_oracle(xyz, 20)
    kept, thr = HU.outlier_rule_oracle(avg, 1.0)
    return xyz, avg, kept, thr


def test_outliers_keep_the_oracles_rows(far_cloud):
    ops = _ops()
    xyz, avg, kept, thr = far_cloud
    gap = float(np.abs(avg - thr).min() / thr)
    print(f"nearest avg to the threshold: {gap:.3g} of it away; kept {len(kept)} of {len(xyz)}")
    assert gap > 1e-9 and len(kept) == 20000
    extra = np.arange(len(xyz), dtype=np.float64)[:, None]
    data = np.hstack([xyz, extra, -extra])
    out = ops.remove_statistical_outliers(data)
    assert isinstance(out, np.ndarray) and out.dtype == np.float64 and np.array_equal(out, data[kept])
    for kind, n, nb, ratio in (("uniform", 1000, 20, 1.0), ("clusters", 1000, 8, 0.5), ("plane", 1000, 64, 2.0)):
        pts = HU.cloud(kind, n)
        a = HU.knn_mean_oracle(pts, nb)
        want, t = HU.outlier_rule_oracle(a, ratio)
        assert float(np.abs(a - t).min() / t) > 1e-9
        assert np.array_equal(ops.remove_statistical_outliers(pts, nb, ratio), pts[want]), (kind, n, nb, ratio)


def test_outliers_dtype_columns_and_device_tensors(far_cloud):
    import torch
    ops = _ops()
    xyz, _avg, kept, _thr = far_cloud
    data32 = np.hstack([xyz, np.arange(len(xyz))[:, None]]).astype(np.float32)
    a32 = HU.knn_mean_oracle(data32[:, :3].astype(np.float64), 20)
    want32, t32 = HU.outlier_rule_oracle(a32, 1.0)
    assert float(np.abs(a32 - t32).min() / t32) > 1e-9
    out32 = ops.remove_statistical_outliers(data32)
    assert out32.dtype == np.float32 and np.array_equal(out32, data32[want32])
    dev = torch.from_numpy(np.hstack([xyz, np.arange(len(xyz))[:, None]])).cuda()
    out = ops.remove_statistical_outliers(dev)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float64
    assert np.array_equal(out.cpu().numpy(), dev.cpu().numpy()[kept])
    same = ops.remove_statistical_outliers(HU.cloud("identical", 200))
    assert same.shape == (0, 3)


def test_outliers_edge_cases_and_errors():
    ops = _ops()
    assert ops.remove_statistical_outliers(np.zeros((0, 5))).shape == (0, 5)
    assert ops.remove_statistical_outliers(np.ones((1, 4))).shape == (0, 4)
    pts = HU.cloud("uniform", 50)
    for nb, ratio in ((0, 1.0), (-3, 1.0), (20, 0.0), (20, -1.0)):
        with pytest.raises(RuntimeError):
            ops.remove_statistical_outliers(pts, nb, ratio)
    with pytest.raises(NotImplementedError, match="64"):
        ops.remove_statistical_outliers(pts, 65)
    for bad in (np.nan, np.inf, -np.inf):
        broken = pts.copy()
        broken[7, 1] = bad
        with pytest.raises(ValueError):
            ops.remove_statistical_outliers(broken)


def test_small_functions_on_device_tensors_agree_with_numpy():
    import torch
    ops = _ops()
    rng = np.random.default_rng(4)
    pts = rng.normal(size=(500, 5))
    box = ops.calculate_aabb(pts)
    dbox = ops.calculate_aabb(torch.from_numpy(pts).cuda())
    assert dbox.is_cuda and np.array_equal(dbox.cpu().numpy(), box)
    corners = ops.convert_to_corners([torch.from_numpy(box).cuda()])[0]
    assert corners.is_cuda and corners.dtype == torch.float32 and np.array_equal(corners.cpu().numpy(), ops.convert_to_corners([box])[0])
    other = box + np.array([0.3, -0.2, 0.1, 0.5, 0.0, 1.0])
    iou = ops.calculate_iou_3d(torch.from_numpy(box).cuda(), torch.from_numpy(other).cuda())
    assert iou.is_cuda and abs(float(iou) - float(ops.calculate_iou_3d(box, other))) <= 4 * 2.0 ** -53 * float(iou)
    m1, m2 = rng.random((30, 40)) > 0.5, rng.random((30, 40)) > 0.7
    got = ops.calculate_iou_2d(torch.from_numpy(m1).cuda(), torch.from_numpy(m2).cuda())
    assert abs(float(got) - ops.calculate_iou_2d(m1, m2)) <= 2.0 ** -23
    assert float(ops.calculate_iou_2d(torch.zeros((3, 3)).cuda(), torch.zeros((3, 3)).cuda())) == 0.0
    ints = rng.integers(0, 6, size=(300, 4)).astype(np.float64)                # ties: the device ranks them stably
    cut = ops.remove_truncated_outliers(torch.from_numpy(ints).cuda(), 0.1, 0.05, 0.2)
    keep = np.ones(300, dtype=bool)
    for axis, t in enumerate((0.1, 0.05, 0.2)):
        c = int(t * 300)
        inside = np.zeros(300, dtype=bool)
        inside[np.argsort(ints[:, axis], kind="stable")[c:-c]] = True
        keep &= inside
    assert cut.is_cuda and np.array_equal(cut.cpu().numpy(), ints[keep])
