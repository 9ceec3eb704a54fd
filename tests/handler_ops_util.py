"""Oracles and inputs shared by test_handler_ops_cpu.py and test_gpu_handler_ops.py: the Laplacian by np.pad, the
statistical-outlier rule on scipy's cKDTree with sequential sums, the test clouds, and a Pillow JPEG maker."""
import io
import math

import numpy as np


# ---- sharpness -----------------------------------------------------------------------------------------------------------
def laplacian(img: np.ndarray) -> np.ndarray:
    """int64 [H, W]: the 4-neighbour Laplacian with reflect-101 borders (np.pad's "reflect"; a dimension of length 1 has
    nothing to reflect, every index maps to its one entry: "edge")."""
    a = np.asarray(img).astype(np.int64)
    p = np.pad(a, ((1, 1), (0, 0)), mode="reflect" if a.shape[0] > 1 else "edge")
    p = np.pad(p, ((0, 0), (1, 1)), mode="reflect" if a.shape[1] > 1 else "edge")
    return p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:] - 4 * a


def moments(img: np.ndarray):
    """(S1, S2) as Python integers."""
    lap = laplacian(img)
    return int(lap.sum()), int((lap * lap).sum())


def variance_numpy(img: np.ndarray) -> float:
    """What upstream computes: the float64 Laplacian's ``.var()``."""
    return float(laplacian(img).astype(np.float64).var())


def small_images(seed: int = 5):
    rng = np.random.default_rng(seed)
    shapes = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (3, 65), (64, 8), (130, 17)]
    return [rng.integers(0, 256, size=s, dtype=np.uint8) for s in shapes]


def checkerboard(h: int = 968, w: int = 1296) -> np.ndarray:
    y, x = np.mgrid[0:h, 0:w]
    return (((x + y) & 1) * 255).astype(np.uint8)


def jpeg_bytes(arr: np.ndarray, subsampling=None, quality: int = 90, restart_blocks: int = 0, progressive: bool = False) -> bytes:
    """A JPEG of ``arr`` ([H, W] grey or [H, W, 3] RGB) as Pillow writes it."""
    from PIL import Image
    buf = io.BytesIO()
    kw = {"quality": quality, "progressive": progressive}
    if subsampling is not None:
        kw["subsampling"] = subsampling
    if restart_blocks:
        kw["restart_marker_blocks"] = restart_blocks
    Image.fromarray(arr).save(buf, "JPEG", **kw)
    return buf.getvalue()


def pillow_luma(data: bytes) -> np.ndarray:
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        im.draft("L", im.size)
        return np.asarray(im.convert("L"))


def smooth_image(h: int, w: int, seed: int, channels: int = 3) -> np.ndarray:
    """Low-frequency content plus a little noise: coefficients of every kind without saturating the IDCT."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    planes = [127 + 90 * np.sin(x / (3.0 + c) + c) * np.cos(y / (4.0 + c)) + rng.normal(0, 8, size=(h, w)) for c in range(channels)]
    img = np.clip(np.stack(planes, axis=-1), 0, 255).astype(np.uint8)
    return img[..., 0] if channels == 1 else img


# ---- clouds ----------------------------------------------------------------------------------------------------------------
def cloud(kind: str, n: int, seed: int = 11) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return rng.random((n, 3))
    if kind == "plane":
        p = rng.random((n, 3))
        p[:, 2] = 0.25
        return p
    if kind == "line":
        t = rng.random(n)
        return np.stack([t, 2.0 * t + 1.0, -0.5 * t], axis=1)
    if kind == "clusters":                       # the same count in a unit cube and in one a tenth the side: 1 000x the density
        p = rng.random((n, 3))
        p[n // 2:] = 5.0 + 0.1 * p[n // 2:]
        return p
    if kind == "identical":
        return np.tile(np.array([[0.3, -1.5, 2.0]]), (n, 1))
    if kind == "far":                            # n uniform points plus 30 at 1 000x the extent
        return np.concatenate([rng.random((n, 3)), (rng.random((30, 3)) - 0.5) * 2000.0])
    raise ValueError(kind)


def knn_mean_oracle(xyz: np.ndarray, k: int) -> np.ndarray:
    """[N]: mean distance to the min(k, N) nearest points, self included, distances summed ascending, one at a time."""
    from scipy.spatial import cKDTree
    xyz = np.asarray(xyz, dtype=np.float64)
    n = len(xyz)
    kk = min(k, n)
    d, _ = cKDTree(xyz).query(xyz, k=kk)
    d = np.sort(d.reshape(n, kk), axis=1)
    total = np.zeros(n)
    for j in range(kk):
        total = total + d[:, j]
    return total / kk


def knn_tolerance(k: int) -> float:
    return 2 * (k + 5) * 2.0 ** -53


def outlier_rule_oracle(avg: np.ndarray, std_ratio: float):
    """(kept indices, threshold) by the rule of handler/ops.py's docstring, sums taken one element at a time."""
    n = len(avg)
    if n == 0:
        return np.zeros(0, dtype=np.int64), math.nan
    total = 0.0
    for a in avg.tolist():
        if a > 0:
            total += a
    mean = total / n
    sq = 0.0
    for a in avg.tolist():
        if a > 0:
            sq += (a - mean) * (a - mean)
    sd = math.sqrt(sq / (n - 1)) if n > 1 else math.nan
    thr = mean + std_ratio * sd
    return np.nonzero((avg > 0) & (avg < thr))[0], thr
