"""Inputs and the NumPy restatement for the instance-split tests (CPU: mspa_instance_split_host; GPU: engine.instance_split).

The restatement is the rule's definition and nothing else: segment (f, v) = ``np.flatnonzero((labels[f] == v) & valid[f])`` for
v = 1 .. 255, segments in (frame, label) order."""
import numpy as np

SIZES = (1, 63, 64, 65, 4095, 4096, 4097, 162 * 121)             # pixels per frame: around a wave (64) and a tile (4 096), then ScanNet / 8
FRAMES = (1, 3)
PATTERNS = ("zero", "one", "round_robin", "blocky", "last_wave", "all_invalid")


def hw_of(P):
    """An (H, W) with H * W = P (the split takes the pixel count apart only for ``rgb``'s shape)."""
    return (121, 162) if P == 162 * 121 else (1, P)


def make_case(F, P, pattern, seed):
    """(labels [F, H, W] uint8, valid [F, P] uint8, xyz [F, P, 3] float64, rgb [F, H, W, 3] uint8)."""
    rng = np.random.default_rng(seed)
    H, W = hw_of(P)
    valid = (rng.random((F, P)) < 0.8).astype(np.uint8) * rng.choice(np.array([1, 255], np.uint8), (F, P))
    if pattern == "zero":
        labels = np.zeros((F, P), np.uint8)
    elif pattern == "one":
        labels = np.full((F, P), 7, np.uint8)
    elif pattern == "round_robin":                                # 255 labels in turn: every wave holds 64 distinct labels
        labels = (np.arange(F * P).reshape(F, P) % 255 + 1).astype(np.uint8)
    elif pattern == "blocky":                                     # runs of 1 .. 200 pixels of one label, label 0 among them
        labels = np.zeros((F, P), np.uint8)
        for f in range(F):
            p = 0
            while p < P:
                n = int(rng.integers(1, 200))
                labels[f, p:p + n] = int(rng.choice(np.array([0, 1, 2, 3, 17, 128, 254, 255])))
                p += n
    elif pattern == "last_wave":                                  # label 9 only in the last, partial wave of the frame
        labels = rng.integers(1, 4, (F, P)).astype(np.uint8)
        tail = max(P - (P % 64 or 64), 0)
        labels[:, tail:] = 9
        valid[:, P - 1] = 1
    elif pattern == "all_invalid":                                # label 5's pixels are all invalid: an empty segment among full ones
        labels = rng.integers(4, 7, (F, P)).astype(np.uint8)
        valid[labels == 5] = 0
    else:
        raise ValueError(pattern)
    xyz = rng.standard_normal((F, P, 3)) * 3.0
    rgb = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    return labels.reshape(F, H, W), valid, xyz, rgb


def numpy_split(labels, valid, xyz, rgb=None):
    """(counts [F, 256] int32, offsets [F * 256 + 1] int64, xyz [total, 3], rgb [total, 3] or None, pixel [total] int32, lo, hi)."""
    F = labels.shape[0]
    P = int(np.prod(labels.shape[1:]))
    lab, val = labels.reshape(F, P), valid.reshape(F, P) != 0
    counts = np.zeros((F, 256), np.int32)
    lo, hi = np.full((F, 256, 3), np.inf), np.full((F, 256, 3), -np.inf)
    rows, cols, pix = [], [], []
    for f in range(F):
        for v in range(1, 256):
            idx = np.flatnonzero((lab[f] == v) & val[f])
            counts[f, v] = len(idx)
            if len(idx):
                rows.append(xyz[f].reshape(P, 3)[idx])
                pix.append(idx.astype(np.int32))
                lo[f, v], hi[f, v] = rows[-1].min(axis=0), rows[-1].max(axis=0)
                if rgb is not None:
                    cols.append(rgb[f].reshape(P, 3)[idx])
    offsets = np.zeros(F * 256 + 1, np.int64)
    np.cumsum(counts.reshape(-1), out=offsets[1:])
    cat = lambda parts, width, dtype: np.concatenate(parts) if parts else np.zeros((0,) + width, dtype)  # noqa: E731
    return (counts, offsets, cat(rows, (3,), np.float64), None if rgb is None else cat(cols, (3,), np.uint8),
            cat(pix, (), np.int32), lo, hi)


def assert_same(got, want, what=""):
    names = ("counts", "offsets", "xyz", "rgb", "pixel", "lo", "hi")
    for name, g, w in zip(names, got, want):
        if w is None:
            assert g is None, (what, name)
            continue
        g = np.asarray(g)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        assert g.tobytes() == w.tobytes(), (what, name)
