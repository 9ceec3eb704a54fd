"""The ragged batch shared by test_cloud_segments_cpu.py, test_gpu_cloud_segments.py and test_gpu_cloud_segments_memory.py, the
Python restatement of the sum order csrc/cloud_segments_core.h states, and the guard in front of every comparison of kept sets."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import handler_ops_util as HU  # noqa: E402

KS = (1, 20, 64)
RATIOS = (1.0, 0.5)
LANES = 256

# Segment lengths, in this order: a zero first, in the middle and last; k - 1, k, k + 1 at k = 20; around the wave width; the
# order-statistic rank goes from 0 to 1 at n = 100; the short neighbours put rows of three segments into one wave.
UNIFORM = (0, 1, 2, 19, 20, 21, 0, 63, 64, 65, 99, 100, 101, 257, 4097, 0)
NEAR_1E3 = 20000


@functools.lru_cache(maxsize=None)
def batch():
    """(xyz [N, 3] float64, offsets [S + 1] int64, names [S]) -- about 30 k rows; built once, never written."""
    parts, names = [], []
    for s, n in enumerate(UNIFORM):
        parts.append(HU.cloud("uniform", n, seed=100 + s))
        names.append(f"uniform-{n}")
    parts.append(HU.cloud("plane", 3000, seed=201))
    parts.append(HU.cloud("line", 500, seed=202))
    parts.append(HU.cloud("identical", 200, seed=203))
    parts.append(HU.cloud("far", 2000, seed=204)[:2005])                   # 2 000 uniform points plus 5 at 1 000 x the extent
    parts.append(HU.cloud("uniform", NEAR_1E3, seed=205) + 1e3)            # coordinates near 1e3: the faces' eps matters
    names += ["plane-3000", "line-500", "identical-200", "far-2005", f"near-1e3-{NEAR_1E3}"]
    offsets = np.zeros(len(parts) + 1, dtype=np.int64)
    np.cumsum([len(p) for p in parts], out=offsets[1:])
    xyz = np.ascontiguousarray(np.concatenate(parts), dtype=np.float64)
    xyz.setflags(write=False)
    offsets.setflags(write=False)
    return xyz, offsets, tuple(names)


def small_batches():
    """Further cases: one segment, every segment empty, no segment at all."""
    one = HU.cloud("uniform", 300, seed=301)
    return {"S=1": (one, np.array([0, 300], dtype=np.int64)),
            "all-empty": (np.zeros((0, 3)), np.zeros(5, dtype=np.int64)),
            "N=0": (np.zeros((0, 3)), np.zeros(1, dtype=np.int64))}


def ordered_sum(terms) -> np.float64:
    """The header's order in NumPy float64 scalars: lane j of 256 adds terms j, j + 256, ... ascending from 0.0, then the partials
    fold by strides 128, 64, ..., 1."""
    terms = np.asarray(terms, dtype=np.float64)
    partial = []
    for j in range(LANES):
        p = np.float64(0.0)
        for x in terms[j::LANES]:
            p = p + x
        partial.append(p)
    t = LANES // 2
    while t >= 1:
        for j in range(t):
            partial[j] = partial[j] + partial[j + t]
        t //= 2
    return partial[0]


def stated_statistics(avg, std_ratio):
    """(mean, sd, thr) of one segment by the header's text."""
    avg = np.asarray(avg, dtype=np.float64)
    n = len(avg)
    nan = np.float64("nan")
    if n == 0:
        return nan, nan, nan
    mean = ordered_sum(np.where(avg > 0, avg, 0.0)) / np.float64(n)
    if n < 2:
        return mean, nan, nan
    dev = avg - mean
    sd = np.sqrt(ordered_sum(np.where(avg > 0, dev * dev, 0.0)) / np.float64(n - 1))
    return mean, sd, mean + np.float64(std_ratio) * sd


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def assert_guard(avg, offsets, thresholds, what=""):
    """No positive avg of any segment lies within 1e-9 relative of one of ``thresholds`` ([S] each): a condition on the batch, in
    front of every comparison of kept sets between two orders of summation.  It is asserted for every segment and skips none.
    One kind of segment cannot meet it by any choice of seed and is held to a stronger condition instead: n = 2 with k >= 2, where
    both avg are the same number d / 2.  x + x and 2x / 2 are exact, so in EVERY order mean = thr = that number exactly; there the
    avg must EQUAL the threshold bit for bit (the strict comparison then drops both rows under every order)."""
    for s in range(len(offsets) - 1):
        v = np.asarray(avg[offsets[s]:offsets[s + 1]])
        for thr in thresholds:
            t = thr[s]
            pos = v[v > 0]
            if len(v) == 2 and len(pos) == 2 and pos[0] == pos[1]:
                assert (pos == t).all(), (what, s, pos, t)
                continue
            if len(pos) and np.isfinite(t):
                assert (np.abs(pos - t) > 1e-9 * abs(t)).all(), (what, s, float(t))


def torch_sum_thresholds(avg, offsets, ratio):
    """[S] float64: the threshold handler/ops.py forms per segment of a device ``avg``, with torch.sum (NaN for an empty segment)."""
    import torch
    out = np.full(len(offsets) - 1, np.nan)
    zero = torch.zeros((), dtype=torch.float64, device=avg.device)
    for s in range(len(offsets) - 1):
        v = avg[int(offsets[s]):int(offsets[s + 1])]
        n = len(v)
        if n:
            pos = v > 0
            mean = torch.where(pos, v, zero).sum() / n
            dev = v - mean
            out[s] = float(mean + ratio * torch.sqrt(torch.where(pos, dev * dev, zero).sum() / (n - 1)))
    return out


def assert_guard_on_device(rows, offsets, k, ratio, what=""):
    """``assert_guard`` for a device batch ``rows`` [N, C >= 3] against the stated order's and torch.sum's thresholds."""
    import torch
    from mspa import cloud_segments as CS
    xyz = rows[:, :3].to(torch.float64).contiguous()
    avg = CS.knn_mean_distance_segments(xyz, offsets, k)
    stated = CS.outlier_stats_segments(avg, offsets, ratio, xyz)["thr"].cpu().numpy()
    assert_guard(avg.cpu().numpy(), offsets, (stated, torch_sum_thresholds(avg, offsets, ratio)), what)
