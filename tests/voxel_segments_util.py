"""The ragged batch shared by test_voxel_segments_cpu.py, test_gpu_voxel_segments.py and test_gpu_voxel_segments_memory.py, and the
oracle of the voxel down-sampling written from the rule's text alone (csrc/voxel_grid_core.h's header comment): NumPy forms the
indices, ``np.unique(axis=0)`` over (segment, ix, iy, iz) gives the order, a Python loop forms every sum in ``np.float64`` scalars.

The batch is tests/cloud_segments_util.py's (30 614 rows in 21 segments, empty segments first, in the middle and last) followed by
  * lattice-3000      coordinates k / 8, k in 0 .. 31: at voxel size 0.25 every operand is exact and every odd k sits exactly on a
                      voxel face (floor must put it in the upper voxel);
  * decimal-2000      coordinates k / 10, k in 0 .. 31: at size 0.1 the rounding of the division decides;
  * wave-20, wave-17, wave-9   three segments of fewer than 64 rows in total: they share one wave;
  * negative-500      uniform points shifted to negative coordinates.
With ``columns = 6`` three further columns hold row-dependent integers, so a wrong row in a run shows in a mean."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_segments_util as U  # noqa: E402
import handler_ops_util as HU  # noqa: E402

SIZES = (0.01, 0.1, 0.25, 100.0)                 # every segment fits at 0.01; both sum regimes at 0.25; voxels that swallow a segment at 100
TOO_SMALL = 1e-6                                 # far-2005 breaks the 2^21 limit
COLUMNS = (3, 6)
AXIS_LIMIT = 1 << 21
SEQUENTIAL, LANES = 64, 64
bits = U.bits


@functools.lru_cache(maxsize=None)
def batch(columns=3):
    """(rows [N, columns] float64, offsets [S + 1] int64, names [S]); built once, never written."""
    xyz, offsets, names = U.batch()
    rng = np.random.default_rng(77)
    parts = [xyz,
             rng.integers(0, 32, size=(3000, 3)) / 8.0,
             rng.integers(0, 32, size=(2000, 3)) / 10.0,
             HU.cloud("uniform", 20, seed=401), HU.cloud("uniform", 17, seed=402), HU.cloud("uniform", 9, seed=403),
             HU.cloud("uniform", 500, seed=404) - 7.5]
    names = tuple(names) + ("lattice-3000", "decimal-2000", "wave-20", "wave-17", "wave-9", "negative-500")
    off = np.concatenate([offsets, offsets[-1] + np.cumsum([len(p) for p in parts[1:]])]).astype(np.int64)
    rows = np.ascontiguousarray(np.concatenate(parts), dtype=np.float64)
    assert (rows[off[-2]:] < 0).all()
    if columns > 3:
        i = np.arange(len(rows), dtype=np.int64)
        extra = np.stack([i, (i * 7) % 1000, (i * i) % 997], axis=1)[:, :columns - 3].astype(np.float64)
        rows = np.ascontiguousarray(np.concatenate([rows, extra], axis=1))
    rows.setflags(write=False)
    off.setflags(write=False)
    return rows, off, names


SCAN_SLOTS = 256 * 2048                          # the compaction's scan: 256 threads, a tile of 2 048 slots each up to here


@functools.lru_cache(maxsize=None)
def scan_batch():
    """(rows [N, 4] float64, offsets [5] int64) for the compaction's scan with TWO tiles per thread: more than 256 tiles of 2 048 slots.
    The first 526 400 points of the integer lattice 81^3 (spacing 1.0) in three segments with an empty one between them, the
    first boundary (200 003) no multiple of a tile; the last segment also holds five of its lattice points 70 more times each, so
    five voxels are runs of 71 rows.  Every lattice point is its own voxel at size 0.5 and its own cluster at eps 0.4, so the heads,
    the voxels and the representatives all pass 256 tiles.  The fourth column is a row-dependent integer.  Built once, never written."""
    n = 526400
    i = np.arange(n, dtype=np.int64)
    lattice = np.stack([i // 6561, i // 81 % 81, i % 81], axis=1).astype(np.float64)
    repeated = lattice[[400000, 411111, 450007, 500000, n - 1]].repeat(70, axis=0)
    xyz = np.concatenate([lattice, repeated])
    r = np.arange(len(xyz), dtype=np.int64)
    rows = np.ascontiguousarray(np.concatenate([xyz, ((r * 7) % 1000)[:, None].astype(np.float64)], axis=1))
    off = np.array([0, 200003, 200003, 400000, len(rows)], dtype=np.int64)
    assert len(rows) > SCAN_SLOTS and n > SCAN_SLOTS and off[1] % 2048 and off[1] % 4096
    rows.setflags(write=False)
    off.setflags(write=False)
    return rows, off


def small_batches():
    """tests/cloud_segments_util.py's further cases (one segment, every segment empty, no segment at all) and one row."""
    out = dict(U.small_batches())
    out["n=1"] = (np.array([[0.25, -3.0, 1e3]]), np.array([0, 0, 1, 1], dtype=np.int64))
    return out


def indices(rows, offsets, size):
    """[N, 4] int64 (segment, ix, iy, iz) by the rule's text: min_bound = lo - size * 0.5, idx = floor((p - min_bound) / size), every
    step one float64 operation."""
    size = np.float64(size)
    out = np.zeros((len(rows), 4), dtype=np.int64)
    for s in range(len(offsets) - 1):
        a, b = int(offsets[s]), int(offsets[s + 1])
        if b > a:
            p = np.asarray(rows[a:b, :3], dtype=np.float64)
            min_bound = p.min(axis=0) - size * np.float64(0.5)
            out[a:b, 0] = s
            out[a:b, 1:] = np.floor((p - min_bound) / size).astype(np.int64)
    return out


def stated_sum(terms) -> np.float64:
    """The rule's order in NumPy float64 scalars: up to 64 terms sequentially from 0.0; above, lane j of 64 adds terms j, j + 64, ...
    ascending from 0.0 and the partials fold by strides 32, 16, ..., 1."""
    if len(terms) <= SEQUENTIAL:
        total = np.float64(0.0)
        for x in terms:
            total = total + x
        return total
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


def oracle(rows, offsets, size):
    """(out_rows [M, C], out_offsets [S + 1], counts [M], voxels [M, 4]) by the rule's text; ``voxels`` the (segment, ix, iy, iz) of
    every output row.  Raises ValueError where the rule refuses."""
    rows = np.asarray(rows, dtype=np.float64)
    if not np.isfinite(rows[:, :3]).all():
        raise ValueError("non-finite")
    idx = indices(rows, offsets, size)
    if len(idx) and idx[:, 1:].max() >= AXIS_LIMIT:
        raise ValueError("voxel_size")
    S = len(offsets) - 1
    if not len(rows):
        return rows[:0].copy(), np.zeros(S + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), idx
    voxels, inverse = np.unique(idx, axis=0, return_inverse=True)           # lexicographic: segment, then ix, iy, iz -- the key order
    by_voxel = np.argsort(inverse.reshape(-1), kind="stable")              # a voxel's rows in ascending input row index
    counts = np.bincount(inverse.reshape(-1), minlength=len(voxels)).astype(np.int32)
    starts = np.concatenate([[0], np.cumsum(counts)])
    out = np.empty((len(voxels), rows.shape[1]), dtype=np.float64)
    for v in range(len(voxels)):
        members = rows[by_voxel[starts[v]:starts[v + 1]]]
        m = np.float64(len(members))
        for c in range(rows.shape[1]):
            out[v, c] = stated_sum(members[:, c]) / m
    out_offsets = np.zeros(S + 1, dtype=np.int64)
    np.cumsum(np.bincount(voxels[:, 0], minlength=S), out=out_offsets[1:])
    return out, out_offsets, counts, voxels


@functools.lru_cache(maxsize=None)
def batch_oracle(size, columns=3):
    rows, offsets, _names = batch(columns)
    return oracle(rows, offsets, size)


@functools.lru_cache(maxsize=None)
def batch_twin(size, columns=3):
    """The host twin on the batch: computed once, shared by the tests that need a reference."""
    from mspa import cloud_segments as CS
    rows, offsets, _names = batch(columns)
    return CS.voxel_down_sample_segments_host(rows, offsets, size)


def assert_same(got, want, what=""):
    """(rows, offsets, counts) against (rows, offsets, counts, ...): shapes, dtypes and every bit."""
    assert got[0].shape == want[0].shape and got[0].dtype == np.float64, (what, got[0].shape, want[0].shape)
    assert np.array_equal(np.asarray(got[1]), want[1]) and np.asarray(got[1]).dtype == np.int64, what
    assert np.array_equal(got[2], want[2]) and got[2].dtype == np.int32, what
    assert np.array_equal(bits(got[0]), bits(want[0])), (what, np.argwhere(bits(got[0]) != bits(want[0]))[:3])
