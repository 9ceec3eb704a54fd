"""The ragged batch shared by test_dbscan_segments_cpu.py, test_gpu_dbscan_segments.py and test_gpu_dbscan_segments_memory.py, the
reference (scikit-learn's DBSCAN per segment, imported only where a test calls it) and the frozen labels of tests/golden.

The batch is the 21 + 6 segments of tests/voxel_segments_util.batch() -- near-1e3-20000 cut to its first 1 000 rows: at eps = 100
every pair of a segment is near, and scikit-learn holds all of a segment's neighbourhoods at once -- followed by
  * chain-3000        points 0.9 * eps apart (eps = 0.05) along a diagonal, rows shuffled: at min_points <= 3 ONE cluster through
                      thousands of cells and many workgroups, the longest paths the union-find sees;
  * bridge            two Gaussian blobs of 300 joined by a line of 25 points;
  * dup8              300 float32-origin points, each 8 times, shuffled;
  * far               bridge shifted by (1234.5, -987.25, 55.125);
  * lattice-eighths   coordinates k / 8, k in 0 .. 7: at eps = 0.125 every lattice neighbour lies at exactly eps;
  * lattice-tenths    coordinates k / 10, k in 0 .. 7: at eps = 0.1 the rounding of dx * dx decides;
  * shared-border, shared-border-swapped   two core groups and one point that is not core near a core point of each; in the second
                      copy the group that comes later in the first comes first (the border point takes the LOWER number, which
                      is then the other group);
  * noise-only        40 points 10 apart;
  * n=1, and empty segments at the front, in the middle and at the end.
Under 25 000 rows.  Every segment has its own eps (0.05 unless said otherwise); the tests run the whole batch at every distinct own
eps, at 0.02 and at 100."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_segments_util as V  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dbscan_labels.npz")
OWN_EPS = {"lattice-eighths": 0.125, "lattice-tenths": 0.1, "lattice-3000": 0.125, "decimal-2000": 0.1}
DEFAULT_EPS = 0.05
MIN_POINTS = (1, 4, 10, 20)
GOLDEN_PARAMETERS = ((0.05, 4), (0.125, 10))
TOO_SMALL = 1e-6                                  # far's and far-2005's extents break the 2^21 limit
CUT = {"near-1e3-20000": 1000}


def _bridge(rng):
    a = rng.normal(0.0, 0.03, size=(300, 3))
    b = rng.normal(0.0, 0.03, size=(300, 3)) + np.array([0.6, 0.0, 0.0])
    line = np.stack([np.linspace(0.0, 0.6, 25), np.zeros(25), np.zeros(25)], axis=1)
    return np.concatenate([a, b, line])


def _shared_border(swapped: bool):
    """Group A: 6 points 0.004 from the origin; group B: 6 points 0.004 from (0.107, 0, 0); the border point at (0.0535, 0, 0) is 0.0495
    from A's point (0.004, 0, 0) and from B's point (0.103, 0, 0) and more than 0.0536 from every other: three near points, itself
    included, so it is not core at min_points = 4, where every point of A and B is."""
    spread = np.array([[0.004, 0, 0], [-0.004, 0, 0], [0, 0.004, 0], [0, -0.004, 0], [0, 0, 0.004], [0, 0, -0.004]])
    a, b = spread, spread * np.array([-1.0, 1.0, 1.0]) + np.array([0.107, 0.0, 0.0])
    border = np.array([[0.0535, 0.0, 0.0]])
    return np.concatenate([b, border, a] if swapped else [a, border, b])


@functools.lru_cache(maxsize=None)
def batch():
    """(rows [N, 3] float64, offsets [S + 1] int64, names [S], eps [S]); built once, never written."""
    rows, offsets, names = V.batch()
    rng = np.random.default_rng(2025)
    parts, out_names = [np.zeros((0, 3))], ["front-empty"]
    for s, name in enumerate(names):
        part = rows[offsets[s]:offsets[s + 1]]
        parts.append(part[:CUT.get(name, len(part))])
        out_names.append(name)
    step = 0.9 * DEFAULT_EPS / np.sqrt(3.0)
    chain = (np.arange(3000, dtype=np.float64) * step)[:, None].repeat(3, axis=1)
    bridge = _bridge(rng)
    dup = np.repeat(rng.random((300, 3)).astype(np.float32).astype(np.float64) * 0.5, 8, axis=0)
    noise = np.arange(40, dtype=np.float64)[:, None] * np.array([10.0, -10.0, 10.0])
    more = [("chain-3000", chain[rng.permutation(3000)]), ("bridge", bridge), ("dup8", dup[rng.permutation(len(dup))]),
            ("middle-empty", np.zeros((0, 3))), ("far", bridge + np.array([1234.5, -987.25, 55.125])),
            ("lattice-eighths", rng.integers(0, 8, size=(500, 3)) / 8.0), ("lattice-tenths", rng.integers(0, 8, size=(500, 3)) / 10.0),
            ("shared-border", _shared_border(False)), ("shared-border-swapped", _shared_border(True)), ("noise-only", noise),
            ("n=1", np.array([[0.25, -3.0, 1e3]])), ("end-empty", np.zeros((0, 3)))]
    for name, part in more:
        parts.append(part)
        out_names.append(name)
    off = np.zeros(len(parts) + 1, dtype=np.int64)
    np.cumsum([len(p) for p in parts], out=off[1:])
    out = np.ascontiguousarray(np.concatenate(parts), dtype=np.float64)
    assert len(out) < 25000
    eps = np.array([OWN_EPS.get(n, DEFAULT_EPS) for n in out_names])
    for a in (out, off, eps):
        a.setflags(write=False)
    return out, off, tuple(out_names), eps


def eps_values():
    """Every segment's own eps, plus 0.02 and 100."""
    return tuple(sorted(set(batch()[3].tolist()) | {0.02, 100.0}))


def small_batches():
    return V.small_batches()


@functools.lru_cache(maxsize=None)
def permuted():
    """The batch with every segment's rows permuted: (rows, offsets, permutation [N]) with rows = batch rows[permutation]."""
    rows, offsets, _names, _eps = batch()
    rng = np.random.default_rng(7)
    perm = np.concatenate([offsets[s] + rng.permutation(int(offsets[s + 1] - offsets[s])) for s in range(len(offsets) - 1)]).astype(np.int64)
    out = np.ascontiguousarray(rows[perm])
    out.setflags(write=False)
    return out, offsets, perm


def sklearn_labels(rows, offsets, eps, min_points):
    """(labels [N] int32, clusters [S] int64): scikit-learn's DBSCAN, kd_tree, per segment."""
    from sklearn.cluster import DBSCAN
    labels = np.full(len(rows), -1, dtype=np.int32)
    clusters = np.zeros(len(offsets) - 1, dtype=np.int64)
    for s in range(len(offsets) - 1):
        a, b = int(offsets[s]), int(offsets[s + 1])
        if b > a:
            got = DBSCAN(eps=eps, min_samples=min_points, algorithm="kd_tree").fit(np.asarray(rows[a:b, :3], dtype=np.float64)).labels_
            labels[a:b] = got
            clusters[s] = got.max() + 1
    return labels, clusters


@functools.lru_cache(maxsize=None)
def batch_sklearn(eps, min_points, shuffled=False):
    rows, offsets = (permuted() if shuffled else batch())[:2]
    return sklearn_labels(rows, offsets, eps, min_points)


@functools.lru_cache(maxsize=None)
def batch_twin(eps, min_points, shuffled=False):
    """The host twin on the batch: computed once, shared by the tests that need a reference."""
    from mspa import cloud_segments as CS
    rows, offsets = (permuted() if shuffled else batch())[:2]
    return CS.dbscan_segments_host(rows, offsets, eps, min_points)


def largest_keep(labels, offsets):
    """(keep [N] bool, kept [S] int64) from labels by the rule's text: np.bincount per segment, argmax (the FIRST maximum: a tie goes
    to the lowest number), nothing for a segment that is all noise."""
    keep = np.zeros(len(labels), dtype=bool)
    kept = np.zeros(len(offsets) - 1, dtype=np.int64)
    for s in range(len(offsets) - 1):
        a, b = int(offsets[s]), int(offsets[s + 1])
        seg = labels[a:b]
        if (seg >= 0).any():
            sizes = np.bincount(seg[seg >= 0])
            best = int(np.argmax(sizes))
            keep[a:b] = seg == best
            kept[s] = sizes[best]
    return keep, kept


def golden():
    """{(eps, min_points): labels [N] int32}: scikit-learn's labels for the batch, frozen by tools/gen_dbscan_golden.py."""
    with np.load(GOLDEN) as z:
        assert int(z["rows"]) == len(batch()[0]) and np.array_equal(z["offsets"], batch()[1])
        return {(float(e), int(m)): z[f"labels_{k}"] for k, (e, m) in enumerate(z["parameters"])}
