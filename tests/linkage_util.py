"""Shared by test_linkage_cpu.py and test_gpu_linkage.py: seeded loss matrices of the kinds that exercise the tie rules, and
SciPy's answer for each (computed once per matrix and threshold, then only read)."""
import functools

import numpy as np

KINDS = ("continuous", "half_zero", "grid10")
NONFINITE_TEXT = "The condensed distance matrix must contain only finite values."


def matrix(kind, n, seed):
    """Symmetric [n, n] float64 with a zero diagonal: continuous values, about half the entries exactly 0.0, or values on a grid
    of ten (ties everywhere)."""
    rng = np.random.default_rng([seed, n, KINDS.index(kind)])
    if kind == "continuous":
        a = rng.random((n, n)) * 0.4
    elif kind == "half_zero":
        a = rng.random((n, n)) * 0.4 * (rng.random((n, n)) < 0.5)
    else:
        a = rng.integers(0, 10, (n, n)) / 10.0
    a = np.triu(a, 1)
    return np.ascontiguousarray(a + a.T)


def on_threshold():
    """Two pairs (heights 0.03 and 0.04) whose cross distances are all 0.1: the last merge is (2 * 0.1 + 2 * 0.1) / 4, exactly
    0.1, so fcluster(0.1) must put all four in one cluster (maximum <= threshold)."""
    m = np.full((4, 4), 0.1)
    m[0, 1] = m[1, 0] = 0.03
    m[2, 3] = m[3, 2] = 0.04
    np.fill_diagonal(m, 0.0)
    return m


def duplicate_rows(n=9, seed=3):
    """Points 2 and 5 are at distance 0 and have identical rows otherwise."""
    m = matrix("continuous", n, seed)
    m[5, :] = m[2, :]
    m[:, 5] = m[:, 2]
    m[2, 5] = m[5, 2] = 0.0
    np.fill_diagonal(m, 0.0)
    assert np.array_equal(m, m.T)
    return m


@functools.lru_cache(maxsize=None)
def _scipy_cached(key, threshold):
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.spatial.distance import squareform
    m = _MATRICES[key]
    Z = linkage(squareform(m, checks=False), method="average")
    labels = fcluster(Z, threshold, criterion="distance").astype(np.int32)
    Z.setflags(write=False)
    labels.setflags(write=False)
    return Z, labels


_MATRICES = {}


def scipy_answer(m, threshold):
    """(Z, labels) of SciPy for one matrix; cached on the matrix's bytes."""
    key = (m.shape[0], m.tobytes())
    _MATRICES.setdefault(key, m)
    return _scipy_cached(key, float(threshold))


def thresholds(m):
    """0.1 (the reference's) and, where there is one, a height of the tree itself (a node exactly on the threshold)."""
    Z, _ = scipy_answer(m, 0.1)
    out = [0.1]
    mid = float(Z[(Z.shape[0] - 1) // 2, 2])
    if mid != 0.1:
        out.append(mid)
    return out


def groups_of(labels):
    """The reference's list of index lists (OM_C:91-92)."""
    return [np.where(labels == i)[0].tolist() for i in range(1, int(max(labels)) + 1)]
