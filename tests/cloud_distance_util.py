"""The batch, the oracle and the restated sums behind the nearest-point distance tests (tests/test_cloud_distance_cpu.py,
tests/test_gpu_cloud_distance.py, tests/test_gpu_cloud_distance_memory.py, tools/gen_cloud_distance_golden.py).

``batch()`` is seeded and holds 13 target segments and 13 query segments, about 9 k rows in all:

  targets   0 empty; 1 one row; 2 two rows; 3 / 4 / 5 a uniform cube of 63 / 64 / 65 rows; 6 a plane of 257 rows (a 2-D grid); 7 a
            uniform cube of 3 000 rows; 8 a line of 300 rows; 9 200 identical rows (one cell); 10 200 rows, every row twice (ties
            must give the lower index); 11 1 000 rows of which 1 % lie far away (the order-statistics box is much smaller than the
            extent); 12 a cube of 500 rows at offset 10^6.
  queries   segment s is made for target s: up to 20 of the target's own rows (distance exactly 0.0), 40 rows inside its box, a row
            outside the box on each of its six sides, two rows 100 extents away; segment 7 has 600 rows inside the box instead of 40;
            segment 4 is EMPTY; segments 3 and 11 end with a NaN row and an inf row.
  pairs     the identity (s, s) for every s, then (3, 4) and (5, 4), (7, 7) a second time, (7, 11), (11, 7), (12, 7) (every query
            some 10^6 away), (7, 0) (an empty target) and (4, 7) (an empty query segment): segments 4, 7 and 11 stand on both sides
            of several pairs.

The oracle is NumPy brute force per pair and shares no code with the library."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cloud_distance.npz")
EXTRA_PAIRS = [(3, 4), (5, 4), (7, 7), (7, 11), (11, 7), (12, 7), (7, 0), (4, 7)]
TAU = 0.05


def _targets(rng):
    cube = lambda n: rng.random((n, 3))                                      # noqa: E731
    plane = cube(257) * [2.0, 1.0, 0.0] + [0.0, 0.0, 0.25]
    line = np.outer(rng.random(300), [1.0, 2.0, -0.5]) + [0.3, 0.1, 0.9]
    same = np.tile([[0.25, -1.5, 3.0]], (200, 1))
    half = cube(100) * 0.5
    twice = np.concatenate([half, half])
    spread = cube(1000) * 0.3
    spread[rng.choice(1000, 10, replace=False)] += rng.normal(size=(10, 3)) * 40.0
    return [np.zeros((0, 3)), cube(1), cube(2), cube(63), cube(64), cube(65), plane, cube(3000), line, same, twice, spread, cube(500) + 1e6]


def _queries(rng, s, t):
    if s == 4:
        return np.zeros((0, 3))
    if len(t) == 0:
        return rng.random((5, 3))
    lo, hi = t.min(axis=0), t.max(axis=0)
    ext = np.maximum(hi - lo, 0.5)
    parts = [t[rng.choice(len(t), min(len(t), 20), replace=False)], lo + rng.random((600 if s == 7 else 40, 3)) * (hi - lo)]
    for ax in range(3):
        for sign in (-1.0, 1.0):
            q = lo + rng.random(3) * (hi - lo)
            q[ax] = (lo[ax] - 1.5 * ext[ax]) if sign < 0 else (hi[ax] + 1.5 * ext[ax])
            parts.append(q[None])
    parts.append(lo + 100.0 * ext * np.array([[1.0, -1.0, 0.5], [-1.0, 0.25, 1.0]]))
    if s in (3, 11):
        parts.append(np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5]]))
    return np.concatenate(parts)


@functools.lru_cache(maxsize=None)
def batch():
    """(t_xyz [Nt, 3], t_offsets [14], q_xyz [Nq, 3], q_offsets [14], pairs [21, 2]) -- read-only float64 / int64 arrays."""
    rng = np.random.default_rng(20260928)
    targets = _targets(rng)
    queries = [_queries(rng, s, t) for s, t in enumerate(targets)]
    offsets = lambda parts: np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)     # noqa: E731
    pairs = np.array([(s, s) for s in range(len(targets))] + EXTRA_PAIRS, dtype=np.int64)
    out = (np.ascontiguousarray(np.concatenate(targets)), offsets(targets), np.ascontiguousarray(np.concatenate(queries)), offsets(queries), pairs)
    for a in out:
        a.setflags(write=False)
    return out


def brute(Q, T):
    """The issue's five lines: (distance [n], index [n], d2 min [n]) of the rows Q against the rows T, len(T) >= 1."""
    d = T[None] - Q[:, None]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    with np.errstate(invalid="ignore"):
        return np.sqrt(d2.min(1)), d2.argmin(1), d2.min(1)


def oracle(t_xyz, t_off, q_xyz, q_off, pairs, max_distance=None):
    """(distance [M], index [M] global, offsets [P + 1]) by brute force per pair; the cap masks it."""
    St = len(t_off) - 1
    if pairs is None:
        pairs = np.array([(s, s) for s in range(St)], dtype=np.int64).reshape(-1, 2)
    dist, index, offsets = [], [], [0]
    for qs, ts in np.asarray(pairs).reshape(-1, 2):
        Q, T = q_xyz[q_off[qs]:q_off[qs + 1]], t_xyz[t_off[ts]:t_off[ts + 1]]
        if len(T) == 0:
            d, i = np.full((len(Q),), np.inf), np.full((len(Q),), -1, dtype=np.int64)
        else:
            d, i, d2 = brute(Q, T)
            i = i.astype(np.int64) + t_off[ts]
            if max_distance is not None:
                cap2 = np.float64(max_distance) * np.float64(max_distance)
                d, i = np.where(d2 > cap2, np.inf, d), np.where(d2 > cap2, -1, i)
        bad = ~np.isfinite(Q).all(axis=1)
        d, i = np.where(bad, np.nan, d), np.where(bad, -1, i)
        dist.append(d)
        index.append(i)
        offsets.append(offsets[-1] + len(Q))
    cat = lambda parts, dtype: np.concatenate(parts).astype(dtype) if parts else np.zeros((0,), dtype=dtype)      # noqa: E731
    return cat(dist, np.float64), cat(index, np.int64), np.array(offsets, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def batch_oracle():
    """The oracle of the whole batch with its pair table, computed once."""
    out = oracle(*batch())
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def batch_twin():
    """The host twin of the whole batch with its pair table (and evals), computed once."""
    from mspa import cloud_segments as CS
    t, t_off, q, q_off, pairs = batch()
    out = CS.nearest_segments_host(q, q_off, t, t_off, pairs, want_evals=True)
    out["fit"] = CS.fit_segments_host(out["distance"], out["offsets"], TAU)
    return out


def ordered_sum(terms):
    """segs::ordered_sum restated: 256 lane sums (lane j adds terms j, j + 256, ... in ascending order from 0.0), folded by strides
    128, 64, ..., 1."""
    terms = np.asarray(terms, dtype=np.float64)
    padded = np.zeros(((len(terms) + 255) // 256 * 256 + 256,), dtype=np.float64)      # + 0.0 changes no non-negative partial
    padded[:len(terms)] = terms
    partial = np.cumsum(padded.reshape(-1, 256), axis=0)[-1].copy()                     # cumsum adds one after the other
    t = 128
    while t >= 1:
        partial[:t] += partial[t:2 * t]
        t //= 2
    return partial[0]


def fit_oracle(distance, offsets, tau):
    """The six per-pair summaries restated in NumPy."""
    out = {k: [] for k in ("rows", "finite", "within", "sum", "sum_sq", "max")}
    for a, b in zip(offsets[:-1], offsets[1:]):
        d = distance[a:b]
        fin = d < np.inf
        out["rows"].append(b - a)
        out["finite"].append(int(fin.sum()))
        with np.errstate(invalid="ignore"):
            out["within"].append(int((d <= tau).sum()))
        out["sum"].append(ordered_sum(np.where(fin, d, 0.0)))
        out["sum_sq"].append(ordered_sum(np.where(fin, d * d, 0.0)))
        out["max"].append(np.max(d[fin]) if fin.any() else -np.inf)
    return {k: np.array(v, dtype=np.int64 if k in ("rows", "finite", "within") else np.float64) for k, v in out.items()}


def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}
