"""The batch, the independent references and the conditions the references satisfy ALONE, behind the neighbour and normal tests
(tests/test_cloud_normals_cpu.py, tests/test_gpu_cloud_normals.py, tests/test_gpu_cloud_normals_memory.py,
tools/gen_cloud_normals_golden.py).

``batch()`` is one seeded ragged batch; its segments, by name:

  empty, 1 row, 2 rows, 3 rows, 4 rows, 7 rows      fewer rows than K = 10 (``k > n``); the first three are FEW
  slab 63 / 64 / 65 / 257 / 1 025                   jittered unit slabs (thickness 2 cm): the wave and workgroup edges; class "near"
  lattice                                           the integer lattice plane z = 3 of 15 x 15: massive d2 ties, the exact-plane identity
  lattice twice                                     the same lattice with every row twice (coincident rows)
  line                                              20 collinear integer rows: DEGENERATE everywhere
  sphere in / sphere out                            a jittered unit sphere of 600 rows, the viewpoint at its centre / far outside
  far plane                                         a tilted jittered plane of 257 rows 10^6 m from the origin; class "far"
  1 cm / 100 m                                      a slab of extent 1 cm (64 rows) and one of 100 m (255 rows); classes "small", "large"

``viewpoints()`` gives the two spheres, the far plane and slab 257 a viewpoint and every other segment a NaN row (none).  ``CAP`` is
a max_distance that cuts some neighbourhoods below 3 (FEW) and some below K.  ``float32_rows()`` is the batch rounded to float32.

The references share no code with the library: a brute-force neighbour search over the full d2 matrix of a segment (the same
expression, ``np.lexsort((row, d2))``), and an mpmath oracle at 60 digits (centroid, centred moments and ``eigsy`` of the same
neighbour set).  What a test relies on is asserted HERE, on the references alone:

  * every row used in an accuracy class has a relative eigenvalue gap (l1 - l0) / (l2 - l0) >= 1e-3 in the oracle;
  * every oriented row has |(v - p) . n| >= 1e-9 |v - p| with the oracle's n, so no rounding can flip a sign;
  * every capped neighbourhood has no d2 within 1e-9 relative of cap2;
  * the slabs, the spheres and the planes have no two equal d2 in any row of their d2 matrix (the permutation test's condition)."""
import functools
import os
from fractions import Fraction

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cloud_normals.npz")
OK, FEW, DEGENERATE = 0, 1, 2
U = 2.0 ** -53
K = 10
CAP = 0.1
GAP = 1e-3
MARGIN = 1e-9
TIE_FREE = ("slab 63", "slab 64", "slab 65", "slab 257", "sphere in", "far plane", "1 cm", "100 m")
FIXTURE = ("empty", "1 row", "2 rows", "3 rows", "4 rows", "7 rows", "slab 63", "slab 64", "slab 65", "lattice", "line", "far plane", "1 cm")


def _offsets(parts):
    return np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def batch():
    """(xyz [N, 3] float64, offsets [S + 1], names): the batch above."""
    rng = np.random.default_rng(20261023)
    parts, names = [], []

    def add(name, rows):
        parts.append(np.asarray(rows, dtype=np.float64).reshape(-1, 3))
        names.append(name)

    def slab(n, extent=1.0):
        return (rng.random((n, 3)) - 0.5) * np.array([1.0, 1.0, 0.02]) * extent

    add("empty", np.zeros((0, 3)))
    for n in (1, 2, 3, 4, 7):
        add(f"{n} row" + ("s" if n > 1 else ""), slab(n))
    for n in (63, 64, 65, 257, 1025):
        add(f"slab {n}", slab(n))
    grid = np.array([(x, y, 3) for x in range(15) for y in range(15)], dtype=np.float64)
    add("lattice", grid)
    add("lattice twice", np.repeat(grid, 2, axis=0))
    add("line", np.array([(i, 2 * i, -i) for i in range(20)], dtype=np.float64))
    ball = rng.normal(size=(600, 3))
    ball = ball / np.linalg.norm(ball, axis=1, keepdims=True) * (1.0 + (rng.random((600, 1)) - 0.5) * 0.01)
    add("sphere in", ball)
    add("sphere out", ball + np.array([4.0, 0.0, 0.0]))
    e1, e2 = np.array([0.6, 0.0, 0.8]), np.array([0.0, 1.0, 0.0])
    uv = rng.random((257, 2)) - 0.5
    plane = uv[:, :1] * e1 + uv[:, 1:] * e2 + (rng.random((257, 1)) - 0.5) * 0.01 * np.cross(e1, e2)
    add("far plane", plane + np.array([1e6, -1e6, 1e6]))
    add("1 cm", slab(64, 0.01) + 0.5)
    add("100 m", slab(255, 100.0))
    xyz = np.ascontiguousarray(np.concatenate(parts))
    assert np.isfinite(xyz).all() and [len(p) for p in parts[:6]] == [0, 1, 2, 3, 4, 7]
    assert {63, 64, 65, 257, 1025} <= {len(p) for p in parts} and all(len(parts[names.index(n)]) < K for n in names[:6])
    return _frozen(xyz, _offsets(parts), tuple(names))


def segment(name):
    xyz, off, names = batch()
    s = names.index(name)
    return s, int(off[s]), int(off[s + 1])


@functools.lru_cache(maxsize=None)
def viewpoints():
    """[S, 3]: a viewpoint for the two spheres, the far plane and slab 257; a NaN row (none) everywhere else."""
    xyz, off, names = batch()
    v = np.full((len(names), 3), np.nan)
    v[names.index("sphere in")] = [0.0, 0.0, 0.0]
    v[names.index("sphere out")] = [50.0, 30.0, -20.0]
    v[names.index("far plane")] = [1e6 + 1.0, -1e6 - 2.0, 1e6 + 3.0]
    v[names.index("slab 257")] = [0.2, -0.1, 2.5]
    assert np.isnan(v[names.index("slab 1025")]).all()
    return _frozen(v)[0]


@functools.lru_cache(maxsize=None)
def float32_rows():
    return _frozen(batch()[0].astype(np.float32))[0]


def fixture_batch():
    """(xyz, offsets, viewpoints) of the ``FIXTURE`` segments alone: the batch behind tests/golden/cloud_normals.npz."""
    xyz, off, names = batch()
    at = [names.index(n) for n in FIXTURE]
    parts = [xyz[off[s]:off[s + 1]] for s in at]
    return np.ascontiguousarray(np.concatenate(parts)), _offsets(parts), np.ascontiguousarray(viewpoints()[at])


# ---- the brute force --------------------------------------------------------------------------------------------------------------

def d2_matrix(P):
    d = P[None] - P[:, None]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def brute_knn(xyz, offsets, k, cap=None):
    """(index [N, k] int64 global rows, -1 behind used; distance [N, k], +inf behind used; used [N] int32) by the full d2 matrix of
    every segment and ``np.lexsort((row, d2))``."""
    xyz = np.asarray(xyz, dtype=np.float64)
    N = len(xyz)
    index, distance, used = np.full((N, k), -1, dtype=np.int64), np.full((N, k), np.inf), np.zeros((N,), dtype=np.int32)
    cap2 = np.inf if cap is None else float(cap) * float(cap)
    for a, b in zip(offsets[:-1], offsets[1:]):
        if a == b:
            continue
        d2 = d2_matrix(xyz[a:b])
        rows = np.arange(b - a)
        for i in range(b - a):
            order = np.lexsort((rows, d2[i]))
            order = order[d2[i][order] <= cap2][:k]
            used[a + i] = len(order)
            index[a + i, :len(order)] = a + order
            distance[a + i, :len(order)] = np.sqrt(d2[i][order])
    return index, distance, used


@functools.lru_cache(maxsize=None)
def brute(cap=None, k=K):
    """``brute_knn`` of the batch, once, with the cap's condition asserted on the d2 alone."""
    xyz, off, _names = batch()
    out = brute_knn(xyz, off, k, cap)
    if cap is not None:
        cap2 = float(cap) * float(cap)
        for a, b in zip(off[:-1], off[1:]):
            if b > a:
                assert (np.abs(d2_matrix(xyz[a:b]) - cap2) > MARGIN * cap2).all()
        if k == K:
            assert ((out[2] < 3) & (out[2] > 0)).any() and ((out[2] >= 3) & (out[2] < k)).any() and (out[2] == k).any()
    return _frozen(*out)


@functools.lru_cache(maxsize=None)
def tie_free_checked():
    """The condition of the permutation test: no two equal d2 in any row of a ``TIE_FREE`` segment's d2 matrix."""
    xyz, _off, _names = batch()
    for name in TIE_FREE:
        _s, a, b = segment(name)
        d2 = np.sort(d2_matrix(xyz[a:b]), axis=1)
        assert (np.diff(d2, axis=1) > 0).all(), name
    return True


# ---- the oracle -------------------------------------------------------------------------------------------------------------------

def oracle_row(P):
    """The neighbours P [m, 3] (m >= 3) at 60 digits -> (normal [3] float64, unit, sign free; curvature; gap (l1 - l0) / (l2 - l0),
    0.0 where l2 == l0)."""
    import mpmath as mp
    with mp.workdps(60):
        m = len(P)
        rows = [[mp.mpf(float(v)) for v in row] for row in P]
        c = [mp.fsum(r[a] for r in rows) / m for a in range(3)]
        M = mp.matrix([[mp.fsum((r[a] - c[a]) * (r[b] - c[b]) for r in rows) for b in range(3)] for a in range(3)])
        E, V = mp.eigsy(M)
        order = sorted(range(3), key=lambda i: E[i])
        l0, l1, l2 = (E[i] for i in order)
        n = [V[i, order[0]] for i in range(3)]
        norm = mp.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
        total = l0 + l1 + l2
        return (np.array([float(v / norm) for v in n]), float(l0 / total) if total != 0 else 0.0,
                float((l1 - l0) / (l2 - l0)) if l2 != l0 else 0.0)


def eigh_row(P):
    """NumPy's answer for the same neighbours: (normal, curvature) from ``np.linalg.eigh`` of the float64 centred moments."""
    d = P - P.mean(0)
    w, v = np.linalg.eigh(d.T @ d)
    return v[:, 0], float(w[0] / ((w[0] + w[1]) + w[2])) if ((w[0] + w[1]) + w[2]) != 0 else 0.0


def angle(a, b):
    """The angle between the lines of two unit vectors (sign free): |a x b|, accurate where it is small."""
    return float(np.linalg.norm(np.cross(a, b)))


CLASSES = {"near": ("3 rows", "4 rows", "7 rows", "slab 63", "slab 64", "slab 65", "slab 257", "slab 1025"), "far": ("far plane",),
           "small": ("1 cm",), "large": ("100 m",), "sphere": ("sphere in", "sphere out"), "lattice": ("lattice", "lattice twice")}
STRIDE = {"slab 1025": 8, "sphere in": 4, "sphere out": 4, "lattice twice": 3}


@functools.lru_cache(maxsize=None)
def references():
    """{cls: tuple of (row, oracle normal, oracle curvature, eigh's angle to the oracle, eigh's curvature error)} over the sampled rows
    of every class whose oracle gap is at least ``GAP``; the neighbour sets are the brute force's at ``K`` without a cap."""
    xyz, _off, _names = batch()
    index, _distance, used = brute()
    out = {}
    for cls, members in CLASSES.items():
        rows = []
        for name in members:
            _s, a, b = segment(name)
            for i in range(a, b, STRIDE.get(name, 1)):
                if used[i] < 3:
                    continue
                P = xyz[index[i, :used[i]]]
                n, curv, gap = oracle_row(P)
                if gap < GAP:
                    continue
                n_np, curv_np = eigh_row(P)
                rows.append((i, n, curv, angle(n_np, n), abs(curv_np - curv)))
        assert len(rows) >= 3, cls
        assert all(oracle_row(xyz[index[i, :used[i]]])[2] >= GAP for i, *_ in rows[:2])
        out[cls] = tuple(rows)
    return out


def within_rule(err, yard):
    """The accuracy rule of tests/cloud_align_util.py: at most 8 x the yardstick, and at least one unit roundoff is allowed."""
    return err <= max(8.0 * yard, U)


@functools.lru_cache(maxsize=None)
def oriented_rows():
    """(row, v) of every sampled OK row whose segment has a viewpoint, with the margin asserted on the oracle's normal."""
    xyz, off, names = batch()
    v = viewpoints()
    out = []
    for cls in references().values():
        for i, n, *_ in cls:
            s = int(np.searchsorted(off, i, side="right") - 1)
            if np.isfinite(v[s]).all():
                w = v[s] - xyz[i]
                assert abs(float(w @ n)) >= MARGIN * float(np.linalg.norm(w)), (names[s], i)
                out.append((i, v[s]))
    assert len(out) >= 100
    return tuple(out)


def exact_dot(v, p, n):
    """(v - p) . n of doubles in exact rational arithmetic."""
    F = lambda x: Fraction(float(x))                                           # noqa: E731
    return sum((F(v[a]) - F(p[a])) * F(n[a]) for a in range(3))


def exact_unit_defect(n):
    """| |n|^2 - 1 | of a vector of doubles, in exact rational arithmetic, as a float."""
    return float(abs(sum(Fraction(float(x)) ** 2 for x in n) - 1))


# ---- point-to-plane: the ICP batch of tests/cloud_align_util.py with estimated normals -------------------------------------------------

PLANE_K = 30
PLANE_ITERATIONS = 12


@functools.lru_cache(maxsize=None)
def plane_batch():
    """(q, q_offsets, t, t_offsets, truth, normals [Nt, 3]): ``cloud_align_util.icp()`` (the L-shaped lattice; pair 0 is 1 degree and 5 mm
    at a cap of 5 cm) with the targets' normals from the host twin at k = 30, every one of them finite."""
    import cloud_align_util as A
    from mspa import cloud_segments as CS
    q, q_off, t, t_off, truth = A.icp()
    normals = CS.normals_segments_host(t, t_off, PLANE_K)["normal"]
    assert np.isfinite(normals).all()
    return _frozen(q, q_off, t, t_off) + (truth,) + _frozen(normals)


@functools.lru_cache(maxsize=None)
def numpy_plane_icp(pair, cap, iterations=PLANE_ITERATIONS):
    """A NumPy point-to-plane ICP of one pair of ``plane_batch()`` that shares no code with the library: brute-force search with ties to
    the lowest row, ``np.linalg.lstsq`` of the 6 unknowns, Rodrigues' matrix of the step composed onto the state -> a dict: ``index``
    [K, n] local rows or -1, ``R``, ``t``, and the smallest margins over all iterations (nearest against second nearest, matched
    distance against the cap), asserted to be at least ``MARGIN`` so that no rounding of a transform can change a correspondence."""
    import cloud_align_util as A
    q, q_off, t, t_off, _truth, normals = plane_batch()
    Q, T, N = q[q_off[pair]:q_off[pair + 1]], t[t_off[pair]:t_off[pair + 1]], normals[t_off[pair]:t_off[pair + 1]]
    R, tr = np.eye(3), np.zeros(3)
    history, m_second, m_cap = [], np.inf, np.inf
    for _ in range(iterations):
        Y = Q @ R.T + tr
        at, d2, second = A.brute_two(Y, T)
        inside = d2 <= cap * cap
        m_second = min(m_second, float((np.sqrt(second) - np.sqrt(d2)).min()))
        m_cap = min(m_cap, float(np.abs(np.sqrt(d2) - cap).min()))
        history.append(np.where(inside, at, -1))
        y, p, n = Y[inside], T[at[inside]], N[at[inside]]
        c = y.mean(0)
        J = np.concatenate([np.cross(y - c, n), n], axis=1)
        x = np.linalg.lstsq(J, -np.einsum("ij,ij->i", y - p, n), rcond=None)[0]
        angle_ = float(np.linalg.norm(x[:3]))
        Rs = A.rotation(x[:3], angle_) if angle_ > 0 else np.eye(3)
        R, tr = Rs @ R, Rs @ (tr - c) + c + x[3:]
    assert m_second >= MARGIN and m_cap >= MARGIN, (pair, m_second, m_cap)
    return {"index": np.array(history), "R": R, "t": tr}


def flat_case():
    """(q, t, normals): a flat target -- the integer lattice plane with the normal (0, 0, 1) everywhere -- and queries a little off it:
    the slides along the plane and the spin about its normal are unconstrained."""
    _s, a, b = segment("lattice")
    t = batch()[0][a:b].copy()
    return t[:100] + np.array([0.01, -0.02, 0.03]), t, np.tile([0.0, 0.0, 1.0], (len(t), 1))


def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}
