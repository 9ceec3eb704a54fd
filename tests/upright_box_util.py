"""The ragged batch shared by test_upright_box_cpu.py, test_gpu_upright_segments.py and test_gpu_upright_segments_memory.py, the
exact oracle (Python integers and ``fractions.Fraction``; nothing of the library's) and the frozen results of tests/golden.

The batch, under 40 000 rows of [x, y, z] float64.  Every segment is there for a reason:
  * front-empty, middle-empty, end-empty   no rows: h = 0, a NaN box;
  * n=1; two-identical (h = 1); two-distinct (h = 2);
  * tiny-a, tiny-b, tiny-c                 3, 2 and 4 rows back to back: three segments inside one wave;
  * collinear-axis, collinear-diagonal     300 points on y = 2 and on y = x, shuffled: h = 2, width 0;
  * collinear-slope                        300 points (x, fl(0.37 x + 0.11)): NOT exactly collinear, the exact hull has a few vertices;
  * kettner                                the 64 x 64 grid (0.5 + i 2^-53, 0.5 + j 2^-53) with (12, 12) and (24, 24): the plain float64
                                           orientation test gets the sign wrong for 2 164 of these points against that line;
  * lattice-eighths, lattice-dup8          the 9 x 9 lattice k / 8 (its hull is its 4 corners), and the same with every point 8 times;
  * rect30-near, rect30-far                a 2.0 x 0.8 rectangle turned by 30 degrees about (4, 5) and about (1000, -2000): 5 000 uniform
                                           rows inside, then its four corners;
  * square45                               the square (1, 0), (0, 1), (-1, 0), (0, -1) with 200 rows inside: four edges that tie;
  * circle-512                             512 points on the unit circle and 2 000 inside: h = 512, two edge tiles;
  * circle-5000                            5 000 points on a circle: no filter can discard one, the survivors exceed one compaction tile
                                           of 2 048, the chains are long;
  * gauss-10000                            10 000 Gaussian rows: three extents tiles;
  * ellipse-thin                           1 000 points on an ellipse of aspect 10^-6.
``float32_segment()`` is gauss-10000's first 3 000 rows as float32 with C = 6.

THE ORACLE.  A segment's doubles are scaled to integers by a common power of two (``exact_points``).  The hull is Andrew's monotone
chain on the exact integer sign of the determinant, over the distinct points in lexicographic order, each the lowest row that holds
it (``exact_hull``).  ``exact_measures`` gives every edge's m_k as a ``Fraction``: the extremes of t and c over the hull are taken
exactly over the CANDIDATES a float64 evaluation leaves -- every vertex whose float value lies within 2^-30 (relative to |q| |d|)
of the float extreme, which is 10^6 times the float evaluation's error, so the exact extreme is always among them."""
import functools
import os
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "upright_boxes.npz")
U = 2.0 ** -53
RECT_BOUND = 64 * U                               # csrc/upright_box_core.h: rect_bound over R^2, R the diagonal of the hull's bounding box
RECT = (2.0, 0.8, 30.0)
RECT_CENTRES = {"rect30-near": (4.0, 5.0), "rect30-far": (1000.0, -2000.0)}
QHULL_UNAMBIGUOUS = ("lattice-eighths", "lattice-dup8", "rect30-near", "rect30-far", "gauss-10000", "circle-512", "circle-5000")
MEMORY_CUT = ("front-empty", "n=1", "tiny-a", "tiny-b", "tiny-c", "middle-empty", "kettner", "lattice-dup8", "circle-5000", "end-empty")


def _turned(local, centre, degrees):
    a = np.deg2rad(degrees)
    c, s = np.cos(a), np.sin(a)
    return np.stack([centre[0] + (local[:, 0] * c - local[:, 1] * s), centre[1] + (local[:, 0] * s + local[:, 1] * c)], axis=1)


def _with_z(xy, rng):
    return np.concatenate([xy, rng.normal(0.0, 0.3, size=(len(xy), 1))], axis=1)


@functools.lru_cache(maxsize=None)
def batch():
    """(rows [N, 3] float64, offsets [S + 1] int64, names [S]); built once, never written."""
    rng = np.random.default_rng(20260)
    length, width, angle = RECT
    inside = (rng.random((5000, 2)) - 0.5) * np.array([length, width]) * 0.999
    corners = np.array([[1.0, 0.4], [-1.0, 0.4], [-1.0, -0.4], [1.0, -0.4]])
    x = rng.random(300) * 10.0 - 3.0
    theta512, theta5000 = np.arange(512) * (2 * np.pi / 512), rng.permutation(5000) * (2 * np.pi / 5000)
    r, phi = 0.99 * np.sqrt(rng.random(2000)), rng.random(2000) * 2 * np.pi
    grid = np.array([(0.5 + i * 2.0 ** -53, 0.5 + j * 2.0 ** -53) for i in range(64) for j in range(64)] + [(12.0, 12.0), (24.0, 24.0)])
    lattice = np.array([(i / 8.0, j / 8.0) for i in range(9) for j in range(9)])
    theta = rng.random(1000) * 2 * np.pi
    square_in = (rng.random((200, 2)) - 0.5) * 0.9
    parts = [
        ("front-empty", np.zeros((0, 2))), ("n=1", np.array([[0.25, -3.0]])), ("two-identical", np.array([[1.5, 2.5], [1.5, 2.5]])),
        ("two-distinct", np.array([[3.0, 1.0], [-1.0, 2.0]])),
        ("tiny-a", np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])), ("tiny-b", np.array([[5.0, 5.0], [4.0, 7.0]])),
        ("tiny-c", np.array([[1.0, 1.0], [0.0, 0.0], [2.0, 2.0], [1.0, 3.0]])), ("middle-empty", np.zeros((0, 2))),
        ("collinear-axis", np.stack([x, np.full(300, 2.0)], axis=1)), ("collinear-diagonal", np.stack([x, x], axis=1)[rng.permutation(300)]),
        ("collinear-slope", np.stack([x, 0.37 * x + 0.11], axis=1)[rng.permutation(300)]),
        ("kettner", grid[rng.permutation(len(grid))]), ("lattice-eighths", lattice[rng.permutation(81)]),
        ("lattice-dup8", np.repeat(lattice, 8, axis=0)[rng.permutation(648)]),
        ("rect30-near", np.concatenate([_turned(inside, RECT_CENTRES["rect30-near"], angle), _turned(corners, RECT_CENTRES["rect30-near"], angle)])),
        ("rect30-far", np.concatenate([_turned(inside, RECT_CENTRES["rect30-far"], angle), _turned(corners, RECT_CENTRES["rect30-far"], angle)])),
        ("square45", np.concatenate([square_in, np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0]])])),
        ("circle-512", np.concatenate([np.stack([r * np.cos(phi), r * np.sin(phi)], axis=1), np.stack([np.cos(theta512), np.sin(theta512)], axis=1)])),
        ("circle-5000", np.stack([3.0 + 2.0 * np.cos(theta5000), -1.0 + 2.0 * np.sin(theta5000)], axis=1)),
        ("gauss-10000", rng.normal(0.0, 1.0, size=(10000, 2)) * np.array([1.5, 0.5]) + np.array([-7.0, 2.0])),
        ("ellipse-thin", np.stack([np.cos(theta), 1e-6 * np.sin(theta)], axis=1)), ("end-empty", np.zeros((0, 2)))]
    rows = np.ascontiguousarray(np.concatenate([_with_z(p, rng) for _n, p in parts]), dtype=np.float64)
    off = np.zeros(len(parts) + 1, dtype=np.int64)
    np.cumsum([len(p) for _n, p in parts], out=off[1:])
    assert len(rows) < 40000
    rows.setflags(write=False)
    off.setflags(write=False)
    return rows, off, tuple(n for n, _p in parts)


def segment(name):
    rows, off, names = batch()
    s = names.index(name)
    return rows[off[s]:off[s + 1]]


@functools.lru_cache(maxsize=None)
def permuted():
    """The batch with every segment's rows permuted: (rows, offsets, permutation [N]) with rows = batch rows[permutation]."""
    rows, off, _names = batch()
    rng = np.random.default_rng(11)
    perm = np.concatenate([off[s] + rng.permutation(int(off[s + 1] - off[s])) for s in range(len(off) - 1)] + [np.zeros(0, dtype=np.int64)])
    out = np.ascontiguousarray(rows[perm.astype(np.int64)])
    out.setflags(write=False)
    return out, off, perm.astype(np.int64)


@functools.lru_cache(maxsize=None)
def memory_batch():
    """The cut of the batch the memory and stream tests run: it keeps the empty segments, the circle, the Kettner grid and the
    lattice with duplicates."""
    rows, off, names = batch()
    parts = [rows[off[names.index(n)]:off[names.index(n) + 1]] for n in MEMORY_CUT]
    cut = np.zeros(len(parts) + 1, dtype=np.int64)
    np.cumsum([len(p) for p in parts], out=cut[1:])
    return np.ascontiguousarray(np.concatenate(parts)), cut


def float32_segment():
    """(rows [3000, 6] float32, offsets): gauss-10000's first rows with three colour columns."""
    rng = np.random.default_rng(5)
    xyz = segment("gauss-10000")[:3000].astype(np.float32)
    return np.ascontiguousarray(np.concatenate([xyz, rng.random((3000, 3)).astype(np.float32)], axis=1)), np.array([0, 3000], dtype=np.int64)


def small_batches():
    one = segment("gauss-10000")[:50]
    return {"S=1": (one, np.array([0, 50], dtype=np.int64)), "N=0": (np.zeros((0, 3)), np.array([0], dtype=np.int64)),
            "all-empty": (np.zeros((0, 3)), np.zeros(4, dtype=np.int64))}


# ---- the exact oracle -----------------------------------------------------------------------------------------------------------

def exact_points(xy):
    """[n, 2] float64 -> (X, Y lists of Python integers, e) with x = X / 2^e exactly for every point."""
    xy = np.asarray(xy, dtype=np.float64)
    mant, exp = np.frexp(xy)                       # x = mant * 2^exp, |mant| in [0.5, 1)
    whole = (mant * 2.0 ** 53).astype(np.int64)     # exact: 53 bits
    exp = exp.astype(np.int64) - 53
    low = int(exp[whole != 0].min()) if (whole != 0).any() else 0
    ints = [[int(w) << int(e - low) if w else 0 for w, e in zip(whole[:, c], exp[:, c])] for c in range(2)]
    return ints[0], ints[1], -low


def _cross(X, Y, a, b, c):
    return (X[b] - X[a]) * (Y[c] - Y[a]) - (Y[b] - Y[a]) * (X[c] - X[a])


def exact_hull(xy):
    """The rule's hull of [n, 2] float64 by exact integer arithmetic: row indices, counter-clockwise from the lexicographically
    smallest vertex, every vertex the lowest row that holds it."""
    xy = np.asarray(xy, dtype=np.float64)
    n = len(xy)
    if n == 0:
        return []
    X, Y, _e = exact_points(xy)
    order = np.lexsort((xy[:, 1], xy[:, 0]))        # stable: equal points in ascending row order
    distinct = [int(order[0])]
    for i in order[1:]:
        if xy[i, 0] != xy[distinct[-1], 0] or xy[i, 1] != xy[distinct[-1], 1]:
            distinct.append(int(i))
    if len(distinct) == 1:
        return distinct

    def half(points):
        out = []
        for p in points:
            while len(out) >= 2 and _cross(X, Y, out[-2], out[-1], p) <= 0:
                out.pop()
            out.append(p)
        return out
    lower, upper = half(distinct), half(distinct[::-1])
    return lower[:-1] + upper[:-1]


def exact_measures(xy, hull):
    """(m [h] Fractions, R^2 Fraction): every hull edge's exact m_k (h >= 2) and the squared diagonal of the hull's bounding box."""
    pts = np.asarray(xy, dtype=np.float64)[hull]
    X, Y, e = exact_points(pts)
    h = len(hull)
    scale = Fraction(1, 1 << (2 * e)) if e >= 0 else Fraction(1 << (-2 * e), 1)
    out = []
    for k in range(h):
        k1 = (k + 1) % h
        d = pts[k1] - pts[k]
        q = pts - pts[k]
        size = np.abs(q).sum(axis=1).max() * np.abs(d).sum() * 2.0 ** -30
        dX, dY = X[k1] - X[k], Y[k1] - Y[k]
        spans = []
        for value, exact in ((q[:, 0] * d[0] + q[:, 1] * d[1], lambda j: (X[j] - X[k]) * dX + (Y[j] - Y[k]) * dY),
                             (q[:, 1] * d[0] - q[:, 0] * d[1], lambda j: (Y[j] - Y[k]) * dX - (X[j] - X[k]) * dY)):
            top = max(exact(int(j)) for j in np.nonzero(value >= value.max() - size)[0])
            bottom = min(exact(int(j)) for j in np.nonzero(value <= value.min() + size)[0])
            spans.append(top - bottom)
        out.append(Fraction(spans[0] * spans[1], dX * dX + dY * dY) * scale)
    diagonal_sq = Fraction((max(X) - min(X)) ** 2 + (max(Y) - min(Y)) ** 2) * scale
    return out, diagonal_sq


@functools.lru_cache(maxsize=None)
def batch_oracle(shuffled=False):
    """Per segment of the batch (or of its permutation) the exact hull as row indices INTO THE BATCH: a tuple of lists."""
    rows, off = (permuted() if shuffled else batch())[:2]
    return tuple([int(off[s]) + k for k in exact_hull(rows[off[s]:off[s + 1], :2])] for s in range(len(off) - 1))


@functools.lru_cache(maxsize=None)
def batch_measures():
    """Per segment of the batch (m_k list, R^2), or None where the hull has fewer than two vertices."""
    rows, _off, _names = batch()
    return tuple(exact_measures(rows[:, :2], hull) if len(hull) >= 2 else None for hull in batch_oracle())


@functools.lru_cache(maxsize=None)
def batch_twin(shuffled=False):
    """The host twin on the batch: (boxes, hull index, hull offsets, edges); computed once, shared by the tests that need it."""
    from mspa import cloud_segments as CS
    rows, off = (permuted() if shuffled else batch())[:2]
    return CS.upright_boxes_segments_host(rows, off, want_hull=True, want_edges=True)


def golden():
    """The frozen results of the twin on the batch (tools/gen_upright_golden.py): a dict of arrays."""
    with np.load(GOLDEN) as z:
        assert int(z["rows"]) == len(batch()[0]) and np.array_equal(z["offsets"], batch()[1])
        return {k: z[k] for k in ("boxes", "hull_index", "hull_offsets", "edges")}
