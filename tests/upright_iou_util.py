"""The batch of box pairs shared by test_upright_iou_cpu.py, test_gpu_upright_iou.py and test_gpu_upright_iou_memory.py, the exact
oracle (``fractions.Fraction``; nothing of the library's) and the frozen results of tests/golden.

The batch: pairs (a [P, 8], b [P, 8]) of upright boxes ``[cx, cy, cz, length, width, height, ux, uy]``, under 3 000 of them.  The named
pairs in front are each there for a reason:
  * identical, identical-turned          the same eight values twice: exactly 1.0;
  * disjoint-xy, disjoint-z              a clear gap in the plane, and in z only: exactly 0.0;
  * touch-edge, touch-corner             footprints that share an edge, and a corner: the exact area is 0;
  * inside                               a small turned box inside a large one: the small one's volume over the large one's;
  * octagon                              a unit square at 45 degrees in a unit square: the area is 2 (sqrt 2 - 1);
  * rect30                               the 2.0 x 0.8 rectangle at 30 degrees against its own axis-aligned box;
  * crossed-90, crossed-1                two 10 x 0.01 boxes crossed at 90 degrees and at 1 degree;
  * aspect-1e-6                          boxes of aspect 10^-6, crossed at 20 degrees;
  * zero-width, zero-height              one box without width, without height: 0.0;
  * both-degenerate                      two boxes of volume 0: NaN (0 / 0);
  * near, far                            a pair near the origin, and the same pair with 10^6 added to both centres;
  * axes-10-01                           the axes (1, 0) against (0, 1);
  * all-nan, infinite, negative-size, axis-1.01    refused: NaN.
Behind them ``N_AABB`` random axis-aligned pairs (built from 6-column boxes, ``aabb_pairs``) and ``N_RANDOM`` seeded random pairs, half
of them near each other and half apart.

THE ORACLE (``exact_pair``).  Each box's four corners c +- (length / 2) u +- (width / 2) n, n = (-uy, ux), as exact rationals from its
eight doubles; the second quadrilateral clipped against the four half-planes of the first by Sutherland-Hodgman in rationals (inside:
cross product >= 0); the shoelace area; the exact z overlap; the exact volumes length * width * (ux^2 + uy^2) * height; the exact IoU, or
None where the union's volume is 0.  ``refused_exact`` restates the refusals on the exact values."""
import functools
import os
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "upright_iou.npz")
N_AABB, N_RANDOM, N_MATRIX = 200, 2000, 70
REFUSED = ("all-nan", "infinite", "negative-size", "axis-1.01")
ZERO_EXACTLY = ("disjoint-xy", "disjoint-z")


def _box(cx, cy, cz, length, width, height, degrees=0.0):
    a = np.deg2rad(degrees)
    return [cx, cy, cz, length, width, height, float(np.cos(a)), float(np.sin(a))]


def aabb_to_upright(boxes6):
    """The NumPy restatement of ``mspa.cloud_segments.upright_of_aabb``."""
    boxes6 = np.asarray(boxes6, dtype=np.float64)
    dx, dy = boxes6[..., 3], boxes6[..., 4]
    turned = dy > dx
    out = np.stack([boxes6[..., 0], boxes6[..., 1], boxes6[..., 2], np.maximum(dx, dy), np.minimum(dx, dy), boxes6[..., 5],
                    np.where(turned, 0.0, 1.0), np.where(turned, 1.0, 0.0)], axis=-1)
    out[np.isnan(boxes6).any(axis=-1)] = np.nan
    return out


@functools.lru_cache(maxsize=None)
def aabb_pairs():
    """(boxes6 a [N_AABB, 6], boxes6 b [N_AABB, 6]): random axis-aligned pairs, most of them overlapping."""
    rng = np.random.default_rng(20271)
    a = np.concatenate([rng.uniform(-1, 1, (N_AABB, 3)), rng.uniform(0.2, 2.5, (N_AABB, 3))], axis=1)
    b = np.concatenate([a[:, :3] + rng.uniform(-1.2, 1.2, (N_AABB, 3)), rng.uniform(0.2, 2.5, (N_AABB, 3))], axis=1)
    return a, b


@functools.lru_cache(maxsize=None)
def batch():
    """(a [P, 8], b [P, 8], names [P]); built once, never written."""
    rect = _box(4.0, 5.0, 0.3, 2.0, 0.8, 1.1, 30.0)
    c30, s30 = np.cos(np.deg2rad(30.0)), np.sin(np.deg2rad(30.0))
    rect_aabb = aabb_to_upright([4.0, 5.0, 0.3, 2.0 * c30 + 0.8 * s30, 2.0 * s30 + 0.8 * c30, 1.1])
    near_a, near_b = _box(0.25, -0.5, 0.1, 1.5, 0.7, 0.9, 17.0), _box(0.5, -0.25, 0.3, 1.2, 0.9, 1.0, 63.0)
    shift = np.array([1e6, 1e6, 1e6, 0, 0, 0, 0, 0])
    nan = [np.nan] * 8
    named = [
        ("identical", _box(1, 2, 3, 2, 1, 1.5), _box(1, 2, 3, 2, 1, 1.5)),
        ("identical-turned", _box(-1, 0.5, 0, 3, 0.25, 2, 37.0), _box(-1, 0.5, 0, 3, 0.25, 2, 37.0)),
        ("disjoint-xy", _box(0, 0, 0, 2, 1, 1, 10.0), _box(5, 0.5, 0, 2, 1, 1, 70.0)),
        ("disjoint-z", _box(0, 0, 0, 2, 1, 1, 10.0), _box(0.25, 0, 3, 2, 1, 1, 40.0)),
        ("touch-edge", _box(0, 0, 0, 2, 1, 1), _box(2, 0, 0, 2, 1, 1)),
        ("touch-corner", _box(0, 0, 0, 2, 1, 1), _box(2, 1, 0, 2, 1, 1)),
        ("inside", _box(0, 0, 0, 4, 3, 2, 5.0), _box(0.25, -0.125, 0.25, 1, 0.5, 1, 50.0)),
        ("octagon", _box(0, 0, 0, 1, 1, 1), _box(0, 0, 0, 1, 1, 1, 45.0)),
        ("rect30", rect, list(rect_aabb)),
        ("crossed-90", _box(0, 0, 0, 10, 0.01, 1), _box(0.5, 0.25, 0, 10, 0.01, 1, 90.0)),
        ("crossed-1", _box(0, 0, 0, 10, 0.01, 1), _box(0.5, 0.001, 0, 10, 0.01, 1, 1.0)),
        ("aspect-1e-6", _box(0, 0, 0, 1, 1e-6, 1, 3.0), _box(0.01, 0, 0.5, 1, 1e-6, 1, 23.0)),
        ("zero-width", _box(0, 0, 0, 2, 0, 1, 15.0), _box(0.25, 0, 0, 2, 1, 1, 40.0)),
        ("zero-height", _box(0, 0, 0, 2, 1, 0, 15.0), _box(0.25, 0, 0, 2, 1, 1, 40.0)),
        ("both-degenerate", _box(0, 0, 0, 2, 0, 1, 15.0), _box(0.25, 0, 0, 2, 1, 0, 40.0)),
        ("near", near_a, near_b),
        ("far", list(np.array(near_a) + shift), list(np.array(near_b) + shift)),
        ("axes-10-01", [0, 0, 0, 2, 1, 1, 1.0, 0.0], [0.25, 0.125, 0.5, 2, 1, 1, 0.0, 1.0]),
        ("all-nan", nan, _box(0, 0, 0, 1, 1, 1)),
        ("infinite", _box(0, 0, 0, 1, 1, 1), [0, np.inf, 0, 1, 1, 1, 1.0, 0.0]),
        ("negative-size", _box(0, 0, 0, 1, -1, 1), _box(0, 0, 0, 1, 1, 1)),
        ("axis-1.01", _box(0, 0, 0, 1, 1, 1), [0, 0, 0, 1, 1, 1, 1.01, 0.0]),
    ]
    names = [n for n, _a, _b in named]
    a = [np.array(x, dtype=np.float64) for _n, x, _b in named]
    b = [np.array(x, dtype=np.float64) for _n, _a, x in named]
    a6, b6 = aabb_pairs()
    a += list(aabb_to_upright(a6))
    b += list(aabb_to_upright(b6))
    names += [f"aabb-{i}" for i in range(N_AABB)]
    rng = np.random.default_rng(20270)
    for i in range(N_RANDOM):
        apart = i % 2 == 1
        ca = rng.uniform(-2, 2, 3)
        offset = rng.uniform(-1.0, 1.0, 3)
        if apart:
            axis = int(rng.integers(0, 3))
            offset[axis] = rng.choice([-1.0, 1.0]) * rng.uniform(4.5, 9.0)
        sizes = rng.uniform(0.2, 3.0, (2, 3))
        sizes[:, :2] = np.sort(sizes[:, :2], axis=1)[:, ::-1]                       # length >= width, as the chain's boxes
        deg = rng.uniform(-90.0, 90.0, 2)
        a.append(np.array(_box(*ca, *sizes[0], deg[0])))
        b.append(np.array(_box(*(ca + offset), *sizes[1], deg[1])))
        names.append(f"random-{i}")
    a, b = np.stack(a), np.stack(b)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b, tuple(names)


def index_of(name):
    return batch()[2].index(name)


@functools.lru_cache(maxsize=None)
def matrix_boxes():
    """[N_MATRIX, 8]: boxes of one crowded scene, an identical couple and a NaN box among them."""
    a, _b, names = batch()
    first = names.index("random-0")
    boxes = a[first:first + 2 * N_MATRIX:2].copy()
    boxes[:, :3] *= 0.5
    boxes[7] = boxes[3]
    boxes[11] = np.nan
    boxes.setflags(write=False)
    return boxes


# ---- the exact oracle ------------------------------------------------------------------------------------------------------------

def refused_exact(box):
    if not np.isfinite(box).all():
        return True
    v = [Fraction(float(x)) for x in box]
    if any(x < 0 for x in v[3:6]):
        return True
    if abs(v[6] * v[6] + v[7] * v[7] - 1) > Fraction(1, 2 ** 20):
        return True
    return any(x != 0 and not (Fraction(1, 2 ** 200) <= abs(x) <= Fraction(2 ** 200)) for x in v[:6])


def _corners(v):
    cx, cy, hl, hw, ux, uy = v[0], v[1], v[3] / 2, v[4] / 2, v[6], v[7]
    ex, ey, fx, fy = hl * ux, hl * uy, -hw * uy, hw * ux
    return [(cx - ex - fx, cy - ey - fy), (cx + ex - fx, cy + ey - fy), (cx + ex + fx, cy + ey + fy), (cx - ex + fx, cy - ey + fy)]


def _clip(poly, p, q):
    """poly against the closed half-plane to the left of p -> q, exactly."""
    def side(v):
        return (q[0] - p[0]) * (v[1] - p[1]) - (q[1] - p[1]) * (v[0] - p[0])
    out = []
    for i, v in enumerate(poly):
        w = poly[(i + 1) % len(poly)]
        sv, sw = side(v), side(w)
        if sv >= 0:
            out.append(v)
        if (sv >= 0) != (sw >= 0):
            t = sv / (sv - sw)
            out.append((v[0] + t * (w[0] - v[0]), v[1] + t * (w[1] - v[1])))
    return out


def _area(poly):
    if len(poly) < 3:
        return Fraction(0)
    return sum(poly[i][0] * poly[(i + 1) % len(poly)][1] - poly[i][1] * poly[(i + 1) % len(poly)][0] for i in range(len(poly))) / 2


def exact_pair(a, b):
    """(area, dz, iou) as Fractions for two accepted boxes; iou is None where the union's volume is 0."""
    va, vb = [Fraction(float(x)) for x in a], [Fraction(float(x)) for x in b]
    window, poly = _corners(va), _corners(vb)
    for k in range(4):
        if not poly:
            break
        poly = _clip(poly, window[k], window[(k + 1) % 4])
    area = _area(poly)
    dz = min(va[2] + va[5] / 2, vb[2] + vb[5] / 2) - max(va[2] - va[5] / 2, vb[2] - vb[5] / 2)
    inter = area * dz if dz > 0 else Fraction(0)
    volume_a = va[3] * va[4] * (va[6] ** 2 + va[7] ** 2) * va[5]
    volume_b = vb[3] * vb[4] * (vb[6] ** 2 + vb[7] ** 2) * vb[5]
    union = volume_a + volume_b - inter
    return area, dz, (inter / union if union != 0 else None)


@functools.lru_cache(maxsize=None)
def batch_oracle():
    """Per pair of the batch None (refused) or ``exact_pair``'s triple; computed once."""
    a, b, _names = batch()
    return tuple(None if refused_exact(x) or refused_exact(y) else exact_pair(x, y) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def batch_twin():
    """(iou [P], parts [P, 2]) of the batch by the host twin; computed once."""
    from mspa import cloud_segments as CS
    a, b, _names = batch()
    return CS.upright_iou_host(a, b, want_parts=True)


@functools.lru_cache(maxsize=None)
def matrix_twin():
    from mspa import cloud_segments as CS
    return CS.upright_iou_matrix_host(matrix_boxes(), matrix_boxes(), want_parts=True)


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        frozen = {k: z[k] for k in z.files}
    a, _b, _names = batch()
    assert int(frozen["pairs"]) == len(a) and frozen["a_sum"].tobytes() == np.nansum(a).tobytes(), "tests/golden/upright_iou.npz is another batch's"
    return frozen
