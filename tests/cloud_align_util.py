"""The batches, the independent references and the conditions the references satisfy ALONE, behind the rigid-alignment tests
(tests/test_cloud_align_cpu.py, tests/test_gpu_cloud_align.py, tests/test_gpu_cloud_align_memory.py, tools/gen_cloud_align_golden.py).

``kabsch()`` is a seeded batch in which segment s of the queries corresponds row by row to segment s of the targets (index = arange):

  rows      0, 1 and 2 (FEW); 3 collinear rows with integer coordinates and 5 coincident rows (DEGENERATE); 3 rows in general position
            and 4 coplanar rows; then 63, 64, 65, 255, 256, 257 and 1 025 rows and a few of those sizes again
  motions   identical clouds (63), a pure translation (64), rotations of 1e-9 rad (65), 1 degree (255), 1 rad (256), pi - 1e-6 (257)
            and exactly pi (1 025) about a tilted axis; a cloud of extent 1 cm (64) and one of 100 m (255); a cloud centred 10^6 m from
            the origin (257); one with noise of extent 1e-3 (256)
  classes   for the accuracy rule: near (the origin), far, tiny (angle), pi (near it), noisy

``kabsch_variant()`` is the same sets with a third of the rows at index -1, two NaN query rows, a pair table in which query segment
``A`` and target segment ``B`` each stand in three pairs (their rows matched modulo the target's size), for float64 and float32 rows.

``icp()`` is the L-shaped 5 cm lattice of 168 points, each jittered by +-1 cm; the queries are those points permuted and moved.  Pair 0
is EASY (1 degree about (1, 2, 3) and about 5 mm, cap 5 cm), pair 1 HARD (6 degrees and 3 cm, cap 8 cm), pair 2 lies beyond any cap,
pair 3 has an empty target segment, pair 4 an empty query segment.

The references share no code with the library: brute-force nearest with ties to the lowest row, Kabsch by ``np.linalg.svd`` with the
determinant fix, a NumPy ICP of the two, and an mpmath oracle at 60 digits (centred sums, ``eigsy`` of Horn's matrix, R from the
quaternion).  What a test relies on is asserted HERE, on the references alone: every row of ``kabsch()`` is used, the expected
statuses follow from the geometry, and the NumPy ICP's margins (nearest against second nearest, matched distance against the cap)
are at least 1e-9 at every iteration, so that no rounding of a transform can change a correspondence."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cloud_align.npz")
OK, FEW, DEGENERATE = 0, 1, 2
U = 2.0 ** -53
EASY, HARD, FAR, NO_TARGET, NO_QUERY = range(5)
CAPS = {EASY: 0.05, HARD: 0.08}
MARGIN = 1e-9
ITERATIONS = 30
AXIS = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)


def rotation(axis, angle):
    """Rodrigues' matrix of a rotation by ``angle`` about ``axis``."""
    a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def _offsets(parts):
    return np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


# ---- the Kabsch batch -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def kabsch():
    """(q [N, 3], p [N, 3], offsets [S + 1], cases): ``cases`` is a tuple of dicts with ``name``, ``rows``, ``status``, ``cls`` (None
    where the accuracy rule does not apply), ``scale`` (the cloud's extent, for |t - t*| / scale)."""
    rng = np.random.default_rng(20261021)
    tilted = np.array([0.3, -0.5, 0.81])
    qs, ps, cases = [], [], []

    def add(name, q, p, status=OK, cls=None):
        q, p = np.asarray(q, dtype=np.float64).reshape(-1, 3), np.asarray(p, dtype=np.float64).reshape(-1, 3)
        qs.append(q), ps.append(p)
        cases.append({"name": name, "rows": len(q), "status": status, "cls": cls,
                      "scale": float(np.abs(p - p.mean(0)).max()) if len(p) > 1 else 1.0})

    def moved(n, angle, shift, extent=1.0, centre=(0.0, 0.0, 0.0), noise=0.0, axis=tilted):
        q = (rng.random((n, 3)) - 0.5) * extent + np.asarray(centre)
        p = q @ rotation(axis, angle).T + np.asarray(shift)
        return q, p + (rng.random((n, 3)) - 0.5) * noise

    add("empty", np.zeros((0, 3)), np.zeros((0, 3)), FEW)
    add("one row", rng.random((1, 3)), rng.random((1, 3)), FEW)
    add("two rows", rng.random((2, 3)), rng.random((2, 3)), FEW)
    line = np.array([[0, 0, 0], [1, 2, -1], [3, 6, -3]], dtype=np.float64)
    add("collinear", line, line[:, [1, 0, 2]] + 2.0, DEGENERATE)
    add("coincident", np.tile([[0.5, 1.5, -2.0]], (5, 1)), np.tile([[1.0, 0.0, 3.0]], (5, 1)), DEGENERATE)
    add("three rows", *moved(3, 0.4, [0.1, 0.2, 0.3]), cls="near")
    flat = (rng.random((4, 3)) - 0.5) * [1.0, 1.0, 0.0]
    add("coplanar", flat, flat @ rotation(tilted, 0.7).T + [0.2, -0.1, 0.4], cls="near")
    same = rng.random((63, 3))
    add("identical", same, same.copy(), cls="near")
    add("translation", *moved(64, 0.0, [0.25, -1.0, 2.0]), cls="near")
    add("1e-9 rad", *moved(65, 1e-9, [0.0, 0.0, 0.0]), cls="tiny")
    add("1 degree", *moved(255, np.deg2rad(1.0), [0.01, 0.02, -0.01]), cls="near")
    add("1 rad", *moved(256, 1.0, [0.5, 0.5, 0.5]), cls="near")
    add("pi - 1e-6", *moved(257, np.pi - 1e-6, [0.1, 0.0, -0.2]), cls="pi")
    add("pi", *moved(1025, np.pi, [0.0, 0.3, 0.0]), cls="pi")
    add("1 cm", *moved(64, 0.3, [0.001, 0.002, 0.003], extent=0.01), cls="near")
    add("100 m", *moved(255, 0.3, [10.0, -20.0, 5.0], extent=100.0), cls="near")
    add("10^6 m away", *moved(257, 0.2, [0.5, 0.25, -0.125], centre=(1e6, -1e6, 1e6)), cls="far")
    add("noisy", *moved(256, 0.5, [0.1, 0.1, 0.1], noise=1e-3), cls="noisy")
    add("noisy, 1 025", *moved(1025, 1.2, [-0.3, 0.2, 0.1], noise=1e-3, axis=[1.0, 1.0, 0.2]), cls="noisy")
    q, p = np.ascontiguousarray(np.concatenate(qs)), np.ascontiguousarray(np.concatenate(ps))
    # the conditions of the batch itself
    assert [c["rows"] for c in cases[:7]] == [0, 1, 2, 3, 5, 3, 4] and {63, 64, 65, 255, 256, 257, 1025} <= {c["rows"] for c in cases}
    assert np.isfinite(q).all() and np.isfinite(p).all()                      # every row is used
    assert {c["cls"] for c in cases} == {None, "near", "far", "tiny", "pi", "noisy"}
    assert np.linalg.matrix_rank(line - line.mean(0)) == 1 and line.dtype == np.float64 and (line == np.round(line)).all()
    for c, a, b in zip(cases, _offsets(qs)[:-1], _offsets(qs)[1:]):
        rank = np.linalg.matrix_rank(q[a:b] - q[a:b].mean(0)) if b - a > 1 else 0
        assert (c["status"] == OK) == (rank >= 2 and b - a >= 3), c["name"]
    return _frozen(q, p, _offsets(qs), tuple(cases))


A_SEGMENT, B_SEGMENT = 11, 10                                                # 256 and 255 rows: A stands in three pairs as the query, B as the target


@functools.lru_cache(maxsize=None)
def kabsch_variant():
    """(q, q_offsets, p, pairs [P, 2], index [M], out_offsets [P + 1]): the Kabsch batch with a third of the rows unmatched, two NaN
    query rows and segments that stand in three pairs."""
    q, p, off, cases = kabsch()
    rng = np.random.default_rng(7)
    S = len(cases)
    q = q.copy()
    q[off[13] + 5] = [np.nan, 0.0, 0.0]                                      # two rows of the 1 025
    q[off[13] + 700] = [0.0, np.inf, 0.0]
    pairs = [(s, s) for s in range(S)] + [(A_SEGMENT, B_SEGMENT), (A_SEGMENT, 12), (9, B_SEGMENT)]
    index, out = [], [0]
    for qs, ts in pairs:
        n, m = off[qs + 1] - off[qs], off[ts + 1] - off[ts]
        rows = off[ts] + np.arange(n) % max(m, 1) if m else np.full((n,), -1)
        index.append(np.where(rng.random(n) < 1.0 / 3.0, -1, rows))
        out.append(out[-1] + n)
    assert sum(1 for a, _ in pairs if a == A_SEGMENT) == 3 and sum(1 for _, b in pairs if b == B_SEGMENT) == 3
    return _frozen(q, off, p, np.array(pairs, dtype=np.int64), np.concatenate(index).astype(np.int64), np.array(out, dtype=np.int64))


def kabsch_svd(Q, P):
    """(R, t) of the least-squares rigid fit of the rows Q onto the rows P by ``np.linalg.svd`` with the determinant fix."""
    qc, pc = Q.mean(0), P.mean(0)
    H = (Q - qc).T @ (P - pc)
    Um, _s, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(Vt.T @ Um.T))
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ Um.T
    return R, pc - R @ qc


def kabsch_mp(Q, P):
    """(R, t) as float64 of the exact-enough fit at 60 digits: centred sums, ``eigsy`` of Horn's matrix, R from the quaternion."""
    import mpmath as mp
    with mp.workdps(60):
        n = len(Q)
        Qm, Pm = [[mp.mpf(float(v)) for v in row] for row in Q], [[mp.mpf(float(v)) for v in row] for row in P]
        qc = [mp.fsum(r[a] for r in Qm) / n for a in range(3)]
        pc = [mp.fsum(r[a] for r in Pm) / n for a in range(3)]
        S = [[mp.fsum((x[a] - qc[a]) * (y[b] - pc[b]) for x, y in zip(Qm, Pm)) for b in range(3)] for a in range(3)]
        N = mp.matrix([[S[0][0] + S[1][1] + S[2][2], S[1][2] - S[2][1], S[2][0] - S[0][2], S[0][1] - S[1][0]],
                       [S[1][2] - S[2][1], S[0][0] - S[1][1] - S[2][2], S[0][1] + S[1][0], S[2][0] + S[0][2]],
                       [S[2][0] - S[0][2], S[0][1] + S[1][0], S[1][1] - S[0][0] - S[2][2], S[1][2] + S[2][1]],
                       [S[0][1] - S[1][0], S[2][0] + S[0][2], S[1][2] + S[2][1], S[2][2] - S[0][0] - S[1][1]]])
        E, V = mp.eigsy(N)
        k = max(range(4), key=lambda i: E[i])
        w, x, y, z = (V[i, k] for i in range(4))
        norm = mp.sqrt(w * w + x * x + y * y + z * z)
        w, x, y, z = w / norm, x / norm, y / norm, z / norm
        R = [[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
             [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
             [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]]
        t = [pc[a] - (R[a][0] * qc[0] + R[a][1] * qc[1] + R[a][2] * qc[2]) for a in range(3)]
        return np.array([[float(v) for v in row] for row in R]), np.array([float(v) for v in t])


@functools.lru_cache(maxsize=None)
def kabsch_references():
    """Per OK case of ``kabsch()`` with a class: (name, cls, scale, (R, t) by SVD, (R, t) by mpmath), computed once."""
    q, p, off, cases = kabsch()
    out = []
    for s, c in enumerate(cases):
        if c["cls"] is not None:
            Q, P = q[off[s]:off[s + 1]], p[off[s]:off[s + 1]]
            out.append((s, c["name"], c["cls"], c["scale"], kabsch_svd(Q, P), kabsch_mp(Q, P)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def variant_references():
    """Per pair of ``kabsch_variant()`` whose used rows (index >= 0, a finite query row) number at least 3 and span a plane on either
    side: (pair, cls, scale, (R, t) by SVD, (R, t) by mpmath) of exactly those rows.  ``cls`` is the segment's class where the pair is
    (s, s), "mixed" where the rows of one segment are matched modulo another's."""
    q, q_off, p, pairs, index, out_off = kabsch_variant()
    cases = kabsch()[3]
    out = []
    for k, (qs, ts) in enumerate(pairs):
        rows, at = np.arange(q_off[qs], q_off[qs + 1]), index[out_off[k]:out_off[k + 1]]
        used = (at >= 0) & np.isfinite(q[rows]).all(axis=1)
        Q, P = q[rows][used], p[at[used]]
        if used.sum() >= 3 and np.linalg.matrix_rank(Q - Q.mean(0)) >= 2 and np.linalg.matrix_rank(P - P.mean(0)) >= 2:
            cls = cases[qs]["cls"] if qs == ts else "mixed"
            out.append((k, cls, float(np.abs(P - P.mean(0)).max()), kabsch_svd(Q, P), kabsch_mp(Q, P)))
    assert {c for _k, c, *_ in out} == {"near", "far", "tiny", "pi", "noisy", "mixed"}
    return tuple(out)


def errors(R, t, R_star, t_star, scale):
    """(max |R - R*|, max |t - t*| / scale)."""
    return float(np.abs(R - R_star).max()), float(np.abs(t - t_star).max() / scale)


def class_worst(per_case):
    """{cls: (worst |R - R*|, worst |t - t*| / scale)} of {(cls, name): (eR, et)}."""
    worst = {}
    for (cls, _name), (eR, et) in per_case.items():
        a, b = worst.get(cls, (0.0, 0.0))
        worst[cls] = (max(a, eR), max(b, et))
    return worst


@functools.lru_cache(maxsize=None)
def svd_class_errors():
    """NumPy-SVD-Kabsch's worst errors against the mpmath oracle, per class: the yardstick of the accuracy rule."""
    return class_worst({(cls, name): errors(*svd, *star, scale) for _s, name, cls, scale, svd, star in kabsch_references()})


def within_rule(err, yard):
    """The accuracy rule: at most 8 x the yardstick, and at least one unit roundoff is allowed."""
    return err <= max(8.0 * yard, U)


def exact_ortho_defect(R):
    """max |R^T R - I| of a matrix of doubles, in exact rational arithmetic."""
    from fractions import Fraction
    F = [[Fraction(float(v)) for v in row] for row in np.asarray(R)]
    worst = Fraction(0)
    for i in range(3):
        for j in range(3):
            worst = max(worst, abs(sum(F[k][i] * F[k][j] for k in range(3)) - (1 if i == j else 0)))
    return float(worst)


# ---- the ICP batch --------------------------------------------------------------------------------------------------------------

def lattice():
    """The L-shaped 5 cm lattice: 8 x 3 x 4 points along x and 3 x 6 x 4 along y, 168 in all."""
    arm = lambda nx, ny, y0: np.array([(x, y0 + y, z) for x in range(nx) for y in range(ny) for z in range(4)], dtype=np.float64)      # noqa: E731
    return np.concatenate([arm(8, 3, 0), arm(3, 6, 3)]) * 0.05


@functools.lru_cache(maxsize=None)
def icp():
    """(q [Nq, 3], q_offsets [6], t [Nt, 3], t_offsets [6], truth): ``truth[p]`` = (R, t) that carries pair p's queries onto its
    targets, for the EASY and the HARD pair."""
    rng = np.random.default_rng(20261022)
    L = lattice()
    L = L + (rng.random(L.shape) * 2.0 - 1.0) * 0.01
    assert len(L) == 168 and 0.2 < np.linalg.norm(L - L.mean(0), axis=1).max() < 0.35
    truth, queries = {}, []
    for pair, angle, shift in ((EASY, np.deg2rad(1.0), 0.005), (HARD, np.deg2rad(6.0), 0.03)):
        R = rotation([1.0, 2.0, 3.0], angle)
        c = L.mean(0)
        t = c - R @ c + shift * np.array([2.0, -1.0, 2.0]) / 3.0             # the rotation turns about the centroid
        truth[pair] = (R, t)
        queries.append(((L - t) @ R)[rng.permutation(len(L))])                # R^T (p - t), permuted
    queries.append(L[:40] + 5.0)                                              # beyond any cap
    queries.append(L[:7])                                                     # against an empty target segment
    queries.append(np.zeros((0, 3)))                                          # an empty query segment
    targets = [L, L, L, np.zeros((0, 3)), L[:50]]
    return _frozen(np.ascontiguousarray(np.concatenate(queries)), _offsets(queries), np.ascontiguousarray(np.concatenate(targets)),
                   _offsets(targets)) + (truth,)


def brute_two(Y, T):
    """Nearest by brute force with ties to the lowest row: (index [n], d2 [n], second smallest d2 [n])."""
    d = T[None] - Y[:, None]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    part = np.sort(d2, axis=1)
    return d2.argmin(1), part[:, 0], part[:, 1]


@functools.lru_cache(maxsize=None)
def numpy_icp(pair, cap, iterations=ITERATIONS, from_fixed_point=False):
    """The NumPy ICP of one pair of ``icp()`` (brute-force search, SVD Kabsch, the fit of the ORIGINAL rows as the next transform) ->
    a dict: ``index`` [K, n] local rows or -1, ``R``, ``t`` the final transform, ``fixed_at`` the first k >= 1 whose correspondences
    equal those of k - 1 (0 when started from the fixed point and they equal the fixed point's), ``margin_second`` and ``margin_cap``
    the smallest margins over all iterations, ``matched`` the rows matched at the end."""
    q, q_off, t, t_off, _truth = icp()
    Q, T = q[q_off[pair]:q_off[pair + 1]], t[t_off[pair]:t_off[pair + 1]]
    R, tr = np.eye(3), np.zeros(3)
    last = None
    if from_fixed_point:
        start = numpy_icp(pair, cap, iterations)
        R, tr, last = start["R"], start["t"], start["index"][-1]
    history, fixed_at, m_second, m_cap = [], -1, np.inf, np.inf
    for k in range(iterations):
        at, d2, second = brute_two(Q @ R.T + tr, T)
        inside = d2 <= cap * cap
        m_second = min(m_second, float((np.sqrt(second) - np.sqrt(d2)).min()))
        m_cap = min(m_cap, float(np.abs(np.sqrt(d2) - cap).min()))
        index = np.where(inside, at, -1)
        if fixed_at < 0 and last is not None and np.array_equal(index, last):
            fixed_at = k
        history.append(index)
        last = index
        if inside.sum() >= 3:
            R, tr = kabsch_svd(Q[inside], T[at[inside]])
    return {"index": np.array(history), "R": R, "t": tr, "fixed_at": fixed_at, "margin_second": m_second, "margin_cap": m_cap,
            "matched": int((history[-1] >= 0).sum())}


@functools.lru_cache(maxsize=None)
def icp_references():
    """{(pair, from_fixed_point): numpy_icp(...)} for the EASY and the HARD pair at their caps, with the conditions a test relies on
    asserted on the references alone."""
    out = {}
    for pair, cap in CAPS.items():
        for again in (False, True):
            ref = out[(pair, again)] = numpy_icp(pair, cap, ITERATIONS, again)
            assert ref["margin_second"] >= MARGIN and ref["margin_cap"] >= MARGIN, (pair, again, ref["margin_second"], ref["margin_cap"])
            assert ref["matched"] == 168 and ref["fixed_at"] == (0 if again else ref["fixed_at"]) and 0 <= ref["fixed_at"] < 12, (pair, again, ref["fixed_at"])
    return out


def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}
