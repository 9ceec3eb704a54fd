"""Nearest-point distances between the clouds of two ragged batches without a GPU: the host twin (csrc/cloud_distance_core.h through
mspa_cloud_distance_host and mspa_cloud_distance_fit_host) against a NumPy brute force that shares no code with it
(tests/cloud_distance_util.py):

  * ``distance`` and ``index`` equal the brute force BYTE FOR BYTE on every pair of the batch, with the pair table and with
    ``pairs=None``; rows equal to a target row give exactly 0.0, doubled rows give the lower index, an empty target +inf / -1, a NaN or
    inf query row NaN / -1; a cap masks the oracle, at an attained distance and one ulp below it;
  * the same bytes for ``_grid_k`` in {1, 8, 64}; SciPy's cKDTree within 8 u d as a second implementation;
  * the six summaries against ``segs::ordered_sum`` restated in NumPy, byte for byte; swapping the roles gives the transposed brute
    force; the MSPA_EINVALs and ValueErrors; the frozen fixture against a fresh run;
  * the headers once more as a stand-alone g++ program under AddressSanitizer + UBSan."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_distance_util as U  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-spatialmllm_amd", "csrc")
fold = lambda text: " ".join(text.split())                                   # noqa: E731


def _segment(out, p):
    a, b = out["offsets"][p], out["offsets"][p + 1]
    return out["distance"][a:b], out["index"][a:b]


def test_the_batch_is_what_its_docstring_says():
    t, t_off, q, q_off, pairs = U.batch()
    assert np.diff(t_off).tolist() == [0, 1, 2, 63, 64, 65, 257, 3000, 300, 200, 200, 1000, 500]
    assert len(t) + len(q) <= 20000 and len(q_off) == len(t_off) == 14 and q_off[5] == q_off[4] and len(pairs) == 21
    assert np.isfinite(t).all() and (~np.isfinite(q)).any(axis=1).sum() == 4
    assert (t[t_off[10]:t_off[10] + 100] == t[t_off[10] + 100:t_off[11]]).all() and (t[t_off[9]:t_off[10]] == t[t_off[9]]).all()
    spread = t[t_off[11]:t_off[12]]
    assert np.ptp(spread, axis=0).min() > 20 * np.ptp(np.sort(spread, axis=0)[10:-10], axis=0).max()      # the box is far smaller than the extent
    assert (t[t_off[6]:t_off[7], 2] == 0.25).all()


def test_distance_and_index_are_the_brute_forces_byte_for_byte_on_every_pair():
    distance, index, offsets = U.batch_oracle()
    twin = U.batch_twin()
    assert twin["offsets"].tobytes() == offsets.tobytes() and twin["distance"].dtype == np.float64 and twin["index"].dtype == np.int64
    assert twin["distance"].tobytes() == distance.tobytes() and twin["index"].tobytes() == index.tobytes()
    t, t_off, q, q_off, pairs = U.batch()
    for p, (qs, ts) in enumerate(pairs):
        d, i = _segment(twin, p)
        assert len(d) == q_off[qs + 1] - q_off[qs]
        if ts == 0 or qs in (0, 4):
            continue
        own = min(int(t_off[qs + 1] - t_off[qs]), 20)
        if qs == ts:
            assert d[:own].tobytes() == np.zeros(own).tobytes(), p            # a target's own rows: exactly +0.0
            assert (t[i[:own]] == q[q_off[qs]:q_off[qs] + own]).all()
    d, i = _segment(twin, 10)
    assert ((i >= t_off[10]) & (i < t_off[10] + 100)).all()                  # every row stands twice: the lower one
    d, i = _segment(twin, 9)
    assert (i[np.isfinite(d)] == t_off[9]).all()                             # 200 identical rows: the first
    d, i = _segment(twin, 0)
    assert np.isposinf(d).all() and (i == -1).all() and len(d) == 5          # an empty target
    d, i = _segment(twin, 19)
    assert np.isposinf(d).all() and (i == -1).all() and len(d) > 600
    assert len(_segment(twin, 20)[0]) == 0 and len(_segment(twin, 4)[0]) == 0
    for p in (3, 11):
        d, i = _segment(twin, p)
        assert np.isnan(d[-2:]).all() and (i[-2:] == -1).all() and np.isfinite(d[:-2]).all()
    d, _i = _segment(twin, 18)
    assert (d > 1e6).all()                                                   # the queries at 10^6 against the unit cube


def test_without_a_pair_table_pair_s_is_s_s():
    from mspa import cloud_segments as CS
    t, t_off, q, q_off, pairs = U.batch()
    out = CS.nearest_segments_host(q, q_off, t, t_off)
    distance, index, offsets = U.batch_oracle()
    M = offsets[13]
    assert out["offsets"].tobytes() == offsets[:14].tobytes()
    assert out["distance"].tobytes() == distance[:M].tobytes() and out["index"].tobytes() == index[:M].tobytes()
    with pytest.raises(ValueError):
        CS.nearest_segments_host(q, q_off, t[:t_off[12]], t_off[:13])        # 13 query segments, 12 target segments, no table


def test_a_cap_masks_the_oracle_and_changes_nothing_else():
    from mspa import cloud_segments as CS
    t, t_off, q, q_off, pairs = U.batch()
    free = U.batch_twin()
    # an attained distance whose square, rounded once, is not below the attained d2 (sqrt may round down: then d * d < d2 and the
    # rule, which compares d2 with cap2 = d * d, drops the row -- the oracle says which)
    a, b = free["offsets"][7], free["offsets"][8]
    d7 = free["distance"][a:b]
    _d, _i, d2 = U.brute(q[q_off[7]:q_off[8]], t[t_off[7]:t_off[8]])
    keeps = np.nonzero((d7 > 0.02) & (d7 * d7 >= d2))[0]
    assert len(keeps) > 10
    attained = d7[keeps[0]]
    for cap in (attained, np.nextafter(attained, 0.0), 0.05, 1e-3, 3.0, 1e7):
        out = CS.nearest_segments_host(q, q_off, t, t_off, pairs, max_distance=cap)
        distance, index, _offsets = U.oracle(t, t_off, q, q_off, pairs, max_distance=cap)
        assert out["distance"].tobytes() == distance.tobytes() and out["index"].tobytes() == index.tobytes(), cap
        kept = np.isfinite(out["distance"])
        assert (out["distance"][kept] == free["distance"][kept]).all() and (out["index"][kept] == free["index"][kept]).all()
        assert (out["index"][~kept] == -1).all()
    at = CS.nearest_segments_host(q, q_off, t, t_off, pairs, max_distance=attained)
    below = CS.nearest_segments_host(q, q_off, t, t_off, pairs, max_distance=np.nextafter(attained, 0.0))
    assert at["distance"][a + keeps[0]] == attained and np.isposinf(below["distance"][a + keeps[0]])
    assert np.isfinite(at["distance"]).sum() > np.isfinite(below["distance"]).sum()
    capped = CS.nearest_segments_host(q, q_off, t, t_off, pairs, max_distance=0.05, want_evals=True)
    assert capped["evals"][free["offsets"][18]:free["offsets"][19]].max() < 3000 == free["evals"][free["offsets"][18]:free["offsets"][19]].min()


def test_the_results_do_not_depend_on_the_grids_neighbour_count():
    from mspa import cloud_segments as CS
    t, t_off, q, q_off, pairs = U.batch()
    free = U.batch_twin()
    evals = {}
    for k in (1, 8, 64):
        out = CS.nearest_segments_host(q, q_off, t, t_off, pairs, want_evals=True, _grid_k=k)
        assert out["distance"].tobytes() == free["distance"].tobytes() and out["index"].tobytes() == free["index"].tobytes(), k
        evals[k] = out["evals"]
        capped = CS.nearest_segments_host(q, q_off, t, t_off, pairs, max_distance=0.05, _grid_k=k)
        assert capped["distance"].tobytes() == CS.nearest_segments_host(q, q_off, t, t_off, pairs, max_distance=0.05)["distance"].tobytes()
    assert evals[CS._lib.CLOUD_DISTANCE_GRID_K].tobytes() == free["evals"].tobytes() and evals[1].tobytes() != evals[64].tobytes()      # only the work differs


def test_scipys_kd_tree_agrees_within_eight_u_d():
    """A second implementation, not the parity claim: one evaluated d2 is within 4 u of the exact one, the root halves that and rounds
    once; SciPy's own evaluation is of the same kind."""
    spatial = pytest.importorskip("scipy.spatial")
    t, t_off, q, q_off, pairs = U.batch()
    twin = U.batch_twin()
    u = 2.0 ** -53
    checked = 0
    for p, (qs, ts) in enumerate(pairs):
        T, Q = t[t_off[ts]:t_off[ts + 1]], q[q_off[qs]:q_off[qs + 1]]
        good = np.isfinite(Q).all(axis=1)
        if len(T) == 0 or not good.any():
            continue
        want, _where = spatial.cKDTree(T).query(Q[good])
        got = _segment(twin, p)[0][good]
        assert (np.abs(got - want) <= 8 * u * want).all(), p
        checked += len(want)
    assert checked > 2500


def test_the_summaries_are_ordered_sums_restated_in_numpy_byte_for_byte():
    from mspa import cloud_segments as CS
    twin = U.batch_twin()
    for distance in (twin["distance"], CS.nearest_segments_host(*_as_call(U.batch()[:4]), U.batch()[4], max_distance=0.3)["distance"]):
        for tau in (0.0, U.TAU, 2.0):
            got = CS.fit_segments_host(distance, twin["offsets"], tau)
            want = U.fit_oracle(distance, twin["offsets"], tau)
            assert list(got) == list(CS.FIT_KEYS) == list(want)
            for key in want:
                assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), (key, tau)
    fit = twin["fit"]
    assert fit["rows"].tolist() == np.diff(twin["offsets"]).tolist()
    assert fit["finite"][0] == 0 and fit["max"][0] == -np.inf and fit["sum"][0] == 0.0 and fit["rows"][4] == 0 and fit["max"][4] == -np.inf
    assert fit["finite"][3] == fit["rows"][3] - 2 and fit["within"][18] == 0 and (fit["within"] <= fit["finite"]).all()
    a, b = twin["offsets"][7], twin["offsets"][8]
    assert fit["max"][7] == np.max(twin["distance"][a:b]) and abs(fit["sum"][7] - twin["distance"][a:b].sum()) < 1e-9
    empty = CS.fit_segments_host(np.zeros((0,)), [0], 1.0)
    assert all(v.shape == (0,) for v in empty.values())


def _as_call(four):
    t, t_off, q, q_off = four
    return q, q_off, t, t_off


def test_swapping_the_roles_gives_the_transposed_brute_force():
    from mspa import cloud_segments as CS
    t, t_off, q, q_off, _pairs = U.batch()
    A, B = t[t_off[7]:t_off[7] + 700], q[q_off[7]:q_off[8]]
    d = B[None] - A[:, None]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]                 # [A, B]
    one = lambda x: np.array([0, len(x)], dtype=np.int64)                    # noqa: E731
    ab = CS.nearest_segments_host(A, one(A), B, one(B))
    ba = CS.nearest_segments_host(B, one(B), A, one(A))
    assert ab["distance"].tobytes() == np.sqrt(d2.min(1)).tobytes() and ab["index"].tobytes() == d2.argmin(1).astype(np.int64).tobytes()
    assert ba["distance"].tobytes() == np.sqrt(d2.min(0)).tobytes() and ba["index"].tobytes() == d2.argmin(0).astype(np.int64).tobytes()
    fit = CS.cloud_fit_segments_host(A, one(A), B, one(B), 0.05)
    assert fit["precision"][0] == (ab["distance"] <= 0.05).sum() / len(A) and fit["recall"][0] == (ba["distance"] <= 0.05).sum() / len(B)
    p, r = fit["precision"][0], fit["recall"][0]
    assert fit["fscore"][0] == (2 * p * r) / (p + r)
    assert fit["chamfer"][0] == fit["a_to_b"]["sum"][0] / len(A) + fit["b_to_a"]["sum"][0] / len(B)
    hollow = CS.cloud_fit_segments_host(A, [0, 0, len(A)], B, [0, len(B), len(B)], 0.05)
    assert np.isnan(hollow["precision"][0]) and np.isnan(hollow["recall"][1]) and np.isnan(hollow["fscore"]).all() and np.isnan(hollow["chamfer"]).all()


def test_compute_point_cloud_distance_is_the_one_pair_case():
    import torch
    from spatial_engine.utils.scannet_utils.handler import ops
    t, t_off, q, q_off, _pairs = U.batch()
    source, target = q[q_off[7]:q_off[7] + 100], t[t_off[7]:t_off[8]]
    got = ops.compute_point_cloud_distance(source, target)
    assert isinstance(got, np.ndarray) and got.tobytes() == U.brute(source, target)[0].tobytes()
    with_colour = np.hstack([source, np.ones((100, 3))]).astype(np.float32)
    assert ops.compute_point_cloud_distance(with_colour, target).tobytes() == U.brute(with_colour[:, :3].astype(np.float64), target)[0].tobytes()
    on_host = ops.compute_point_cloud_distance(torch.from_numpy(source.copy()), torch.from_numpy(target.copy()))
    assert isinstance(on_host, torch.Tensor) and on_host.numpy().tobytes() == got.tobytes()
    assert np.isposinf(ops.compute_point_cloud_distance(source, np.zeros((0, 3)))).all()
    assert ops.compute_point_cloud_distance(np.zeros((0, 3)), target).shape == (0,)
    with pytest.raises(ValueError):
        ops.compute_point_cloud_distance(source, np.array([[0.0, np.nan, 0.0]]))
    doc = fold(ops.compute_point_cloud_distance.__doc__)
    assert "not checked against Open3D" in doc and "No reference counterpart" in doc and "compute_point_cloud_distance" not in ops.__all__


def test_the_python_functions_refuse_what_is_outside_their_domain():
    from mspa import cloud_segments as CS
    t, t_off, q, q_off, pairs = U.batch()
    bad_calls = [
        lambda: CS.nearest_segments_host(q, q_off, t, t_off, [[0, 13]]), lambda: CS.nearest_segments_host(q, q_off, t, t_off, [[13, 0]]),
        lambda: CS.nearest_segments_host(q, q_off, t, t_off, [[-1, 0]]), lambda: CS.nearest_segments_host(q, q_off, t, t_off, [[0, 1, 2]]),
        lambda: CS.nearest_segments_host(q, q_off, t, t_off, pairs, max_distance=0.0),
        lambda: CS.nearest_segments_host(q, q_off, t, t_off, pairs, max_distance=-1.0),
        lambda: CS.nearest_segments_host(q, q_off, t, t_off, pairs, max_distance=np.inf),
        lambda: CS.nearest_segments_host(q, q_off, t, t_off, pairs, max_distance=np.nan),
        lambda: CS.nearest_segments_host(q, q_off, t, t_off, pairs, _grid_k=0), lambda: CS.nearest_segments_host(q, q_off, t, t_off, pairs, _grid_k=65),
        lambda: CS.nearest_segments_host(q, q_off[:-1], t, t_off, pairs), lambda: CS.nearest_segments_host(q[:, :2], q_off, t, t_off, pairs),
        lambda: CS.nearest_segments_host(q, q_off, np.where(np.arange(len(t))[:, None] == 5, np.inf, t), t_off, pairs),
        lambda: CS.fit_segments_host(np.zeros(4), [0, 4], -1.0), lambda: CS.fit_segments_host(np.zeros(4), [0, 4], np.inf),
        lambda: CS.fit_segments_host(np.zeros(4), [0, 4], np.nan), lambda: CS.fit_segments_host(np.zeros(4), [0, 5], 1.0),
        lambda: CS.fit_segments_host(np.zeros((4, 1)), [0, 4], 1.0)]
    for n, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {n} was accepted")
    for call in (lambda: CS.target_index(t, t_off), lambda: CS.nearest_segments(q, q_off, t, t_off), lambda: CS.fit_segments(np.zeros(4), [0, 4], 1.0)):
        with pytest.raises((ValueError, RuntimeError)):
            call()                                                           # NumPy rows have no device: no quiet fallback
    assert "Enqueue only: the keys pass, the sort and the search on the current stream, the host tables go up through pinned memory and nothing is read back." \
        in fold(CS.TargetIndex.nearest.__doc__)
    assert "Enqueue only: one launch on the current stream, the offsets go up through pinned memory and nothing is read back." \
        in fold(CS.fit_segments.__doc__)
    assert "not a fallback" in fold(CS.nearest_segments_host.__doc__) and "not a fallback" in fold(CS.fit_segments_host.__doc__)
    assert "One read-back per call" in fold(CS.target_index.__doc__)


def test_the_c_entry_points_refuse_bad_arguments_before_anything_is_enqueued():
    """Every refusal below returns MSPA_EINVAL from the argument checks; none of the pointers is a device pointer, and none is ever
    dereferenced as one (the checks come before the launch)."""
    from mspa import _lib
    lib = _lib.load()
    p = lambda x: None if x is None else x.ctypes.data                       # noqa: E731
    t_off, q_off = np.array([0, 4, 4, 10], dtype=np.int64), np.array([0, 3, 5, 5], dtype=np.int64)
    t, q = np.random.default_rng(1).random((10, 3)), np.random.default_rng(2).random((5, 3))
    pairs, out_off = np.array([[0, 2], [1, 0], [0, 0]], dtype=np.int64), np.array([0, 3, 5, 8], dtype=np.int64)
    lo, hi = np.array([t[:4].min(0), [0, 0, 0], t[4:].min(0)]), np.array([t[:4].max(0), [0, 0, 0], t[4:].max(0)])
    grids = np.zeros((3, _lib.KNN_GRID_BYTES), dtype=np.uint8)
    assert lib.mspa_knn_segments_grids_host(p(lo), p(hi), p(t_off), 3, 8, p(grids)) == 0
    dist, index, evals = np.zeros(8), np.zeros(8, dtype=np.int64), np.zeros(8, dtype=np.int32)
    starts, order, base = np.zeros(64, dtype=np.int32), np.arange(10, dtype=np.int64), np.zeros(4, dtype=np.int64)
    good = dict(pts=t, starts=starts, order=order, t_off=t_off, St=3, k=8, grids=grids, q=q, q_off=q_off, Sq=3, pairs=pairs, P=3, out_off=out_off,
                cap=np.inf, dist=dist, index=index, evals=evals)

    def device(**change):
        a = dict(good, **change)
        shift = lambda name: (p(a[name]) or 0) + a.get(name + "_shift", 0) or None                  # noqa: E731
        return lib.mspa_cloud_distance_device(shift("pts"), shift("starts"), a.get("slots", 64), shift("order"), p(a["t_off"]), a["St"], a["k"], p(a["grids"]),
                                              p(a["t_off"]), p(a["grids"]), p(base), shift("q"), p(a["q_off"]), a["Sq"], p(a["q_off"]),
                                              p(a["pairs"]), p(a["pairs"]), a["P"], p(a["out_off"]), p(a["out_off"]), None, a["cap"], shift("dist"),
                                              shift("index"), shift("evals"), None)

    def host(**change):
        a = dict(good, **change)
        return lib.mspa_cloud_distance_host(p(a["pts"]), p(a["t_off"]), a["St"], a["k"], p(a["q"]), p(a["q_off"]), a["Sq"], p(a["pairs"]), a["P"],
                                            p(a["out_off"]), a["cap"], p(a["dist"]), p(a["index"]), p(a["evals"]))

    refused = {}
    for name, call in (("device", device), ("host", host)):
        refused.update({
            f"{name}: target offsets not from 0": call(t_off=np.array([1, 4, 4, 10], dtype=np.int64)),
            f"{name}: query offsets descending": call(q_off=np.array([0, 3, 2, 5], dtype=np.int64)),
            f"{name}: negative St": call(St=-1), f"{name}: null query offsets": call(q_off=None),
            f"{name}: pair beyond Sq": call(pairs=np.array([[3, 2], [1, 0], [0, 0]], dtype=np.int64)),
            f"{name}: pair beyond St": call(pairs=np.array([[0, 3], [1, 0], [0, 0]], dtype=np.int64)),
            f"{name}: negative pair": call(pairs=np.array([[0, -1], [1, 0], [0, 0]], dtype=np.int64)),
            f"{name}: no table, P != Sq": call(pairs=None, P=2, out_off=np.array([0, 3, 5], dtype=np.int64)),
            f"{name}: negative P": call(P=-1), f"{name}: too many pairs": call(P=(1 << 24) + 1),
            f"{name}: out_offsets of other pairs": call(out_off=np.array([0, 3, 6, 8], dtype=np.int64)),
            f"{name}: out_offsets short at the end": call(out_off=np.array([0, 3, 5, 7], dtype=np.int64)),
            f"{name}: null out_offsets": call(out_off=None),
            f"{name}: cap 0": call(cap=0.0), f"{name}: cap negative": call(cap=-2.0), f"{name}: cap NaN": call(cap=np.nan),
            f"{name}: grid_k 0": call(k=0), f"{name}: grid_k 65": call(k=65),
            f"{name}: null queries": call(q=None), f"{name}: null distance": call(dist=None), f"{name}: null targets": call(pts=None)})
    broken = grids.copy()
    broken[2, 96:100] = 0                                                    # dim[0] = 0
    refused.update({"device: grids that fail grids_ok": device(grids=broken),
                    "device: null starts": device(starts=None), "device: too few slots": device(slots=8), "device: null order": device(order=None),
                    "device: pts at 4 mod 8": device(pts_shift=4), "device: queries at 4 mod 8": device(q_shift=4),
                    "device: distance at 4 mod 8": device(dist_shift=4), "device: index at 4 mod 8": device(index_shift=4),
                    "device: starts at 2 mod 4": device(starts_shift=2), "device: evals at 2 mod 4": device(evals_shift=2),
                    "host: non-finite target": host(pts=np.where(np.arange(10)[:, None] == 7, np.nan, t))})
    six = [np.zeros(3, dtype=np.int64) for _ in range(3)] + [np.zeros(3) for _ in range(3)]

    def fit(who, distance=dist, offsets=out_off, P=3, tau=1.0, outs=six, shift=0):
        ptrs = [None if o is None else p(o) + shift for o in outs]
        if who == "device":
            return lib.mspa_cloud_distance_fit_device(p(distance), p(offsets), P, tau, p(offsets), *ptrs, None)
        return lib.mspa_cloud_distance_fit_host(p(distance), p(offsets), P, tau, *ptrs)

    for who in ("device", "host"):
        refused.update({f"fit {who}: tau negative": fit(who, tau=-0.5), f"fit {who}: tau inf": fit(who, tau=np.inf), f"fit {who}: tau NaN": fit(who, tau=np.nan),
                        f"fit {who}: offsets not from 0": fit(who, offsets=np.array([2, 3, 5, 8], dtype=np.int64)), f"fit {who}: negative P": fit(who, P=-1),
                        f"fit {who}: null offsets": fit(who, offsets=None), f"fit {who}: null distance": fit(who, distance=None),
                        f"fit {who}: null sum": fit(who, outs=six[:3] + [None] + six[4:])})
    refused["fit device: an output at 4 mod 8"] = fit("device", shift=4)
    idx = dict(xyz=t, off=t_off, S=3, k=8, grids=grids, order=order, pts=np.zeros((10, 3)), keys=np.zeros(10, dtype=np.int64), starts=starts,
               slots=64, pts_shift=0, starts_shift=0)

    def index_device(**change):
        a = dict(idx, **change)
        at = lambda name: None if a[name] is None else p(a[name]) + a[name + "_shift"]               # noqa: E731
        return lib.mspa_knn_segments_index_device(p(a["xyz"]), p(a["off"]), a["S"], a["k"], p(a["grids"]), p(a["off"]), p(a["grids"]), p(base),
                                                  p(a["order"]), at("pts"), p(a["keys"]), at("starts"), a["slots"], None)
    refused.update({"index: k 0": index_device(k=0), "index: null xyz": index_device(xyz=None), "index: null starts": index_device(starts=None),
                    "index: too few slots": index_device(slots=8), "index: bad offsets": index_device(off=np.array([0, 4, 3, 10], dtype=np.int64)),
                    "index: grids that fail grids_ok": index_device(grids=broken), "index: pts at 4 mod 8": index_device(pts_shift=4),
                    "index: starts at 2 mod 4": index_device(starts_shift=2)})
    assert {k: v for k, v in refused.items() if v != _lib.MSPA_EINVAL} == {}
    assert b"mspa_knn_segments_index_device" in lib.mspa_last_error_string()
    # zero output rows enqueue nothing, and the buffers of the rows that do not exist may be null
    none = np.array([0, 0, 0, 0], dtype=np.int64)
    assert device(q_off=none, out_off=none, q=None, dist=None, index=None, evals=None) == 0
    assert device(P=0, pairs=pairs[:0], out_off=np.array([0], dtype=np.int64), dist=None, index=None, evals=None) == 0
    assert index_device(off=none, xyz=None, pts=None, keys=None, order=None) == 0
    assert lib.mspa_cloud_distance_fit_device(None, p(none), 0, 1.0, None, None, None, None, None, None, None, None) == 0
    assert host() == 0 and host(index=None, evals=None) == 0 and host(cap=0.25) == 0 and fit("host") == 0          # the good arguments are good
    assert dist.tobytes() == U.oracle(t, t_off, q, q_off, pairs, 0.25)[0].tobytes()


def test_the_frozen_results_are_a_fresh_runs():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_cloud_distance_golden as G
    frozen, fresh, twin = U.golden(), G.frozen(), U.batch_twin()
    assert sorted(frozen) == sorted(fresh)
    for key in fresh:
        assert frozen[key].dtype == fresh[key].dtype and frozen[key].tobytes() == np.asarray(fresh[key]).tobytes(), key
    first = int(frozen["first_pair"])
    a = twin["offsets"][first]
    assert (twin["offsets"][first:] - a).tobytes() == frozen["offsets"].tobytes()
    assert twin["distance"][a:].tobytes() == frozen["distance"].tobytes() and twin["index"][a:].tobytes() == frozen["index"].tobytes()
    for key in ("rows", "finite", "within", "sum", "sum_sq", "max"):
        assert twin["fit"][key][first:].tobytes() == frozen["fit_" + key].tobytes(), key
    assert os.path.getsize(U.GOLDEN) < 100_000


# One record: int64 St, Sq, P, grid_k; float64 max_distance, tau; then t_offsets [St + 1], q_offsets [Sq + 1], pairs [P, 2], out_offsets
# [P + 1] (int64), t_xyz [Nt, 3], q_xyz [Nq, 3] (float64) -> distance [M] float64, index [M] int64, evals [M] int32, then rows, finite,
# within [P] int64 and sum, sum_sq, max [P] float64.  Every buffer is a heap block of exactly its size.
DRIVER = r"""
#include "cloud_distance_core.h"
#include <cstdio>
#include <cstdlib>
template <typename T> static T *block(int64_t n) { return (T *)malloc((size_t)(n > 0 ? n : 1) * sizeof(T)); }
template <typename T> static bool get(T *p, int64_t n) { return fread(p, sizeof(T), (size_t)n, stdin) == (size_t)n; }
template <typename T> static void put(const T *p, int64_t n) { fwrite(p, sizeof(T), (size_t)n, stdout); }
int main() {
    int64_t head[4];
    double knobs[2];
    while (fread(head, 8, 4, stdin) == 4) {
        const int64_t St = head[0], Sq = head[1], P = head[2];
        if (!get(knobs, 2)) return 4;
        int64_t *t_off = block<int64_t>(St + 1), *q_off = block<int64_t>(Sq + 1), *pairs = block<int64_t>(2 * P), *out_off = block<int64_t>(P + 1);
        if (!get(t_off, St + 1) || !get(q_off, Sq + 1) || !get(pairs, 2 * P) || !get(out_off, P + 1)) return 5;
        const int64_t Nt = mspa::segs::batch_rows(t_off, St), Nq = mspa::segs::batch_rows(q_off, Sq);
        int64_t *check = block<int64_t>(P + 1);
        const int64_t M = mspa::cdist::pair_rows(q_off, Sq, St, pairs, P, check);
        if (Nt < 0 || Nq < 0 || M < 0) return 6;
        for (int64_t p = 0; p <= P; ++p)
            if (check[p] != out_off[p]) return 7;
        double *t = block<double>(3 * Nt), *q = block<double>(3 * Nq), *distance = block<double>(M);
        int64_t *index = block<int64_t>(M);
        int32_t *evals = block<int32_t>(M);
        if (!get(t, 3 * Nt) || !get(q, 3 * Nq)) return 8;
        if (!mspa::cdist::nearest_segments_all(t, t_off, St, q, q_off, pairs, P, out_off, (int32_t)head[3], mspa::cdist::cap2_of(knobs[0]), distance,
                                               index, evals))
            return 9;
        int64_t *rows = block<int64_t>(P), *finite = block<int64_t>(P), *within = block<int64_t>(P);
        double *sum = block<double>(P), *sum_sq = block<double>(P), *max = block<double>(P);
        mspa::cdist::fit_segments_all(distance, out_off, P, knobs[1], rows, finite, within, sum, sum_sq, max);
        put(distance, M), put(index, M), put(evals, M), put(rows, P), put(finite, P), put(within, P), put(sum, P), put(sum_sq, P), put(max, P);
        void *all[] = {t_off, q_off, pairs, out_off, check, t, q, distance, index, evals, rows, finite, within, sum, sum_sq, max};
        for (void *p : all) free(p);
    }
    return 0;
}
"""


def test_the_headers_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    from mspa import cloud_segments as CS
    (tmp_path / "driver.cpp").write_text(DRIVER)
    exe = str(tmp_path / "driver")
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", CSRC, str(tmp_path / "driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    t, t_off, q, q_off, pairs = U.batch()
    offsets = U.batch_oracle()[2]
    none = np.zeros((0, 3))
    records = [(t, t_off, q, q_off, pairs, offsets, 8, np.inf, U.TAU), (t, t_off, q, q_off, pairs, offsets, 1, 0.05, 0.01),
               (t, t_off, q, q_off, pairs[:13], offsets[:14], 64, 3.0, 0.0),
               (none, np.array([0, 0]), q[:7], np.array([0, 7]), np.array([[0, 0]]), np.array([0, 7]), 8, np.inf, 1.0),
               (none, np.array([0]), none, np.array([0]), np.zeros((0, 2)), np.array([0]), 8, np.inf, 1.0)]
    i8 = lambda x: np.asarray(x, dtype="<i8").tobytes()                      # noqa: E731
    f8 = lambda x: np.asarray(x, dtype="<f8").tobytes()                      # noqa: E731
    inp = b"".join(struct.pack("<qqqqdd", len(to) - 1, len(qo) - 1, len(pr), k, cap, tau) + i8(to) + i8(qo) + i8(pr) + i8(oo) + f8(tx) + f8(qx)
                   for tx, to, qx, qo, pr, oo, k, cap, tau in records)
    run = subprocess.run([exe], input=inp, capture_output=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:].decode(errors="replace"))
    at = 0

    def take(count, dtype):
        nonlocal at
        got = np.frombuffer(run.stdout, dtype=dtype, count=count, offset=at)
        at += got.nbytes
        return got

    for tx, to, qx, qo, pr, oo, k, cap, tau in records:
        M, P = int(oo[-1]), len(pr)
        distance, index, evals = take(M, "<f8"), take(M, "<i8"), take(M, "<i4")
        want = CS.nearest_segments_host(qx, qo, tx, to, pr, None if np.isinf(cap) else cap, want_evals=True, _grid_k=k)
        assert distance.tobytes() == want["distance"].tobytes() and index.tobytes() == want["index"].tobytes() and evals.tobytes() == want["evals"].tobytes()
        fit = CS.fit_segments_host(want["distance"], want["offsets"], tau)
        for key in CS.FIT_KEYS:
            assert take(P, "<i8" if key in CS.FIT_KEYS[:3] else "<f8").tobytes() == fit[key].tobytes(), key
    assert at == len(run.stdout)
