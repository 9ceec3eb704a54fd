"""Nearest-point distances between the clouds of two ragged batches on the device (``mspa.cloud_segments.target_index`` /
``TargetIndex.nearest`` / ``fit_segments`` / ``cloud_fit_segments``, ``ops.compute_point_cloud_distance``,
``InstanceClouds.view_coverage``, ``instance_boxes(coverage=...)``) against the host twin, the NumPy brute force and the frozen fixture of
tests/cloud_distance_util.py -- byte for byte, twice."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_distance_util as U  # noqa: E402

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def _same(got: dict, want: dict, keys=("distance", "index", "evals")):
    for key in keys:
        assert _np(got[key]).dtype == want[key].dtype and _np(got[key]).tobytes() == want[key].tobytes(), key
    assert got["offsets"].tobytes() == want["offsets"].tobytes()


@pytest.fixture(scope="module")
def index():
    from mspa import cloud_segments as CS
    t, t_off, _q, _q_off, _pairs = U.batch()
    return CS.target_index(_dev(t), t_off)


def test_the_device_is_the_twin_and_the_fixture_byte_for_byte_twice(index):
    from mspa import cloud_segments as CS
    t, t_off, q, q_off, pairs = U.batch()
    twin, frozen = U.batch_twin(), U.golden()
    distance, order, _offsets = U.batch_oracle()
    q_dev = _dev(q)
    for _ in range(2):
        out = index.nearest(q_dev, q_off, pairs, want_evals=True)
        _same(out, twin)
        assert _np(out["distance"]).tobytes() == distance.tobytes() and _np(out["index"]).tobytes() == order.tobytes()
        fit = CS.fit_segments(out["distance"], out["offsets"], U.TAU)
        for key in CS.FIT_KEYS:
            assert _np(fit[key]).dtype == twin["fit"][key].dtype and _np(fit[key]).tobytes() == twin["fit"][key].tobytes(), key
        first = int(frozen["first_pair"])
        a = out["offsets"][first]
        assert _np(out["distance"])[a:].tobytes() == frozen["distance"].tobytes() and _np(out["index"])[a:].tobytes() == frozen["index"].tobytes()
        for key in CS.FIT_KEYS:
            assert _np(fit[key])[first:].tobytes() == frozen["fit_" + key].tobytes(), key
    fresh = CS.nearest_segments(q_dev, q_off, _dev(t), t_off, pairs, want_evals=True)           # a second index: the same bits
    _same(fresh, twin)
    none = index.nearest(q_dev, q_off, want_evals=True)                                          # pair s is (s, s)
    _same(none, CS.nearest_segments_host(q, q_off, t, t_off, want_evals=True))
    for ordered in (False, True):                                           # which lane computes a row changes no byte
        _same(index.nearest(q_dev, q_off, pairs, max_distance=0.3, want_evals=True, _ordered=ordered),
              CS.nearest_segments_host(q, q_off, t, t_off, pairs, max_distance=0.3, want_evals=True))
        _same(index.nearest(q_dev, q_off, pairs, want_evals=True, _ordered=ordered), twin)
    without = index.nearest(q_dev, q_off, pairs, want_index=False)
    assert sorted(without) == ["distance", "offsets"] and _np(without["distance"]).tobytes() == twin["distance"].tobytes()


@pytest.mark.parametrize("cap", [0.05, 1e-3, 3.0])
@pytest.mark.parametrize("grid_k", [None, 1, 64])
def test_caps_and_grid_sizes_give_the_twins_bytes(cap, grid_k):
    from mspa import cloud_segments as CS
    t, t_off, q, q_off, pairs = U.batch()
    got = CS.nearest_segments(_dev(q), q_off, _dev(t), t_off, pairs, max_distance=cap, want_evals=True, _grid_k=grid_k)
    _same(got, CS.nearest_segments_host(q, q_off, t, t_off, pairs, max_distance=cap, want_evals=True, _grid_k=grid_k))
    distance, order, _offsets = U.oracle(t, t_off, q, q_off, pairs, max_distance=cap)
    assert _np(got["distance"]).tobytes() == distance.tobytes() and _np(got["index"]).tobytes() == order.tobytes()


@pytest.mark.parametrize("rows", [0, 1, 63, 64, 65, 256, 257, 1025])
def test_every_count_of_output_rows(index, rows):
    from mspa import cloud_segments as CS
    t, t_off, _q, _q_off, _pairs = U.batch()
    q = np.random.default_rng(rows).random((rows, 3)) * 1.2 - 0.1
    q_off = np.array([0, rows], dtype=np.int64)
    pairs = np.array([[0, 7]], dtype=np.int64)
    out = index.nearest(_dev(q), q_off, pairs, want_evals=True)
    _same(out, CS.nearest_segments_host(q, q_off, t, t_off, pairs, want_evals=True))
    fit = CS.fit_segments(out["distance"], out["offsets"], U.TAU)
    want = CS.fit_segments_host(_np(out["distance"]), out["offsets"], U.TAU)
    for key in CS.FIT_KEYS:
        assert _np(fit[key]).tobytes() == want[key].tobytes(), key
    assert int(fit["rows"][0]) == rows


def test_views_that_are_not_contiguous_and_float32_rows_widened(index):
    from mspa import cloud_segments as CS
    t, t_off, q, q_off, pairs = U.batch()
    twin = U.batch_twin()
    wide = torch.zeros((2 * len(q), 7), dtype=torch.float64, device="cuda")
    wide[::2, :3] = _dev(q)
    view = wide[::2, :6]                                                     # every second row, six of seven columns
    assert not view.is_contiguous()
    _same(index.nearest(view, q_off, pairs, want_evals=True), twin)
    t_wide = torch.zeros((len(t), 5), dtype=torch.float64, device="cuda")
    t_wide[:, :3] = _dev(t)
    _same(CS.target_index(t_wide[:, :4], t_off).nearest(view, q_off, pairs, want_evals=True), twin)
    finite = np.where(np.isfinite(q), q, 0.5)
    q32, t32 = finite.astype(np.float32), t.astype(np.float32)
    got = CS.nearest_segments(_dev(q32), q_off, _dev(t32), t_off, pairs, want_evals=True)
    _same(got, CS.nearest_segments_host(q32.astype(np.float64), q_off, t32.astype(np.float64), t_off, pairs, want_evals=True))
    with pytest.raises(ValueError, match="finite coordinates"):
        CS.target_index(_dev(np.where(np.arange(len(t))[:, None] == 70, np.nan, t)), t_off)


def test_one_index_queried_three_times_with_different_pair_tables(index):
    from mspa import cloud_segments as CS
    t, t_off, q, q_off, pairs = U.batch()
    q_dev = _dev(q)
    tables = [pairs[::-1].copy(), np.array([[7, 7]] * 3 + [[3, 7], [7, 3]], dtype=np.int64), np.zeros((0, 2), dtype=np.int64)]
    for table in tables:
        out = index.nearest(q_dev, q_off, table, want_evals=True)
        _same(out, CS.nearest_segments_host(q, q_off, t, t_off, table, want_evals=True))
    empty_side = CS.target_index(torch.zeros((0, 3), dtype=torch.float64, device="cuda"), np.zeros((14,), dtype=np.int64))
    out = empty_side.nearest(q_dev, q_off)
    assert torch.isposinf(out["distance"][torch.isfinite(q_dev).all(dim=1)]).all() and (out["index"] == -1).all()


def test_cloud_fit_segments_is_the_composition_of_its_parts():
    from mspa import cloud_segments as CS
    t, t_off, q, q_off, _pairs = U.batch()
    q = np.where(np.isfinite(q), q, 0.5)                                     # both sides become targets: finite
    a, b = _dev(q), _dev(t)
    for cap in (None, 0.2):
        got = CS.cloud_fit_segments(a, q_off, b, t_off, U.TAU, max_distance=cap)
        want = CS.cloud_fit_segments_host(q, q_off, t, t_off, U.TAU, max_distance=cap)
        for side in ("a_to_b", "b_to_a"):
            for key in CS.FIT_KEYS:
                assert _np(got[side][key]).tobytes() == want[side][key].tobytes(), (side, key)
        ab = CS.fit_segments(CS.nearest_segments(a, q_off, b, t_off, max_distance=cap)["distance"], q_off, U.TAU)
        assert _np(got["precision"]).tobytes() == _np(ab["within"].double() / ab["rows"].double()).tobytes()
        for key in ("precision", "recall", "fscore", "chamfer"):
            assert _np(got[key]).tobytes() == want[key].tobytes(), key
        assert np.isnan(_np(got["precision"])[4]) and np.isnan(_np(got["recall"])[0]) and np.isfinite(_np(got["fscore"])[7])


def test_compute_point_cloud_distance_with_numpy_and_with_device_input():
    from spatial_engine.utils.scannet_utils.handler import ops
    t, t_off, q, q_off, _pairs = U.batch()
    source, target = q[q_off[7]:q_off[8]], t[t_off[7]:t_off[8]]
    want = U.brute(source, target)[0]
    on_host = ops.compute_point_cloud_distance(source, target)
    assert isinstance(on_host, np.ndarray) and on_host.tobytes() == want.tobytes()
    on_device = ops.compute_point_cloud_distance(_dev(source), _dev(target))
    assert isinstance(on_device, torch.Tensor) and on_device.is_cuda and _np(on_device).tobytes() == want.tobytes()
    mixed = ops.compute_point_cloud_distance(_dev(source), target)
    assert mixed.is_cuda and _np(mixed).tobytes() == want.tobytes()


def _hand_made_clouds():
    """Two frames, labels 0 .. 2: frame 0 shows all 600 rows of object 0 (label 1), frame 1 the half of them with x < 0.5; object 1
    (label 2) is in frame 1 alone."""
    from mspa.instances import InstanceClouds
    rng = np.random.default_rng(11)
    whole = rng.random((600, 3))
    half = whole[whole[:, 0] < 0.5]
    other = rng.random((50, 3)) + 5.0
    counts = np.array([[0, len(whole), 0], [0, len(half), len(other)]], dtype=np.int64)
    rows = _dev(np.concatenate([whole, half, other]))
    lo = torch.full((2, 3, 3), float("inf"), dtype=torch.float64, device="cuda")
    fused = np.concatenate([whole, half])                                    # object 0 over both frames
    return InstanceClouds([10, 20], counts, rows, None, lo, -lo), np.float64((U.brute(fused, half)[0] <= 0.01).sum()) / np.float64(len(fused))


def test_a_frame_that_shows_the_whole_object_scores_above_one_that_shows_half():
    clouds, share = _hand_made_clouds()
    coverage = _np(clouds.view_coverage(0.01))
    assert coverage.shape == (2, 3) and np.isnan(coverage[:, 0]).all() and np.isnan(coverage[0, 2])
    assert coverage[0, 1] == 1.0 and coverage[1, 2] == 1.0
    assert coverage[1, 1] == share and 0.5 < share < 0.8                     # the half's rows stand twice among the fused 600 + half
    thinned = _np(clouds.view_coverage(0.05, voxel_size=0.05))
    assert thinned[0, 1] > thinned[1, 1] > 0.2 and thinned[0, 1] > 0.9


def _coverage_twin(clouds, tau, voxel_size):
    """``view_coverage`` from the downloaded clouds through the host twins, pairs built here."""
    from mspa import cloud_segments as CS
    fused, fused_off, object_ids = clouds.by_object(voxel_size)
    F, L = clouds.counts.shape
    pairs, where = [], []
    for k in range(F):
        for j, t in enumerate(object_ids):
            if clouds.counts[k, t + 1]:
                pairs.append((j, k * L + t + 1))
                where.append((k, t + 1))
    found = CS.nearest_segments_host(_np(fused), fused_off, _np(clouds.rows), clouds.offsets, np.array(pairs, dtype=np.int64).reshape(-1, 2),
                                     max_distance=tau)
    fit = CS.fit_segments_host(found["distance"], found["offsets"], tau)
    out = np.full((F, L), np.nan)
    for (k, v), within, rows in zip(where, fit["within"], fit["rows"]):
        out[k, v] = np.float64(within) / np.float64(rows)
    return out


def test_view_coverage_and_instance_boxes_on_the_synthetic_scene(tmp_path):
    from test_gpu_instance_boxes import NB, RATIO, _annotate, _synth_scene
    _ns, h, sid, _ids, _with_color, n_objects = _synth_scene(str(tmp_path))
    clouds = h.instance_clouds(sid)
    _annotate(h, sid, clouds, n_objects)
    for tau, voxel_size in ((0.02, None), (0.05, 0.03)):
        got = _np(clouds.view_coverage(tau, voxel_size))
        want = _coverage_twin(clouds, tau, voxel_size)
        assert got.tobytes() == want.tobytes(), (tau, voxel_size)
        shown = clouds.counts > 0
        shown[:, 0] = False
        assert (np.isnan(got) == ~shown).all() and (got[shown] >= 0).all() and (got[shown] <= 1).all() and shown.sum() > 8
        assert voxel_size is not None or (got[shown] > 0).all()             # a frame's own rows are rows of the fused cloud
    plain = h.instance_boxes(sid, nb_neighbors=NB, std_ratio=RATIO)
    scored = h.instance_boxes(sid, nb_neighbors=NB, std_ratio=RATIO, coverage=(0.02, None))
    assert sorted(scored) == sorted(list(plain) + ["coverage"])
    for key, value in plain.items():
        if isinstance(value, torch.Tensor):
            assert _np(value).tobytes() == _np(scored[key]).tobytes(), key
        else:
            assert np.array_equal(np.asarray(value), np.asarray(scored[key])), key
    assert _np(scored["coverage"]).tobytes() == _np(clouds.view_coverage(0.02)).tobytes()
    with pytest.raises(ValueError, match="per='image'"):
        h.instance_boxes(sid, per="object", coverage=(0.02, None))
