"""The k nearest rows and the normals of a ragged batch on the device (``mspa.cloud_segments.knn_segments``, ``normals_segments``,
``ops.estimate_normals``, ``InstanceClouds.normals``) against the host twin and the frozen fixture of tests/golden/cloud_normals.npz,
BYTE FOR BYTE: the neighbour table, ``normal``, ``curvature``, ``used`` and ``status`` -- on the batch of tests/cloud_normals_util.py,
run twice, with and without viewpoints (host and device), the cap and the table, from views that are not contiguous and from float32
rows; ``InstanceClouds.normals`` on hand-made views and on the synthetic scene of tests/test_gpu_instance_boxes.py; and the existing
per-scene outputs with their default arguments, unchanged."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_normals_util as U  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("normal", "curvature", "used", "status")
TABLE = ("index", "distance")


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def _same(got: dict, want: dict, keys):
    for key in keys:
        a, b = np.ascontiguousarray(_np(got[key])), np.ascontiguousarray(want[key])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), key


def CS():
    from mspa import cloud_segments
    return cloud_segments


@pytest.mark.parametrize("k", [1, 3, U.K, 30, 64])
def test_knn_segments_is_the_twin_byte_for_byte_twice(k):
    xyz, off, _names = U.batch()
    rows = _dev(xyz)
    for cap in (None, U.CAP):
        index, distance = CS().knn_segments_host(xyz, off, k, cap)
        for _ in range(2):
            got_index, got_distance = CS().knn_segments(rows, off, k, cap)
            _same({"index": got_index, "distance": got_distance}, {"index": index, "distance": distance}, TABLE)
    if k == U.K:                                                             # and the brute force's, through the twin's own test
        assert np.array_equal(index, U.brute(U.CAP)[0])


def test_normals_segments_is_the_twin_and_the_fixture_byte_for_byte_twice():
    xyz, off, _names = U.batch()
    views = U.viewpoints()
    rows = _dev(xyz)
    for cap in (None, U.CAP):
        for given in (None, views, _dev(views)):                             # none, host or device
            twin = CS().normals_segments_host(xyz, off, U.K, cap, None if given is None else views, want_neighbours=True)
            for _ in range(2):
                _same(CS().normals_segments(rows, off, U.K, cap, given, want_neighbours=True), twin, KEYS + TABLE)
            plain = CS().normals_segments(rows, off, U.K, cap, given)        # without the table: the same walk, the same bytes
            _same(plain, twin, KEYS)
            assert sorted(plain) == sorted(KEYS)
    for k in (30, 64):                                                       # the default and the largest list
        _same(CS().normals_segments(rows, off, k, viewpoints=views), CS().normals_segments_host(xyz, off, k, viewpoints=views), KEYS)
    frozen = U.golden()
    fx, foff, fviews = U.fixture_batch()
    got = CS().normals_segments(_dev(fx), foff, U.K, None, fviews)
    _same(got, {k: frozen["viewed_" + k] for k in KEYS}, KEYS)
    capped = CS().normals_segments(_dev(fx), foff, U.K, U.CAP)
    _same(capped, {"used": frozen["capped_used"], "status": frozen["capped_status"]}, ("used", "status"))
    index, distance = CS().knn_segments(_dev(fx), foff, 3)
    assert np.array_equal(_np(index), frozen["table_index"].astype(np.int64)) and _np(distance).tobytes() == frozen["table_distance"].tobytes()


def test_the_exact_plane_on_the_device():
    xyz, off, _names = U.batch()
    out = CS().normals_segments(_dev(xyz), off, U.K)
    for name in ("lattice", "lattice twice"):
        _s, a, b = U.segment(name)
        assert _np(out["normal"][a:b]).tobytes() == np.tile([0.0, 0.0, 1.0], (b - a, 1)).tobytes() and not _np(out["curvature"][a:b]).any()


def test_views_that_are_not_contiguous_and_float32_rows():
    xyz, off, names = U.batch()
    views = U.viewpoints()
    twin = CS().normals_segments_host(xyz, off, U.K, None, views, want_neighbours=True)
    wide = torch.zeros((len(xyz), 7), dtype=torch.float64, device="cuda")
    wide[:, :3] = _dev(xyz)
    wide[:, 3:] = float("nan")                                               # the other columns are not read
    wide_views = torch.zeros((len(names), 5), dtype=torch.float64, device="cuda")
    wide_views[:, 1:4] = _dev(views)
    _same(CS().normals_segments(wide, off, U.K, None, wide_views[:, 1:4], want_neighbours=True), twin, KEYS + TABLE)
    strided = torch.zeros((2 * len(xyz), 3), dtype=torch.float64, device="cuda")
    strided[::2] = _dev(xyz)
    _same(CS().normals_segments(strided[::2], off, U.K, None, views), twin, KEYS)
    narrow = U.float32_rows()
    _same(CS().normals_segments(_dev(narrow), off, U.K), CS().normals_segments_host(narrow, off, U.K), KEYS)


def test_the_value_errors_and_the_empty_shapes():
    xyz, off, names = U.batch()
    rows = _dev(xyz)
    for kw in ({"k": 0}, {"k": 65}, {"max_distance": 0.0}, {"max_distance": np.inf}, {"viewpoints": np.zeros((3, 3))},
               {"viewpoints": torch.zeros((len(names), 3), dtype=torch.float64)[:, :2]}):
        with pytest.raises(ValueError):
            CS().normals_segments(rows, off, **kw)
    with pytest.raises(ValueError):
        CS().knn_segments(xyz, off, 3)                                       # not a device tensor
    with pytest.raises(ValueError):
        CS().knn_segments(rows, off[:-2], 3)
    bad = rows.clone()
    bad[17, 1] = float("nan")
    with pytest.raises(ValueError, match="finite coordinates"):
        CS().normals_segments(bad, off)
    none = torch.zeros((0, 3), dtype=torch.float64, device="cuda")
    for offsets in ([0], [0, 0, 0]):
        out = CS().normals_segments(none, offsets, 7, want_neighbours=True)
        assert out["normal"].shape == (0, 3) and out["index"].shape == (0, 7) and out["status"].dtype == torch.uint8


def test_estimate_normals_on_numpy_and_device_input():
    from spatial_engine.utils.scannet_utils.handler import ops
    xyz, _off, _names = U.batch()
    for name, view, radius in (("slab 257", None, None), ("sphere in", [0.0, 0.0, 0.0], None), ("slab 1025", [0.0, 0.0, 5.0], 0.08)):
        _s, a, b = U.segment(name)
        cloud = xyz[a:b]
        want = CS().normals_segments_host(cloud, [0, b - a], 30, radius, None if view is None else np.array([view]))["normal"]
        host = ops.estimate_normals(cloud, radius=radius, camera_location=view)
        assert isinstance(host, np.ndarray) and host.tobytes() == want.tobytes(), name
        for location in (view, None if view is None else torch.tensor(view, dtype=torch.float64, device="cuda")):
            got = ops.estimate_normals(_dev(cloud), radius=radius, camera_location=location)
            assert got.is_cuda and _np(got).tobytes() == want.tobytes(), name
        on_host = ops.estimate_normals(torch.from_numpy(cloud.copy()), 30, radius, view)
        assert isinstance(on_host, torch.Tensor) and not on_host.is_cuda and on_host.numpy().tobytes() == want.tobytes()
    _s, a, b = U.segment("sphere in")
    assert (np.einsum("ij,ij->i", ops.estimate_normals(xyz[a:b], 10, camera_location=[0.0, 0.0, 0.0]), xyz[a:b]) < 0).all()
    assert "not checked against Open3D" in " ".join(ops.estimate_normals.__doc__.split())


def test_instance_clouds_normals_on_hand_made_views():
    from mspa.instances import InstanceClouds
    xyz, off, names = U.batch()
    at = [names.index(n) for n in ("slab 257", "sphere in", "slab 64", "far plane")]        # frame 0: labels 1, 2; frame 1: labels 1, 2
    L = 3
    counts = np.zeros((2, L), dtype=np.int64)
    parts = []
    for slot, s in zip(((0, 1), (0, 2), (1, 1), (1, 2)), at):
        counts[slot] = off[s + 1] - off[s]
        parts.append(xyz[off[s]:off[s + 1]])
    rows = np.concatenate(parts)
    inf = torch.full((2, L, 3), float("inf"), dtype=torch.float64, device="cuda")
    centres = np.array([[0.0, 0.0, 0.0], [np.nan, np.nan, np.nan]])          # frame 1 has no centre: unoriented
    clouds = InstanceClouds([10, 11], counts, _dev(rows), None, inf, -inf, centres=centres)
    got = clouds.normals(k=U.K)
    want = CS().normals_segments_host(rows, clouds.offsets, U.K, None, np.repeat(centres, L, axis=0))
    _same(got, want, KEYS)
    a, b = int(clouds.offsets[2]), int(clouds.offsets[3])                    # the sphere seen from its centre
    assert (np.einsum("ij,ij->i", _np(got["normal"][a:b]), rows[a:b]) < 0).all()
    bare = InstanceClouds([10, 11], counts, _dev(rows), None, inf, -inf)     # made without centres: unoriented everywhere
    assert bare.centres is None
    _same(bare.normals(k=U.K, max_distance=0.3), CS().normals_segments_host(rows, clouds.offsets, U.K, 0.3), KEYS)
    assert clouds.cleaned(20, 1.0).centres.tobytes() == clouds.centres.tobytes()


def test_instance_clouds_normals_on_the_synthetic_scene_and_the_default_outputs_unchanged(tmp_path):
    from test_gpu_instance_boxes import _annotate, _synth_scene
    ns, h, sid, ids, _with_color, n_objects = _synth_scene(str(tmp_path))
    clouds = h.instance_clouds(sid, with_color=False)
    A = np.asarray(h.get_world_to_axis_align_matrix(sid), np.float64)
    want_centres = np.stack([(A @ np.asarray(h.get_extrinsic_matrix(sid, i), np.float64))[:3, 3] for i in ids])
    assert clouds.centres.tobytes() == want_centres.tobytes()
    got = clouds.normals(k=8)
    rows = _np(clouds.rows)
    want = CS().normals_segments_host(rows, clouds.offsets, 8, None, np.repeat(want_centres, clouds.n_labels, axis=0))
    _same(got, want, KEYS)
    ok = want["status"] == U.OK
    assert ok.sum() > 1000
    frame = np.searchsorted(clouds.offsets, np.arange(len(rows)), side="right") - 1
    towards = np.einsum("ij,ij->i", want_centres[frame // clouds.n_labels] - rows[:, :3], want["normal"])
    assert (towards[ok] >= 0).all()                                          # every normal faces its frame's camera
    # the centres leak into nothing: the same calls on an InstanceClouds made WITHOUT them give the same keys and bytes.  Both sides are
    # this tree's code, so this does not show equality with the outputs of the tree before -- that is what the untouched
    # tests/test_gpu_instance_boxes.py and tests/test_gpu_cloud_align.py hold, against the single-cloud loop and the host twin
    from mspa.instances import InstanceClouds
    bare = InstanceClouds(clouds.image_ids, clouds.counts, clouds.rows, clouds.pixel, clouds.lo, clouds.hi, clouds.rgb)
    a, b = clouds.view_alignment(0.05, voxel_size=0.02, iterations=3), bare.view_alignment(0.05, voxel_size=0.02, iterations=3)
    assert sorted(a) == sorted(b) == ["R", "angle", "fitness", "inlier_rmse", "shift", "status", "t"]
    for key in a:
        assert _np(a[key]).tobytes() == _np(b[key]).tobytes(), key
    _annotate(h, sid, clouds, n_objects)
    boxes = h.instance_boxes(sid)
    assert sorted(boxes) == ["boxes", "image_ids", "iou", "kept"]
    assert _np(boxes["boxes"]).tobytes() == _np(bare.cleaned(20, 1.0).boxes()).tobytes()


# ---- point-to-plane (csrc/cloud_align_plane.hip) --------------------------------------------------------------------------------------

PLANE_KEYS = ("R", "t", "status", "used", "converged_at", "fitness", "inlier_rmse")
STEP_KEYS = ("R", "t", "status", "used", "rmse")


def test_plane_fit_segments_is_the_twin_and_the_fixture_byte_for_byte_twice():
    q, q_off, t, t_off, _truth, normals = U.plane_batch()
    frozen = U.golden()
    found = CS().nearest_segments_host(q, q_off, t, t_off, None, 0.05)["index"]
    twin = CS().plane_fit_segments_host(q, q_off, t, normals, found)
    rng = np.random.default_rng(4)
    init = np.concatenate([np.tile(np.eye(3), (5, 1, 1)), rng.random((5, 3, 1)) * 0.002], axis=2)
    moved = CS().plane_fit_segments_host(q, q_off, t, normals, found, init=init)
    for _ in range(2):
        got = CS().plane_fit_segments(_dev(q), q_off, _dev(t), _dev(normals), _dev(found))
        _same(got, twin, STEP_KEYS)
        _same(got, {k: frozen["step_" + k] for k in STEP_KEYS}, STEP_KEYS)
        for given in (init, _dev(init)):                                     # host or device
            _same(CS().plane_fit_segments(_dev(q), q_off, _dev(t), _dev(normals), _dev(found), init=given), moved, STEP_KEYS)
    wide_q, wide_n = torch.zeros((len(q), 6), dtype=torch.float64, device="cuda"), torch.zeros((len(t), 5), dtype=torch.float64, device="cuda")
    wide_q[:, :3], wide_n[:, 1:4] = _dev(q), _dev(normals)                   # views that are not contiguous
    strided = torch.zeros((2 * len(q),), dtype=torch.int64, device="cuda")
    strided[::2] = _dev(found)
    _same(CS().plane_fit_segments(wide_q, q_off, _dev(t), wide_n[:, 1:4], strided[::2]), twin, STEP_KEYS)
    fq, ft, fn = U.flat_case()                                               # a flat target: DEGENERATE, init kept
    flat = CS().plane_fit_segments(_dev(fq), [0, len(fq)], _dev(ft), _dev(fn), _dev(np.arange(len(fq), dtype=np.int64)))
    _same(flat, CS().plane_fit_segments_host(fq, [0, len(fq)], ft, fn, np.arange(len(fq), dtype=np.int64)), STEP_KEYS)
    assert _np(flat["status"]).tolist() == [U.DEGENERATE] and _np(flat["R"]).tobytes() == np.eye(3)[None].tobytes()
    for rows in (0, 5, 6, 255, 256, 257):                                    # around FEW and the workgroup's 256
        index = np.arange(rows, dtype=np.int64) % len(t)
        rq = np.tile(t, (2, 1))[:rows] + 0.001
        _same(CS().plane_fit_segments(_dev(rq), [0, rows], _dev(t), _dev(normals), _dev(index)),
              CS().plane_fit_segments_host(rq, [0, rows], t, normals, index), STEP_KEYS)


def test_register_point_to_plane_is_the_twin_and_the_fixture_byte_for_byte_twice_and_sync_every_is_the_plain_loop():
    q, q_off, t, t_off, _truth, normals = U.plane_batch()
    frozen = U.golden()
    kw = dict(max_distance=0.05, iterations=U.PLANE_ITERATIONS, estimation="point_to_plane")
    twin = CS().register_segments_host(q, q_off, t, t_off, normals=normals, want_history=True, **kw)
    index = CS().target_index(_dev(t), t_off)
    for _ in range(2):
        got = index.register(_dev(q), q_off, normals=_dev(normals), want_history=True, **kw)
        _same(got, twin, PLANE_KEYS + ("history_used", "history_rmse"))
        _same(got, {k: frozen["plane_" + k] for k in PLANE_KEYS}, PLANE_KEYS)
    synced = index.register(_dev(q), q_off, normals=_dev(normals), sync_every=5, **kw)
    _same(synced, twin, PLANE_KEYS)
    assert synced["all_converged"] is False
    init = np.tile(np.eye(3, 4), (5, 1, 1))
    init[:, :, 3] = 0.001
    want = CS().register_segments_host(q, q_off, t, t_off, normals=normals, init=init, **kw)
    for given in (init, _dev(init)):
        _same(CS().register_segments(_dev(q), q_off, _dev(t), t_off, normals=_dev(normals), init=given, **kw), want, PLANE_KEYS)
    own = CS().register_segments(_dev(t), t_off, _dev(t), t_off, normals=_dev(normals), **kw)       # a cloud against itself: the identity exactly
    assert _np(own["R"]).tobytes() == np.tile(np.eye(3), (5, 1, 1)).tobytes() and not _np(own["t"]).any() and not _np(own["converged_at"]).any()
    # the default is the point-to-point loop, byte for byte
    a = index.register(_dev(q), q_off, max_distance=0.05, iterations=6)
    b = index.register(_dev(q), q_off, max_distance=0.05, iterations=6, estimation="point_to_point")
    _same(a, {k: _np(v) for k, v in b.items() if k != "offsets"}, PLANE_KEYS)
    with pytest.raises(ValueError):
        index.register(_dev(q), q_off, max_distance=0.05, estimation="point_to_plane")
    with pytest.raises(ValueError):
        index.register(_dev(q), q_off, max_distance=0.05, normals=_dev(normals))
    with pytest.raises(ValueError):
        index.register(_dev(q), q_off, max_distance=0.05, estimation="point_to_plane", normals=normals)      # a host array


def test_registration_icp_point_to_plane_on_numpy_and_device_input():
    import cloud_align_util as A
    from spatial_engine.utils.scannet_utils.handler import ops
    q, q_off, t, t_off, truth, normals = U.plane_batch()
    src, tgt, nrm = q[q_off[A.EASY]:q_off[A.EASY + 1]], t[t_off[A.EASY]:t_off[A.EASY + 1]], normals[t_off[A.EASY]:t_off[A.EASY + 1]]
    host = ops.registration_icp(src, tgt, 0.05, max_iteration=U.PLANE_ITERATIONS, estimation="point_to_plane", target_normals=nrm)
    assert np.abs(host["transformation"][:3, :3] - truth[A.EASY][0]).max() < 1e-12
    for given in (nrm, _dev(nrm), None):                                     # given on the host, on the device, or estimated at k = 30
        got = ops.registration_icp(_dev(src), _dev(tgt), 0.05, max_iteration=U.PLANE_ITERATIONS, estimation="point_to_plane", target_normals=given)
        assert got["transformation"].is_cuda and _np(got["transformation"]).tobytes() == host["transformation"].tobytes()
        assert float(got["fitness"]) == host["fitness"] and _np(got["inlier_rmse"]).tobytes() == np.asarray(host["inlier_rmse"]).tobytes()
    plain = ops.registration_icp(_dev(src), _dev(tgt), 0.05, max_iteration=4)
    keyed = ops.registration_icp(_dev(src), _dev(tgt), 0.05, max_iteration=4, estimation="point_to_point")
    assert _np(plain["transformation"]).tobytes() == _np(keyed["transformation"]).tobytes()
