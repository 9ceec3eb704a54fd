"""Rigid alignment of the clouds of two ragged batches on the device (``mspa.cloud_segments.rigid_fit_segments``,
``transform_segments``, ``TargetIndex.register``, ``register_segments``, ``ops.registration_icp``,
``InstanceClouds.view_alignment``) against the host twin and the frozen fixture of tests/golden/cloud_align.npz, BYTE FOR BYTE: ``R``, ``t``, ``used``, ``status``, the eigenvalues, ``converged_at``, ``fitness``,
``inlier_rmse`` and the history -- on the Kabsch batch, its variant and the ICP batch of tests/cloud_align_util.py, run twice, with the
lanes of the search in both orders, from views that are not contiguous; ``transform_segments`` on every count of rows around the
workgroup's 256; ``sync_every`` against the plain loop."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_align_util as U  # noqa: E402

pytestmark = pytest.mark.gpu
REG_KEYS = ("R", "t", "status", "used", "converged_at", "fitness", "inlier_rmse", "history_used", "history_rmse")


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


@pytest.fixture(scope="module")
def icp_index():
    _q, _q_off, t, t_off, _truth = U.icp()
    return CS().target_index(_dev(t), t_off)


def test_the_kabsch_batches_are_the_twin_and_the_fixture_byte_for_byte_twice():
    frozen = U.golden()
    q, p, off, _cases = U.kabsch()
    index = np.arange(len(q), dtype=np.int64)
    twin = CS().rigid_fit_segments_host(q, off, p, index, want_parts=True)
    vq, vq_off, vp, pairs, vindex, _out = U.kabsch_variant()
    vtwin = CS().rigid_fit_segments_host(vq, vq_off, vp, vindex, pairs, want_parts=True)
    keys = ("R", "t", "used", "status", "eigen")
    for _ in range(2):
        got = CS().rigid_fit_segments(_dev(q), off, _dev(p), _dev(index), want_parts=True)
        _same(got, twin, keys)
        _same(got, {k: frozen["kabsch_" + k] for k in keys}, keys)
        got = CS().rigid_fit_segments(_dev(vq), vq_off, _dev(vp), _dev(vindex), pairs, want_parts=True)
        _same(got, vtwin, keys)
        _same(got, {k: frozen["variant_" + k] for k in keys}, keys)
    assert got["offsets"].tobytes() == vtwin["offsets"].tobytes()


def test_init_is_kept_where_the_fit_is_not_ok_and_float32_rows_widen():
    q, p, off, cases = U.kabsch()
    rng = np.random.default_rng(3)
    init = rng.random((len(cases), 3, 4))
    index = np.arange(len(q), dtype=np.int64)
    twin = CS().rigid_fit_segments_host(q, off, p, index, init=init)
    for given in (init, _dev(init)):                                         # host or device
        _same(CS().rigid_fit_segments(_dev(q), off, _dev(p), _dev(index), init=given), twin, ("R", "t", "used", "status"))
    q32 = q.astype(np.float32)
    _same(CS().rigid_fit_segments(_dev(q32), off, _dev(p), _dev(index)), CS().rigid_fit_segments_host(q32, off, p, index), ("R", "t", "used", "status"))


def test_views_that_are_not_contiguous():
    q, p, off, _cases = U.kabsch()
    index = np.arange(len(q), dtype=np.int64)
    twin = CS().rigid_fit_segments_host(q, off, p, index)
    wide_q, wide_p = torch.zeros((len(q), 7), dtype=torch.float64, device="cuda"), torch.zeros((len(p), 5), dtype=torch.float64, device="cuda")
    wide_q[:, :3], wide_p[:, :3] = _dev(q), _dev(p)
    strided = torch.zeros((2 * len(q),), dtype=torch.int64, device="cuda")
    strided[::2] = _dev(index)
    got = CS().rigid_fit_segments(wide_q, off, wide_p, strided[::2])
    _same(got, twin, ("R", "t", "used", "status"))
    moved = CS().transform_segments(wide_q, off, got["R"].transpose(1, 2).contiguous().transpose(1, 2), got["t"])
    _same(moved, CS().transform_segments_host(q, off, twin["R"], twin["t"]), ("xyz",))


@pytest.mark.parametrize("rows", [0, 1, 63, 64, 65, 256, 257, 1025])
def test_transform_segments_on_every_count_of_rows(rows):
    rng = np.random.default_rng(rows)
    q = rng.random((rows + 5, 3)) * 10.0 - 5.0
    off = np.array([0, rows, rows, rows + 5], dtype=np.int64)
    R, t = rng.random((4, 3, 3)), rng.random((4, 3))
    pairs = np.array([[0, 0], [2, 1], [1, 1], [0, 2]], dtype=np.int64)
    got = CS().transform_segments(_dev(q), off, _dev(R), _dev(t), pairs)
    want = CS().transform_segments_host(q, off, R, t, pairs)
    _same(got, want, ("xyz",))
    assert got["offsets"].tolist() == [0, rows, rows + 5, rows + 5, 2 * rows + 5]
    fit = CS().rigid_fit_segments(_dev(q), off, _dev(q), _dev(np.arange(2 * rows + 5) % max(rows, 1)), pairs)
    _same(fit, CS().rigid_fit_segments_host(q, off, q, np.arange(2 * rows + 5) % max(rows, 1), pairs), ("R", "t", "used", "status"))


@pytest.mark.parametrize("cap", sorted(U.CAPS.values()))
def test_register_is_the_twin_and_the_fixture_byte_for_byte_twice_with_the_lanes_in_both_orders(icp_index, cap, monkeypatch):
    q, q_off, t, t_off, _truth = U.icp()
    frozen = U.golden()
    twin = CS().register_segments_host(q, q_off, t, t_off, max_distance=cap, iterations=12, want_history=True)
    for ordered in (True, False, True):
        monkeypatch.setattr(CS(), "ORDER_QUERIES", ordered)
        got = icp_index.register(_dev(q), q_off, max_distance=cap, iterations=12, want_history=True)
        _same(got, twin, REG_KEYS)
        _same(got, {k: frozen[f"icp{int(cap * 100)}_" + k] for k in REG_KEYS}, REG_KEYS)
    pair = {v: k for k, v in U.CAPS.items()}[cap]
    assert int(got["converged_at"][pair]) == U.icp_references()[(pair, False)]["fixed_at"]
    one_call = CS().register_segments(_dev(q), q_off, _dev(t), t_off, max_distance=cap, iterations=12, want_history=True)
    _same(one_call, twin, REG_KEYS)


def test_sync_every_is_the_plain_loop_and_an_index_without_its_targets_rebuilds_them(icp_index):
    q, q_off, _t, _t_off, _truth = U.icp()
    cap = U.CAPS[U.HARD]
    plain = icp_index.register(_dev(q), q_off, max_distance=cap, iterations=30, want_history=True)
    synced = icp_index.register(_dev(q), q_off, max_distance=cap, iterations=30, sync_every=5, want_history=True)
    _same(synced, {k: _np(v) for k, v in plain.items() if k in REG_KEYS}, REG_KEYS)
    assert synced["all_converged"] is True
    bare = CS().TargetIndex(icp_index.offsets, icp_index.grid_k, icp_index.grids, icp_index.off_dev, icp_index.grids_dev, icp_index.base_dev, icp_index.pts,
                            icp_index.order, icp_index.starts, icp_index.device)
    _same(bare.register(_dev(q), q_off, max_distance=cap, iterations=12), {k: _np(v) for k, v in plain.items() if k in REG_KEYS[:7]}, REG_KEYS[:7])
    init = torch.cat([plain["R"], plain["t"][:, :, None]], dim=2)            # from the answer, on the device: converged at once
    again = icp_index.register(_dev(q), q_off, max_distance=cap, iterations=2, init=init)
    assert _np(again["converged_at"]).tolist() == [0] * 5 and _np(again["R"]).tobytes() == _np(plain["R"]).tobytes()


def test_pairs_that_share_segments_and_empty_shapes(icp_index):
    q, q_off, t, t_off, _truth = U.icp()
    pairs = np.array([[1, 0], [0, 1], [1, 2], [1, 3], [4, 0], [2, 4]], dtype=np.int64)
    got = icp_index.register(_dev(q), q_off, pairs, max_distance=0.08, iterations=8, want_history=True)
    _same(got, CS().register_segments_host(q, q_off, t, t_off, pairs, max_distance=0.08, iterations=8, want_history=True), REG_KEYS)
    none = torch.zeros((0, 3), dtype=torch.float64, device="cuda")
    out = CS().register_segments(none, [0], none, [0], max_distance=1.0)
    assert out["R"].shape == (0, 3, 3) and out["fitness"].shape == (0,)
    out = CS().register_segments(none, [0, 0], none, [0, 0], max_distance=1.0, iterations=2)
    assert _np(out["status"]).tolist() == [U.FEW] and _np(out["converged_at"]).tolist() == [0] and _np(out["R"]).tobytes() == np.eye(3).tobytes()
    assert CS().rigid_fit_segments(none, [0], none, torch.zeros((0,), dtype=torch.int64, device="cuda"))["R"].shape == (0, 3, 3)
    with pytest.raises(ValueError):
        icp_index.register(_dev(q), q_off, max_distance=None)
    with pytest.raises(ValueError):
        icp_index.register(_dev(q), q_off, max_distance=0.05, iterations=0)


def test_registration_icp_with_numpy_and_with_device_input():
    from spatial_engine.utils.scannet_utils.handler import ops
    q, q_off, t, t_off, _truth = U.icp()
    src, tgt = q[q_off[U.HARD]:q_off[U.HARD + 1]], t[t_off[U.HARD]:t_off[U.HARD + 1]]
    host = ops.registration_icp(src, tgt, U.CAPS[U.HARD])
    dev = ops.registration_icp(_dev(src), _dev(tgt), U.CAPS[U.HARD])
    assert isinstance(host["transformation"], np.ndarray) and dev["transformation"].is_cuda
    assert _np(dev["transformation"]).tobytes() == host["transformation"].tobytes()
    assert _np(dev["fitness"]).tobytes() == np.asarray(host["fitness"]).tobytes() and _np(dev["inlier_rmse"]).tobytes() == np.asarray(host["inlier_rmse"]).tobytes()
    again = ops.registration_icp(_dev(src), _dev(tgt), U.CAPS[U.HARD], init=dev["transformation"], max_iteration=2)
    assert _np(again["transformation"]).tobytes() == host["transformation"].tobytes()


def _hand_made_views():
    """Three frames, labels 0 .. 2.  Object 0 (label 1) is the ICP batch's lattice: all of it in frame 0, every second row in frame 1,
    and in frame 2 the EASY pair's queries -- the lattice permuted and moved by a known motion.  Object 1 (label 2) has 30 rows, in
    frame 2 alone.  Returns (all three frames, frames 0 and 1 alone, the motion that carries frame 2's rows back)."""
    from mspa.instances import InstanceClouds
    q, q_off, t, t_off, truth = U.icp()
    L, moved = t[t_off[U.EASY]:t_off[U.EASY + 1]], q[q_off[U.EASY]:q_off[U.EASY + 1]]
    other = np.random.default_rng(12).random((30, 3)) + 3.0
    lo = torch.full((3, 3, 3), float("inf"), dtype=torch.float64, device="cuda")
    views = InstanceClouds([10, 20, 30], np.array([[0, len(L), 0], [0, len(L[::2]), 0], [0, len(moved), len(other)]]), _dev(np.concatenate([L, L[::2], moved, other])),
                           None, lo, -lo)
    rest = InstanceClouds([10, 20], np.array([[0, len(L), 0], [0, len(L[::2]), 0]]), _dev(np.concatenate([L, L[::2]])), None, lo[:2], -lo[:2])
    return views, rest, truth[U.EASY], moved


def test_view_alignment_against_its_own_fused_cloud_is_the_identity_and_against_the_other_frames_the_known_motion():
    """What can be derived.  The fused cloud of ``by_object(None)`` holds every frame's own rows, so each row finds itself at distance 0
    and the fit of rows to themselves is R = I, t = 0 exactly: a moved frame CANNOT report its motion against a target that contains
    it (the docstring's 'pulled towards itself', at its extreme).  Against ``fused=`` the other frames' ``by_object()``, which leaves
    the moved frame out, the moved frame reports the inverse of its motion within the accuracy rule (8 x NumPy-SVD's worst error on
    the near-origin class), as the host twin does against the same truth in tests/test_cloud_align_cpu.py."""
    views, rest, (R_true, t_true), moved = _hand_made_views()
    shown = views.counts > 0
    own = {k: _np(v) for k, v in views.view_alignment(0.05).items()}
    assert own["R"].shape == (3, 3, 3, 3) and own["t"].shape == (3, 3, 3) and all(own[k].shape == (3, 3) for k in ("angle", "shift", "fitness", "inlier_rmse", "status"))
    for key in ("R", "t", "angle", "shift", "fitness", "inlier_rmse"):
        assert (np.isnan(own[key].reshape(3, 3, -1)).all(axis=2) == ~shown).all() and not np.isnan(own[key][shown]).any(), key
    assert (own["status"][~shown] == -1).all() and (own["status"][shown] == U.OK).all()
    assert own["R"][shown].tobytes() == np.tile(np.eye(3), (4, 1, 1)).tobytes() and own["t"][shown].tobytes() == np.zeros((4, 3)).tobytes()
    assert (own["angle"][shown] == 0).all() and (own["shift"][shown] == 0).all() and (own["fitness"][shown] == 1).all() and (own["inlier_rmse"][shown] == 0).all()
    out = {k: _np(v) for k, v in views.view_alignment(0.05, fused=rest.by_object()).items()}
    yard = U.svd_class_errors()["near"][0]
    eR, et = U.errors(out["R"][2, 1], out["t"][2, 1], R_true, t_true, 0.27)
    assert U.within_rule(eR, yard) and U.within_rule(et, yard), (eR, et, yard)
    # angle = atan2(sin, cos) with sin and cos sums of three entries of R over 2: each within 1.5 eR, the angle within their sum
    assert abs(out["angle"][2, 1] - np.deg2rad(1.0)) <= 4 * 8 * yard and out["status"][2, 1] == U.OK and out["fitness"][2, 1] == 1.0
    centre = moved.mean(0)
    assert abs(out["shift"][2, 1] - np.linalg.norm(R_true @ centre + t_true - centre)) <= 4 * 8 * yard * (np.abs(centre).sum() + 1.0)
    assert out["inlier_rmse"][2, 1] < 1e-15                                   # the moved rows land on the rows they were made from
    for k in (0, 1):                                                         # frames that ARE in the target: themselves, exactly
        assert out["R"][k, 1].tobytes() == np.eye(3).tobytes() and out["angle"][k, 1] == 0 and out["status"][k, 1] == U.OK
    assert out["status"][2, 2] == U.FEW and out["fitness"][2, 2] == 0.0 and out["R"][2, 2].tobytes() == np.eye(3).tobytes()      # an object the target lacks
    assert (np.isnan(out["R"].reshape(3, 3, -1)).all(axis=2) == ~shown).all()


def _alignment_twin(clouds, max_distance, voxel_size, iterations):
    """``view_alignment``'s R, t, status, fitness and inlier_rmse from the downloaded clouds through the host twins, pairs built here."""
    fused, fused_off, object_ids = clouds.by_object(voxel_size)
    F, L = clouds.counts.shape
    pairs, where = [], []
    for k in range(F):
        for v in range(1, L):
            if clouds.counts[k, v]:
                pairs.append((k * L + v, list(object_ids).index(v - 1)))
                where.append((k, v))
    reg = CS().register_segments_host(_np(clouds.rows), clouds.offsets, _np(fused), fused_off, np.array(pairs, dtype=np.int64).reshape(-1, 2),
                                      max_distance=max_distance, iterations=iterations)
    return where, reg


def test_view_alignment_and_instance_boxes_on_the_synthetic_scene(tmp_path):
    from test_gpu_instance_boxes import NB, RATIO, _annotate, _synth_scene
    _ns, h, sid, _ids, _with_color, n_objects = _synth_scene(str(tmp_path))
    clouds = h.instance_clouds(sid)
    _annotate(h, sid, clouds, n_objects)
    F, L = clouds.counts.shape
    shown = clouds.counts > 0
    shown[:, 0] = False
    got = {k: _np(v) for k, v in clouds.view_alignment(0.05, voxel_size=0.03, iterations=8).items()}
    where, reg = _alignment_twin(clouds, 0.05, 0.03, 8)
    assert len(where) == shown.sum() > 8 and got["R"].shape == (F, L, 3, 3) and got["status"].shape == (F, L)
    for key in ("R", "t", "status", "fitness", "inlier_rmse"):
        picked = np.stack([got[key][k, v] for k, v in where])
        assert picked.dtype == reg[key].dtype and picked.tobytes() == np.ascontiguousarray(reg[key]).tobytes(), key
    for key in ("R", "t", "angle", "shift", "fitness", "inlier_rmse"):
        assert (np.isnan(got[key].reshape(F, L, -1)).all(axis=2) == ~shown).all(), key
    assert (got["status"][~shown] == -1).all() and (got["status"][shown] >= 0).all()
    ok = shown & (got["status"] == U.OK)
    assert ok.sum() > 4 and (got["angle"][ok] >= 0).all() and (got["angle"][ok] < 0.5).all() and (got["shift"][ok] < 0.05 + 1e-9).all()
    own = {k: _np(v) for k, v in clouds.view_alignment(0.05, iterations=3).items()}      # no thinning: every row finds itself
    same = shown & (own["status"] == U.OK)
    assert same.sum() > 4 and (own["angle"][same] == 0).all() and (own["shift"][same] == 0).all() and (own["inlier_rmse"][same] == 0).all()
    # instance_boxes is not part of this feature: its default dict has the keys it had, and the same bytes run after run
    first = h.instance_boxes(sid, nb_neighbors=NB, std_ratio=RATIO)
    assert sorted(first) == ["boxes", "image_ids", "iou", "kept"]
    second = h.instance_boxes(sid, nb_neighbors=NB, std_ratio=RATIO)
    for key, value in first.items():
        if isinstance(value, torch.Tensor):
            assert _np(value).tobytes() == _np(second[key]).tobytes(), key
        else:
            assert np.array_equal(np.asarray(value), np.asarray(second[key])), key
