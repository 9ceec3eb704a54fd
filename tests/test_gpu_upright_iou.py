"""``mspa.cloud_segments.upright_iou`` / ``upright_iou_matrix`` on the MI355X against the host twin of the same header, bit for bit, on
the batch of tests/upright_iou_util.py (which tests/test_upright_iou_cpu.py holds to an exact oracle); the wave and workgroup edges;
the matrix shapes; ``upright_of_aabb``; ``ops.calculate_iou_upright``; and ``instance_boxes(upright=True, upright_iou=True)`` on the
synthetic scene of tests/test_gpu_instance_boxes.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import upright_iou_util as U  # noqa: E402

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _same(a, b):
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def test_the_device_equals_the_host_twin_bit_for_bit_twice_and_the_frozen_results():
    from mspa import cloud_segments as CS
    a, b, _names = U.batch()
    want, want_parts = U.batch_twin()
    frozen = U.golden()
    da, db = _dev(a), _dev(b)
    for _run in range(2):
        out, parts = CS.upright_iou(da, db, want_parts=True)
        assert out.is_cuda and out.dtype == torch.float64 and out.shape == (len(a),) and parts.shape == (len(a), 2)
        assert _np(out).tobytes() == want.tobytes() and _np(parts).tobytes() == want_parts.tobytes()
    assert _np(out).tobytes() == frozen["iou"].tobytes() and _np(parts).tobytes() == frozen["parts"].tobytes()
    assert _np(CS.upright_iou(da, db)).tobytes() == want.tobytes()                                # without the second output
    assert _np(CS.upright_iou(db, da)).tobytes() == want.tobytes()                                # symmetric as bytes


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 256, 257, 1025])
def test_pair_counts_at_the_wave_and_workgroup_edges(count):
    from mspa import cloud_segments as CS
    a, b, _names = U.batch()
    want, want_parts = U.batch_twin()
    out, parts = CS.upright_iou(_dev(a[:count]), _dev(b[:count]), want_parts=True)
    assert out.shape == (count,) and parts.shape == (count, 2)
    assert _np(out).tobytes() == want[:count].tobytes() and _np(parts).tobytes() == want_parts[:count].tobytes()


def test_the_matrices():
    from mspa import cloud_segments as CS
    a, b, _names = U.batch()
    boxes = U.matrix_boxes()
    want, want_parts = U.matrix_twin()
    frozen = U.golden()
    d = _dev(boxes)
    out, parts = CS.upright_iou_matrix(d, d, want_parts=True)
    got = _np(out)
    assert got.tobytes() == want.tobytes() == frozen["matrix"].tobytes() and _np(parts).tobytes() == want_parts.tobytes()
    assert got.tobytes() == np.ascontiguousarray(got.T).tobytes()                                 # symmetric as bytes
    diagonal = np.diag(got)
    assert np.isnan(diagonal[11]) and (np.delete(diagonal, 11) == 1.0).all()
    small = CS.upright_iou_matrix(_dev(a[30:33]), _dev(b[30:35]))                                 # 3 x 5
    assert small.shape == (3, 5) and _np(small).tobytes() == CS.upright_iou_matrix_host(a[30:33], b[30:35]).tobytes()
    none, none_parts = CS.upright_iou_matrix(_dev(a[:0]), _dev(b[:4]), want_parts=True)           # 0 x 4
    assert none.shape == (0, 4) and none_parts.shape == (0, 4, 2)
    assert CS.upright_iou_matrix(_dev(a[:4]), _dev(b[:0])).shape == (4, 0)
    grouped = CS.upright_iou_matrix(_dev(a[:6].reshape(2, 3, 8)), _dev(b[:10].reshape(2, 5, 8)))  # [2, 3, 8] against [2, 5, 8]
    assert grouped.shape == (2, 3, 5)
    assert _np(grouped).tobytes() == CS.upright_iou_matrix_host(a[:6].reshape(2, 3, 8), b[:10].reshape(2, 5, 8)).tobytes()


def test_one_box_against_many_leading_shapes_and_a_view_that_is_not_contiguous():
    from mspa import cloud_segments as CS
    a, b, _names = U.batch()
    want, _parts = U.batch_twin()
    one = a[U.index_of("near")]
    many = CS.upright_iou(_dev(one), _dev(b[:65]))
    assert many.shape == (65,) and _np(many).tobytes() == CS.upright_iou_host(one, b[:65]).tobytes()
    assert _np(CS.upright_iou(_dev(b[:65]), _dev(one.reshape(1, 8)))).tobytes() == _np(many).tobytes()
    assert CS.upright_iou(_dev(one), _dev(b[5])).shape == ()
    shaped = CS.upright_iou(_dev(a[:12].reshape(3, 4, 8)), _dev(b[:12].reshape(3, 4, 8)))
    assert shaped.shape == (3, 4) and _np(shaped).tobytes() == want[:12].tobytes()
    wide = torch.full((300, 11), 7.0, dtype=torch.float64, device="cuda")                         # the boxes are columns 2 .. 9 of wider rows
    wide[:, 2:10] = _dev(a[:300])
    view = wide[:, 2:10]
    assert not view.is_contiguous()
    assert _np(CS.upright_iou(view, _dev(b[:300]))).tobytes() == want[:300].tobytes()
    every_other = _dev(a[:600])[::2]
    assert not every_other.is_contiguous()
    assert _np(CS.upright_iou(every_other, _dev(b[:600:2]))).tobytes() == CS.upright_iou_host(a[:600:2], b[:600:2]).tobytes()


def test_the_value_errors():
    from mspa import cloud_segments as CS
    a, b, _names = U.batch()
    da, db = _dev(a[:8]), _dev(b[:8])
    for call in (CS.upright_iou, CS.upright_iou_matrix):
        with pytest.raises(ValueError):
            call(da.to(torch.float32), db)
        with pytest.raises(ValueError):
            call(da, db.to(torch.float32))
        with pytest.raises(ValueError):
            call(da[:, :6], db[:, :6])
        with pytest.raises(ValueError):
            call(da.cpu(), db)
        with pytest.raises(ValueError):
            call(a[:8], db)
    with pytest.raises(ValueError):
        CS.upright_iou(da[:4], db[:5])
    with pytest.raises(ValueError):
        CS.upright_iou(da.reshape(2, 4, 8), db)
    with pytest.raises(ValueError):
        CS.upright_iou_matrix(da.reshape(2, 4, 8), db.reshape(4, 2, 8))
    with pytest.raises(ValueError):
        CS.upright_iou_matrix(da[0], db)


def test_upright_of_aabb_is_the_numpy_restatement():
    from mspa import cloud_segments as CS
    a6, b6 = U.aabb_pairs()
    boxes = np.concatenate([a6, b6, [[0, 0, 0, 1, 1, 2], [1, 2, 3, 0.5, 2, 1], [np.nan] * 6, [0, 0, 0, 1, np.nan, 1]]])
    got = CS.upright_of_aabb(_dev(boxes))
    assert got.is_cuda and _np(got).tobytes() == U.aabb_to_upright(boxes).tobytes()
    assert CS.upright_of_aabb(_dev(boxes.reshape(4, -1, 6))).shape == (4, len(boxes) // 4, 8)
    first = U.index_of("aabb-0")
    scored = CS.upright_iou(CS.upright_of_aabb(_dev(a6)), CS.upright_of_aabb(_dev(b6)))
    assert _np(scored).tobytes() == U.batch_twin()[0][first:first + U.N_AABB].tobytes()


# ---- the scene: instance_boxes(upright=True, upright_iou=True) and ops.calculate_iou_upright ---------------------------------------

NB, RATIO = 20, 1.0


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    import test_gpu_instance_boxes as TB
    root = str(tmp_path_factory.mktemp("upright_iou_scene"))
    ns, h, sid, ids, with_color, n_objects = TB._synth_scene(root)
    clouds = h.instance_clouds(sid, with_color=with_color)
    TB._annotate(h, sid, clouds, n_objects)
    return ns, h, sid, n_objects


def _gt(h, sid, targets, n_objects):
    gt = np.full((len(targets), 6), np.nan)
    for j, t in enumerate(targets):
        if 0 <= t < n_objects:
            gt[j] = np.asarray(h.get_object_gt_bbox(sid, int(t), axis_aligned=True), dtype=np.float64)[:6]
    return _dev(gt)


@pytest.mark.parametrize("per", ["image", "object"])
def test_instance_boxes_scores_the_upright_boxes_and_the_default_is_todays(scene, per):
    from mspa import cloud_segments as CS
    _ns, h, sid, n_objects = scene
    out = h.instance_boxes(sid, nb_neighbors=NB, std_ratio=RATIO, per=per, upright=True, upright_iou=True)
    today = h.instance_boxes(sid, nb_neighbors=NB, std_ratio=RATIO, per=per, upright=True)
    plain = h.instance_boxes(sid, nb_neighbors=NB, std_ratio=RATIO, per=per, upright=True, upright_iou=False)
    assert list(today) == list(plain) and "iou_upright" not in today and list(out) == list(today) + ["iou_upright"]
    for key, value in today.items():
        for other in (plain[key], out[key]):
            if isinstance(value, torch.Tensor):
                assert other.dtype == value.dtype and _np(other).tobytes() == _np(value).tobytes(), key
            else:
                assert np.array_equal(np.asarray(other), np.asarray(value)), key
    targets = np.arange(out["boxes"].shape[1], dtype=np.int64) - 1 if per == "image" else out["object_ids"]
    gt = CS.upright_of_aabb(_gt(h, sid, targets, n_objects))
    want = CS.upright_iou(out["upright"], gt.expand_as(out["upright"]))
    got = out["iou_upright"]
    assert got.is_cuda and got.dtype == torch.float64 and got.shape == out["iou"].shape
    assert _np(got).tobytes() == _np(want).tobytes()
    assert torch.equal(torch.isnan(got), torch.isnan(out["iou"]))
    live = ~torch.isnan(got)
    assert int(live.sum()) > 0 and bool(((got[live] >= 0) & (got[live] <= 1)).all()) and float(got[live].max()) > 0
    assert _np(got).tobytes() == CS.upright_iou_host(_np(out["upright"]), np.broadcast_to(_np(gt), out["upright"].shape)).tobytes()
    with pytest.raises(ValueError, match="upright=True"):
        h.instance_boxes(sid, nb_neighbors=NB, std_ratio=RATIO, per=per, upright_iou=True)


def test_ops_calculate_iou_upright_with_numpy_and_with_device_input(scene):
    ns = scene[0]
    a, b, _names = U.batch()
    want, _parts = U.batch_twin()
    for name in ("near", "octagon", "rect30", "identical", "disjoint-z", "all-nan"):
        i = U.index_of(name)
        on_host = ns.OPS.calculate_iou_upright(a[i], b[i])
        assert isinstance(on_host, float) and np.float64(on_host).tobytes() == want[i].tobytes(), name
        on_device = ns.OPS.calculate_iou_upright(_dev(a[i]), _dev(b[i]))
        assert on_device.is_cuda and on_device.shape == () and _np(on_device).tobytes() == want[i].tobytes(), name
    mixed = ns.OPS.calculate_iou_upright(_dev(a[U.index_of("near")]), b[U.index_of("near")])       # one device tensor: the device's
    assert mixed.is_cuda and _np(mixed).tobytes() == want[U.index_of("near")].tobytes()
