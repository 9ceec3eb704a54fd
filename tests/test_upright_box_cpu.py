"""The upright minimal boxes of a ragged batch without a GPU (csrc/upright_box_core.h through the library's host twin,
mspa_upright_segments_host), on the batch of tests/upright_box_util.py:

  * the twin's hull against the exact oracle of the utilities (Python integers), vertex for vertex and in order, on every segment,
    and again with every segment's rows permuted; against SciPy's Qhull on the segments where Qhull is unambiguous;
  * the rectangle against the oracle's exact rational m_k and the header's derived bound, rect_bound = 64 * 2^-53 * R^2 (R the
    diagonal of the hull's bounding box): the exact m of the chosen edge exceeds the exact minimum by no more than the bound, and
    length * width lies within the bound of the chosen edge's exact m.  The worst observed error over the bound is printed;
  * the box's properties, the refusals, every argument error, the small shapes, the frozen results against a fresh run;
  * the header once more as a stand-alone g++ program under AddressSanitizer + UBSan, also with the chain's cap lowered.
SciPy is imported plainly: a machine without it fails that test."""
import inspect
import os
import shutil
import struct
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import upright_box_util as B  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-spatialmllm_amd", "csrc")
fold = lambda text: " ".join(text.split())                                   # noqa: E731


def _ops():
    for name in [m for m in sys.modules if m == "spatial_engine" or m.startswith("spatial_engine.")]:
        if not (getattr(sys.modules[name], "__file__", None) or "").startswith(ROOT):
            del sys.modules[name]                   # the reference's modules of the same names, left by another test
    from spatial_engine.utils.scannet_utils.handler import ops
    return ops


def _hulls(index, hull_offsets):
    return [index[hull_offsets[s]:hull_offsets[s + 1]].tolist() for s in range(len(hull_offsets) - 1)]


def test_the_batch_is_what_its_docstring_says():
    rows, off, names = B.batch()
    assert len(rows) == off[-1] < 40000 and len(names) == len(off) - 1
    lengths = dict(zip(names, np.diff(off)))
    assert names[0] == "front-empty" and names[-1] == "end-empty"
    assert lengths["front-empty"] == lengths["middle-empty"] == lengths["end-empty"] == 0 and lengths["n=1"] == 1
    assert max(lengths["tiny-a"], lengths["tiny-b"], lengths["tiny-c"]) <= 4 and lengths["gauss-10000"] > 2 * 4096
    h = dict(zip(names, (len(v) for v in B.batch_oracle())))
    assert [h[n] for n in ("front-empty", "n=1", "two-identical", "two-distinct", "collinear-axis", "collinear-diagonal")] == [0, 1, 1, 2, 2, 2]
    assert h["collinear-slope"] > 2 and h["lattice-eighths"] == h["lattice-dup8"] == h["rect30-near"] == h["rect30-far"] == h["square45"] == 4
    assert h["circle-512"] == 512 > 256 and h["circle-5000"] == 5000 > 2048 and h["ellipse-thin"] == 1000 and h["kettner"] == 4
    # the plain float64 determinant gets the sign wrong for more than half of the grid against the line through (12, 12) and (24, 24)
    grid = np.array([(0.5 + i * 2.0 ** -53, 0.5 + j * 2.0 ** -53) for i in range(64) for j in range(64)])
    plain = np.sign((12.0 - grid[:, 0]) * (24.0 - grid[:, 1]) - (12.0 - grid[:, 1]) * (24.0 - grid[:, 0]))       # orient(p, (12, 12), (24, 24))
    assert int((plain != np.sign(grid[:, 1] - grid[:, 0])).sum()) == 2164
    # the rectangles' hulls are their four corners, the last four rows
    for name in B.RECT_CENTRES:
        s = names.index(name)
        assert sorted(B.batch_oracle()[s]) == list(range(int(off[s + 1]) - 4, int(off[s + 1])))


@pytest.mark.parametrize("shuffled", [False, True], ids=["input-order", "rows-permuted"])
def test_the_twins_hull_is_the_exact_hull_vertex_for_vertex(shuffled):
    _rows, _off, names = B.batch()
    _boxes, index, hull_offsets, _edges = B.batch_twin(shuffled)
    assert index.dtype == np.int64 and hull_offsets.dtype == np.int64 and hull_offsets[0] == 0 and hull_offsets[-1] == len(index)
    for name, got, want in zip(names, _hulls(index, hull_offsets), B.batch_oracle(shuffled)):
        assert got == want, name


def test_the_hull_as_coordinates_and_the_boxes_do_not_depend_on_the_order_of_the_rows():
    rows, _off, _names = B.batch()
    shuffled_rows, _off2, _perm = B.permuted()
    boxes, index, hull_offsets, edges = B.batch_twin(False)
    boxes2, index2, hull_offsets2, edges2 = B.batch_twin(True)
    assert np.array_equal(hull_offsets, hull_offsets2) and np.array_equal(edges, edges2)
    assert np.array_equal(rows[index, :2], shuffled_rows[index2, :2])
    assert boxes.tobytes() == boxes2.tobytes()


def test_scipys_hull_has_the_same_vertices_where_qhull_is_unambiguous():
    from scipy.spatial import ConvexHull
    rows, off, names = B.batch()
    _boxes, index, hull_offsets, _edges = B.batch_twin()
    for name in B.QHULL_UNAMBIGUOUS:
        s = names.index(name)
        part = rows[off[s]:off[s + 1], :2]
        got = index[hull_offsets[s]:hull_offsets[s + 1]] - off[s]
        want = ConvexHull(part).vertices
        assert {tuple(p) for p in part[got]} == {tuple(p) for p in part[want]}, name      # as coordinates: a duplicate has several rows
        assert len(got) == len({tuple(p) for p in part[want]}), name


def test_the_chosen_edge_and_the_area_are_within_the_derived_bound_of_the_exact_values():
    _rows, _off, names = B.batch()
    boxes, _index, hull_offsets, edges = B.batch_twin()
    worst = (0.0, 0.0)
    for s, (name, exact) in enumerate(zip(names, B.batch_measures())):
        h = int(hull_offsets[s + 1] - hull_offsets[s])
        if exact is None:
            assert h < 2 and edges[s] == (0 if h else -1), name
            continue
        m, diagonal_sq = exact
        bound = Fraction(B.RECT_BOUND) * diagonal_sq
        chosen = m[int(edges[s])]
        area = Fraction(float(boxes[s, 3])) * Fraction(float(boxes[s, 4]))
        over_minimum, off_area = float((chosen - min(m)) / bound), float(abs(area - chosen) / bound)
        print(f"{name:20s} h {h:5d} edge {int(edges[s]):5d}  (m(chosen) - min m) / bound {over_minimum:.3e}  |length * width - m| / bound {off_area:.3e}")
        worst = (max(worst[0], over_minimum), max(worst[1], off_area))
        assert 0 <= chosen - min(m) <= bound, name
        assert abs(area - chosen) <= bound, name
    print(f"worst over the bound: chosen edge {worst[0]:.3e}, area {worst[1]:.3e}")


def test_length_is_not_below_width_the_axis_has_its_sign_and_every_row_lies_in_its_box():
    rows, off, names = B.batch()
    boxes, _index, hull_offsets, _edges = B.batch_twin()
    for s, name in enumerate(names):
        part, box = rows[off[s]:off[s + 1]], boxes[s]
        if len(part) == 0:
            assert np.isnan(box).all(), name
            continue
        cx, cy, cz, length, width, height, ux, uy = box
        assert length >= width >= 0 and (ux > 0 or (ux == 0 and uy > 0)) and abs(ux * ux + uy * uy - 1) <= 8 * B.U, name
        assert cz == (part[:, 2].max() + part[:, 2].min()) / 2 and height == part[:, 2].max() - part[:, 2].min(), name        # calculate_aabb's z
        if hull_offsets[s + 1] - hull_offsets[s] == 1:
            assert (cx, cy, length, width, ux, uy) == (part[0, 0], part[0, 1], 0, 0, 1, 0), name
        # the header: each span within 12 u R of the exact extent (half of it per side), the centre within 12 u R + u |centre|, the
        # axis within 2 u of unit length; this test's own float64 projection adds at most 4 u (|p| + |centre|) -- 32 u (R + |p|max)
        diagonal = float(np.hypot(np.ptp(part[:, 0]), np.ptp(part[:, 1])))
        slack = 32 * B.U * (diagonal + float(np.abs(part[:, :2]).max()))
        along = (part[:, 0] - cx) * ux + (part[:, 1] - cy) * uy
        across = (part[:, 1] - cy) * ux - (part[:, 0] - cx) * uy
        assert np.abs(along).max() <= length / 2 + slack and np.abs(across).max() <= width / 2 + slack, name
        assert np.abs(along).max() >= length / 2 - slack and np.abs(across).max() >= width / 2 - slack, name                 # and it is tight
    for name in ("collinear-axis", "collinear-diagonal", "two-distinct", "tiny-b"):
        assert boxes[names.index(name), 4] == 0 and boxes[names.index(name), 3] > 0, name
    assert boxes[names.index("collinear-axis"), 6:].tolist() == [1.0, 0.0]
    assert boxes[names.index("collinear-diagonal"), 6] == boxes[names.index("collinear-diagonal"), 7] > 0.7


def test_the_turned_rectangles_come_back_with_their_sizes_and_their_angle():
    _rows, _off, names = B.batch()
    boxes, _index, _hull_offsets, _edges = B.batch_twin()
    length, width, angle = B.RECT
    want = np.array([np.cos(np.deg2rad(angle)), np.sin(np.deg2rad(angle))])
    for name, centre in B.RECT_CENTRES.items():
        box = boxes[names.index(name)]
        # each corner as generated lies within eta = 4 u (2 + |centre|max) of the ideal one (two products, two sums), so an edge of
        # length >= 0.8 points within 2 eta / 0.8 of its ideal direction; the rule's axis adds 4 u, cos / sin of the test 2 u
        eta = 4 * B.U * (2 + max(abs(c) for c in centre))
        tolerance = 2 * eta / width + 6 * B.U
        assert np.abs(box[6:] - want).max() <= tolerance, (name, box[6:] - want, tolerance)
        assert abs(box[3] - length) <= 4 * eta + 12 * B.U * 3 and abs(box[4] - width) <= 4 * eta + 12 * B.U * 3, name
        assert np.abs(box[:2] - np.array(centre)).max() <= 4 * eta + 12 * B.U * 3 + B.U * max(abs(c) for c in centre), name
    square = boxes[names.index("square45")]                   # four edges that tie: edge 0, from (-1, 0) counter-clockwise to (0, -1)
    assert _edges[names.index("square45")] == 0 and square[3] == square[4] and abs(square[3] - np.sqrt(2.0)) <= 8 * B.U
    assert np.abs(square[6:] - np.array([np.sqrt(0.5), -np.sqrt(0.5)])).max() <= 4 * B.U


@pytest.mark.parametrize("name", ["S=1", "N=0", "all-empty"])
def test_one_segment_no_rows_and_only_empty_segments(name):
    from mspa import cloud_segments as CS
    rows, off = B.small_batches()[name]
    boxes, index, hull_offsets, edges = CS.upright_boxes_segments_host(rows, off, want_hull=True, want_edges=True)
    S = len(off) - 1
    assert boxes.shape == (S, 8) and hull_offsets.shape == (S + 1,) and edges.shape == (S,) and index.dtype == np.int64
    if name == "S=1":
        assert index.tolist() == B.exact_hull(rows[:, :2]) and np.isfinite(boxes).all()
        assert np.array_equal(CS.footprint_hull_segments_host(rows, off)[0], index)
        assert np.array_equal(_ops().calculate_upright_box(rows), boxes[0])
    else:
        assert len(index) == 0 and np.isnan(boxes).all() and (edges == -1).all() and (hull_offsets == 0).all()


def test_the_frozen_results_are_a_fresh_runs():
    frozen = B.golden()
    boxes, index, hull_offsets, edges = B.batch_twin()
    assert frozen["boxes"].tobytes() == boxes.tobytes()
    assert np.array_equal(frozen["hull_index"], index) and np.array_equal(frozen["hull_offsets"], hull_offsets)
    assert np.array_equal(frozen["edges"], edges) and frozen["edges"].dtype == np.int32
    assert os.path.getsize(B.GOLDEN) < 1 << 20


def test_the_python_functions_refuse_what_the_rule_refuses():
    from mspa import cloud_segments as CS
    ops = _ops()
    rows, off, _names = B.batch()
    calls = (CS.upright_boxes_segments_host, CS.footprint_hull_segments_host)
    for call in calls:
        for value in (np.nan, np.inf, -np.inf):
            for column in range(3):
                bad = rows.copy()
                bad[20000, column] = value
                with pytest.raises(ValueError, match="non-finite"):
                    call(bad, off)
        for value in (1e300, -1e300, 1e-300, 2.0 ** 201, 2.0 ** -201):
            for column in range(2):
                bad = rows.copy()
                bad[20000, column] = value
                with pytest.raises(ValueError, match="outside"):
                    call(bad, off)
        edge = rows.copy()
        edge[20000, :2] = (2.0 ** 200, -2.0 ** -200)                           # the ends of the window are inside it; z has no window
        edge[20001, :3] = (0.0, -0.0, 1e300)
        call(edge, off)
        with pytest.raises(ValueError):
            call(rows, off[:-2])                                             # offsets that do not end at N
        with pytest.raises(ValueError):
            call(rows, off[::-1])
        with pytest.raises(ValueError):
            call(rows[:, :2], off)                                           # C < 3
        with pytest.raises(ValueError):
            call(rows.reshape(-1), off)
    bad = rows[:100].copy()
    bad[17, 0] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        ops.calculate_upright_box(bad)
    for call in (CS.upright_boxes_segments, CS.footprint_hull_segments):
        with pytest.raises((ValueError, RuntimeError)):
            call(rows, off)                                                  # NumPy rows have no device: no quiet fallback


def test_the_c_entry_points_refuse_bad_arguments_before_anything_is_enqueued():
    """Every refusal below returns MSPA_EINVAL from the argument checks; none of the pointers is a device pointer, and none is ever
    dereferenced as one (the checks come before the first launch)."""
    from mspa import _lib
    lib = _lib.load()
    rows = np.random.default_rng(1).random((10, 4))
    good = np.array([0, 4, 4, 10], dtype=np.int64)
    hull_good = np.array([0, 3, 3, 8], dtype=np.int64)
    S, C = 3, 4
    p = lambda a: a.ctypes.data                                              # noqa: E731
    filter_bytes, boxes_bytes = lib.mspa_upright_filter_workspace_bytes(p(good), S), lib.mspa_upright_boxes_workspace_bytes(p(hull_good), S)
    assert filter_bytes > 0 and filter_bytes % 16 == 0 and boxes_bytes > 0 and boxes_bytes % 16 == 0
    work = np.zeros(max(filter_bytes, boxes_bytes) + 16, dtype=np.uint8)
    aligned = (work.ctypes.data + 15) // 16 * 16
    rows_list, ext, seg = np.zeros(10, dtype=np.int64), np.zeros((S, 10)), np.zeros(2 * S + 1, dtype=np.int32)
    pts, row, stack = np.zeros((10, 2)), np.zeros(10, dtype=np.int64), np.zeros((2, 10), dtype=np.int32)
    hull_index, edges, boxes, flags = np.zeros(10, dtype=np.int64), np.zeros(S, dtype=np.int32), np.zeros((S, 8)), np.zeros(1, dtype=np.int32)
    descending = np.array([0, 5, 4, 10], dtype=np.int64)
    not_from_zero = np.array([1, 4, 4, 10], dtype=np.int64)
    too_long = np.array([0, (1 << 30) + 1], dtype=np.int64)
    too_many_vertices = np.array([0, 5, 5, 10], dtype=np.int64)              # segment 0 has four survivors
    many = (1 << 24) + 1

    def filter_call(off=good, n_seg=S, c=C, rows_p=p(rows), off_p=p(good), base_p=p(good), list_p=p(rows_list), ext_p=p(ext), seg_p=p(seg),
                    w=aligned, w_bytes=filter_bytes):
        return lib.mspa_upright_filter_device(rows_p, c, p(off), n_seg, off_p, base_p, list_p, ext_p, seg_p, w, w_bytes, None)

    def hull_call(off=good, n_seg=S, pts_p=p(pts), off_p=p(good), stack_p=p(stack), seg_p=p(seg)):
        return lib.mspa_upright_hull_device(pts_p, p(off), n_seg, off_p, stack_p, seg_p, None)

    def boxes_call(off=good, hull=hull_good, n_seg=S, pts_p=p(pts), row_p=p(row), off_p=p(good), hull_p=p(hull_good), base_p=p(good),
                   stack_p=p(stack), counts_p=p(seg), ext_p=p(ext), index_p=p(hull_index), edge_p=p(edges), boxes_p=p(boxes), w=aligned,
                   w_bytes=boxes_bytes):
        return lib.mspa_upright_boxes_device(pts_p, row_p, p(off), p(hull), n_seg, off_p, hull_p, base_p, stack_p, counts_p, ext_p, index_p, edge_p,
                                             boxes_p, w, w_bytes, None)

    def host_call(off=good, n_seg=S, c=C, rows_p=p(rows), index_p=p(hull_index), hull_p=p(hull_good.copy()), edge_p=p(edges), boxes_p=p(boxes),
                  flags_p=p(flags)):
        return lib.mspa_upright_segments_host(rows_p, c, p(off), n_seg, index_p, hull_p, edge_p, boxes_p, flags_p)

    refused = {}
    for name, call in (("filter", filter_call), ("hull", hull_call), ("boxes", boxes_call), ("host", host_call)):
        refused.update({
            f"{name}: descending offsets": call(off=descending), f"{name}: offsets[0] != 0": call(off=not_from_zero),
            f"{name}: N > 2^30": call(off=too_long, n_seg=1), f"{name}: negative S": call(n_seg=-1), f"{name}: S > 2^24": call(n_seg=many)})
    refused.update({
        "filter: C = 2": filter_call(c=2), "filter: C = 65537": filter_call(c=65537), "filter: null rows": filter_call(rows_p=None),
        "filter: null offsets_dev": filter_call(off_p=None), "filter: null tile_base": filter_call(base_p=None),
        "filter: null list": filter_call(list_p=None), "filter: null ext": filter_call(ext_p=None), "filter: null seg": filter_call(seg_p=None),
        "filter: null workspace": filter_call(w=None), "filter: workspace too small": filter_call(w_bytes=filter_bytes - 16),
        "filter: workspace misaligned": filter_call(w=aligned + 8), "filter: rows at 4 mod 8": filter_call(rows_p=p(rows) + 4),
        "filter: list at 4 mod 8": filter_call(list_p=p(rows_list) + 4), "filter: ext at 4 mod 8": filter_call(ext_p=p(ext) + 4),
        "filter: seg at 2 mod 4": filter_call(seg_p=p(seg) + 2), "filter: tile_base at 4 mod 8": filter_call(base_p=p(good) + 4),
        "hull: null pts": hull_call(pts_p=None), "hull: null offsets_dev": hull_call(off_p=None), "hull: null stack": hull_call(stack_p=None),
        "hull: null seg": hull_call(seg_p=None), "hull: pts at 4 mod 8": hull_call(pts_p=p(pts) + 4), "hull: stack at 2 mod 4": hull_call(stack_p=p(stack) + 2),
        "hull: seg at 2 mod 4": hull_call(seg_p=p(seg) + 2),
        "boxes: descending hull offsets": boxes_call(hull=descending), "boxes: more vertices than survivors": boxes_call(hull=too_many_vertices),
        "boxes: null pts": boxes_call(pts_p=None), "boxes: null row": boxes_call(row_p=None), "boxes: null offsets_dev": boxes_call(off_p=None),
        "boxes: null hull_offsets_dev": boxes_call(hull_p=None), "boxes: null edge_base": boxes_call(base_p=None),
        "boxes: null stack": boxes_call(stack_p=None), "boxes: null counts": boxes_call(counts_p=None), "boxes: null ext": boxes_call(ext_p=None),
        "boxes: null hull_index": boxes_call(index_p=None), "boxes: null edges": boxes_call(edge_p=None), "boxes: null boxes": boxes_call(boxes_p=None),
        "boxes: null workspace": boxes_call(w=None), "boxes: workspace too small": boxes_call(w_bytes=boxes_bytes - 16),
        "boxes: workspace misaligned": boxes_call(w=aligned + 8), "boxes: pts at 4 mod 8": boxes_call(pts_p=p(pts) + 4),
        "boxes: row at 4 mod 8": boxes_call(row_p=p(row) + 4), "boxes: counts at 2 mod 4": boxes_call(counts_p=p(seg) + 2),
        "boxes: boxes at 4 mod 8": boxes_call(boxes_p=p(boxes) + 4), "boxes: edges at 2 mod 4": boxes_call(edge_p=p(edges) + 2),
        "host: C = 2": host_call(c=2), "host: null rows": host_call(rows_p=None), "host: null hull_index": host_call(index_p=None),
        "host: null hull_offsets": host_call(hull_p=None), "host: null edges": host_call(edge_p=None), "host: null boxes": host_call(boxes_p=None),
        "host: null flags": host_call(flags_p=None),
    })
    assert {k: v for k, v in refused.items() if v != _lib.MSPA_EINVAL} == {}
    assert b"mspa_upright_segments_host" in lib.mspa_last_error_string()
    assert lib.mspa_upright_filter_workspace_bytes(p(descending), S) == -1 and lib.mspa_upright_boxes_workspace_bytes(p(too_long), 1) == -1
    assert host_call() == 0 and flags[0] == 0                                # the good arguments are good
    # the flag word: a NaN row and a coordinate outside the window, reported, not refused by the C layer
    nan_rows = rows.copy()
    nan_rows[7, 2] = np.nan
    assert host_call(rows_p=p(nan_rows)) == 0 and flags[0] == 1
    wide = rows.copy()
    wide[0, 1] = 1e-300
    assert host_call(rows_p=p(wide)) == 0 and flags[0] == 2


def test_ops_calculate_upright_box_is_the_one_segment_batch_and_the_docstrings_keep_their_sentences():
    import torch
    from mspa import cloud_segments as CS
    ops = _ops()
    assert "No reference counterpart" in fold(ops.calculate_upright_box.__doc__) and "calculate_upright_box" not in ops.__all__
    rows, off, names = B.batch()
    boxes = B.batch_twin()[0]
    for name in ("rect30-near", "kettner", "n=1", "front-empty"):
        s = names.index(name)
        got = ops.calculate_upright_box(rows[off[s]:off[s + 1]])
        assert isinstance(got, np.ndarray) and got.shape == (8,) and got.dtype == np.float64
        assert got.tobytes() == boxes[s].tobytes(), name
    cloud = B.segment("rect30-near")
    wide = np.concatenate([cloud, np.arange(len(cloud) * 3, dtype=np.float64).reshape(-1, 3)], axis=1)       # extra columns are not read
    assert np.array_equal(ops.calculate_upright_box(wide), ops.calculate_upright_box(cloud))
    narrow, narrow_off = B.float32_segment()                                 # float32 in, C = 6: widened exactly
    assert np.array_equal(ops.calculate_upright_box(narrow), CS.upright_boxes_segments_host(narrow[:, :3].astype(np.float64), narrow_off)[0])
    on_host = ops.calculate_upright_box(torch.from_numpy(cloud.copy()))      # a host tensor in gives a host tensor out
    assert isinstance(on_host, torch.Tensor) and np.array_equal(on_host.numpy(), ops.calculate_upright_box(cloud))
    sentence = ("At most two read-backs per call, whatever S is: the survivor counts with the flag word, and the hull counts with the flag word.")
    assert sentence in fold(CS.upright_boxes_segments.__doc__) and sentence in fold(CS.footprint_hull_segments.__doc__)
    assert "not a fallback" in fold(CS.upright_boxes_segments_host.__doc__) and "not a fallback" in fold(CS.footprint_hull_segments_host.__doc__)
    assert "not pinned" in fold(CS.upright_yaw.__doc__) and "Enqueue only" in fold(CS.upright_yaw.__doc__)
    assert "Enqueue only" in fold(CS.upright_corners.__doc__)
    assert inspect.signature(CS.upright_boxes_segments).parameters["want_hull"].default is False


def test_the_corners_and_the_yaw_of_a_box_on_the_host():
    import torch
    from mspa import cloud_segments as CS
    _rows, _off, names = B.batch()
    boxes = torch.from_numpy(B.batch_twin()[0].copy())
    corners, yaw = CS.upright_corners(boxes), CS.upright_yaw(boxes)
    assert corners.shape == (len(names), 8, 3) and yaw.shape == (len(names),)
    s = names.index("rect30-near")
    assert abs(float(yaw[s]) - np.deg2rad(30.0)) < 1e-12
    want = B.segment("rect30-near")[-4:, :2]                                 # the generated corners, in some order
    got = corners[s, :4, :2].numpy()
    assert all(np.abs(want - g).sum(axis=1).min() < 1e-12 for g in got)
    assert np.array_equal(corners[s, :4, :2].numpy(), corners[s, 4:, :2].numpy())
    assert float(corners[s, 0, 2]) == float(boxes[s, 2] - boxes[s, 5] / 2) and float(corners[s, 7, 2]) == float(boxes[s, 2] + boxes[s, 5] / 2)
    assert torch.isnan(corners[names.index("front-empty")]).all() and torch.isnan(yaw[names.index("end-empty")])


# One record: int64 S, int64 cap (-1: the rule's), (S + 1) int64 offsets, N * 3 float64 -> int32 flags, (S + 1) int64 hull offsets,
# H int64 hull rows, S int32 edges, S * 8 float64 boxes.  Every buffer is a heap block of exactly its size.
DRIVER = r"""
#include "upright_box_core.h"
#include <cstdio>
#include <cstdlib>
template <typename T> static T *block(int64_t n) { return (T *)malloc((size_t)(n > 0 ? n : 1) * sizeof(T)); }
int main() {
    int64_t head[2];
    while (fread(head, 8, 2, stdin) == 2) {
        const int64_t S = head[0], cap = head[1];
        int64_t *offsets = block<int64_t>(S + 1);
        if (fread(offsets, 8, (size_t)(S + 1), stdin) != (size_t)(S + 1)) return 4;
        const int64_t N = mspa::upright::batch_rows(offsets, S);
        if (N < 0) return 5;
        double *rows = block<double>(N * 3), *boxes = block<double>(S * 8);
        int64_t *hull_index = block<int64_t>(N), *hull_offsets = block<int64_t>(S + 1);
        int32_t *edges = block<int32_t>(S);
        if (fread(rows, 8, (size_t)(N * 3), stdin) != (size_t)(N * 3)) return 6;
        const int32_t flags = mspa::upright::upright_all(rows, 3, offsets, S, hull_index, hull_offsets, edges, boxes, cap);
        fwrite(&flags, 4, 1, stdout);
        fwrite(hull_offsets, 8, (size_t)(S + 1), stdout);
        fwrite(hull_index, 8, (size_t)hull_offsets[S], stdout);
        fwrite(edges, 4, (size_t)S, stdout);
        fwrite(boxes, 8, (size_t)(S * 8), stdout);
        void *all[] = {offsets, rows, boxes, hull_index, hull_offsets, edges};
        for (void *b : all) free(b);
    }
    return 0;
}
"""


def test_the_header_under_sanitizers_and_the_cap_of_the_chain(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    (tmp_path / "driver.cpp").write_text(DRIVER)
    exe = str(tmp_path / "driver")
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", CSRC, str(tmp_path / "driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    rows, off, _names = B.batch()
    records = [(rows, off, -1), (B.permuted()[0], off, -1)] + [(x, o, -1) for x, o in B.small_batches().values()]
    nan_rows, tiny = rows.copy(), rows.copy()
    nan_rows[123, 0] = np.nan
    tiny[30000, 1] = 1e-300
    records += [(nan_rows, off, -1), (tiny, off, -1)]
    circle = (B.segment("circle-512"), np.array([0, 2512], dtype=np.int64))
    records += [(*circle, 2512), (*circle, 3), (*circle, 0)]                  # the rule's cap, and two that the chain reaches
    inp = b"".join(struct.pack("<qq", len(o) - 1, cap) + np.asarray(o, dtype="<i8").tobytes() + np.asarray(x, dtype="<f8").tobytes()
                   for x, o, cap in records)
    run = subprocess.run([exe], input=inp, capture_output=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:].decode(errors="replace"))
    at = 0

    def take(dtype, count):
        nonlocal at
        a = np.frombuffer(run.stdout, dtype=dtype, count=count, offset=at)
        at += a.nbytes
        return a

    from mspa import cloud_segments as CS
    for n, (x, o, cap) in enumerate(records):
        S = len(o) - 1
        flags = int(take("<i4", 1)[0])
        hull_offsets = take("<i8", S + 1)
        index, edges, boxes = take("<i8", int(hull_offsets[S])), take("<i4", S), take("<f8", S * 8).reshape(S, 8)
        lowered = 0 <= cap < len(x)
        assert flags == (1 if np.isnan(x).any() else 2 if (np.abs(x[:, :2]) == 1e-300).any() else 4 if lowered else 0), (n, flags)
        if not flags:
            want = CS.upright_boxes_segments_host(x, o, want_hull=True, want_edges=True)
            assert boxes.tobytes() == want[0].tobytes() and np.array_equal(index, want[1]) and np.array_equal(hull_offsets, want[2]), n
            assert np.array_equal(edges, want[3]), n
    assert at == len(run.stdout)
