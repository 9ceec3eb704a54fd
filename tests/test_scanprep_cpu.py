"""Scan preparation, host side (no GPU): the PLY reader on hand-packed bytes, the aggregation replay on a hand-written case, the
native integer-list parser against json.loads, and -- where the reference is mounted -- the restated NumPy order of export()
against the unmodified reference running under a plyfile stand-in."""
import json
import os
import struct

import numpy as np
import pytest

import scanprep_util as U
from mspa import engine, scanprep, synth


def _ply(header_props, rows, fmt="binary_little_endian", packer=None, extra=b"", count=None):
    head = ["ply", f"format {fmt} 1.0", "comment hand-packed", f"element vertex {len(rows) if count is None else count}"]
    head += [f"property {t} {n}" for n, t in header_props] + ["element face 1", "property list uchar int vertex_indices", "end_header"]
    body = b"".join(packer(r) for r in rows) if packer else "".join(" ".join(str(v) for v in r) + "\n" for r in rows).encode()
    return ("\n".join(head) + "\n").encode() + body + extra


def test_ply_reader_reordered_and_extra_properties(tmp_path):
    # colours first, a double, a short and an alpha in between, x y z out of order
    props = [("red", "uchar"), ("quality", "double"), ("z", "float"), ("green", "uchar"), ("x", "float"), ("flags", "short"), ("blue", "uchar"),
             ("alpha", "uchar"), ("y", "float")]
    rows = [(10, 0.5, 3.0, 20, 1.0, -7, 30, 255, 2.0), (11, 1.5, 6.25, 21, 4.5, 9, 31, 254, 5.125)]
    data = _ply(props, rows, packer=lambda r: struct.pack("<BdfBfhBBf", *r), extra=struct.pack("<Biii", 3, 0, 1, 0))
    p = tmp_path / "a.ply"
    p.write_bytes(data)
    got = scanprep.read_mesh_vertices_rgb(str(p))
    assert got.dtype == np.float32 and got.tolist() == [[1.0, 2.0, 3.0, 10.0, 20.0, 30.0], [4.5, 5.125, 6.25, 11.0, 21.0, 31.0]]
    assert scanprep.read_mesh_vertices(str(p)).tolist() == [[1.0, 2.0, 3.0], [4.5, 5.125, 6.25]]
    v = scanprep.read_ply_vertices(str(p))
    assert v.dtype.names == tuple(n for n, _ in props) and v["flags"].tolist() == [-7, 9] and v["quality"].tolist() == [0.5, 1.5]


def test_ply_reader_ascii(tmp_path):
    props = [("x", "float"), ("y", "float"), ("z", "float"), ("red", "uchar"), ("green", "uchar"), ("blue", "uchar")]
    rows = [(0.1, -2.5, 3e-3, 1, 2, 3), (7.0, 8.0, 9.0, 255, 0, 128)]
    p = tmp_path / "a.ply"
    p.write_bytes(_ply(props, rows, fmt="ascii", extra=b"3 0 1 0\n"))
    got = scanprep.read_mesh_vertices_rgb(str(p))
    assert got.dtype == np.float32 and np.array_equal(got, np.array(rows, dtype=np.float64).astype(np.float32))


def test_ply_reader_refuses_what_it_cannot_read(tmp_path):
    props = [("x", "float"), ("y", "float"), ("z", "float"), ("red", "uchar"), ("green", "uchar"), ("blue", "uchar")]
    pack = lambda r: struct.pack("<fffBBB", *r)                                                    # noqa: E731
    p = tmp_path / "short.ply"
    p.write_bytes(_ply(props, [(1, 2, 3, 4, 5, 6)] * 3, packer=pack)[:-20])
    with pytest.raises(ValueError, match="short.ply.*truncated"):
        scanprep.read_mesh_vertices_rgb(str(p))
    p = tmp_path / "be.ply"
    p.write_bytes(_ply(props, [(1, 2, 3, 4, 5, 6)], fmt="binary_big_endian", packer=pack))
    with pytest.raises(ValueError, match="be.ply.*binary_big_endian"):
        scanprep.read_mesh_vertices_rgb(str(p))
    p = tmp_path / "ragged.ply"
    p.write_bytes(_ply(props, [(1, 2, 3, 4, 5, 6), (1, 2, 3)], fmt="ascii"))
    with pytest.raises(ValueError, match="ragged.ply"):
        scanprep.read_mesh_vertices_rgb(str(p))
    p = tmp_path / "nocolour.ply"
    p.write_bytes(_ply(props[:3], [(1, 2, 3)], packer=lambda r: struct.pack("<fff", *r)))
    with pytest.raises(ValueError, match="nocolour.ply.*red"):
        scanprep.read_mesh_vertices_rgb(str(p))
    p = tmp_path / "junk.ply"
    p.write_bytes(b"not a ply at all")
    with pytest.raises(ValueError, match="junk.ply"):
        scanprep.read_mesh_vertices_rgb(str(p))


def _write_agg(path, groups):
    path.write_text(json.dumps({"segGroups": [{"objectId": o, "label": l, "segments": s} for o, l, s in groups]}))
    return str(path)


def test_aggregation_replay_aliasing_duplicate_id_and_shared_segment(tmp_path):
    # two chairs (objects 1 and 3: the first chair's list is the label's list and swallows the second's segments), objectId 1
    # given twice (the second group replaces the table's list but the label keeps the first), segment 4 listed by two objects
    agg = _write_agg(tmp_path / "agg.json", [(0, "chair", [1, 2]), (1, "table", [3, 4]), (2, "chair", [5]), (1, "door", [4, 6])])
    o2s, l2s = scanprep.read_aggregation(agg)
    assert o2s == {1: [1, 2, 5], 2: [4, 6], 3: [5]} and o2s[1] is l2s["chair"]
    assert l2s == {"chair": [1, 2, 5], "table": [3, 4], "door": [4, 6]}
    label_map = {"chair": 5, "table": 7, "door": 8}
    present = np.ones(8, dtype=bool)
    t = scanprep.build_tables(o2s, l2s, label_map, present)
    #                             seg: 0  1  2  3  4  5  6
    assert t.seg2inst.tolist() == [0, 1, 1, 0, 2, 3, 2]           # segment 5: object 1 owns it through the alias, object 3 comes later and wins
    assert t.label_value[t.seg2label].tolist() == [0, 5, 5, 7, 8, 5, 8]      # segment 3 keeps its label though no object lists it any more
    assert t.object_id_to_label_id == {1: 5, 2: 8, 3: 5} and all(type(v) is np.uint32 for v in t.object_id_to_label_id.values())
    assert t.object_id_to_raw_category == {1: "chair", 2: "door", 3: "chair"} and t.n_slots == 3
    assert t.label_names.tolist() == [None, "chair", "table", "door"]
    present[6] = False                                            # a listed segment without vertices: upstream's KeyError
    with pytest.raises(KeyError, match="6"):
        scanprep.build_tables(o2s, l2s, label_map, present)
    with pytest.raises(KeyError, match="sofa"):
        scanprep.build_tables({1: [1]}, {"sofa": [1]}, label_map, np.ones(8, dtype=bool))


def test_axis_alignment_strip_semantics(tmp_path):
    p = tmp_path / "scan.txt"
    p.write_text("colorHeight = 968\naxisAlignment = 0.945519 0.325568 0 -5.38439 -0.325568 0.945519 0 -2.87178 0 0 1 -0.06435 0 0 0 1 \nx = 1\n")
    m = scanprep.read_axis_alignment(str(p))
    assert m.shape == (4, 4) and m[0, 3] == -5.38439 and m[2, 3] == -0.06435 and m[3].tolist() == [0, 0, 0, 1]
    p.write_text("colorHeight = 968\n")
    assert np.array_equal(scanprep.read_axis_alignment(str(p)), np.eye(4))


WELL_FORMED = [b"", b"  ", b"0", b"7", b"1,2,3", b"1, 2, 3", b" 1 ,\t2\n,\r\n3 ", b"2147483647,0", b"-5, -0, 12", b"10,200,3000,40000,500000",
               b"-2147483648"]
GARBAGE = [b"1,,2", b",1", b"1,", b"1 2", b"01", b"1.5", b"1e3", b"2147483648", b"99999999999", b"abc", b"1,x", b"-", b"- 1", b"[1]", b"\"1\"", b"1;2"]


def test_int_list_host_parser_against_json():
    got, status = engine.parse_int_lists_host(WELL_FORMED + GARBAGE, n_threads=3)
    for text, g, st in zip(WELL_FORMED, got, status):
        assert st == 0 and g.dtype == np.int32 and g.tolist() == json.loads(b"[" + text + b"]"), text
    for text, g, st in zip(GARBAGE, got[len(WELL_FORMED):], status[len(WELL_FORMED):]):
        assert st != 0 and g is None, text
    big = np.random.default_rng(1).integers(0, 60000, 200001)
    for sep in (",", ", ", " ,\n"):
        text = sep.join(map(str, big.tolist())).encode()
        assert np.array_equal(engine.parse_int_lists([text])[0], big)
    # a count that does not fit the room the caller gives is declined, not truncated
    assert engine.parse_int_lists_host([b"1,2,3"], capacities=[2])[1].tolist() == [16]
    lib = engine._lib.load()
    assert lib.mspa_parse_int_list_host(None, None, 1, None, None, None, None, 1) == engine._lib.MSPA_EINVAL
    assert lib.mspa_parse_int_list_host(None, None, -1, None, None, None, None, 1) == engine._lib.MSPA_EINVAL
    assert lib.mspa_parse_int_list_host(None, None, 0, None, None, None, None, 1) == engine._lib.MSPA_OK


def test_seg_indices_reader_and_fallback(tmp_path):
    p = tmp_path / "s.segs.json"
    p.write_text(json.dumps({"params": {"a": [1, 2]}, "sceneId": "s", "segIndices": [5, 5, 9, 0, 12]}, indent=1))
    assert scanprep.read_seg_indices(str(p)).tolist() == [5, 5, 9, 0, 12]
    p.write_text('{"segIndices": [1, 2.0, 3]}')                  # not the native parsers' business: json decides
    with pytest.raises(ValueError, match="32-bit integers"):
        scanprep.read_seg_indices(str(p))
    p.write_text('{"segIndices": [1, 2,')
    with pytest.raises(json.JSONDecodeError):
        scanprep.read_seg_indices(str(p))


def test_seg_indices_fast_path_leaves_odd_files_to_json(tmp_path):
    p = tmp_path / "s.segs.json"
    p.write_text('{"note": "\\"segIndices\\": [7, 7]", "segIndices": [1, 2, 3]}')          # the key shows up inside a string first
    assert scanprep.read_seg_indices(str(p)).tolist() == [1, 2, 3]
    p.write_text('{"nested": {"segIndices": [9]}, "segIndices": [4, 5]}')                 # ... and inside a nested value
    assert scanprep.read_seg_indices(str(p)).tolist() == [4, 5]
    p.write_text('{"segIndices": [1, 2, 3], "params": {broken}')                          # sound list, file broken elsewhere
    with pytest.raises(json.JSONDecodeError):
        scanprep.read_seg_indices(str(p))
    p.write_text('{"segIndices": [1, 2, 3]} trailing')
    with pytest.raises(json.JSONDecodeError):
        scanprep.read_seg_indices(str(p))
    assert engine.parse_int_lists([]) == [] and engine.parse_int_lists_host([])[1].shape == (0,)


def test_fma_chain_reproduces_numpy_dot_for_n_by_4_times_4_by_4():
    """The order the align kernel spells out (m0*x, fma(m1,y,.), fma(m2,z,.), fma(m3,1.0,.)) against np.dot(pts, A.T) as BL:66-69
    calls it: bit for bit, on general matrices and on sizes around NumPy's / BLAS's blocking.  N = 1 is the exception NumPy makes
    (a [1, 4] operand goes to BLAS as a vector): there the four products are rounded and added as (k0 + k2) + (k1 + k3)."""
    rng = np.random.default_rng(7)
    for n in (1, 1, 1, 2, 2, 3, 4, 5, 64, 257, 5000):
        A = rng.normal(0, 3, (4, 4))
        A[3] = [0, 0, 0, 1]
        xyz = rng.uniform(-9, 9, (n, 3)).astype(np.float32)
        pts = np.ones((n, 4))
        pts[:, :3] = xyz
        ref = np.dot(pts, A.transpose())
        if n == 1:
            x, y, z = (float(v) for v in xyz[0])
            got = np.array([[(A[r, 0] * x + A[r, 2] * z) + (A[r, 1] * y + A[r, 3]) for r in range(3)]])
        else:
            got = np.array([[U.fma_chain_row(A[r], *p) for r in range(3)] for p in xyz])
        assert got.tobytes() == ref[:, :3].tobytes(), n


def _load_synth(tmp_path, name, n_vertices, n_objects, **kw):
    paths = synth.write_raw_scan(str(tmp_path), name, n_vertices, n_objects, **kw)
    label_map = scanprep.read_label_mapping(paths["label_map_file"])
    files = {k: paths[k] for k in ("mesh_file", "agg_file", "seg_file", "meta_file")}
    return paths, files, scanprep.load_raw_scan(name, label_map=label_map, **files)


def test_synthetic_raw_scan_has_the_cases_the_replay_is_sensitive_to(tmp_path):
    paths, files, scan = _load_synth(tmp_path, "scene0000_00", 5000, 12, seed=3)
    head = open(paths["mesh_file"], "rb").read(400)
    assert b"property uchar alpha" in head and b"element face" in head and b"binary_little_endian" in head
    groups = json.load(open(paths["agg_file"]))["segGroups"]
    labels = [g["label"] for g in groups]
    assert len(set(labels)) < len(labels)                                                         # repeated labels
    res = U.numpy_export(scan)
    assert any(c is None for c in res.unaligned_obj_point_clouds)                                 # an object without vertices
    listed = {s for g in groups for s in g["segments"]}
    assert set(np.unique(scan.seg).tolist()) - listed                                             # segments no object lists
    assert (res.instance_ids == 0).any() and res.unaligned_bboxes.shape == (len(groups), 7)


@pytest.mark.reference
@pytest.mark.skipif(not U.reference_available(), reason="/root/reference not mounted")
@pytest.mark.parametrize("case", [dict(n_vertices=6000, n_objects=14, seed=1, axis_align="z"),
                                  dict(n_vertices=4097, n_objects=9, seed=2, axis_align="general"),
                                  dict(n_vertices=3000, n_objects=5, seed=3, axis_align=None),
                                  dict(n_vertices=300, n_objects=4, seed=4, axis_align="z", ascii=True),
                                  dict(n_vertices=1, n_objects=1, seed=5, axis_align="z"),
                                  dict(n_vertices=500, n_objects=0, seed=6, axis_align="z")])
def test_restated_export_equals_the_reference_live(tmp_path, case):
    BL, SU = U.import_reference()
    paths, files, scan = _load_synth(tmp_path, "scene0001_00", **case)
    ref = BL.export(label_map_file=paths["label_map_file"], **files)
    U.assert_same_export(U.numpy_export(scan).as_tuple(), ref)
    # the readers of the drop-in module, one by one
    mine = U.load_facade("scannet_utils")
    assert U.same_array(mine.read_mesh_vertices_rgb(files["mesh_file"]), SU.read_mesh_vertices_rgb(files["mesh_file"]))
    assert U.same_array(mine.read_mesh_vertices(files["mesh_file"]), SU.read_mesh_vertices(files["mesh_file"]))
    assert mine.read_aggregation(files["agg_file"]) == SU.read_aggregation(files["agg_file"])
    got_seg, ref_seg = mine.read_segmentation(files["seg_file"]), SU.read_segmentation(files["seg_file"])
    assert got_seg == ref_seg and list(got_seg[0]) == list(ref_seg[0])
    assert mine.read_label_mapping(paths["label_map_file"]) == SU.read_label_mapping(paths["label_map_file"])
    if ref[5].shape[0]:
        got = mine.extract_bbox(ref[0], SU.read_aggregation(files["agg_file"])[0], ref[10], ref[4])
        assert U.same_array(got[0], ref[5]) and all(U.same_array(a, b) for a, b in zip(got[1], ref[7]))


@pytest.mark.reference
@pytest.mark.skipif(not U.reference_available(), reason="/root/reference not mounted")
def test_restated_export_on_the_hand_written_aggregation(tmp_path):
    """The aliasing / duplicate id / shared segment case of above, end to end against the reference."""
    BL, _ = U.import_reference()
    paths, files, _ = _load_synth(tmp_path, "scene0002_00", 700, 3, seed=9)
    seg = np.repeat(np.arange(7), 100)
    json.dump({"segIndices": seg.tolist()}, open(files["seg_file"], "w"))
    _write_agg(tmp_path / "scene0002_00" / "scene0002_00.aggregation.json", [(0, "chair", [1, 2]), (1, "table", [3, 4]), (2, "chair", [5]), (1, "door", [4, 6])])
    scan = scanprep.load_raw_scan("scene0002_00", label_map=scanprep.read_label_mapping(paths["label_map_file"]), **files)
    U.assert_same_export(U.numpy_export(scan).as_tuple(), BL.export(label_map_file=paths["label_map_file"], **files))
