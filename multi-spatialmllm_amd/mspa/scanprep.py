"""ScanNet instance data from raw scans: the host readers and the batched device pass behind the drop-in
``utils/scannet_utils/batch_load_scannet_data.py`` / ``scannet_utils.py`` (BL / SU below are those two reference files).

Host side, per scan (threads): the PLY vertex element viewed through a structured dtype (no ``plyfile``), the aggregation JSON
replayed over SEGMENTS into two small tables (segment id -> instance id, segment id -> label index), the axis alignment, and
the ``segIndices`` integers (native host threads, or the device).  Device side, per WINDOW of scans (one launch each,
``csrc/scene_prep.hip``): labels, alignment, per-object extents and the stable split.  DESIGN.md section 0.13.
"""
from __future__ import annotations

import csv
import json
import os
import re
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


# ---- PLY ---------------------------------------------------------------------------------------------------------------------------

def read_ply_vertices(filename: str, data: Optional[bytes] = None) -> np.ndarray:
    """The ``vertex`` element of a PLY file as a structured array (one field per declared property).  ``binary_little_endian``
    is a view of the file's bytes, ``ascii`` a plain text path; faces are never touched.  ``ValueError`` names the file."""
    if data is None:
        with open(filename, "rb") as f:
            data = f.read()

    def bad(why):
        return ValueError(f"{filename}: {why}")

    end = data.find(b"end_header")
    nl = data.find(b"\n", end)
    if not data.startswith(b"ply") or end < 0 or nl < 0:
        raise bad("not a PLY file (no 'ply' ... 'end_header' header)")
    fmt, elements = None, []                     # elements: [name, count, [(property name, dtype or None for a list)]]
    for line in data[:end].decode("ascii", "replace").splitlines()[1:]:
        tok = line.split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format" and len(tok) >= 2:
            fmt = tok[1]
        elif tok[0] == "element" and len(tok) == 3:
            elements.append([tok[1], int(tok[2]), []])
        elif tok[0] == "property" and elements and len(tok) >= 3:
            if tok[1] == "list":
                elements[-1][2].append((tok[-1], None))
            elif tok[1] in _PLY_TYPES:
                elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]]))
            else:
                raise bad(f"unknown property type {tok[1]!r}")
        else:
            raise bad(f"unreadable header line {line!r}")
    if fmt not in ("binary_little_endian", "ascii"):
        raise bad(f"format {fmt!r} is not supported (binary_little_endian and ascii are)")
    body = nl + 1
    names = [e[0] for e in elements]
    if "vertex" not in names:
        raise bad("no vertex element")
    k = names.index("vertex")
    _, count, props = elements[k]
    if any(t is None for _, t in props) or any(t is None for e in elements[:k] for _, t in e[2]):
        raise bad("a list property in or in front of the vertex element")
    dtype = np.dtype([(n, "<" + t) for n, t in props])
    if fmt == "binary_little_endian":
        skip = sum(e[1] * np.dtype([(n, "<" + t) for n, t in e[2]]).itemsize for e in elements[:k] if e[2])
        if len(data) < body + skip + count * dtype.itemsize:
            raise bad(f"truncated: {count} vertices of {dtype.itemsize} bytes declared, {max(len(data) - body - skip, 0)} bytes present")
        return np.frombuffer(data, dtype=dtype, count=count, offset=body + skip)
    lines = data[body:].split(b"\n")
    first = sum(e[1] for e in elements[:k])
    rows = [ln.split() for ln in lines[first:first + count]]
    if len(rows) < count or any(len(r) != len(props) for r in rows):
        raise bad(f"truncated or ragged ascii vertex element ({count} rows of {len(props)} values declared)")
    out = np.empty(count, dtype=dtype)
    try:
        for c, (n, t) in enumerate(props):
            col = np.array([r[c] for r in rows], dtype="S") if count else np.zeros(0, "S1")
            out[n] = col.astype(np.float64).astype(t) if t[0] == "f" else col.astype(np.int64).astype(t)
    except ValueError as e:
        raise bad(f"unreadable ascii value ({e})") from None
    return out


def _vertex_columns(filename: str, columns: Sequence[str], data: Optional[bytes] = None) -> np.ndarray:
    v = read_ply_vertices(filename, data)
    missing = [c for c in columns if c not in (v.dtype.names or ())]
    if missing:
        raise ValueError(f"{filename}: vertex element has no property {missing[0]!r}")
    out = np.zeros((v.shape[0], len(columns)), dtype=np.float32)         # SU:138 / SU:158: assignment converts, as upstream
    for c, name in enumerate(columns):
        out[:, c] = v[name]
    return out


def read_mesh_vertices(filename: str) -> np.ndarray:
    return _vertex_columns(filename, ("x", "y", "z"))


def read_mesh_vertices_rgb(filename: str, data: Optional[bytes] = None) -> np.ndarray:
    return _vertex_columns(filename, ("x", "y", "z", "red", "green", "blue"), data)


# ---- small text files ----------------------------------------------------------------------------------------------------------------

def read_label_mapping(filename: str, label_from: str = "raw_category", label_to: str = "nyu40id") -> dict:
    assert os.path.isfile(filename)
    mapping = {}
    with open(filename) as f:
        for row in csv.DictReader(f, delimiter="\t"):
            mapping[row[label_from]] = int(row[label_to])
    if mapping and represents_int(next(iter(mapping))):
        mapping = {int(k): v for k, v in mapping.items()}
    return mapping


def represents_int(s) -> bool:
    try:
        int(s)
        return True
    except ValueError:
        return False


def read_axis_alignment(meta_file: str) -> np.ndarray:
    """BL:54-63: the first line holding ``axisAlignment``, its characters of "axisAlignment = " STRIPPED as a set from both ends
    (``str.strip`` semantics, as upstream), split on single spaces; identity when there is no such line."""
    matrix = np.eye(4)
    with open(meta_file) as f:
        for line in f:
            if "axisAlignment" in line:
                matrix = [float(x) for x in line.rstrip().strip("axisAlignment = ").split(" ")]
                break
    return np.array(matrix).reshape((4, 4))


def read_aggregation(filename: str) -> Tuple[dict, dict]:
    """SU:17-35 with its aliasing: the first object of a label shares ONE list between ``object_id_to_segs`` and ``label_to_segs``,
    and later objects of that label extend it -- so that object ends up owning their segments too."""
    assert os.path.isfile(filename)
    with open(filename) as f:
        groups = json.load(f)["segGroups"]
    object_id_to_segs, label_to_segs = {}, {}
    for g in groups:
        segs = g["segments"]
        object_id_to_segs[g["objectId"] + 1] = segs                # ids are 1-based
        shared = label_to_segs.setdefault(g["label"], segs)
        if shared is not segs:
            shared.extend(segs)
    return object_id_to_segs, label_to_segs


_SEG_KEY = re.compile(rb'"segIndices"\s*:\s*\[')


def seg_indices_span(data: bytes) -> Optional[Tuple[int, int]]:
    """Byte span of the text between the brackets of the top-level ``"segIndices"`` array, or None: then ``json.loads`` of the
    whole file decides.  The file WITHOUT that text (a few hundred bytes) goes through ``json.loads`` here, so a file that is
    broken elsewhere, or one that only shows the key inside a string or a nested value, is not taken by the fast path."""
    m = _SEG_KEY.search(data)
    if m is None:
        return None
    end = data.find(b"]", m.end())
    if end < 0:
        return None
    try:
        rest = json.loads(data[:m.end()] + data[end:])
    except ValueError:
        return None
    if not isinstance(rest, dict) or rest.get("segIndices") != []:
        return None
    return m.end(), end


def seg_indices_fallback(data: bytes, filename: str) -> np.ndarray:
    """What neither native parser takes: ``json.loads`` decides (and raises what upstream's ``json.load`` raises)."""
    seg = np.asarray(json.loads(data)["segIndices"])
    if seg.size and (seg.dtype.kind not in "iu" or seg.min() < -2 ** 31 or seg.max() >= 2 ** 31):
        raise ValueError(f"{filename}: segIndices are not 32-bit integers")
    return seg.astype(np.int32).reshape(-1)


def read_seg_indices(filename: str) -> np.ndarray:
    with open(filename, "rb") as f:
        data = f.read()
    span = seg_indices_span(data)
    if span is not None:
        from . import engine
        got = engine.parse_int_lists([data[span[0]:span[1]]], n_threads=1)[0]
        if got is not None:
            return got
    return seg_indices_fallback(data, filename)


# ---- the replay: aggregation -> per-segment tables ---------------------------------------------------------------------------------

@dataclass
class SceneTables:
    seg2inst: np.ndarray                  # int32 [T]: segment id -> instance id (0: no object lists it)
    seg2label: np.ndarray                 # int32 [T]: segment id -> label index (0: none)
    label_value: np.ndarray               # uint32 [L + 1]: label index -> nyu40 id; entry 0 is 0
    label_names: np.ndarray               # object [L + 1]: label index -> raw category; entry 0 is None
    object_id_to_segs: dict
    object_id_to_label_id: dict           # BL:94-97, np.uint32 values, in upstream's insertion order
    object_id_to_raw_category: dict
    n_slots: int                          # largest object id: the device keeps one slot per id 1 .. n_slots


def build_tables(object_id_to_segs: dict, label_to_segs: dict, label_map: dict, seg_present: np.ndarray) -> SceneTables:
    """BL:80-101 replayed over segments.  Both tables start at zero and are filled in upstream's order -- labels in
    ``label_to_segs`` order, then objects in ``object_id_to_segs`` order -- so "the later one wins" resolves a segment listed twice
    exactly as the per-vertex assignments do.  ``seg_present[s]``: segment s has a vertex; one that has none is upstream's KeyError."""
    top = -1
    for segs in list(object_id_to_segs.values()) + list(label_to_segs.values()):     # a duplicate objectId leaves segments no object lists
        for s in segs:
            if s < 0:
                raise ValueError(f"negative segment id {s}")
            top = max(top, s)
    present = np.zeros(top + 1, dtype=bool)
    n = min(top + 1, seg_present.shape[0])
    present[:n] = seg_present[:n]

    def checked(segs):
        a = np.asarray(segs, dtype=np.int64).reshape(-1)
        if a.size and not present[a].all():
            raise KeyError(int(a[~present[a]][0]))                          # BL:85 / BL:92: seg_to_verts[seg]
        return a

    seg2inst, seg2label = np.zeros(top + 1, dtype=np.int32), np.zeros(top + 1, dtype=np.int32)
    label_value, label_names = [0], [None]
    for index, (raw_category, segs) in enumerate(label_to_segs.items(), 1):
        label_value.append(label_map[raw_category])
        label_names.append(raw_category)
        seg2label[checked(segs)] = index
    label_value = np.asarray(label_value, dtype=np.uint32)
    names = np.empty(len(label_names), dtype=object)
    names[:] = label_names
    to_label, to_category = {}, {}
    for object_id, segs in object_id_to_segs.items():
        a = checked(segs)
        seg2inst[a] = object_id
        if a.size and object_id not in to_label:                             # first vertex of the first segment: the segment's label
            to_label[object_id] = label_value[seg2label[a[0]]]
            to_category[object_id] = names[seg2label[a[0]]]
    return SceneTables(seg2inst, seg2label, label_value, names, object_id_to_segs, to_label, to_category,
                       max(object_id_to_segs) if object_id_to_segs else 0)


# ---- one scan on the host, a window of scans on the device -------------------------------------------------------------------------

@dataclass
class RawScan:
    name: str
    vertices: np.ndarray                              # [N, 6] float32
    axis_align_matrix: np.ndarray                     # [4, 4] float64
    seg: Optional[np.ndarray] = None                  # int32 [N]; None in test mode
    tables: Optional[SceneTables] = None
    seg_text: Optional[bytes] = None                  # the segIndices text when the parse is left to the window (device parse)
    files: dict = field(default_factory=dict)


def scan_files(scannet_dir: str, scan_name: str) -> dict:
    d = os.path.join(scannet_dir, scan_name)
    return {"mesh_file": os.path.join(d, scan_name + "_vh_clean_2.ply"), "agg_file": os.path.join(d, scan_name + ".aggregation.json"),
            "seg_file": os.path.join(d, scan_name + "_vh_clean_2.0.010000.segs.json"), "meta_file": os.path.join(d, scan_name + ".txt")}


def _attach_seg(scan: RawScan, seg: np.ndarray, label_map: dict):
    agg = read_aggregation(scan.files["agg_file"])
    if seg.shape[0] != scan.vertices.shape[0]:
        raise IndexError(f"{scan.files['seg_file']}: {seg.shape[0]} segIndices for {scan.vertices.shape[0]} vertices")
    if seg.size and seg.min() < 0:
        raise ValueError(f"{scan.files['seg_file']}: negative segment id")
    present = np.bincount(seg).astype(bool) if seg.size else np.zeros(0, dtype=bool)
    scan.seg, scan.tables = seg, build_tables(agg[0], agg[1], label_map, present)


def load_raw_scan(name: str, mesh_file: str, agg_file: str, seg_file: str, meta_file: str, label_map: dict, test_mode: bool = False,
                  defer_seg_parse: bool = False) -> RawScan:
    """Everything the host does for one scan (thread-safe; the heavy parts -- file reads, the native parser -- release the GIL)."""
    scan = RawScan(name, read_mesh_vertices_rgb(mesh_file), read_axis_alignment(meta_file),
                   files={"mesh_file": mesh_file, "agg_file": agg_file, "seg_file": seg_file, "meta_file": meta_file})
    if test_mode:
        return scan
    if defer_seg_parse:
        with open(seg_file, "rb") as f:
            data = f.read()
        span = seg_indices_span(data)
        if span is not None:
            scan.seg_text = data[span[0]:span[1]]
            return scan
        _attach_seg(scan, seg_indices_fallback(data, seg_file), label_map)
        return scan
    _attach_seg(scan, read_seg_indices(seg_file), label_map)
    return scan


def finish_deferred(scans: Sequence[RawScan], label_map: dict, device):
    """The window's ``segIndices`` texts parsed in one device pass (declined ones by the host threads, the rest by json.loads)."""
    from . import engine
    todo = [s for s in scans if s.seg_text is not None]
    if not todo:
        return
    got = engine.parse_int_lists([s.seg_text for s in todo], device=device, expected_counts=[s.vertices.shape[0] for s in todo])
    for s, seg in zip(todo, got):
        if seg is None:
            with open(s.files["seg_file"], "rb") as f:
                seg = seg_indices_fallback(f.read(), s.files["seg_file"])
        s.seg_text = None
        _attach_seg(s, np.ascontiguousarray(seg), label_map)


@dataclass
class ScanResult:
    """``export()``'s twelve values for one scan (BL:122-135)."""
    mesh_vertices: np.ndarray
    aligned_mesh_vertices: np.ndarray
    label_ids: Optional[np.ndarray]
    raw_categories: Optional[np.ndarray]
    instance_ids: Optional[np.ndarray]
    unaligned_bboxes: Optional[np.ndarray]
    aligned_bboxes: Optional[np.ndarray]
    unaligned_obj_point_clouds: Optional[list]
    aligned_obj_point_clouds: Optional[list]
    object_id_to_raw_category: Optional[dict]
    object_id_to_label_id: Optional[dict]
    axis_align_matrix: np.ndarray
    num_unique_instances: Optional[int] = None

    def as_tuple(self):
        return (self.mesh_vertices, self.aligned_mesh_vertices, self.label_ids, self.raw_categories, self.instance_ids,
                self.unaligned_bboxes, self.aligned_bboxes, self.unaligned_obj_point_clouds, self.aligned_obj_point_clouds,
                self.object_id_to_raw_category, self.object_id_to_label_id, self.axis_align_matrix)


def _cat(arrays: List[np.ndarray], dtype, tail=()) -> np.ndarray:
    return np.concatenate(arrays) if arrays else np.zeros((0,) + tuple(tail), dtype=dtype)


def _boxes(tables: SceneTables, count, lo, hi, as_f32: bool, vertices: np.ndarray, lists: List[np.ndarray]):
    """SU:69-94 from the device's per-object numbers: same dtypes, same order of host operations, same exceptions."""
    num_instances = len(tables.object_id_to_segs)
    boxes = np.zeros((num_instances, 7))
    clouds = [None] * num_instances
    for object_id in tables.object_id_to_segs:
        label_id = tables.object_id_to_label_id[object_id]                   # KeyError for an object without segments, as upstream
        if count[object_id - 1] == 0:
            print(f"WARNING: object id {object_id} does not have points. Corresponding entry is set to None.")
            continue
        mn, mx = lo[object_id - 1], hi[object_id - 1]
        if as_f32:
            mn, mx = mn.astype(np.float32), mx.astype(np.float32)            # exact: they ARE float32 values
        boxes[object_id - 1, :] = np.concatenate([(mn + mx) / 2.0, mx - mn, np.array([label_id])])
        clouds[object_id - 1] = vertices[lists[object_id - 1]]
    return boxes, clouds


def prepare_window(scans: Sequence[RawScan], device, test_mode: bool = False, timings: Optional[dict] = None) -> List[ScanResult]:
    """One launch of each K11 kernel over all ``scans`` (ragged), then the per-scan host assembly."""
    import time

    import torch

    from . import engine

    def mark(stage, t0):
        if timings is not None:
            torch.cuda.synchronize(device)
            timings[stage] = timings.get(stage, 0.0) + time.perf_counter() - t0
        return time.perf_counter()

    if not scans:
        return []
    t = time.perf_counter()
    spans = engine.prep_spans([s.vertices.shape[0] for s in scans], device)
    verts = torch.from_numpy(_cat([s.vertices for s in scans], np.float32, (6,))).to(device)
    mats = torch.from_numpy(np.stack([np.asarray(s.axis_align_matrix, dtype=np.float64) for s in scans])).to(device)
    if not test_mode:
        tabs = [s.tables for s in scans]
        seg = torch.from_numpy(_cat([s.seg for s in scans], np.int32)).to(device)
        tab_off = torch.from_numpy(engine._ragged_offsets([t_.seg2inst.shape[0] for t_ in tabs])).to(device)
        lab_off = torch.from_numpy(engine._ragged_offsets([t_.label_value.shape[0] for t_ in tabs])).to(device)
        pad = [np.zeros(1, dtype=np.int32)]                      # scans without objects have empty tables: never hand over a null pointer
        seg2inst = torch.from_numpy(_cat([t_.seg2inst for t_ in tabs] + pad, np.int32)).to(device)
        seg2label = torch.from_numpy(_cat([t_.seg2label for t_ in tabs] + pad, np.int32)).to(device)
        label_value = torch.from_numpy(_cat([t_.label_value for t_ in tabs], np.uint32).view(np.int32)).to(device)
    t = mark("upload", t)
    aligned = engine.prep_align(spans, verts, mats)
    if not test_mode:
        inst, label, index = engine.prep_labels(spans, seg, tab_off, seg2inst, seg2label, lab_off, label_value)
        obj = engine.prep_objects(spans, inst, verts, aligned, [t_.n_slots for t_ in tabs])
    t = mark("kernels", t)
    aligned_h = aligned.cpu().numpy()
    if not test_mode:
        inst_h, label_h, index_h = (x.cpu().numpy() for x in (inst, label, index))
        inst_h, label_h = inst_h.view(np.uint32), label_h.view(np.uint32)
        obj_h = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in obj.items()}
    t = mark("download", t)
    out = []
    vo = spans["vert_off_host"]
    for i, s in enumerate(scans):
        a, b = int(vo[i]), int(vo[i + 1])
        al = aligned_h[a:b]
        if test_mode:
            out.append(ScanResult(s.vertices, al, None, None, None, None, None, None, None, None, None, s.axis_align_matrix))
            continue
        tb = s.tables
        o0, o1 = int(obj_h["obj_off_host"][i]), int(obj_h["obj_off_host"][i + 1])
        off = obj_h["offsets"][o0:o1 + 1]
        lists = [obj_h["indices"][off[k]:off[k + 1]] for k in range(o1 - o0)]
        count = obj_h["count"][o0:o1]
        ub, uc = _boxes(tb, count, obj_h["lo_unaligned"][o0:o1], obj_h["hi_unaligned"][o0:o1], True, s.vertices, lists)
        ab, ac = _boxes(tb, count, obj_h["lo_aligned"][o0:o1], obj_h["hi_aligned"][o0:o1], False, al, lists)
        out.append(ScanResult(s.vertices, al, label_h[a:b], tb.label_names[index_h[a:b]], inst_h[a:b], ub, ab, uc, ac,
                              tb.object_id_to_raw_category, tb.object_id_to_label_id, s.axis_align_matrix, int(obj_h["unique"][i])))
    if timings is not None:
        timings["assemble"] = timings.get("assemble", 0.0) + time.perf_counter() - t
    return out


def default_device():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("mspa.scanprep needs a ROCm GPU: the labels, the alignment and the per-object extents are HIP kernels "
                           "and there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())
