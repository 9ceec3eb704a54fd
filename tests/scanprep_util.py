"""Shared by the scan-preparation tests and tools/gen_scanprep_golden.py: the reference's two modules imported unmodified under a
``plyfile`` stand-in, a NumPy restatement of ``export()`` in the kernels' order, and helpers to compare results."""
import importlib.util
import os
import sys
import types
from fractions import Fraction

import numpy as np

from mspa import scanprep

REFERENCE_ROOT = os.environ.get("MSPA_REFERENCE_ROOT", "/root/reference")
REF_DIR = os.path.join(REFERENCE_ROOT, "spatial_engine", "utils", "scannet_utils")


FACADE_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multi-spatialmllm_amd", "spatial_engine", "utils", "scannet_utils")


def load_facade(name):
    """A drop-in module of THIS repository by file path under a private name: other tests import the reference, which owns the
    package name ``spatial_engine`` in this process from then on."""
    spec = importlib.util.spec_from_file_location("_mspa_facade_" + name, os.path.join(FACADE_DIR, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_available():
    return os.path.isfile(os.path.join(REF_DIR, "batch_load_scannet_data.py"))


def plyfile_stand_in():
    """A module object with the one thing the reference uses: ``PlyData.read(f)["vertex"]`` with ``.count`` and ``.data``."""
    mod = types.ModuleType("plyfile")

    class PlyData(dict):
        @staticmethod
        def read(f):
            data = scanprep.read_ply_vertices(getattr(f, "name", "<stream>"), f.read())
            return PlyData(vertex=types.SimpleNamespace(count=data.shape[0], data=data))

    mod.PlyData = PlyData
    return mod


def import_reference():
    """(batch_load_scannet_data, scannet_utils) of the reference, loaded by path under private names."""
    saved = {k: sys.modules.get(k) for k in ("plyfile", "scannet_utils")}
    sys.modules["plyfile"] = plyfile_stand_in()
    try:
        mods = []
        for name in ("scannet_utils", "batch_load_scannet_data"):
            spec = importlib.util.spec_from_file_location(name if name == "scannet_utils" else "_ref_" + name, os.path.join(REF_DIR, name + ".py"))
            mod = importlib.util.module_from_spec(spec)
            if name == "scannet_utils":
                sys.modules["scannet_utils"] = mod               # batch_load_scannet_data imports it by this name
            spec.loader.exec_module(mod)
            mods.append(mod)
        return mods[1], mods[0]
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def fma_chain_row(m, x, y, z):
    """m0*x, fma(m1,y,.), fma(m2,z,.), fma(m3,1.0,.) with every step rounded once (exact rationals in between)."""
    acc = float(m[0]) * float(x)
    for coeff, v in ((m[1], y), (m[2], z), (m[3], 1.0)):
        acc = float(Fraction(float(coeff)) * Fraction(float(v)) + Fraction(acc))
    return acc


def _boxes_by_masks(points, tables, inst):
    """Boxes and clouds with nothing shared with the code under test: one boolean mask over all vertices per object, NumPy's own
    reductions in the points' dtype, the row stored into a float64 table (SU:69-94 in other words)."""
    ids = list(tables.object_id_to_segs)
    boxes = np.zeros((len(set(ids)), 7), dtype=np.float64)
    clouds = [None for _ in range(len(set(ids)))]
    for oid in ids:
        label = tables.object_id_to_label_id[oid]
        cloud = points[inst == oid]
        if cloud.shape[0] == 0:
            continue
        low, high = cloud[:, :3].min(axis=0), cloud[:, :3].max(axis=0)
        assert low.dtype == points.dtype
        boxes[oid - 1, 0:3] = (low + high) / 2.0
        boxes[oid - 1, 3:6] = high - low
        boxes[oid - 1, 6] = label
        clouds[oid - 1] = cloud
    return boxes, clouds


def numpy_export(scan):
    """``export()`` restated over the per-segment tables, in the order the kernels work: gather, affine map, per-object extents,
    stable split.  Returns a ``scanprep.ScanResult``."""
    t, seg, v = scan.tables, scan.seg, scan.vertices
    inside = seg < t.seg2inst.shape[0]                       # a segment beyond the tables is one no object lists
    s = np.where(inside, seg, 0)
    inst = np.where(inside, np.append(t.seg2inst, 0)[s], 0).astype(np.uint32)
    index = np.where(inside, np.append(t.seg2label, 0)[s], 0)
    pts = np.ones((v.shape[0], 4))
    pts[:, :3] = v[:, :3]
    aligned = np.concatenate([np.dot(pts, scan.axis_align_matrix.transpose())[:, :3], v[:, 3:]], axis=1)
    ub, uc = _boxes_by_masks(v, t, inst)
    ab, ac = _boxes_by_masks(aligned, t, inst)
    return scanprep.ScanResult(v, aligned, t.label_value[index], t.label_names[index], inst, ub, ab, uc, ac, t.object_id_to_raw_category,
                               t.object_id_to_label_id, scan.axis_align_matrix, len(np.unique(inst)))


def same_array(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return bool((a == b).all()) if a.dtype == object else a.tobytes() == b.tobytes()


def assert_same_export(got, ref):
    """Two twelve-tuples of ``export()``: arrays with equal dtype, shape and bytes; dicts with equal keys, order and values."""
    names = ("mesh_vertices", "aligned_mesh_vertices", "label_ids", "raw_categories", "instance_ids", "unaligned_bboxes", "aligned_bboxes",
             "unaligned_obj_point_clouds", "aligned_obj_point_clouds", "object_id_to_raw_category", "object_id_to_label_id", "axis_align_matrix")
    assert len(got) == len(ref) == 12
    for name, g, r in zip(names, got, ref):
        if isinstance(r, list):
            assert isinstance(g, list) and len(g) == len(r), name
            for k, (x, y) in enumerate(zip(g, r)):
                assert same_array(x, y), f"{name}[{k}]"
        elif isinstance(r, dict):
            assert list(g.keys()) == list(r.keys()), name
            for k in r:
                assert type(g[k]) is type(r[k]) and g[k] == r[k], f"{name}[{k}]"
        else:
            assert same_array(g, r), name
