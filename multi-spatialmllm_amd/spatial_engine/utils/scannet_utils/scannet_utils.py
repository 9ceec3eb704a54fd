"""Drop-in for the reference's ``utils/scannet_utils/scannet_utils.py``: same names, arguments and return values, no ``plyfile``.

The readers live in ``mspa/scanprep.py``; ``extract_bbox`` keeps upstream's contract (it is a host function of arrays the caller
already holds -- the batched path of ``batch_load_scannet_data.py`` computes the same boxes on the device instead)."""
from __future__ import annotations

import os

import numpy as np

from mspa import scanprep
from mspa.scanprep import read_aggregation, read_label_mapping, read_mesh_vertices, represents_int  # noqa: F401


def read_mesh_vertices_rgb(filename):
    """XYZ and RGB (0-255) of every vertex, [N, 6] float32."""
    assert os.path.isfile(filename)
    return scanprep.read_mesh_vertices_rgb(filename)


def read_segmentation(filename):
    """``(seg_to_verts, num_verts)``: segment id -> ascending list of its vertices, keys in order of first appearance."""
    assert os.path.isfile(filename)
    seg = scanprep.read_seg_indices(filename)
    order = np.argsort(seg, kind="stable")
    ids, starts = np.unique(seg[order], return_index=True)
    groups = np.split(order, starts[1:]) if ids.size else []
    by_first = np.argsort([g[0] for g in groups], kind="stable") if groups else []
    return {int(ids[k]): groups[k].tolist() for k in by_first}, int(seg.shape[0])


def extract_bbox(mesh_vertices, object_id_to_segs, object_id_to_label_id, instance_ids):
    """Per object ``[(min + max) / 2, max - min, label_id]`` over its vertices and the vertices themselves (None without any);
    row ``object_id - 1``."""
    num_instances = len(np.unique(list(object_id_to_segs.keys())))
    instance_bboxes = np.zeros((num_instances, 7))
    instance_pcs = [None] * num_instances
    for obj_id in object_id_to_segs:
        label_id = object_id_to_label_id[obj_id]
        cloud = mesh_vertices[instance_ids == obj_id, :]
        if len(cloud) == 0:
            print(f"WARNING: object id {obj_id} does not have points. Corresponding entry is set to None.")
            continue
        lo, hi = np.min(cloud[:, 0:3], axis=0), np.max(cloud[:, 0:3], axis=0)
        instance_bboxes[obj_id - 1, :] = np.concatenate([(lo + hi) / 2.0, hi - lo, np.array([label_id])])
        instance_pcs[obj_id - 1] = cloud
    return instance_bboxes, instance_pcs
