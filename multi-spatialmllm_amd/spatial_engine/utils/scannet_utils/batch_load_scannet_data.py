"""Drop-in for the reference's ``utils/scannet_utils/batch_load_scannet_data.py``: raw ScanNet scans -> the instance data every
later stage reads (``aligned_points.npy``, the three masks, ``object_<k>_*_points.npy``, ``scenes_train_val_info.pkl``).

Same functions, arguments and files; every numeric ``.npy`` has the reference's bytes, ``raw_category_mask.npy`` and the pickle its
values.  What differs is where the work happens: scans are read and parsed on host threads, and WINDOWS of scans go through one
launch of each K11 kernel (``mspa/scanprep.py``, ``csrc/scene_prep.hip``).  Also different: the ``segIndices`` list is parsed
natively from its byte span once the REST of the ``segs.json`` has passed ``json.loads`` (any file the span search is unsure of
goes to ``json.loads`` whole, which then raises what upstream raises); NaN coordinates and signed zeros in a box are not
reproduced; scans need a GPU, and a missing one is an error.
"""
from __future__ import annotations

import argparse
import os
import pickle
from concurrent.futures import ThreadPoolExecutor
from os import path as osp

import numpy as np

from mspa import hostinfo, scanprep

DONOTCARE_CLASS_IDS = np.array([])
WINDOW_SCANS = 64                      # scans per launch
WINDOW_VERTICES = 12_000_000           # ... or this many vertices (~1.5 GB of device memory for points, labels and results)
WINDOW_ROW_WORDS = 16_000_000          # ... or this many words of membership rows: object slots of the window x words of its longest
                                       # scan (the rows are dense; with K9's counts and offsets 28 bytes per word, ~450 MB)


def export(mesh_file, agg_file, seg_file, meta_file, label_map_file, test_mode=False):
    """One scan -> the reference's twelve-tuple: vertices, aligned vertices, label ids, raw categories, instance ids, unaligned
    and aligned boxes, unaligned and aligned object point clouds, object id -> raw category, object id -> label id, axis
    alignment matrix (everything past the second entry is None in test mode)."""
    label_map = scanprep.read_label_mapping(label_map_file, label_from="raw_category", label_to="nyu40id")
    scan = scanprep.load_raw_scan(osp.basename(mesh_file), mesh_file, agg_file, seg_file, meta_file, label_map, test_mode)
    return scanprep.prepare_window([scan], scanprep.default_device(), test_mode)[0].as_tuple()


def _plan_scan(scan_name, output_filename_prefix, max_num_point, test_mode, result):
    """BL:171-251 on one scan's results, up to the files: the same prints, the same draw from NumPy's global stream.  Returns the
    scan's info entry and the ``(path, array)`` pairs still to be saved -- the saves draw nothing, so they may run on any thread."""
    os.makedirs(output_filename_prefix, exist_ok=True)
    mesh_vertices, semantic_labels, instance_labels, raw_categories = (result.mesh_vertices, result.label_ids, result.instance_ids,
                                                                       result.raw_categories)
    if not test_mode:
        print(f"Num of instances: {result.num_unique_instances - 1}")
        assert result.unaligned_bboxes.shape[0] == result.aligned_bboxes.shape[0]
        print(f"Num of care instances: {result.unaligned_bboxes.shape[0]}")
    if max_num_point is not None:
        max_num_point = int(max_num_point)
        N = mesh_vertices.shape[0]
        if N > max_num_point:
            choices = np.random.choice(N, max_num_point, replace=False)
            mesh_vertices = mesh_vertices[choices, :]                 # upstream leaves the aligned points unsampled
            if not test_mode:
                semantic_labels, instance_labels, raw_categories = semantic_labels[choices], instance_labels[choices], raw_categories[choices]
    saves = [(f"{output_filename_prefix}/unaligned_points.npy", mesh_vertices),
             (f"{output_filename_prefix}/aligned_points.npy", result.aligned_mesh_vertices)]
    scene_info = {}
    if not test_mode:
        saves += [(f"{output_filename_prefix}/semantic_mask.npy", semantic_labels), (f"{output_filename_prefix}/instance_mask.npy", instance_labels),
                  (f"{output_filename_prefix}/raw_category_mask.npy", raw_categories)]
        assert len(semantic_labels) == len(instance_labels) == len(raw_categories) == len(mesh_vertices), \
            "Lengths of semantic_labels, instance_labels, raw_categories, and mesh_vertices are not equal."
        for obj_id, (aligned_bbox, unaligned_bbox) in enumerate(zip(result.aligned_bboxes, result.unaligned_bboxes)):
            raw_category_name = result.object_id_to_raw_category.get(obj_id + 1, "None")
            if raw_category_name == "None":
                print(f"Something wrong for the raw category name of object {obj_id} in scan {scan_name}.")
                exit(0)
            scene_info[obj_id] = {"aligned_bbox": aligned_bbox, "unaligned_bbox": unaligned_bbox, "raw_category": raw_category_name}
            saves += [(f"{output_filename_prefix}/object_{obj_id}_aligned_points.npy", result.aligned_obj_point_clouds[obj_id]),
                      (f"{output_filename_prefix}/object_{obj_id}_unaligned_points.npy", result.unaligned_obj_point_clouds[obj_id])]
        scene_info["axis_align_matrix"] = result.axis_align_matrix
        scene_info["num_objects"] = len(result.aligned_bboxes)
    return {scan_name: scene_info}, saves


def _save_all(saves):
    for path, array in saves:
        np.save(path, array)


def _write_scan(scan_name, output_filename_prefix, max_num_point, test_mode, result):
    info, saves = _plan_scan(scan_name, output_filename_prefix, max_num_point, test_mode, result)
    _save_all(saves)
    return info


def _load(scan_name, label_map, scannet_dir, test_mode, defer_seg_parse=False):
    return scanprep.load_raw_scan(scan_name, label_map=label_map, test_mode=test_mode, defer_seg_parse=defer_seg_parse,
                                  **scanprep.scan_files(scannet_dir, scan_name))


def export_one_scan(scan_name, output_filename_prefix, max_num_point, label_map_file, scannet_dir, test_mode=False):
    label_map = scanprep.read_label_mapping(label_map_file, label_from="raw_category", label_to="nyu40id")
    scan = _load(scan_name, label_map, scannet_dir, test_mode)
    result = scanprep.prepare_window([scan], scanprep.default_device(), test_mode)[0]
    return _write_scan(scan_name, output_filename_prefix, max_num_point, test_mode, result)


def worker(args):
    scan_name, output_filename_prefix, max_num_point, label_map_file, scannet_dir, test_mode = args
    print("-" * 20 + f"begin for {scan_name}.")
    return export_one_scan(scan_name, output_filename_prefix, max_num_point, label_map_file, scannet_dir, test_mode)


def _windows(scans):
    window, vertices, slots, words = [], 0, 0, 0
    for s in scans:
        n, k = s.vertices.shape[0], (s.tables.n_slots if s.tables is not None else 0)
        w = max(words, (n + 63) // 64)
        if window and (len(window) >= WINDOW_SCANS or vertices + n > WINDOW_VERTICES or (slots + k) * w > WINDOW_ROW_WORDS):
            yield window
            window, vertices, slots, w = [], 0, 0, (n + 63) // 64
        window.append(s)
        vertices, slots, words = vertices + n, slots + k, w
    if window:
        yield window


def batch_export(max_num_point, output_folder, scan_names_file, label_map_file, scannet_dir, test_mode=False, num_workers=20,
                 device_seg_parse=False):
    """All scans of ``scan_names_file``.  ``num_workers`` host threads (at most the CPUs this process may use) read and parse;
    windows of scans run through one launch each; draws are made in sorted scan order on the calling thread, the ``np.save``
    calls run on the same threads, and the next group of scans is read while the current one computes and writes.
    ``device_seg_parse``: parse the ``segIndices`` text on the device as well (opt-in: DESIGN.md section 0.13)."""
    if test_mode and not os.path.exists(scannet_dir):
        return
    os.makedirs(output_folder, exist_ok=True)
    scan_names = sorted(line.rstrip() for line in open(scan_names_file))
    label_map = scanprep.read_label_mapping(label_map_file, label_from="raw_category", label_to="nyu40id")
    device = scanprep.default_device()
    n_threads = max(1, min(int(num_workers), hostinfo.effective_cpus()))
    all_scene_info = {}
    groups = [scan_names[first:first + WINDOW_SCANS] for first in range(0, len(scan_names), WINDOW_SCANS)]

    def load(names):
        return [pool.submit(_load, n, label_map, scannet_dir, test_mode, device_seg_parse) for n in names]

    with ThreadPoolExecutor(n_threads) as pool:
        writes = []
        ahead = load(groups[0]) if groups else []
        for g, names in enumerate(groups):
            for name in names:
                print("-" * 20 + f"begin for {name}.")
            loaded = [f.result() for f in ahead]
            ahead = load(groups[g + 1]) if g + 1 < len(groups) else []     # the next group is read and parsed while this one computes and writes
            for done in writes:                                            # at most one group's arrays wait for the disk
                done.result()
            writes = []
            scanprep.finish_deferred(loaded, label_map, device)            # device_seg_parse: one pass over the group's texts
            for window in _windows(loaded):
                results = scanprep.prepare_window(window, device, test_mode)
                for scan, result in zip(window, results):          # in order: max_num_point draws from the global NumPy stream ...
                    info, saves = _plan_scan(scan.name, osp.join(output_folder, scan.name), max_num_point, test_mode, result)
                    all_scene_info.update(info)
                    writes.append(pool.submit(_save_all, saves))   # ... the saves draw nothing and go to the threads
        for done in writes:
            done.result()
    file_name = "scenes_test_info.pkl" if test_mode else "scenes_train_val_info.pkl"
    with open(osp.join(output_folder, file_name), "wb") as f:
        pickle.dump(all_scene_info, f)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--max_num_point", default=None, help="The maximum number of the points.")
    parser.add_argument("--output_folder", default="data/scannet/scannet_instance_data", help="output folder of the result.")
    parser.add_argument("--train_scannet_dir", default="scans", help="scannet data directory.")
    parser.add_argument("--test_scannet_dir", default="scans_test", help="scannet data directory.")
    parser.add_argument("--label_map_file", default="data/scannet/meta_data/scannetv2-labels.combined.tsv", help="The path of label map file.")
    parser.add_argument("--train_scan_names_file", default="data/scannet/meta_data/scannet_train.txt",
                        help="The path of the file that stores the scan names.")
    parser.add_argument("--test_scan_names_file", default="data/scannet/meta_data/scannetv2_test.txt",
                        help="The path of the file that stores the scan names.")
    args = parser.parse_args()
    batch_export(args.max_num_point, args.output_folder, args.train_scan_names_file, args.label_map_file, args.train_scannet_dir, test_mode=False)
    args.output_folder = args.output_folder.replace("scannet", "scannet_test")
    batch_export(args.max_num_point, args.output_folder, args.test_scan_names_file, args.label_map_file, args.test_scannet_dir, test_mode=True)


if __name__ == "__main__":
    main()
