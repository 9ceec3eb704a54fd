"""Freeze the reference's scan preparation on three synthetic raw scans into tests/golden/scanprep.npz (data only).

Runs the unmodified reference (``batch_export`` -> ``export_one_scan``) under the plyfile stand-in of tests/scanprep_util.py.
Inputs are stored as the raw file bytes (uint8), outputs as the arrays the reference wrote; the unaligned points and the per-object
point files, which repeat the input or rows of the point arrays, as the SHA-256 of their .npy bytes.  Needs the reference tree (MSPA_REFERENCE_ROOT)."""
import hashlib
import os
import pickle
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "multi-spatialmllm_amd"), ROOT):
    sys.path.insert(0, p)

import scanprep_util as U  # noqa: E402
from mspa import synth  # noqa: E402

# a coarse grid and fewer vertices where the alignment fills every mantissa bit: the file has to stay small
SCANS = (("scene0900_00", dict(n_vertices=20000, n_objects=24, seed=11, axis_align=None, quantum=1.0 / 32)),
         ("scene0901_00", dict(n_vertices=16021, n_objects=17, seed=12, axis_align="z", quantum=1.0 / 32)),
         ("scene0902_00", dict(n_vertices=9001, n_objects=9, seed=13, axis_align="general", quantum=1.0 / 32)))
INPUTS = (("ply", "mesh_file"), ("segs", "seg_file"), ("agg", "agg_file"), ("txt", "meta_file"))


def main(out_path):
    BL, _ = U.import_reference()
    root = tempfile.mkdtemp(prefix="scanprep_golden_")
    scans, out = os.path.join(root, "scans"), os.path.join(root, "out")
    data = {"scan_names": np.array([n for n, _ in SCANS])}
    for name, kw in SCANS:
        paths = synth.write_raw_scan(scans, name, **kw)
        for key, which in INPUTS:
            data[f"in_{name}_{key}"] = np.fromfile(paths[which], dtype=np.uint8)
    data["in_labels"] = np.fromfile(paths["label_map_file"], dtype=np.uint8)
    names_file = os.path.join(root, "names.txt")
    open(names_file, "w").write("\n".join(n for n, _ in reversed(SCANS)) + "\n")
    BL.Pool = __import__("multiprocessing.dummy", fromlist=["Pool"]).Pool         # same map(), no fork of this process
    BL.batch_export(None, out, names_file, paths["label_map_file"], scans, test_mode=False, num_workers=1)
    info = pickle.load(open(os.path.join(out, "scenes_train_val_info.pkl"), "rb"))
    assert list(info) == sorted(n for n, _ in SCANS)
    for name, _ in SCANS:
        d = os.path.join(out, name)
        for f in ("aligned_points", "semantic_mask", "instance_mask"):
            data[f"out_{name}_{f}"] = np.load(os.path.join(d, f + ".npy"))
        # the unaligned points repeat the PLY's vertex element (an input above): their .npy bytes as a digest
        data[f"out_{name}_unaligned_points_sha256"] = np.array(hashlib.sha256(open(os.path.join(d, "unaligned_points.npy"), "rb").read()).hexdigest())
        raw = np.load(os.path.join(d, "raw_category_mask.npy"), allow_pickle=True)
        cats = sorted({c for c in raw.tolist() if c is not None})
        data[f"out_{name}_raw_names"] = np.array(cats)
        data[f"out_{name}_raw_index"] = np.array([-1 if c is None else cats.index(c) for c in raw.tolist()], dtype=np.int16)
        si = info[name]
        n = si["num_objects"]
        data[f"out_{name}_aligned_bbox"] = np.stack([si[k]["aligned_bbox"] for k in range(n)])
        data[f"out_{name}_unaligned_bbox"] = np.stack([si[k]["unaligned_bbox"] for k in range(n)])
        data[f"out_{name}_object_category"] = np.array([si[k]["raw_category"] for k in range(n)])
        data[f"out_{name}_axis_align_matrix"] = si["axis_align_matrix"]
        data[f"out_{name}_object_sha256"] = np.array([[hashlib.sha256(open(os.path.join(d, f"object_{k}_{w}_points.npy"), "rb").read()).hexdigest()
                                                       for w in ("aligned", "unaligned")] for k in range(n)])
    np.savez_compressed(out_path, **data)
    print(out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "scanprep.npz"))
