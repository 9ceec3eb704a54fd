"""Stage timings of the scan preparation on synthetic raw scans: read, parse, upload, kernels, download, write -- and the
``segIndices`` parse on the device against the native host threads.  For comparison the same scans go through a plain NumPy
restatement of the reference's export (below; the per-vertex Python loops replaced by their vectorised equivalents, so this is a
FASTER baseline than the reference itself) on one core and on the quota's cores.  Prints a markdown table; medians of the warm passes.

    python tools/scanprep_bench.py --scans 64 --vertices 150000 --passes 4 > profiles/scanprep.md
"""
import argparse
import contextlib
import io
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
from concurrent.futures import ProcessPoolExecutor, ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "multi-spatialmllm_amd"), ROOT):
    sys.path.insert(0, p)

from mspa import engine, hostinfo, scanprep, synth  # noqa: E402


def numpy_scan(args):
    """One scan the reference's way, vectorised: json.load, masks per object, np.dot, np.save."""
    files, label_map, out = args
    v = scanprep.read_mesh_vertices_rgb(files["mesh_file"])
    A = scanprep.read_axis_alignment(files["meta_file"])
    pts = np.ones((v.shape[0], 4))
    pts[:, :3] = v[:, :3]
    aligned = np.concatenate([np.dot(pts, A.T)[:, :3], v[:, 3:]], axis=1)
    o2s, l2s = scanprep.read_aggregation(files["agg_file"])
    seg = np.asarray(json.load(open(files["seg_file"]))["segIndices"])
    label_ids, inst = np.zeros(seg.shape[0], np.uint32), np.zeros(seg.shape[0], np.uint32)
    raw_categories = np.array([None] * seg.shape[0])
    for raw, segs in l2s.items():
        m = np.isin(seg, segs)
        label_ids[m] = label_map[raw]
        raw_categories[m] = raw
    for oid, segs in o2s.items():
        inst[np.isin(seg, segs)] = oid
    os.makedirs(out, exist_ok=True)
    for arr in (v, aligned):
        for oid in o2s:
            m = inst == oid
            if m.any():
                pc = arr[m]
                np.concatenate([(pc[:, :3].min(0) + pc[:, :3].max(0)) / 2.0, pc[:, :3].max(0) - pc[:, :3].min(0)])
                np.save(os.path.join(out, f"object_{oid - 1}_{'aligned' if arr is aligned else 'unaligned'}_points.npy"), pc)
    np.save(os.path.join(out, "unaligned_points.npy"), v)
    np.save(os.path.join(out, "aligned_points.npy"), aligned)
    np.save(os.path.join(out, "semantic_mask.npy"), label_ids)
    np.save(os.path.join(out, "instance_mask.npy"), inst)
    np.save(os.path.join(out, "raw_category_mask.npy"), raw_categories)
    return v.shape[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=64)
    ap.add_argument("--vertices", type=int, default=150000)
    ap.add_argument("--objects", type=int, default=40)
    ap.add_argument("--passes", type=int, default=4)
    a = ap.parse_args()
    from spatial_engine.utils.scannet_utils import batch_load_scannet_data as BL
    root = tempfile.mkdtemp(prefix="scanprep_bench_")
    cpus = hostinfo.effective_cpus()
    try:
        names = [f"scene{k:04d}_00" for k in range(a.scans)]
        for k, n in enumerate(names):
            paths = synth.write_raw_scan(os.path.join(root, "scans"), n, a.vertices, a.objects, seed=k)
        label_map = scanprep.read_label_mapping(paths["label_map_file"])
        names_file = os.path.join(root, "names.txt")
        open(names_file, "w").write("\n".join(names) + "\n")
        files = [scanprep.scan_files(os.path.join(root, "scans"), n) for n in names]
        dev = scanprep.default_device()
        rows = {}
        for p in range(a.passes + 1):                                 # pass 0 warms up (page cache, allocator, kernels)
            t = {}
            with ThreadPoolExecutor(cpus) as pool:
                t0 = time.perf_counter()
                blobs = list(pool.map(lambda f: (open(f["mesh_file"], "rb").read(), open(f["seg_file"], "rb").read()), files))
                t["read"] = time.perf_counter() - t0
                t0 = time.perf_counter()
                scans = list(pool.map(lambda f: scanprep.load_raw_scan("s", label_map=label_map, **f), files))
                t["read + parse (host threads)"] = time.perf_counter() - t0
            texts = [b[1][slice(*scanprep.seg_indices_span(b[1]))] for b in blobs]
            t0 = time.perf_counter()
            got = engine.parse_int_lists(texts, n_threads=cpus)
            t["segIndices: native host threads"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            vals, off, status = engine.parse_int_lists_device(texts, dev)
            host = vals.cpu()
            t["segIndices: device (upload + kernels + download)"] = time.perf_counter() - t0
            assert not status.any() and np.array_equal(host.numpy()[:got[0].size], got[0])
            stage = {}
            out = os.path.join(root, "out")
            with contextlib.redirect_stdout(io.StringIO()):           # the stage prints upstream's per-object warnings
                results = scanprep.prepare_window(scans, dev, timings=stage)
                t.update({k: v for k, v in stage.items()})
                t0 = time.perf_counter()
                with ThreadPoolExecutor(cpus) as pool:                # as batch_export writes: plans in order, saves on the threads
                    jobs = [pool.submit(BL._save_all, BL._plan_scan(n, os.path.join(out, n), None, False, r)[1]) for n, r in zip(names, results)]
                    for j in jobs:
                        j.result()
                t["write (saves on the host threads)"] = time.perf_counter() - t0
                shutil.rmtree(out)
                del results, scans
                for label, dp in (("batch_export end to end", False), ("batch_export end to end, device_seg_parse", True)):
                    t0 = time.perf_counter()
                    BL.batch_export(None, out, names_file, paths["label_map_file"], os.path.join(root, "scans"), num_workers=cpus, device_seg_parse=dp)
                    t[label] = time.perf_counter() - t0
                    shutil.rmtree(out)
            if p:
                for k, v in t.items():
                    rows.setdefault(k, []).append(v)
        base = {}
        work = [(f, label_map, os.path.join(root, "np", n)) for f, n in zip(files, names)]
        for label, n_proc in (("NumPy restatement, 1 core", 1), (f"NumPy restatement, {cpus} processes", cpus)):
            sub = work if n_proc > 1 else work[:max(4, a.scans // 8)]
            t0 = time.perf_counter()
            if n_proc == 1:
                for w in sub:
                    numpy_scan(w)
            else:
                with ProcessPoolExecutor(n_proc) as pool:
                    list(pool.map(numpy_scan, sub))
            base[label] = (time.perf_counter() - t0) * len(work) / len(sub)
            shutil.rmtree(os.path.join(root, "np"))
        print(f"# Scan preparation: {a.scans} synthetic scans of {a.vertices} vertices, {a.objects} objects ({cpus} host CPUs)\n")
        print(f"Medians of {a.passes} warm passes, one window (one launch per kernel), seconds for all scans.  The stage rows are timed one after")
        print("the other with a device synchronisation in between and do not add up to a wall time; `batch_export end to end` is the")
        print("product's own call, start to finish (reads, parse, launches, assembly, draws, saves, pickle), on the same files.\n")
        print("| stage | seconds |\n|---|---|")
        for k, v in rows.items():
            print(f"| {k} | {statistics.median(v):.4f} |")
        for k, v in base.items():
            print(f"| {k} (whole stage, scaled to all scans) | {v:.3f} |")
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
