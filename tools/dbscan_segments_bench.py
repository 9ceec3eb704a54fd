#!/usr/bin/env python3
"""DBSCAN of every object cloud of a scene: ``dbscan_segments`` and ``largest_cluster_segments`` on the fused per-object clouds
thinned at several voxel sizes and on the per-image batch, their stages, and the loop of ``sklearn.cluster.DBSCAN`` over the same
segments for scale.  Prints markdown (profiles/dbscan_segments_device.md).

    python tools/dbscan_segments_bench.py [--passes 5] [--frames 64] [--objects 30] [--sizes 0.005,0.01,0.02] [--slow 4] [--sklearn-budget 45]

The scene is tools/cloud_segments_bench.py's: ``--frames`` frames at ScanNet's shape with about ``--objects`` objects per frame, from
files; ``instance_clouds`` and the batches are built once, outside every timed window.  Per batch and parameter set: one warm-up pass
of each line, then the lines alternate; medians of the timed passes, all listed; a host clock around work that ends in a device
synchronise.  A batch whose warm-up pass takes more than ``--slow`` seconds is timed with ONE pass per line, and the table says so:
the cost of a point grows with the rows of the 27 cells around it, and an un-thinned batch is there to be written down, not to be
waited for.  The scikit-learn loop (``algorithm="kd_tree", n_jobs=16``, download included) runs over the same segments in
descending size until ``--sklearn-budget`` seconds have passed; where it stops early the table gives the rows it covered, and no
extrapolation.  Where scikit-learn is not installed the line says so."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "multi-spatialmllm_amd"), ROOT, os.path.join(ROOT, "tools")]
NB, RATIO = 20, 1.0
PARAMETERS = ((0.03, 10), (0.05, 20))


def fmt(xs):
    return ", ".join(f"{x * 1e3:.1f}" for x in xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--objects", type=int, default=30)
    ap.add_argument("--sizes", default="0.005,0.01,0.02")
    ap.add_argument("--slow", type=float, default=4.0)
    ap.add_argument("--sklearn-budget", type=float, default=45.0)
    ap.add_argument("--no-image-batch", action="store_true")
    args = ap.parse_args()
    sizes = [float(s) for s in args.sizes.split(",")]
    import torch
    from cloud_segments_bench import build_scene
    from mspa import _lib, cloud_segments as CS, instances
    from mspa.engine import _ptr, _stream_ptr, _workspace
    try:
        from sklearn.cluster import DBSCAN
    except ImportError:
        DBSCAN = None
    handler, sid, _ids = build_scene(args.frames, args.objects)
    clouds = handler.instance_clouds(sid, num_workers=16)
    assert instances.LAST_INSTANCE_CLOUDS["path"] == "device", instances.LAST_INSTANCE_CLOUDS
    lib = _lib.load()
    info = _lib.device_info(0)
    # the scene carries no annotation: every object's ground-truth box is the box of its own fused, un-cleaned points, so the IoU
    # below says how much of that box a cleaned (and clustered) cloud still spans -- not how well boxes fit a real scan's annotation
    object_ids = clouds.by_object()[2]
    handler.infos[sid]["num_objects"] = int(object_ids.max()) + 1 if len(object_ids) else 0
    for t in range(handler.infos[sid]["num_objects"]):
        pts = clouds.object_cloud(t)[:, :3]
        box = torch.cat([(pts.amax(0) + pts.amin(0)) / 2, pts.amax(0) - pts.amin(0)]).cpu().numpy() if len(pts) else np.array([1e6, 1e6, 1e6, 1.0, 1.0, 1.0])
        handler.infos[sid][t] = {"aligned_bbox": np.concatenate([box, [1.0]])}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def staged(rows, off, eps, m, clock):
        """The op's own steps, each alone with a synchronise behind it."""
        N, S = int(rows.shape[0]), off.size - 1
        xyz = rows[:, :3].contiguous()
        tile_base = np.zeros((S + 1,), dtype=np.int64)
        _lib.check(lib.mspa_voxel_segments_tables_host(off.ctypes.data, S, tile_base.ctypes.data))
        o_dev, base_dev = CS._upload(off, tile_base, device=rows.device)
        keys = torch.empty((N,), dtype=torch.int64, device=rows.device)
        segment = torch.empty((N,), dtype=torch.int32, device=rows.device)
        seg = torch.empty((2 * S + 1,), dtype=torch.int32, device=rows.device)
        labels = torch.empty((N,), dtype=torch.int32, device=rows.device)
        keep = torch.empty((N,), dtype=torch.uint8, device=rows.device)
        lo, hi = torch.empty((S, 3), dtype=torch.float64, device=rows.device), torch.empty((S, 3), dtype=torch.float64, device=rows.device)
        cells = _workspace(int(lib.mspa_voxel_segments_workspace_bytes(off.ctypes.data, S)), rows.device)
        work = _workspace(int(lib.mspa_dbscan_segments_workspace_bytes(off.ctypes.data, S)), rows.device)
        t_keys = wall(lambda: _lib.check(lib.mspa_voxel_segments_keys_device(
            _ptr(xyz), 3, off.ctypes.data, S, lib.mspa_dbscan_cell_side(eps), _ptr(o_dev), _ptr(base_dev), _ptr(keys), _ptr(segment), _ptr(seg[S:]),
            _ptr(cells), int(cells.numel()), _stream_ptr())))[0]

        def sorts():
            order = torch.sort(keys, stable=True).indices
            return order.gather(0, torch.sort(segment.gather(0, order), stable=True).indices) if S > 1 else order
        t_sorts, order = wall(sorts)

        def device(keep_or_none):
            return wall(lambda: _lib.check(lib.mspa_dbscan_segments_device(
                _ptr(xyz), 3, off.ctypes.data, S, eps, m, _ptr(o_dev), _ptr(keys), _ptr(order), _ptr(base_dev), _ptr(labels), _ptr(keep_or_none),
                _ptr(lo), _ptr(hi), _ptr(seg), _ptr(work), int(work.numel()), _stream_ptr())))[0]
        t_labels, t_keep = device(None), device(keep)
        t_back = wall(lambda: seg.cpu().numpy())[0]
        clock.append((t_keys, t_sorts, t_labels, t_keep - t_labels, t_back))

    def sklearn_loop(rows, off, eps, m):
        """(seconds, rows covered, segments covered, all covered) of the host loop, largest segments first, within the budget."""
        t0 = time.perf_counter()
        host = rows[:, :3].cpu().numpy()
        done_rows = done = 0
        order = np.argsort(-np.diff(off), kind="stable")
        for s in order:
            a, b = int(off[s]), int(off[s + 1])
            if b == a:
                continue
            if time.perf_counter() - t0 > args.sklearn_budget:
                return time.perf_counter() - t0, done_rows, done, False
            DBSCAN(eps=eps, min_samples=m, algorithm="kd_tree", n_jobs=16).fit(host[a:b])
            done_rows += b - a
            done += 1
        return time.perf_counter() - t0, done_rows, done, True

    def mean_iou(out):
        iou = out["iou"].reshape(-1)
        ok = ~torch.isnan(iou)
        return (float(iou[ok].mean()), int(ok.sum())) if bool(ok.any()) else (float("nan"), 0)

    print("# DBSCAN of every object cloud of a scene: `dbscan_segments` and `largest_cluster_segments`\n")
    print(f"`python tools/dbscan_segments_bench.py --passes {args.passes} --frames {args.frames} --objects {args.objects} --sizes {args.sizes}` on one "
          f"{info['name']} ({info['n_cu']} CUs; the runtime reports a shader clock of {info['clock_khz'] / 1e3:.0f} MHz), one process.  "
          "`instance_clouds` and the batches are built once outside every timed window; per batch and parameter set one warm-up pass of each "
          "line, then the lines alternate; median of the timed passes (all listed, ms); a host clock around work that ends in a device "
          f"synchronise.  nb_neighbors = {NB}, std_ratio = {RATIO} where a cleaning runs.  The labels are scikit-learn's value for value "
          "(tests/test_dbscan_segments_cpu.py, tests/test_gpu_dbscan_segments.py); this file is about time.\n")
    batches = [(f"`by_object(voxel_size={size})`", "object", size) + clouds.by_object(size)[:2] for size in sizes]
    if not args.no_image_batch:
        batches.append(("the per-image batch (`InstanceClouds.rows`, un-thinned)", "image", None, clouds.rows, clouds.offsets))
    for name, per, size, rows, off in batches:
        N, S = int(rows.shape[0]), int((np.diff(off) > 0).sum())
        print(f"## {name}: {S:,} clouds, {N:,} rows\n")
        for eps, m in PARAMETERS:
            t_warm, (labels, clusters) = wall(lambda: CS.dbscan_segments(rows, off, eps, m))
            again = CS.dbscan_segments(rows, off, eps, m)[0]
            same = bool(torch.equal(labels, again))
            kept_offsets = CS.largest_cluster_segments(rows, off, eps, m)[1]
            noise = int((labels < 0).sum())
            del again
            passes = 1 if t_warm > args.slow else args.passes
            times = {"labels": [], "largest": []}
            stage_clock = []
            staged(rows, off, eps, m, [])
            for _ in range(passes):
                times["labels"].append(wall(lambda: CS.dbscan_segments(rows, off, eps, m))[0])
                times["largest"].append(wall(lambda: CS.largest_cluster_segments(rows, off, eps, m))[0])
                staged(rows, off, eps, m, stage_clock)
            print(f"### eps = {eps}, min_points = {m}\n")
            print(f"{int(clusters.sum()):,} clusters, {noise:,} noise rows; the largest clusters hold **{int(kept_offsets[-1]):,} rows** of {N:,}; two runs "
                  f"give equal labels: **{same}**." + (f"  The warm-up pass took {t_warm:.1f} s: ONE timed pass per line." if passes == 1 else "") + "\n")
            print("| line | median (ms) | passes (ms) |")
            print("|---|---|---|")
            print(f"| `dbscan_segments(rows, offsets, {eps}, {m})` | **{statistics.median(times['labels']) * 1e3:.1f}** | {fmt(times['labels'])} |")
            print(f"| `largest_cluster_segments(rows, offsets, {eps}, {m})` | **{statistics.median(times['largest']) * 1e3:.1f}** | {fmt(times['largest'])} |")
            if DBSCAN is None:
                print("| the scikit-learn loop | not measured: scikit-learn is not installed here | |")
            else:
                t_sk, sk_rows, sk_segments, whole = sklearn_loop(rows, off, eps, m)
                covered = "all segments" if whole else f"STOPPED at the budget after {sk_segments:,} segments, {sk_rows:,} rows ({100.0 * sk_rows / max(N, 1):.1f} %)"
                print(f"| `sklearn.cluster.DBSCAN(algorithm=\"kd_tree\", n_jobs=16)` looped, download included: {covered} | {t_sk * 1e3:.0f} | one pass |")
            print()
            print("| stage, alone with a synchronise behind it | median (ms) | passes (ms) |")
            print("|---|---|---|")
            stage_names = ("cells: extents and keys (section 0.24's kernels at the cell side)", "sorts (torch.sort by key, then by segment, gathers)",
                           "the nine launches of the labels (gather, core, link, roots, representatives, counts, labels)",
                           "the four further launches of the largest cluster and its extents (difference of the call with and without keep)",
                           "the read-back of the counts and the flag word")
            for j, stage in enumerate(stage_names):
                v = [c[j] for c in stage_clock]
                print(f"| {stage} | {statistics.median(v) * 1e3:.2f} | {fmt(v)} |")
            print()
            del labels
            torch.cuda.empty_cache()
        # what the step is for: boxes and IoU with and without it
        kw = dict(nb_neighbors=NB, std_ratio=RATIO, per=per, num_workers=16)
        if per == "object":
            kw["voxel_size"] = size
        plain = handler.instance_boxes(sid, **kw)
        print("| `instance_boxes` | rows kept | mean IoU (entries with an annotated object) |")
        print("|---|---|---|")
        iou, n = mean_iou(plain)
        print(f"| without `cluster` | {int(np.sum(plain['kept'])):,} | {iou:.4f} ({n}) |")
        for eps, m in PARAMETERS:
            out = handler.instance_boxes(sid, cluster=(eps, m), **kw)
            iou, n = mean_iou(out)
            print(f"| `cluster=({eps}, {m})` | {int(np.sum(out['kept'])):,} | {iou:.4f} ({n}) |")
        print()
        del rows
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
