#!/usr/bin/env python3
"""Cleaning and boxing every object cloud of a scene: the loop over the single-cloud functions against the batched pass of
``mspa.cloud_segments``.  Prints markdown (profiles/cloud_segments_device.md).

    python tools/cloud_segments_bench.py [--passes 5] [--frames 64] [--objects 30] [--trace]

The scene is tools/instance_clouds_bench.py's: ``--frames`` frames at ScanNet's shape (colour grid 1296 x 968, depth 640 x 480) with
about ``--objects`` objects per frame, from files; ``instance_clouds`` is built once, outside every timed window.
  (a) the loop a user writes today: for every present (image, object) ``ops.remove_statistical_outliers(clouds.cloud(i, t))`` and
      ``ops.calculate_aabb`` of the result;
  (b) ``clouds.cleaned()`` + ``boxes()``;
and the same pair for the per-object grouping (``object_cloud`` per object against ``cleaned_objects``).  Before anything is timed,
the kept rows of (a) and (b) are counted per segment and every difference is reported.  One warm-up pass of each, then the two
alternate; medians of the timed passes, all listed; a host clock around work that ends in a device synchronise.  The read-backs per
pass are torch's own synchronisation warnings, counted.  ``--trace`` runs one warm and one more pass of (b) and of the per-object batched form and nothing
else: the run to put under ``rocprofv3 --kernel-trace --stats``."""
import argparse
import os
import pickle
import statistics
import sys
import tempfile
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "multi-spatialmllm_amd"), ROOT, os.path.join(ROOT, "tools")]
NB, RATIO = 20, 1.0


def build_scene(frames, objects):
    """(handler, scene id, image ids) of instance_clouds_bench.py's scene (b), written under a temporary directory."""
    from PIL import Image
    from instance_clouds_bench import DHW, HW, label_map
    from mspa import synth
    from spatial_engine.utils.scannet_utils.handler.info_handler import SceneInfoHandler
    rng = np.random.default_rng(30)
    root = tempfile.mkdtemp(prefix="cloud_segments_bench_")
    distinct = 8
    seeds = os.path.join(root, "seed")
    os.makedirs(seeds)
    for k in range(distinct):
        Image.fromarray(label_map(rng, objects), mode="L").save(os.path.join(seeds, f"{k}.png"))
    sc = synth.make_scene(77, n_points=1024, n_frames=distinct, color_hw=HW, depth_hw=DHW, invalid_pose_frac=0.0, with_color=False,
                          scene_id="scene0977_00")
    base = sc.image_ids
    ids = [f"{k:05d}" for k in range(frames)]
    sc.E = {i: sc.E[base[k % distinct]] for k, i in enumerate(ids)}
    sc.depth = {i: sc.depth[base[k % distinct]] for k, i in enumerate(ids)}
    where = synth.write_scannet_layout([sc], root, link_identical=True)
    scans = os.path.join(root, "scans")
    os.makedirs(os.path.join(scans, sc.scene_id, "instance-filt"))
    for k, i in enumerate(ids):
        os.link(os.path.join(seeds, f"{k % distinct}.png"), os.path.join(scans, sc.scene_id, "instance-filt", f"{int(i)}.png"))
    handler = SceneInfoHandler(pickle.load(open(where["info_path"], "rb")), posed_images_root=where["posed_images_root"],
                               instance_data_root=where["instance_data_root"], mask_image_root=scans)
    return handler, sc.scene_id, ids


def fmt(xs):
    return ", ".join(f"{x * 1e3:.1f}" for x in xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--objects", type=int, default=30)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    import torch
    from mspa import _lib, cloud_segments as CS, instances
    from mspa.engine import _ptr, _stream_ptr, _workspace
    from spatial_engine.utils.scannet_utils.handler import ops
    handler, sid, ids = build_scene(args.frames, args.objects)
    clouds = handler.instance_clouds(sid, num_workers=16)
    assert instances.LAST_INSTANCE_CLOUDS["path"] == "device", instances.LAST_INSTANCE_CLOUDS
    present = [(i, t) for i in ids for t in clouds.present(i)]
    object_ids = clouds.by_object()[2]

    def loop_per_image():
        out = {}
        for i, t in present:
            kept = ops.remove_statistical_outliers(clouds.cloud(i, t), NB, RATIO)
            out[i, t] = (len(kept), ops.calculate_aabb(kept) if len(kept) else None)
        return out

    def batch_per_image():
        cleaned = clouds.cleaned(NB, RATIO)
        return cleaned, cleaned.boxes()

    def loop_per_object():
        out = {}
        for t in object_ids:
            kept = ops.remove_statistical_outliers(clouds.object_cloud(int(t)), NB, RATIO)
            out[int(t)] = (len(kept), ops.calculate_aabb(kept) if len(kept) else None)
        return out

    def batch_per_object():
        return clouds.cleaned_objects(NB, RATIO)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    if args.trace:
        for fn in (batch_per_image, batch_per_object, batch_per_image, batch_per_object):
            wall(fn)
        return

    def host_waits(fn):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        return sum("synchroniz" in str(w.message) for w in seen)

    # warm-up passes, which are also the equality check of the timed input
    want, (cleaned, boxes) = loop_per_image(), batch_per_image()
    differ = [(i, t) for i, t in present if want[i, t][0] != cleaned.count(i, t)]
    same_boxes = sum(bool(torch.equal(want[i, t][1], cleaned.aabb(i, t))) for i, t in present if want[i, t][0])
    want_o, (_rows_o, offsets_o, ids_o, _boxes_o) = loop_per_object(), batch_per_object()
    differ_o = [int(t) for j, t in enumerate(ids_o) if want_o[int(t)][0] != int(offsets_o[j + 1] - offsets_o[j])]
    rows, kept_rows = int(clouds.offsets[-1]), int(cleaned.offsets[-1])
    waits = {"a": host_waits(loop_per_image), "b": host_waits(batch_per_image), "ao": host_waits(loop_per_object), "bo": host_waits(batch_per_object)}
    times = {k: [] for k in ("a", "b", "ao", "bo")}
    for _ in range(args.passes):                              # alternately, in one process
        for key, fn in (("a", loop_per_image), ("b", batch_per_image), ("ao", loop_per_object), ("bo", batch_per_object)):
            times[key].append(wall(fn)[0])
    med = {k: statistics.median(v) for k, v in times.items()}

    print("# Cleaning and boxing every object cloud of a scene: the single-cloud loop against `mspa.cloud_segments`\n")
    print(f"`python tools/cloud_segments_bench.py --passes {args.passes} --frames {args.frames} --objects {args.objects}` on one MI355X, one "
          "process.  `instance_clouds` is built once outside every timed window; one warm-up pass of each line, then the lines alternate; "
          "median of the timed passes (all listed, ms); a host clock around work that ends in a device synchronise.  "
          f"nb_neighbors = {NB}, std_ratio = {RATIO}.\n")
    print(f"The timed input: {args.frames} frames, **{len(present)} (image, object) segments** of {clouds.counts.size} table entries, "
          f"**{rows:,} rows**, {kept_rows:,} kept; per object: {len(object_ids)} segments over the same rows.  Before timing, the kept "
          f"rows of (a) and (b) were counted per segment: they differ in **{len(differ)}** of the {len(present)} segments and in "
          f"**{len(differ_o)}** of the {len(object_ids)} per-object ones; {same_boxes} of the {sum(1 for v in want.values() if v[0])} boxes "
          "were bit-identical.\n")
    print("| line | median (ms) | passes (ms) | host waits per pass |")
    print("|---|---|---|---|")
    print(f"| (a) loop: `ops.remove_statistical_outliers(clouds.cloud(i, t))` + `ops.calculate_aabb`, per (image, object) | **{med['a'] * 1e3:.0f}** | "
          f"{fmt(times['a'])} | {waits['a']} |")
    print(f"| (b) `clouds.cleaned()` + `boxes()` | **{med['b'] * 1e3:.1f}** | {fmt(times['b'])} | {waits['b']} |")
    print(f"| (a) per object: the same loop over `clouds.object_cloud(t)` | **{med['ao'] * 1e3:.0f}** | {fmt(times['ao'])} | {waits['ao']} |")
    print(f"| (b) per object: `clouds.cleaned_objects()` | **{med['bo'] * 1e3:.1f}** | {fmt(times['bo'])} | {waits['bo']} |")
    print(f"\n(a) over (b): **{med['a'] / med['b']:.1f} x** per (image, object), **{med['ao'] / med['bo']:.1f} x** per object.\n")

    # the stages of (b), each with a synchronise behind it
    lib = _lib.load()
    off = clouds.offsets
    S, N = off.size - 1, rows
    xyz = clouds.rows[:, :3].contiguous()
    st = {k: [] for k in ("order statistics, boxes' read-back, grids and tables (torch.sort x 2, host)", "keys (seg_cells_kernel)",
                          "torch.sort of the keys", "search (seg_gather / seg_starts / seg_knn kernels)", "statistics (seg_stats_kernel)",
                          "compaction (kept counts' read-back, nonzero_static, index_select of rows and pixel)", "boxes()")}
    names = list(st)
    for k in range(args.passes + 1):
        t, (grids, off_dev, grids_dev, base_dev) = wall(lambda: CS._search_tables(xyz, off, NB))
        stage = [t]
        keys = torch.empty((N,), dtype=torch.int64, device="cuda")
        stage.append(wall(lambda: _lib.check(lib.mspa_knn_segments_cells_device(_ptr(xyz), off.ctypes.data, S, grids.ctypes.data, _ptr(off_dev),
                                                                                _ptr(grids_dev), _ptr(base_dev), _ptr(keys), _stream_ptr())))[0])
        t, order = wall(lambda: torch.sort(keys, stable=True).indices)
        stage.append(t)
        mean = torch.empty((N,), dtype=torch.float64, device="cuda")
        work = _workspace(int(lib.mspa_knn_segments_workspace_bytes(off.ctypes.data, S, NB)), "cuda")
        stage.append(wall(lambda: _lib.check(lib.mspa_knn_segments_mean_distance_device(
            _ptr(xyz), off.ctypes.data, S, NB, grids.ctypes.data, _ptr(off_dev), _ptr(grids_dev), _ptr(base_dev), _ptr(order), _ptr(mean), None,
            _ptr(work), int(work.numel()), _stream_ptr())))[0])
        t, stats = wall(lambda: CS.outlier_stats_segments(mean, off, RATIO, xyz))
        stage.append(t)

        def compact():
            kept = stats["kept"].cpu().numpy()
            index = torch.nonzero_static(stats["keep"], size=int(kept.sum())).flatten()
            return clouds.rows.index_select(0, index), clouds.pixel.index_select(0, index)
        stage.append(wall(compact)[0])
        stage.append(wall(lambda: CS.boxes_of(stats["lo"].reshape(clouds.counts.shape + (3,)), stats["hi"].reshape(clouds.counts.shape + (3,))))[0])
        del keys, order, mean, work, stats
        if k:
            for name, t in zip(names, stage):
                st[name].append(t)
    print(f"Stages of (b), each alone with a synchronise behind it ({S} segments, {N:,} rows):\n")
    print("| stage | median (ms) | passes (ms) |")
    print("|---|---|---|")
    for name, v in st.items():
        print(f"| {name} | {statistics.median(v) * 1e3:.1f} | {fmt(v)} |")
    worst = max(st, key=lambda n: statistics.median(st[n]))
    print(f"\nThe stage that bounds (b): **{worst}**, {statistics.median(st[worst]) * 1e3:.1f} ms of "
          f"{sum(statistics.median(v) for v in st.values()) * 1e3:.1f} ms.\n")


if __name__ == "__main__":
    main()
