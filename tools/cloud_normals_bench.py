#!/usr/bin/env python3
"""Normals for every cloud of a ragged batch: ``mspa.cloud_segments.normals_segments`` against the download plus, per segment, a
``scipy.spatial.cKDTree.query(k)`` and one batched ``numpy.linalg.eigh``.  Prints markdown (profiles/cloud_normals_device.md).

    python tools/cloud_normals_bench.py [--passes 5] [--frames 64] [--objects 30] [--trace] [--skip-host]

The scene is tools/cloud_segments_bench.py's; ``instance_clouds`` and the thinned fused clouds are built once, outside every timed
window.  The shapes:
  (i) the per-image batch: every (image, object) cloud as decoded, oriented towards its frame's camera centre;
  (f) the fused clouds of the objects thinned at 5 mm, unoriented.
Each at k = 10 and k = 30.  One warm-up pass of each line, then medians of the timed passes, all listed; a host clock around work that
ends in a device synchronise.  A device line is the whole call: the search tables with their one read-back, the keys, the sort, the
index and the one launch of the search and the fit.  ``--trace`` runs every device line twice and nothing else: the run to put under
``rocprofv3 --kernel-trace --stats``."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "multi-spatialmllm_amd"), ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
THIN = 0.005


def fmt(xs):
    return ", ".join(f"{x * 1e3:.1f}" for x in xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--objects", type=int, default=30)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--skip-host", action="store_true", help="leave the host baseline lines out (they take minutes)")
    args = ap.parse_args()
    import torch
    from cloud_segments_bench import build_scene
    from mspa import cloud_segments as CS, instances
    handler, sid, _ids = build_scene(args.frames, args.objects)
    clouds = handler.instance_clouds(sid, num_workers=16)
    assert instances.LAST_INSTANCE_CLOUDS["path"] == "device", instances.LAST_INSTANCE_CLOUDS

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def timed(fn, passes=args.passes):
        wall(fn)
        return [wall(fn)[0] for _ in range(passes)]

    fused, fused_off, _object_ids = clouds.by_object(THIN)
    views = np.repeat(clouds.centres, clouds.n_labels, axis=0)
    shapes = {"i": (clouds.rows[:, :3].contiguous(), clouds.offsets, views), "f": (fused[:, :3].contiguous(), np.asarray(fused_off), None)}

    def device(shape, k):
        rows, off, v = shapes[shape]
        return CS.normals_segments(rows, off, k, None, v)

    # point-to-plane beside point-to-point on tools/cloud_align_bench.py's shape (a): every per-image cloud against its object's fused
    # cloud thinned at 5 mm, cap 5 cm; the index and the fused clouds' normals (k = 30, unoriented) are built once, outside the windows
    L = clouds.n_labels
    run_of = np.full((L,), -1, dtype=np.int64)
    run_of[np.asarray(_object_ids) + 1] = np.arange(len(_object_ids))
    frames, labels = np.nonzero(clouds.counts[:, 1:])
    labels = labels + 1
    pairs_a = np.stack([frames * L + labels, run_of[labels]], axis=1).astype(np.int64)
    index_a = CS.target_index(fused, fused_off)
    normals_a = device("f", 30)["normal"]

    def register(estimation, iterations):
        extra = {"estimation": estimation, "normals": normals_a} if estimation == "point_to_plane" else {}
        return index_a.register(shapes["i"][0], clouds.offsets, pairs_a, max_distance=0.05, iterations=iterations, **extra)

    if args.trace:
        for _ in range(2):
            for shape in ("i", "f"):
                for k in (10, 30):
                    wall(lambda: device(shape, k))
            wall(lambda: register("point_to_plane", 10))
        return

    def host(shape, k):
        from concurrent.futures import ThreadPoolExecutor
        from scipy.spatial import cKDTree
        rows, off, v = shapes[shape]
        xyz = rows.cpu().numpy()                                               # the download
        live = [s for s in range(len(off) - 1) if off[s + 1] - off[s] >= 3]

        def one_segment(s):
            P = xyz[off[s]:off[s + 1]]
            _d, at = cKDTree(P).query(P, k=min(k, len(P)))
            nb = P[at.reshape(len(P), -1)]
            d = nb - nb.mean(axis=1, keepdims=True)
            _w, vec = np.linalg.eigh(np.einsum("nka,nkb->nab", d, d))
            n = vec[:, :, 0]
            if v is not None:
                n = np.where((np.einsum("na,na->n", v[s] - P, n) < 0)[:, None], -n, n)
            return n

        with ThreadPoolExecutor(16) as pool:
            return list(pool.map(one_segment, live))

    print("# Normals for every cloud of a batch: `normals_segments` against a `cKDTree` and a batched `eigh` per segment\n")
    print(f"`python tools/cloud_normals_bench.py --passes {args.passes} --frames {args.frames} --objects {args.objects}` on one MI355X, one process.  "
          "`instance_clouds` and the thinned fused clouds are built once outside every timed window; one warm-up pass of each line; median of the "
          "timed passes (all listed, ms); a host clock around work that ends in a device synchronise.  A device line is the whole call, its one "
          "read-back included.  A host line is the download plus, per segment on 16 worker threads, a `cKDTree` build, `query(k)` and one batched "
          "`numpy.linalg.eigh`; one timed pass.\n")
    for shape, what in (("i", "the per-image batch (oriented towards each frame's camera centre)"), ("f", f"the fused clouds thinned at {THIN * 1e3:.0f} mm")):
        rows, off, _v = shapes[shape]
        print(f"Shape ({shape}): {what}: **{int(off[-1]):,} rows** in {int((np.diff(off) > 0).sum())} non-empty segments of {len(off) - 1}.")
    print("\n| line | median (ms) | passes (ms) |")
    print("|---|---|---|")
    med = {}
    for shape in ("i", "f"):
        for k in (10, 30):
            ts = timed(lambda: device(shape, k))
            med[(shape, k, "device")] = statistics.median(ts)
            print(f"| ({shape}) `normals_segments`, k = {k} | **{statistics.median(ts) * 1e3:.1f}** | {fmt(ts)} |")
            if args.skip_host:
                continue
            t_host = wall(lambda: host(shape, k))[0]
            med[(shape, k, "host")] = t_host
            print(f"| ({shape}) host, k = {k} | **{t_host * 1e3:.1f}** | {fmt([t_host])} |")
    print("\n| shape | k | device (ms) | host (ms) | host / device | device rows / s |")
    print("|---|---|---|---|---|---|")
    for shape in ("i", "f"):
        for k in (10, 30):
            if args.skip_host:
                continue
            d, h = med[(shape, k, "device")], med[(shape, k, "host")]
            print(f"| ({shape}) | {k} | {d * 1e3:.1f} | {h * 1e3:.1f} | {h / d:.1f} | {int(shapes[shape][1][-1]) / d:,.0f} |")
    out = device("i", 30)
    status = out["status"].cpu().numpy()
    print(f"\nShape (i), k = 30: status ok / few / degenerate = {(status == 0).sum():,} / {(status == 1).sum():,} / {(status == 2).sum():,} rows; "
          f"median curvature of the ok rows {float(out['curvature'][out['status'] == 0].median()):.4f}.")

    # ---- point-to-plane beside point-to-point ---------------------------------------------------------------------------------
    print(f"\n## Point-to-plane beside point-to-point\n\nShape (a) of `tools/cloud_align_bench.py`: {len(pairs_a)} pairs, every per-image cloud against its "
          "object's fused cloud thinned at 5 mm, cap 5 cm, from the identity; the fused clouds' normals at k = 30.  `moved` is how far the "
          "last iteration still moved the transform: the largest absolute difference of its 12 numbers between the run of n and of n - 1 iterations.\n")
    print("| estimation | 10 iterations: median (ms) | passes (ms) |")
    print("|---|---|---|")
    for estimation in ("point_to_point", "point_to_plane"):
        ts = timed(lambda: register(estimation, 10))
        print(f"| {estimation} | **{statistics.median(ts) * 1e3:.1f}** | {fmt(ts)} |")
    print("\n| estimation | n | ok pairs | converged (`converged_at` != -1) | still moving by more than 1e-12 | by more than 1e-9 | by more than 1e-6 | "
          "median inlier rmse (mm) | median fitness |")
    print("|---|---|---|---|---|---|---|---|---|")
    for estimation in ("point_to_point", "point_to_plane"):
        for n in (5, 10):
            now, before = register(estimation, n), register(estimation, n - 1)
            T = torch.cat([now["R"].reshape(-1, 9), now["t"]], dim=1)
            T0 = torch.cat([before["R"].reshape(-1, 9), before["t"]], dim=1)
            ok = now["status"] == 0
            moved = (T - T0).abs().max(dim=1).values[ok]
            print(f"| {estimation} | {n} | {int(ok.sum())} | {float((now['converged_at'][ok] != -1).double().mean()):.3f} | "
                  f"{float((moved > 1e-12).double().mean()):.3f} | {float((moved > 1e-9).double().mean()):.3f} | {float((moved > 1e-6).double().mean()):.3f} | "
                  f"{float(now['inlier_rmse'][ok].nanmedian()) * 1e3:.3f} | {float(now['fitness'][ok].nanmedian()):.3f} |")
    st = register("point_to_plane", 10)["status"].cpu().numpy()
    print(f"\nPoint-to-plane, 10 iterations: status ok / few / degenerate = {(st == 0).sum()} / {(st == 1).sum()} / {(st == 2).sum()} pairs.")


if __name__ == "__main__":
    main()
