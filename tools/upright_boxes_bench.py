#!/usr/bin/env python3
"""The upright minimal boxes of every object cloud of a scene: ``upright_boxes_segments`` on the device beside the host way -- download
the rows, then ``scipy.spatial.ConvexHull`` plus a NumPy all-edges rectangle per segment on 16 worker processes.  Prints markdown
(profiles/upright_boxes_device.md).

    python tools/upright_boxes_bench.py [--passes 5] [--frames 64] [--objects 30] [--workers 16] [--trace image|object]

The scene is tools/cloud_segments_bench.py's: ``--frames`` frames at ScanNet's shape with about ``--objects`` objects per frame, from
files.  Two batches, both built once outside every timed window: the per-image batch (``InstanceClouds.rows`` / ``offsets``: every
(image, label) cloud) and ``by_object(0.005)`` (every object's fused cloud, down-sampled).  Per batch one warm-up pass of each line,
then the lines alternate; medians of the timed passes, all listed; a host clock around work that ends in a device synchronise.  The
device clock is not sampled.  The host line's time includes the download of the rows (``.cpu()``) and their copy into the shared
memory the workers read; the workers are started once, before the GPU is touched, and never touch it.  ``--trace image`` or
``--trace object`` runs one warm and one more pass of ``upright_boxes_segments`` on that batch and nothing else, and starts no worker:
the run to put under ``rocprofv3 --kernel-trace --stats``."""
import argparse
import os
import statistics
import sys
import time
from concurrent.futures import ProcessPoolExecutor
from multiprocessing import get_context, shared_memory

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "multi-spatialmllm_amd"), ROOT, os.path.join(ROOT, "tools")]


def host_box(xyz):
    """One segment the host way: Qhull's vertices (counter-clockwise), every edge's spans over the hull, the smallest area."""
    from scipy.spatial import ConvexHull
    if len(xyz) == 0:
        return np.full(8, np.nan)
    z_lo, z_hi = xyz[:, 2].min(), xyz[:, 2].max()
    try:
        v = xyz[ConvexHull(xyz[:, :2]).vertices, :2]
    except Exception:                               # fewer than three points, or all collinear: Qhull has no hull
        return np.full(8, np.nan)
    d = np.roll(v, -1, axis=0) - v
    q = v[None, :, :] - v[:, None, :]               # [edge, vertex]
    t = q[..., 0] * d[:, None, 0] + q[..., 1] * d[:, None, 1]
    c = q[..., 1] * d[:, None, 0] - q[..., 0] * d[:, None, 1]
    dd = (d * d).sum(axis=1)
    k = int(np.argmin((t.max(axis=1) - t.min(axis=1)) * (c.max(axis=1) - c.min(axis=1)) / dd))
    L = np.sqrt(dd[k])
    tm, cm = (t[k].max() + t[k].min()) / 2, (c[k].max() + c[k].min()) / 2
    length, width, u = (t[k].max() - t[k].min()) / L, (c[k].max() - c[k].min()) / L, d[k] / L
    if width > length:
        length, width, u = width, length, np.array([-u[1], u[0]])
    if u[0] < 0 or (u[0] == 0 and u[1] < 0):
        u = -u
    centre = v[k] + (tm * d[k] + cm * np.array([-d[k, 1], d[k, 0]])) / dd[k]
    return np.array([centre[0], centre[1], (z_hi + z_lo) / 2, length, width, z_hi - z_lo, u[0], u[1]])


def host_chunk(job):
    name, n_rows, pairs = job
    shm = shared_memory.SharedMemory(name=name)
    try:
        rows = np.ndarray((n_rows, 3), dtype=np.float64, buffer=shm.buf)
        return [host_box(rows[a:b]) for a, b in pairs]
    finally:
        shm.close()


def fmt(xs):
    return ", ".join(f"{x * 1e3:.1f}" for x in xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--objects", type=int, default=30)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--trace", choices=["image", "object"])
    args = ap.parse_args()
    pool = None
    if not args.trace:
        pool = ProcessPoolExecutor(args.workers, mp_context=get_context("spawn"))
        warm = shared_memory.SharedMemory(create=True, size=24 * 8)
        np.ndarray((8, 3), dtype=np.float64, buffer=warm.buf)[:] = np.random.default_rng(0).random((8, 3))
        list(pool.map(host_chunk, [(warm.name, 8, [(0, 8)])] * args.workers * 4))    # the workers are up and have SciPy loaded
        warm.close()
        warm.unlink()
    import torch
    from cloud_segments_bench import build_scene
    from mspa import cloud_segments as CS, instances
    handler, sid, _ids = build_scene(args.frames, args.objects)
    clouds = handler.instance_clouds(sid, num_workers=16)
    assert instances.LAST_INSTANCE_CLOUDS["path"] == "device", instances.LAST_INSTANCE_CLOUDS
    fused_rows, fused_off, _object_ids = clouds.by_object(0.005)
    batches = [("per image: every (image, label) cloud", clouds.rows, clouds.offsets), ("`by_object(0.005)`: every object's fused cloud", fused_rows,
                                                                                         fused_off)]

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    if args.trace:
        _name, rows, off = batches[0 if args.trace == "image" else 1]
        for _ in range(2):
            wall(lambda: CS.upright_boxes_segments(rows, off))
        return

    def host_way(rows, off):
        host = rows[:, :3].to(torch.float64).cpu().numpy()
        shm = shared_memory.SharedMemory(create=True, size=max(host.nbytes, 8))
        try:
            np.ndarray(host.shape, dtype=np.float64, buffer=shm.buf)[:] = host
            live = [(int(a), int(b)) for a, b in zip(off[:-1], off[1:])]
            order = np.argsort([a - b for a, b in live], kind="stable")              # the longest first, dealt round-robin
            chunks = [[live[j] for j in order[w::args.workers * 4]] for w in range(args.workers * 4)]
            got = list(pool.map(host_chunk, [(shm.name, len(host), c) for c in chunks]))
            out = np.full((len(live), 8), np.nan)
            for w, part in enumerate(got):
                for j, box in zip(order[w::args.workers * 4], part):
                    out[j] = box
            return out
        finally:
            shm.close()
            shm.unlink()

    print("# Upright minimal boxes for every object cloud of a scene: `upright_boxes_segments` beside the host way\n")
    print(f"`python tools/upright_boxes_bench.py --passes {args.passes} --frames {args.frames} --objects {args.objects} --workers {args.workers}` on one "
          "MI355X, one process plus the host way's worker processes.  Both batches are built once outside every timed window; per batch one "
          "warm-up pass of each line, then the lines alternate; median of the timed passes (all listed, ms); a host clock around work that ends "
          "in a device synchronise; the device clock was not sampled.  The host way: the rows' download, then `scipy.spatial.ConvexHull` plus a "
          f"NumPy all-edges rectangle per segment on {args.workers} worker processes that read the rows from shared memory.\n")
    for name, rows, off in batches:
        N, S = int(rows.shape[0]), off.size - 1
        boxes, survivors = CS.upright_boxes_segments(rows, off, want_survivors=True)                  # warm-up passes: also the comparison
        again = CS.upright_boxes_segments(rows, off)
        same = bool(torch.equal(boxes.view(torch.int64), again.view(torch.int64)))
        host = host_way(rows, off)
        got = boxes.cpu().numpy()
        both = ~np.isnan(host[:, 0]) & ~np.isnan(got[:, 0])
        area = np.abs(got[both, 3] * got[both, 4] - host[both, 3] * host[both, 4]) / np.maximum(host[both, 3] * host[both, 4], 1e-300)
        times = {"device": [], "host": []}
        for _ in range(args.passes):
            times["device"].append(wall(lambda: CS.upright_boxes_segments(rows, off))[0])
            times["host"].append(wall(lambda: host_way(rows, off))[0])
        med = {k: statistics.median(v) for k, v in times.items()}
        print(f"## {name}\n")
        print(f"**{S:,} clouds, {N:,} rows** ({int((np.diff(off) > 0).sum()):,} clouds with rows).  The filter leaves **{int(survivors.sum()):,} rows** "
              f"for the sort and the hull, {100.0 * survivors.sum() / max(N, 1):.3f} % of the batch (the largest segment keeps {int(survivors.max()):,}).  "
              f"Two runs of the op bit-identical: **{same}**; the host way's area `length * width` differs from the op's by at most "
              f"{area.max() if len(area) else 0.0:.2e} relative over the {int(both.sum()):,} clouds both box.\n")
        print("| line | median (ms) | passes (ms) |")
        print("|---|---|---|")
        print(f"| `upright_boxes_segments(rows, offsets)` | **{med['device'] * 1e3:.1f}** | {fmt(times['device'])} |")
        print(f"| the host way, download included | **{med['host'] * 1e3:.1f}** | {fmt(times['host'])} |")
        print(f"\nThe device op takes {med['device'] / med['host']:.2f} of the host way's time"
              + (" -- it LOSES to the host on this batch.\n" if med["device"] > med["host"] else ".\n"))
        del boxes, again
        torch.cuda.empty_cache()
    pool.shutdown()


if __name__ == "__main__":
    main()
