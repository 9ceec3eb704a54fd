#!/usr/bin/env python3
"""Nearest-point distances between the clouds of two ragged batches: ``mspa.cloud_segments.target_index`` / ``TargetIndex.nearest`` /
``fit_segments`` against the download plus one ``scipy.spatial.cKDTree`` per target segment.  Prints markdown
(profiles/cloud_distance_device.md).

    python tools/cloud_distance_bench.py [--passes 5] [--host-passes 1] [--frames 64] [--objects 30] [--trace]

The scene is tools/cloud_segments_bench.py's: ``--frames`` frames at ScanNet's shape with about ``--objects`` objects per frame;
``instance_clouds`` is built once, outside every timed window.  The shapes:
  (a) every per-image cloud against its object's fused cloud thinned at 5 mm (``by_object(0.005)``): one index, one query, one summary;
  (b) ``InstanceClouds.view_coverage`` at 2 cm and at 5 cm (fused clouds thinned at 5 mm);
  (c) one cloud of 307 200 rows against another (two noisy samplings of one surface);
  (d) shape (c) with 1 % of the queries moved 50 extents away, with and without a cap of 5 cm.
One warm-up pass of each line, then medians of the timed passes, all listed; a host clock around work that ends in a device
synchronise.  The host baseline is the download of both batches plus, per target segment, ``cKDTree(T).query(Q, workers=16)``; it
runs ``--host-passes`` times.  Further tables: the ``_grid_k`` sweep (1, 4, 8, 16) with the mean evaluations per row, and the lanes in
input order against the lanes ordered by their query's cell in the target's grid (``_ordered``: the keys pass and the sort counted in).  ``--trace`` runs
shapes (a) and (c) twice and nothing else: the run to put under ``rocprofv3 --kernel-trace --stats``."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "multi-spatialmllm_amd"), ROOT, os.path.join(ROOT, "tools")]
THIN, CAP = 0.005, 0.05


def fmt(xs):
    return ", ".join(f"{x * 1e3:.1f}" for x in xs)


def surface(rng, n):
    """n rows on a wavy sheet of 2 m x 2 m with 2 mm of noise: what one depth frame of 640 x 480 leaves of a wall."""
    uv = rng.random((n, 2)) * 2.0
    z = 0.2 * np.sin(3.0 * uv[:, 0]) * np.cos(2.0 * uv[:, 1]) + rng.normal(size=n) * 0.002
    return np.ascontiguousarray(np.column_stack([uv, z]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--host-passes", type=int, default=1)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--objects", type=int, default=30)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    import torch
    from cloud_segments_bench import build_scene
    from mspa import _lib, cloud_segments as CS, instances
    handler, sid, _ids = build_scene(args.frames, args.objects)
    clouds = handler.instance_clouds(sid, num_workers=16)
    assert instances.LAST_INSTANCE_CLOUDS["path"] == "device", instances.LAST_INSTANCE_CLOUDS
    F, L = clouds.counts.shape

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def timed(fn, passes=args.passes):
        wall(fn)
        return [wall(fn)[0] for _ in range(passes)]

    # ---- the shapes ---------------------------------------------------------------------------------------------------------
    fused, fused_off, object_ids = clouds.by_object(THIN)
    run_of = np.full((L,), -1, dtype=np.int64)
    run_of[np.asarray(object_ids) + 1] = np.arange(len(object_ids))
    frames, labels = np.nonzero(clouds.counts[:, 1:])
    labels = labels + 1
    pairs_a = np.stack([frames * L + labels, run_of[labels]], axis=1).astype(np.int64)       # (image segment, object run)
    q_a, q_off_a = clouds.rows[:, :3].contiguous(), clouds.offsets
    rng = np.random.default_rng(307200)
    one = np.array([0, 307200], dtype=np.int64)
    t_c, q_c = torch.from_numpy(surface(rng, 307200)).cuda(), surface(rng, 307200)
    q_d = q_c.copy()
    q_d[rng.choice(len(q_d), len(q_d) // 100, replace=False)] += np.array([100.0, -100.0, 50.0])
    q_c, q_d = torch.from_numpy(q_c).cuda(), torch.from_numpy(q_d).cuda()
    shapes = {"a": (q_a, q_off_a, fused, fused_off, pairs_a), "c": (q_c, one, t_c, one, None), "d": (q_d, one, t_c, one, None)}

    def device(shape, cap=None, grid_k=None, want_evals=False):
        q, q_off, t, t_off, pairs = shapes[shape]
        out = CS.target_index(t, t_off, grid_k).nearest(q, q_off, pairs, cap, want_index=True, want_evals=want_evals)
        out["fit"] = CS.fit_segments(out["distance"], out["offsets"], CAP)
        return out

    if args.trace:
        for shape in ("a", "c", "a", "c"):
            wall(lambda: device(shape))
        return

    def host(shape, cap=None):
        from scipy.spatial import cKDTree
        q, q_off, t, t_off, pairs = shapes[shape]
        q, t = q.cpu().numpy(), t[:, :3].cpu().numpy()                         # the download
        if pairs is None:
            pairs = np.array([[0, 0]])
        out = []
        trees = {}
        for qs, ts in pairs:
            if ts not in trees:
                trees[ts] = cKDTree(t[t_off[ts]:t_off[ts + 1]])
            out.append(trees[ts].query(q[q_off[qs]:q_off[qs + 1]], workers=16, distance_upper_bound=np.inf if cap is None else cap)[0])
        return np.concatenate(out)

    print("# Nearest-point distances between the clouds of two batches: `mspa.cloud_segments` against a `cKDTree` per segment\n")
    print(f"`python tools/cloud_distance_bench.py --passes {args.passes} --host-passes {args.host_passes} --frames {args.frames} --objects "
          f"{args.objects}` on one MI355X, one process, 16 CPU threads for the host lines.  `instance_clouds` and the thinned fused clouds are built "
          "once outside every timed window; one warm-up pass of each line; median of the timed passes (all listed, ms); a host clock around "
          "work that ends in a device synchronise.  The device lines are `target_index` + `nearest` + `fit_segments`, the index build included; "
          "the host lines are the download of both batches plus `cKDTree(T).query(Q, workers=16)` per target segment.\n")
    print(f"Shape (a): {len(pairs_a)} pairs, **{int(q_off_a[-1]):,} query rows** (every per-image cloud) against {len(object_ids)} fused clouds of "
          f"{int(fused_off[-1]):,} rows thinned at {THIN * 1e3:.0f} mm.  Shapes (c), (d): 307,200 rows against 307,200 rows; in (d) 1 % of the "
          f"queries lie 50 extents away; the cap is {CAP * 100:.0f} cm.\n")
    # the device's distances against SciPy's before anything is timed (a second implementation: 8 u d, as tests/test_cloud_distance_cpu.py)
    for shape in ("a", "c"):
        got, want = device(shape)["distance"].cpu().numpy(), host(shape)
        print(f"Before timing, shape ({shape}): the device's distances differ from SciPy's by more than 8 u d in "
              f"**{int((np.abs(got - want) > 8 * 2.0 ** -53 * want).sum())}** of {len(want):,} rows.\n")
    print("| line | median (ms) | passes (ms) |")
    print("|---|---|---|")
    lines = [("(a) device", lambda: device("a"), args.passes), ("(a) host", lambda: host("a"), args.host_passes),
             ("(b) `view_coverage(0.02, 0.005)` (its own `by_object(0.005)` included)", lambda: clouds.view_coverage(0.02, THIN), args.passes),
             ("(b) `view_coverage(0.05, 0.005)`", lambda: clouds.view_coverage(0.05, THIN), args.passes),
             ("(c) device", lambda: device("c"), args.passes), ("(c) host", lambda: host("c"), args.host_passes),
             ("(d) device, no cap", lambda: device("d"), args.passes), ("(d) device, cap", lambda: device("d", CAP), args.passes),
             ("(d) host, no cap", lambda: host("d"), args.host_passes), ("(d) host, cap", lambda: host("d", CAP), args.host_passes)]
    med = {}
    for name, fn, passes in lines:
        ts = timed(fn, passes)
        med[name] = statistics.median(ts)
        print(f"| {name} | **{med[name] * 1e3:.1f}** | {fmt(ts)} |")
    print(f"\nHost over device: (a) **{med['(a) host'] / med['(a) device']:.1f} x**, (c) **{med['(c) host'] / med['(c) device']:.1f} x**, "
          f"(d) no cap **{med['(d) host, no cap'] / med['(d) device, no cap']:.1f} x**, (d) cap **{med['(d) host, cap'] / med['(d) device, cap']:.1f} x**.\n")

    # ---- the stages of the device line, the sweep of the grid's neighbour count, the evaluations ------------------------------
    print(f"The library's choices in the lines above: `_grid_k` = {_lib.CLOUD_DISTANCE_GRID_K}, ordered lanes = {CS.ORDER_QUERIES}.\n")
    print("Stages of the device line and the `_grid_k` sweep (lanes in input order), each stage alone with a synchronise behind it; evals = mean distances evaluated per row:\n")
    print("| shape | _grid_k | `target_index` (ms) | `nearest` (ms) | `fit_segments` (ms) | evals per row |")
    print("|---|---|---|---|---|---|")
    for shape, cap in (("a", None), ("c", None), ("d", None), ("d", CAP)):
        q, q_off, t, t_off, pairs = shapes[shape]
        for k in (1, 4, 8, 16):
            build = timed(lambda: CS.target_index(t, t_off, k), 3)
            ix = CS.target_index(t, t_off, k)
            near = timed(lambda: ix.nearest(q, q_off, pairs, cap, _ordered=False), 3)
            out = ix.nearest(q, q_off, pairs, cap, want_evals=True, _ordered=False)
            fit = timed(lambda: CS.fit_segments(out["distance"], out["offsets"], CAP), 3)
            print(f"| ({shape}){' cap' if cap else ''} | {k} | {statistics.median(build) * 1e3:.1f} | {statistics.median(near) * 1e3:.2f} | "
                  f"{statistics.median(fit) * 1e3:.2f} | {float(out['evals'].double().mean()):.1f} |")
            del ix, out

    # ---- the queries ordered by their cell in the target's grid ------------------------------------------------------------
    print("\nLanes in input order against lanes that take the output rows in the order of their cell in the target's grid (`query_keys_kernel`, "
          "one `torch.sort`, the permutation read by `nearest_pairs_kernel`; the same bytes out, asserted).  `nearest` alone, ms:\n")
    print("| shape | _grid_k | input order | ordered (keys + sort + search) |")
    print("|---|---|---|---|")
    for shape, cap in (("a", None), ("c", None), ("d", None), ("d", CAP)):
        q, q_off, t, t_off, pairs = shapes[shape]
        for k in (1, 4, 8):
            ix = CS.target_index(t, t_off, k)
            plain, ordered = ix.nearest(q, q_off, pairs, cap, _ordered=False), ix.nearest(q, q_off, pairs, cap, _ordered=True)
            assert plain["distance"].cpu().numpy().tobytes() == ordered["distance"].cpu().numpy().tobytes() and bool((plain["index"] == ordered["index"]).all())
            del plain, ordered
            t_plain = timed(lambda: ix.nearest(q, q_off, pairs, cap, _ordered=False), 3)
            t_ordered = timed(lambda: ix.nearest(q, q_off, pairs, cap, _ordered=True), 3)
            print(f"| ({shape}){' cap' if cap else ''} | {k} | {statistics.median(t_plain) * 1e3:.2f} | {statistics.median(t_ordered) * 1e3:.2f} |")
            del ix

if __name__ == "__main__":
    main()
