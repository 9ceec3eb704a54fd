#!/usr/bin/env python3
"""Rigid alignment of the clouds of two ragged batches: ``mspa.cloud_segments.TargetIndex.register`` (point-to-point ICP, batched)
against the download plus, per pair, a ``scipy.spatial.cKDTree`` query and a NumPy Kabsch fit per iteration.  Prints markdown
(profiles/cloud_align_device.md).

    python tools/cloud_align_bench.py [--passes 5] [--host-iterations 10] [--frames 64] [--objects 30] [--trace]

The scene is tools/cloud_segments_bench.py's; ``instance_clouds``, the thinned fused clouds and the ``target_index`` are built once,
outside every timed window (``register`` is the repeated search the index was built for).  The shapes:
  (a) every per-image cloud against its object's fused cloud thinned at 5 mm, ``register`` at 10 and at 30 iterations, cap 5 cm;
  (c) one pair of 307 200 rows: a second noisy sampling of one surface, turned by 1 degree and moved by 5 mm.
One warm-up pass of each line, then medians of the timed passes, all listed; a host clock around work that ends in a device
synchronise.  Further: ``rigid_fit_segments`` and ``transform_segments`` alone, the share of pairs converged by iteration, and what
``sync_every=5`` saves.  ``--trace`` runs shapes (a) at 10 iterations and (c) at 30 twice and nothing else: the run to put under
``rocprofv3 --kernel-trace --stats``."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "multi-spatialmllm_amd"), ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
THIN, CAP = 0.005, 0.05


def fmt(xs):
    return ", ".join(f"{x * 1e3:.1f}" for x in xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--host-iterations", type=int, default=10)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--objects", type=int, default=30)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    import torch
    from cloud_align_util import kabsch_svd, rotation
    from cloud_distance_bench import surface
    from cloud_segments_bench import build_scene
    from mspa import cloud_segments as CS, instances
    handler, sid, _ids = build_scene(args.frames, args.objects)
    clouds = handler.instance_clouds(sid, num_workers=16)
    assert instances.LAST_INSTANCE_CLOUDS["path"] == "device", instances.LAST_INSTANCE_CLOUDS
    _F, L = clouds.counts.shape

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def timed(fn, passes=args.passes):
        wall(fn)
        return [wall(fn)[0] for _ in range(passes)]

    fused, fused_off, object_ids = clouds.by_object(THIN)
    run_of = np.full((L,), -1, dtype=np.int64)
    run_of[np.asarray(object_ids) + 1] = np.arange(len(object_ids))
    frames, labels = np.nonzero(clouds.counts[:, 1:])
    labels = labels + 1
    pairs_a = np.stack([frames * L + labels, run_of[labels]], axis=1).astype(np.int64)       # (image segment, object run)
    q_a, q_off_a = clouds.rows[:, :3].contiguous(), clouds.offsets
    rng = np.random.default_rng(307200)
    one = np.array([0, 307200], dtype=np.int64)
    t_c = surface(rng, 307200)
    q_c = (surface(rng, 307200) - [1.0, 1.0, 0.0]) @ rotation([1.0, 2.0, 3.0], np.deg2rad(1.0)).T + [1.0, 1.0, 0.0] + 0.005 * np.array([2.0, -1.0, 2.0]) / 3.0
    t_c, q_c = torch.from_numpy(t_c).cuda(), torch.from_numpy(np.ascontiguousarray(q_c)).cuda()
    shapes = {"a": (q_a, q_off_a, fused, fused_off, pairs_a), "c": (q_c, one, t_c, one, None)}
    index = {name: CS.target_index(t, t_off) for name, (_q, _qo, t, t_off, _p) in shapes.items()}

    def device(shape, iterations, **kw):
        q, q_off, _t, _t_off, pairs = shapes[shape]
        return index[shape].register(q, q_off, pairs, max_distance=CAP, iterations=iterations, **kw)

    if args.trace:
        for shape, iterations in (("a", 10), ("c", 30), ("a", 10), ("c", 30)):
            wall(lambda: device(shape, iterations))
        return

    def host(shape, iterations):
        from concurrent.futures import ThreadPoolExecutor
        from scipy.spatial import cKDTree
        q, q_off, t, t_off, pairs = shapes[shape]
        q, t = q.cpu().numpy(), t[:, :3].cpu().numpy()                         # the download
        if pairs is None:
            pairs = np.array([[0, 0]])
        trees = {ts: cKDTree(t[t_off[ts]:t_off[ts + 1]]) for ts in sorted(set(pairs[:, 1].tolist()))}
        inner = 16 if len(pairs) == 1 else 1

        def one_pair(pair):
            qs, ts = pair
            Q, T = q[q_off[qs]:q_off[qs + 1]], t[t_off[ts]:t_off[ts + 1]]
            R, tr = np.eye(3), np.zeros(3)
            for _ in range(iterations):
                d, at = trees[ts].query(Q @ R.T + tr, workers=inner, distance_upper_bound=CAP)
                ok = np.isfinite(d)
                if ok.sum() >= 3:
                    R, tr = kabsch_svd(Q[ok], T[at[ok]])
            return R, tr

        with ThreadPoolExecutor(16) as pool:
            return list(pool.map(one_pair, pairs))

    print("# Rigid alignment of the clouds of two batches: `TargetIndex.register` against a `cKDTree` and a NumPy Kabsch per pair and iteration\n")
    print(f"`python tools/cloud_align_bench.py --passes {args.passes} --host-iterations {args.host_iterations} --frames {args.frames} --objects "
          f"{args.objects}` on one MI355X, one process.  `instance_clouds`, the thinned fused clouds and the `target_index` are built once outside "
          "every timed window; one warm-up pass of each line; median of the timed passes (all listed, ms); a host clock around work that ends in a "
          f"device synchronise.  The host lines are the download of both batches plus, per pair on 16 worker threads, {args.host_iterations} "
          "iterations of `cKDTree.query` (the trees built once per target segment, inside the window) and a NumPy SVD Kabsch; one timed pass.\n")
    print(f"Shape (a): {len(pairs_a)} pairs, **{int(q_off_a[-1]):,} query rows** (every per-image cloud) against {len(object_ids)} fused clouds of "
          f"{int(fused_off[-1]):,} rows thinned at {THIN * 1e3:.0f} mm.  Shape (c): one pair, 307,200 rows against 307,200 rows, 1 degree and 5 mm "
          f"apart.  The cap is {CAP * 100:.0f} cm.\n")
    print("| line | median (ms) | passes (ms) |")
    print("|---|---|---|")
    lines = [("(a) `register`, 10 iterations", lambda: device("a", 10), args.passes), ("(a) `register`, 30 iterations", lambda: device("a", 30), args.passes),
             ("(a) `register`, 30 iterations, `sync_every=5`", lambda: device("a", 30, sync_every=5), args.passes),
             ("(a) one `nearest` with the cap (keys, sort and search)", lambda: index["a"].nearest(q_a, q_off_a, pairs_a, CAP), args.passes),
             (f"(a) host, {args.host_iterations} iterations", lambda: host("a", args.host_iterations), 1),
             ("(c) `register`, 10 iterations", lambda: device("c", 10), args.passes), ("(c) `register`, 30 iterations", lambda: device("c", 30), args.passes),
             ("(c) one `nearest` with the cap", lambda: index["c"].nearest(q_c, one, None, CAP), args.passes),
             (f"(c) host, {args.host_iterations} iterations", lambda: host("c", args.host_iterations), 1)]
    med = {}
    for name, fn, passes in lines:
        ts = timed(fn, passes) if passes > 1 else [wall(fn)[0]]
        med[name] = statistics.median(ts)
        print(f"| {name} | **{med[name] * 1e3:.1f}** | {fmt(ts)} |")
    for shape in ("a", "c"):
        per = (med[f"({shape}) `register`, 30 iterations"] - med[f"({shape}) `register`, 10 iterations"]) / 20.0
        print(f"\nShape ({shape}): one iteration costs **{per * 1e3:.2f} ms** (the difference of the 30- and the 10-iteration line over 20); the host line per "
              f"iteration is {med[f'({shape}) host, {args.host_iterations} iterations'] / args.host_iterations * 1e3:.0f} ms, download and trees included.")

    # ---- the two new steps alone ---------------------------------------------------------------------------------------------
    print("\nThe two new steps alone, each with a synchronise behind it (ms, median of the passes):\n")
    print("| shape | `transform_segments` | `rigid_fit_segments` (both launches) |")
    print("|---|---|---|")
    for shape in ("a", "c"):
        q, q_off, t, _t_off, pairs = shapes[shape]
        found = index[shape].nearest(q, q_off, pairs, CAP)
        fit = CS.rigid_fit_segments(q, q_off, t, found["index"], pairs)
        t_move = timed(lambda: CS.transform_segments(q, q_off, fit["R"], fit["t"], pairs))
        t_fit = timed(lambda: CS.rigid_fit_segments(q, q_off, t, found["index"], pairs))
        print(f"| ({shape}) | {statistics.median(t_move) * 1e3:.2f} | {statistics.median(t_fit) * 1e3:.2f} |")
        del found, fit

    # ---- the early stop ------------------------------------------------------------------------------------------------------
    reg = device("a", 30)
    at = reg["converged_at"].cpu().numpy()
    status = reg["status"].cpu().numpy()
    print(f"\nShape (a), 30 iterations: status ok / few / degenerate = {(status == 0).sum()} / {(status == 1).sum()} / {(status == 2).sum()} pairs; "
          f"median fitness {float(reg['fitness'].nanmedian()):.3f}, median inlier rmse {float(reg['inlier_rmse'].nanmedian()) * 1e3:.2f} mm.  "
          "The share of pairs that have reached their fixed point by iteration k (`converged_at <= k`):\n")
    print("| k | " + " | ".join(str(k) for k in (0, 1, 2, 4, 9, 14, 19, 24, 29)) + " | never |")
    print("|---|" + "---|" * 10)
    print("| share | " + " | ".join(f"{((at >= 0) & (at <= k)).mean():.3f}" for k in (0, 1, 2, 4, 9, 14, 19, 24, 29)) + f" | {(at < 0).mean():.3f} |")
    synced = device("a", 30, sync_every=5)
    same = all(synced[k].cpu().numpy().tobytes() == reg[k].cpu().numpy().tobytes() for k in ("R", "t", "converged_at")) if synced["all_converged"] else None
    print(f"\n`sync_every=5`: all converged at the last read-back = {synced['all_converged']}; its result equals the full loop's byte for byte = {same}.")


if __name__ == "__main__":
    main()
