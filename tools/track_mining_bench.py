#!/usr/bin/env python3
"""Object-movement pair mining, host line against MSPA_TRACK_MINING=device, on the heads_bench track block (T = 300, P = 256,
8 groups) at (npoints_per_group, npairs_per_bin) = (15, 30) and (1, 1).  Prints markdown (profiles/track_mining_device.md).

    python tools/track_mining_bench.py [--passes 7]

* host line: the switch unset in this process -- K5c per group, every distance downloaded, NumPy on them;
* device: statistics, bin counts, order and resolve each end with a device synchronise (so the stages add up to a little more than
  an unsplit run takes), ``plan_track_draws`` is timed on the host, "rest" is uploads, downloads, the edges and the list;
* the om() row of tools/heads_bench.py (grouping + mining + records) both ways, and the mining's share of it.
One warm-up pass, then the median of the warm passes, all listed.  Both lines must return the same list and leave the same
generator state, or the run stops.  (Registers and LDS of the kernels: ``python tools/kernel_resources.py track_mining``.)"""
import argparse
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "multi-spatialmllm_amd"), ROOT]


class Timed:
    """mspa.engine's four K5d calls, each followed by a synchronise and a clock."""

    def __init__(self, engine, torch):
        self.engine, self.torch, self.t = engine, torch, {}
        self.TRACK_MINING_BUDGET_BYTES, self.TRACK_MINING_PAIR_BYTES = engine.TRACK_MINING_BUDGET_BYTES, engine.TRACK_MINING_PAIR_BYTES

    def __getattr__(self, name):
        fn = getattr(self.engine, name)

        def call(*a, **k):
            self.torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn(*a, **k)
            self.torch.cuda.synchronize()
            self.t[name] = self.t.get(name, 0.0) + time.perf_counter() - t0
            return r
        return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    args = ap.parse_args()
    import torch
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.spatial.distance import squareform
    from mspa import engine, heads, synth, templates as T
    dev = "cuda:0"
    os.environ.pop("MSPA_TRACK_MINING", None)
    tr = synth.make_tracks(5, T=300, P=256, n_groups=8)
    tracks = torch.from_numpy(np.ascontiguousarray(tr.tracks_XYZ)).to(dev)

    def prepare():
        loss = engine.track_rigidity_loss(tracks).cpu().numpy()
        labels = fcluster(linkage(squareform(loss, checks=False), method="average"), 0.1, criterion="distance")
        groups = [g for g in (np.where(labels == i)[0].tolist() for i in range(1, max(labels) + 1)) if len(g) > 5]
        c2w = torch.from_numpy(np.linalg.inv(tr.extrinsics_w2c).reshape(-1, 16)).to(dev)
        return groups, engine.track_to_world(tracks, c2w, tr.fx_fy_cx_cy, tr.image_hw, ("world",))["world"]

    def records(pairs):
        return heads.object_movement_records(tr.scene_id, tr.tracks_XYZ, tr.extrinsics_w2c, tr.fx_fy_cx_cy, tr.image_hw, pairs,
                                             "tapvid3d_displacement_vector", T.OBJECT_MOVEMENT, random.Random(6))

    base_groups, world = prepare()
    downloaded = [0]

    def distance_fn(p, f):
        out = engine.track_pair_distances(world, p, f)
        downloaded[0] += sum(d.nbytes for d in out)
        return out

    def mine(mode, npoints, npairs, backend=None):
        os.environ["MSPA_TRACK_MINING"] = mode
        heads.TRACK_MINING_BACKEND = backend
        rng, groups = random.Random(5), [list(g) for g in base_groups]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pairs = heads.object_movement_mine_pairs(tr.visibility, groups, distance_fn, npoints, npairs, True, 0.05, rng, world=world)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert heads.LAST_TRACK_MINING["path"] == mode, heads.LAST_TRACK_MINING
        return dt, [(int(s["point_index"]), int(s["frame1"]), int(s["frame2"])) for s in pairs], rng.getstate(), pairs

    def fmt(xs):
        return ", ".join(f"{x * 1e3:.2f}" for x in xs)

    n_members = len({p for g in base_groups for p in g})
    print("# Object-movement pair mining: host line against `MSPA_TRACK_MINING=device`\n")
    print(f"`python tools/track_mining_bench.py --passes {args.passes}` on one MI355X, one process: the `heads_bench` block "
          f"(`synth.make_tracks(5, T=300, P=256, n_groups=8)`), {len(base_groups)} rigid groups of more than 5 points, {n_members} grouped "
          "points.  One warm-up pass, then the median of the warm passes (all listed, ms).  The device stages each end with a "
          "synchronise; `rest` is uploads, downloads, the edges and the list.  Both lines returned the same list and left the "
          "same generator state in every pass.\n")
    for npoints, npairs in ((15, 30), (1, 1)):
        mine("host", npoints, npairs)
        host_t, ref = [], None
        for _ in range(args.passes):
            downloaded[0] = 0
            dt, keys, state, _ = mine("host", npoints, npairs)
            host_t.append(dt)
            ref = (keys, state)
        host_bytes = downloaded[0]
        timed = Timed(engine, torch)
        real_plan = heads.plan_track_draws
        draws = [0.0]

        def plan(*a, **k):
            t0 = time.perf_counter()
            r = real_plan(*a, **k)
            draws[0] += time.perf_counter() - t0
            return r
        mine("device", npoints, npairs)
        dev_t, split_t, stages = [], [], []
        for _ in range(args.passes):
            dt, keys, state, pairs = mine("device", npoints, npairs)
            assert (keys, state) == ref, "the device line differs from the host line"
            dev_t.append(dt)
        heads.plan_track_draws = plan
        for _ in range(args.passes):
            timed.t, draws[0] = {}, 0.0
            dt, keys, state, pairs = mine("device", npoints, npairs, timed)
            assert (keys, state) == ref
            split_t.append(dt)
            stages.append(dict(timed.t, draws=draws[0], wall=dt))
        heads.plan_track_draws = real_plan
        mid = sorted(stages, key=lambda s: s["wall"])[len(stages) // 2]
        n_out = sum(1 for _ in pairs)
        print(f"## npoints_per_group = {npoints}, npairs_per_bin = {npairs}: {n_out} pairs returned\n")
        print("| line | median (ms) | passes (ms) | downloaded |")
        print("|---|---|---|---|")
        print(f"| host (switch unset) | **{statistics.median(host_t) * 1e3:.2f}** | {fmt(host_t)} | {host_bytes:,} B of distances |")
        dev_bytes = n_members * (6 * 8 + 10 * 4)
        print(f"| device | **{statistics.median(dev_t) * 1e3:.2f}** | {fmt(dev_t)} | {dev_bytes:,} B of statistics and bin counts, "
              f"then 8 B per pick |")
        print(f"\nHost line over device: **{statistics.median(host_t) / statistics.median(dev_t):.2f} x**.\n")
        print(f"Device, split (the pass of median wall, {mid['wall'] * 1e3:.2f} ms; walls {fmt(split_t)}):\n")
        print("| stage | ms |")
        print("|---|---|")
        rest = mid["wall"]
        for label, k in (("statistics (every grouped point)", "track_pair_stats"), ("bin counts", "track_pair_bin_counts"),
                         ("draws (host)", "draws"), ("order (compaction + segmented sort)", "track_pair_order"),
                         ("resolve", "track_pair_resolve")):
            print(f"| {label} | {mid.get(k, 0.0) * 1e3:.3f} |")
            rest -= mid.get(k, 0.0)
        print(f"| rest | {rest * 1e3:.3f} |\n")
        if (npoints, npairs) == (15, 30):
            st = engine.track_pair_stats(world, torch.from_numpy(tr.visibility.astype(np.uint8)).to(dev),
                                         torch.tensor(sorted({k[0] for k in ref[0]}), dtype=torch.int32, device=dev))
            moving = int(st["stats"][:, 2].sum())
            print(f"The order stage sorted {moving:,} moving pairs of {st['stats'].shape[0]} picked points: "
                  f"{moving / max(mid.get('track_pair_order', 0.0), 1e-9) / 1e6:,.0f} M pairs/s, compaction included.\n")
            # the om() row of tools/heads_bench.py, both ways
            om = {}
            for mode in ("host", "device"):
                os.environ["MSPA_TRACK_MINING"] = mode
                heads.TRACK_MINING_BACKEND = None
                whole, part = [], []
                for k in range(args.passes + 1):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    groups, w = prepare()
                    t1 = time.perf_counter()
                    pairs = heads.object_movement_mine_pairs(tr.visibility, groups, lambda p, f: engine.track_pair_distances(w, p, f),
                                                             15, 30, True, 0.05, random.Random(5), world=w)
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    n = len(records(pairs))
                    t3 = time.perf_counter()
                    if k:
                        whole.append(t3 - t0)
                        part.append(t2 - t1)
                om[mode] = (statistics.median(whole), statistics.median(part), n, whole)
            print("The `om()` row of `tools/heads_bench.py` (K7 + SciPy linkage, K5a, mining, K5a/K5b records), (15, 30):\n")
            print("| mining | whole row, median (ms) | mining (ms) | share | records | passes (ms) |")
            print("|---|---|---|---|---|---|")
            for mode in ("host", "device"):
                w_, p_, n, allw = om[mode]
                print(f"| {mode} | {w_ * 1e3:.1f} | {p_ * 1e3:.1f} | {100 * p_ / w_:.0f} % | {n} | {fmt(allw)} |")
            print()
    os.environ.pop("MSPA_TRACK_MINING", None)

if __name__ == "__main__":
    main()
