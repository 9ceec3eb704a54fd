#!/usr/bin/env python3
"""Voxel down-sampling every fused object cloud of a scene in front of the batched cleaning: ``voxel_down_sample_segments`` and its
stages, ``cleaned_objects()`` as it was beside ``cleaned_objects(voxel_size=...)``, and the same op composed from
``torch.unique(dim=0, return_inverse=True)`` + ``index_add_`` for scale.  Prints markdown (profiles/voxel_segments_device.md).

    python tools/voxel_segments_bench.py [--passes 5] [--frames 64] [--objects 30] [--sizes 0.005,0.01,0.02,0.05] [--trace]

The scene is tools/cloud_segments_bench.py's: ``--frames`` frames at ScanNet's shape with about ``--objects`` objects per frame, from
files; ``instance_clouds`` and ``by_object()`` are built once, outside every timed window.  Per voxel size: one warm-up pass of each
line, then the lines alternate; medians of the timed passes, all listed; a host clock around work that ends in a device
synchronise.  The torch composition's sums are atomic and differ in the last bits from run to run; its rows are compared with the
op's within 1e-9 relative, its counts exactly.  ``--trace`` runs one warm and one more pass of ``voxel_down_sample_segments`` per
size and nothing else: the run to put under ``rocprofv3 --kernel-trace --stats``."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "multi-spatialmllm_amd"), ROOT, os.path.join(ROOT, "tools")]
NB, RATIO = 20, 1.0


def fmt(xs):
    return ", ".join(f"{x * 1e3:.1f}" for x in xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--objects", type=int, default=30)
    ap.add_argument("--sizes", default="0.005,0.01,0.02,0.05")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    sizes = [float(s) for s in args.sizes.split(",")]
    import torch
    from cloud_segments_bench import build_scene
    from mspa import _lib, cloud_segments as CS, instances
    from mspa.engine import _ptr, _stream_ptr, _workspace
    handler, sid, _ids = build_scene(args.frames, args.objects)
    clouds = handler.instance_clouds(sid, num_workers=16)
    assert instances.LAST_INSTANCE_CLOUDS["path"] == "device", instances.LAST_INSTANCE_CLOUDS
    rows, off, object_ids = clouds.by_object()
    N, S, C = int(rows.shape[0]), off.size - 1, int(rows.shape[1])
    lib = _lib.load()

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    if args.trace:
        for size in sizes:
            for _ in range(2):
                wall(lambda: CS.voxel_down_sample_segments(rows, off, size))
        return

    off_dev, = CS._upload(off, device=rows.device)
    segment_of_row = torch.searchsorted(off_dev[1:], torch.arange(N, dtype=torch.int64, device=rows.device), right=True)

    def torch_composition(size, clock):
        """(means, counts, offsets): the same grid, ordered by torch.unique, summed by index_add_'s atomics; ``clock`` collects the
        three parts' times."""
        def index():
            # (one amin per object: scatter_reduce_ "amin" onto these S x 3 cells takes 255 ms on 5.5 M rows, all of it contention)
            lo = torch.stack([rows[int(a):int(b), :3].amin(dim=0) if b > a else torch.zeros((3,), dtype=torch.float64, device=rows.device)
                              for a, b in zip(off[:-1], off[1:])])
            idx = torch.floor((rows[:, :3] - (lo - size * 0.5)[segment_of_row]) / size).to(torch.int64)
            return torch.cat([segment_of_row[:, None], idx], dim=1)
        t_index, key = wall(index)
        t_unique, (voxels, inverse) = wall(lambda: torch.unique(key, dim=0, return_inverse=True))

        def add():
            sums = torch.zeros((voxels.shape[0], C), dtype=torch.float64, device=rows.device).index_add_(0, inverse, rows)
            counts = torch.bincount(inverse, minlength=voxels.shape[0])
            return sums / counts[:, None].to(torch.float64), counts
        t_add, (means, counts) = wall(add)
        clock.append((t_index, t_unique, t_add))
        return means, counts

    def staged(size, clock):
        """``voxel_down_sample_segments``' own steps, each alone with a synchronise behind it."""
        tile_base = np.zeros((S + 1,), dtype=np.int64)
        _lib.check(lib.mspa_voxel_segments_tables_host(off.ctypes.data, S, tile_base.ctypes.data))
        o_dev, base_dev = CS._upload(off, tile_base, device=rows.device)
        keys = torch.empty((N,), dtype=torch.int64, device=rows.device)
        segment = torch.empty((N,), dtype=torch.int32, device=rows.device)
        seg_voxels = torch.empty((S + 1,), dtype=torch.int32, device=rows.device)
        work = _workspace(int(lib.mspa_voxel_segments_workspace_bytes(off.ctypes.data, S)), rows.device)
        t_keys = wall(lambda: _lib.check(lib.mspa_voxel_segments_keys_device(
            _ptr(rows), C, off.ctypes.data, S, size, _ptr(o_dev), _ptr(base_dev), _ptr(keys), _ptr(segment), _ptr(seg_voxels), _ptr(work),
            int(work.numel()), _stream_ptr())))[0]

        def sorts():
            order = torch.sort(keys, stable=True).indices
            return order.gather(0, torch.sort(segment.gather(0, order), stable=True).indices) if S > 1 else order
        t_sorts, order = wall(sorts)
        t_heads = wall(lambda: _lib.check(lib.mspa_voxel_segments_heads_device(off.ctypes.data, S, _ptr(o_dev), _ptr(keys), _ptr(order),
                                                                               _ptr(seg_voxels), _ptr(work), int(work.numel()), _stream_ptr())))[0]
        t_back, back = wall(lambda: seg_voxels.cpu().numpy())
        M = int(back[:S].sum())
        out = torch.empty((M, C), dtype=torch.float64, device=rows.device)
        counts = torch.empty((M,), dtype=torch.int32, device=rows.device)
        t_means = wall(lambda: _lib.check(lib.mspa_voxel_segments_means_device(_ptr(rows), C, off.ctypes.data, S, _ptr(o_dev), _ptr(order), M,
                                                                               _ptr(out), _ptr(counts), _ptr(work), int(work.numel()), _stream_ptr())))[0]
        clock.append((t_keys, t_sorts, t_heads, t_back, t_means))

    print("# Voxel down-sampling every fused object cloud of a scene: `voxel_down_sample_segments` in front of the batched cleaning\n")
    print(f"`python tools/voxel_segments_bench.py --passes {args.passes} --frames {args.frames} --objects {args.objects} --sizes {args.sizes}` on one "
          "MI355X, one process.  `instance_clouds` and `by_object()` are built once outside every timed window; per voxel size one warm-up pass "
          "of each line, then the lines alternate; median of the timed passes (all listed, ms); a host clock around work that ends in a device "
          f"synchronise.  nb_neighbors = {NB}, std_ratio = {RATIO}.\n")
    print(f"The timed input: the `by_object()` batch of {args.frames} frames, **{S} objects, {N:,} rows** of {C} columns.  The rule restates "
          "Open3D's `voxel_down_sample` and is not checked against Open3D.\n")
    for size in sizes:
        out_rows, out_offsets, counts = CS.voxel_down_sample_segments(rows, off, size)                  # warm-up passes: also the comparison
        again = CS.voxel_down_sample_segments(rows, off, size)
        same = bool(torch.equal(out_rows.view(torch.int64), again[0].view(torch.int64))) and bool(torch.equal(counts, again[2]))
        t_means, t_counts = torch_composition(size, [])
        agree = (tuple(t_means.shape) == tuple(out_rows.shape) and bool(torch.equal(t_counts, counts.to(torch.int64)))
                 and bool(((t_means - out_rows).abs() <= 1e-9 * out_rows.abs().clamp(min=1e-30) + 1e-12).all()))
        kept_plain = clouds.cleaned_objects(NB, RATIO)[1][-1]
        kept_voxel = clouds.cleaned_objects(NB, RATIO, voxel_size=size)[1][-1]
        staged(size, [])
        del again, t_means, t_counts
        times = {k: [] for k in ("op", "plain", "voxel")}
        stage_clock, torch_clock = [], []
        for _ in range(args.passes):
            times["op"].append(wall(lambda: CS.voxel_down_sample_segments(rows, off, size))[0])
            times["plain"].append(wall(lambda: clouds.cleaned_objects(NB, RATIO))[0])
            times["voxel"].append(wall(lambda: clouds.cleaned_objects(NB, RATIO, voxel_size=size))[0])
            staged(size, stage_clock)
            torch_composition(size, torch_clock)
        med = {k: statistics.median(v) for k, v in times.items()}
        M = int(out_offsets[-1])
        long_runs, longest = int((counts > 64).sum()), int(counts.max())
        print(f"## voxel_size = {size}\n")
        print(f"**{M:,} rows out** of {N:,} ({N / max(M, 1):.1f} rows per voxel; {long_runs:,} runs longer than 64 rows, the longest {longest:,}); two "
              f"runs of the op bit-identical: **{same}**; the torch composition has the same voxels and counts and means within 1e-9: **{agree}**.  "
              f"`cleaned_objects()` keeps {int(kept_plain):,} rows, `cleaned_objects(voxel_size={size})` {int(kept_voxel):,}.\n")
        print("| line | median (ms) | passes (ms) |")
        print("|---|---|---|")
        print(f"| `voxel_down_sample_segments(rows, offsets, {size})` | **{med['op'] * 1e3:.1f}** | {fmt(times['op'])} |")
        print(f"| `cleaned_objects()` as it is at the parent commit (regroup + clean) | **{med['plain'] * 1e3:.1f}** | {fmt(times['plain'])} |")
        print(f"| `cleaned_objects(voxel_size={size})` (regroup + down-sample + clean) | **{med['voxel'] * 1e3:.1f}** | {fmt(times['voxel'])} |")
        print()
        print("| stage of the op, alone with a synchronise behind it | median (ms) | passes (ms) |")
        print("|---|---|---|")
        names = ("extents and keys (extent_tiles<1, TakeAll> / extent_fold<1> / vox_keys kernels)", "sorts (torch.sort by key, then by segment, gathers)",
                 "heads (vox_heads, count / scan / place, vox_segment_counts kernels)", "the read-back of the counts and the flag word",
                 "means (long-run list, vox_short_means / vox_long_means kernels)")
        stage_med = []
        for j, name in enumerate(names):
            v = [c[j] for c in stage_clock]
            stage_med.append(statistics.median(v))
            print(f"| {name} | {stage_med[-1] * 1e3:.2f} | {fmt(v)} |")
        print()
        print("| the torch composition, for scale | median (ms) | passes (ms) |")
        print("|---|---|---|")
        torch_med = []
        for j, name in enumerate(("indices (one amin per object, floor of the quotient, cat)", "`torch.unique(dim=0, return_inverse=True)` (its sort)",
                                  "`index_add_`, `bincount`, the division")):
            v = [c[j] for c in torch_clock]
            torch_med.append(statistics.median(v))
            print(f"| {name} | {torch_med[-1] * 1e3:.2f} | {fmt(v)} |")
        ours = stage_med[0] + stage_med[2] + stage_med[4]
        theirs = torch_med[0] + torch_med[2]
        print(f"\nSorts excluded: the new kernels take **{ours * 1e3:.2f} ms**, the torch composition's non-sort part **{theirs * 1e3:.2f} ms**"
              + (" -- the new kernels take LONGER." if ours > theirs else ".")
              + f"  Whole: {sum(stage_med) * 1e3:.1f} ms staged ({med['op'] * 1e3:.1f} ms in one call) against {sum(torch_med) * 1e3:.1f} ms.\n")
        del out_rows, counts
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
