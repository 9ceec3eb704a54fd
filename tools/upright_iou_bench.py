#!/usr/bin/env python3
"""The IoU of upright boxes: ``upright_iou`` / ``upright_iou_matrix`` on the device beside the host twin of the same header
(``mspa_upright_iou_host``) on one thread and on 16 worker processes over the same boxes.  Prints markdown
(profiles/upright_iou_device.md).

    python tools/upright_iou_bench.py [--passes 5] [--frames 64] [--objects 30] [--workers 16] [--large 16384] [--trace]

Three shapes: (a) the per-image upright boxes of tools/cloud_segments_bench.py's scene (every (image, label) cloud with rows)
against their objects' fused boxes (``by_object(0.005)``), as pairs; (b) the matrix of those per-image boxes against themselves;
(c) a ``--large`` x ``--large`` matrix of seeded random boxes.  The boxes are built once outside every timed window.  Per line one
warm-up pass, then medians of the timed passes, all listed; a host clock around work that ends in a device synchronise; the device
clock is not sampled.  A device call of shape (a) or (b) takes microseconds, so its window holds ``--calls`` calls (a tenth of them
for (b)) and the figure is the window over the calls.  The host lines time the twin's compute only: the boxes are already NumPy
arrays, the 16 workers (started once, before the GPU is touched, and never touching it) each take a slab of rows and keep their
results -- gathering them is not timed.  The host lines of shape (c) time the first 1 / 128 (one thread) and 1 / 8 (workers) of the
rows and are scaled up, and say so.  ``--trace`` runs the three device calls once warm and once more and nothing else, and starts
no worker: the run to put under ``rocprofv3 --kernel-trace
--stats``."""
import argparse
import os
import statistics
import sys
import time
from concurrent.futures import ProcessPoolExecutor
from multiprocessing import get_context

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "multi-spatialmllm_amd"), ROOT, os.path.join(ROOT, "tools")]


def host_slab(job):
    """One worker's share: rows of a against all of b (matrix), or a slab of pairs; the sum of the finite results comes back."""
    from mspa import cloud_segments as CS
    kind, a, b = job
    out = CS.upright_iou_matrix_host(a, b) if kind == "matrix" else CS.upright_iou_host(a, b)
    return float(np.nansum(out))


def random_boxes(n, seed):
    rng = np.random.default_rng(seed)
    sizes = rng.uniform(0.2, 3.0, (n, 3))
    sizes[:, :2] = np.sort(sizes[:, :2], axis=1)[:, ::-1]
    angle = rng.uniform(-np.pi / 2, np.pi / 2, n)
    return np.concatenate([rng.uniform(-8, 8, (n, 2)), rng.uniform(-1, 1, (n, 1)), sizes, np.cos(angle)[:, None], np.sin(angle)[:, None]], axis=1)


def fmt(xs, scale=1e3):
    return ", ".join(f"{x * scale:.3f}" for x in xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--objects", type=int, default=30)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--large", type=int, default=16384)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    pool = None
    if not args.trace:
        pool = ProcessPoolExecutor(args.workers, mp_context=get_context("spawn"))
        warm = random_boxes(64, 1)
        list(pool.map(host_slab, [("matrix", warm, warm)] * args.workers * 2))        # the workers are up and have the library loaded
    import torch
    from cloud_segments_bench import build_scene
    from mspa import cloud_segments as CS, instances
    handler, sid, _ids = build_scene(args.frames, args.objects)
    clouds = handler.instance_clouds(sid, num_workers=16)
    assert instances.LAST_INSTANCE_CLOUDS["path"] == "device", instances.LAST_INSTANCE_CLOUDS
    per_image = clouds.upright_boxes()                                              # [F, L, 8]
    fused_rows, fused_off, object_ids = clouds.by_object(0.005)
    fused = torch.full((per_image.shape[1], 8), float("nan"), dtype=torch.float64, device=per_image.device)
    fused[torch.as_tensor(np.asarray(object_ids) + 1, device=per_image.device)] = CS.upright_boxes_segments(fused_rows, fused_off)
    live = torch.nonzero(~torch.isnan(per_image[..., 0]).reshape(-1)).flatten()         # the (image, label) clouds with rows (a read-back, untimed)
    flat = per_image.reshape(-1, 8).index_select(0, live).contiguous()
    against = fused.expand_as(per_image).reshape(-1, 8).index_select(0, live).contiguous()
    large = torch.from_numpy(random_boxes(args.large, 2)).cuda()
    torch.cuda.synchronize()

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    if args.trace:
        for _ in range(2):
            wall(lambda: CS.upright_iou(flat, against))
            wall(lambda: CS.upright_iou_matrix(flat, flat))
            wall(lambda: CS.upright_iou_matrix(large, large))
        return

    def spread(kind, a, b):
        """The twin on the worker processes: a's rows (or the pairs) in ``workers`` slabs."""
        cuts = np.linspace(0, len(a), args.workers + 1).astype(int)
        jobs = [(kind, a[lo:hi], b if kind == "matrix" else b[lo:hi]) for lo, hi in zip(cuts[:-1], cuts[1:])]
        return sum(pool.map(host_slab, jobs))

    P = int(flat.shape[0])
    shapes = [
        (f"(a) pairs: the {P:,} per-image boxes against their objects' fused boxes", "pairs", flat, against, args.calls, 1, 1),
        (f"(b) matrix: the {P:,} per-image boxes against themselves ({P * P:,} entries)", "matrix", flat, flat, max(args.calls // 10, 1), 1, 1),
        (f"(c) matrix: {args.large:,} x {args.large:,} seeded random boxes ({args.large * args.large:,} entries)", "matrix", large, large, 1, 128, 8),
    ]
    print("# IoU between upright boxes: `upright_iou` / `upright_iou_matrix` beside the host twin\n")
    print(f"`python tools/upright_iou_bench.py --passes {args.passes} --frames {args.frames} --objects {args.objects} --workers {args.workers} "
          f"--large {args.large} --calls {args.calls}` on one MI355X, one process plus the twin's worker processes.  The boxes are built once "
          "outside every timed window; per line one warm-up pass, then the median of the timed passes (all listed); a host clock around work "
          "that ends in a device synchronise; the device clock was not sampled.  A device window of the two small shapes holds several calls "
          "(the count is in the table) and the figure is per call.  The host lines time the twin's compute on NumPy boxes that are already "
          f"there; the {args.workers} workers keep their results (gathering them is not timed).\n")
    for title, kind, a, b, calls, one_thread_cut, workers_cut in shapes:
        call = CS.upright_iou_matrix if kind == "matrix" else CS.upright_iou
        host_call = CS.upright_iou_matrix_host if kind == "matrix" else CS.upright_iou_host
        a_host, b_host = a.cpu().numpy(), b.cpu().numpy()
        rows, worker_rows = len(a_host) // one_thread_cut, len(a_host) // workers_cut
        first = call(a, b)
        same = bool(torch.equal(first.view(torch.int64), call(a, b).view(torch.int64)))
        check_rows = min(rows, 256)
        twin_equal = first[:check_rows].cpu().numpy().tobytes() == host_call(a_host[:check_rows], b_host if kind == "matrix" else
                                                                           b_host[:check_rows]).tobytes()
        share = float((first > 0).sum()) / max(first.numel(), 1)
        del first
        times = {"device": [], "one": [], "workers": []}
        host_call(a_host[:rows], b_host if kind == "matrix" else b_host[:rows])
        spread(kind, a_host[:worker_rows], b_host if kind == "matrix" else b_host[:worker_rows])
        for _ in range(args.passes):
            def many():
                for _k in range(calls):
                    out = call(a, b)
                return out
            times["device"].append(wall(many)[0] / calls)
            t0 = time.perf_counter()
            host_call(a_host[:rows], b_host if kind == "matrix" else b_host[:rows])
            times["one"].append((time.perf_counter() - t0) * one_thread_cut)
            t0 = time.perf_counter()
            spread(kind, a_host[:worker_rows], b_host if kind == "matrix" else b_host[:worker_rows])
            times["workers"].append((time.perf_counter() - t0) * workers_cut)
        med = {k: statistics.median(v) for k, v in times.items()}
        scaled = f" (the first 1 / {one_thread_cut} of the rows, times {one_thread_cut})" if one_thread_cut > 1 else ""
        print(f"## {title}\n")
        print(f"Two device runs bit-identical: **{same}**; the device's first {check_rows} rows equal the twin's bytes: **{twin_equal}**; "
              f"{100.0 * share:.1f} % of the entries are positive.\n")
        print("| line | median (ms) | passes (ms) |")
        print("|---|---|---|")
        print(f"| device, per call ({calls} calls per window) | **{med['device'] * 1e3:.3f}** | {fmt(times['device'])} |")
        print(f"| `mspa_upright_iou_host`, one thread{scaled} | **{med['one'] * 1e3:.3f}** | {fmt(times['one'])} |")
        cut = f" (the first 1 / {workers_cut} of the rows, times {workers_cut})" if workers_cut > 1 else ""
        print(f"| `mspa_upright_iou_host`, {args.workers} worker processes{cut} | **{med['workers'] * 1e3:.3f}** | {fmt(times['workers'])} |")
        best = min(med["one"], med["workers"])
        print(f"\nThe device call takes {med['device'] / best:.4f} of the faster host line's time"
              + (" -- it LOSES to the host twin at this size.\n" if med["device"] > best else ".\n"))
        torch.cuda.empty_cache()
    pool.shutdown()


if __name__ == "__main__":
    main()
