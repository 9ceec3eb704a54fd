#!/usr/bin/env python3
"""Image resizing on the MI355X beside Pillow on the same box, for the two shapes of the training-shape step:
    python tools/resize_bench.py [--frames 1024] [--reps 5] [--pillow-frames 256] [--out FILE]
For 512x512 -> 1296x968 and 1296x968 -> 648x484 (bicubic), three legs each:
  kernels   engine.resize_rgb_device alone on frames resident on the device (device events; chunks of 128 frames, the tree
            tool's chunk), with the bytes it must read and write over the time;
  pipeline  files (page cache) -> decode + resize + encode -> file bytes in host memory, nothing written (decode calls of
            1 024 files, as the tree tool);
  tree      resize_tree from disk to disk.
Every leg is measured for the device path and for Pillow on hostinfo.effective_cpus() threads in the same run: one warm-up,
then --reps repetitions, all listed, and their median.  Pillow legs run over --pillow-frames frames (their rate does not depend
on the count).  Each leg is a child process under its own time limit; the first failure ends the run.  One JSON line per leg."""
import argparse
import io
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "multi-spatialmllm_amd"), os.path.join(ROOT, "tests")]

SHAPES = [((512, 512), (968, 1296)), ((968, 1296), (484, 648))]
DECODE_CHUNK, CHUNK = 1024, 128               # as mspa.resize: files per decode call, frames per resize / encode call
HBM_MIXED_GBS = 5000.0                      # profiles/r01_hbm_ceilings.md: one kernel that reads and writes, 5.0-5.5 TB/s


def frames_of(hw, n):
    from jpeg_util import content
    base = [content(hw[0], hw[1], s) for s in range(16)]
    return np.stack([np.roll(base[k % 16], k // 16, axis=1) for k in range(n)])


def make_files(root, hw, n):
    from PIL import Image
    os.makedirs(root, exist_ok=True)
    imgs = frames_of(hw, 16)
    for k in range(16):
        Image.fromarray(imgs[k]).save(os.path.join(root, f"{k:05d}.jpg"), quality=90)
    for k in range(16, n):
        shutil.copy(os.path.join(root, f"{k % 16:05d}.jpg"), os.path.join(root, f"{k:05d}.jpg"))
    return [os.path.join(root, f"{k:05d}.jpg") for k in range(n)]


def timed(fn, reps):
    fn()                                                   # warm-up
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def report(what, shape, n, times, extra=None):
    rec = {"leg": what, "shape": f"{shape[0][1]}x{shape[0][0]}->{shape[1][1]}x{shape[1][0]}", "frames": n,
           "seconds": [round(t, 4) for t in times], "median_s": round(statistics.median(times), 4),
           "frames_s": round(n / statistics.median(times), 1)}
    rec.update(extra or {})
    print(json.dumps(rec), flush=True)


def leg_kernels(shape, n, reps, threads, n_pillow, tmp):
    import torch
    from mspa import engine
    from resize_util import pillow_resize
    (h, w), HW = shape
    imgs = frames_of((h, w), n)
    src = torch.from_numpy(imgs).cuda()
    out = torch.empty((n, HW[0], HW[1], 3), dtype=torch.uint8, device="cuda")

    def run():
        for c in range(0, n, CHUNK):
            engine.resize_rgb_device(src[c:c + CHUNK], HW, "bicubic", out=out[c:c + CHUNK])
    run()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / 1e3)
    same = all(np.array_equal(out[k].cpu().numpy(), pillow_resize(imgs[k], HW, 3)) for k in range(0, n, max(1, n // 8)))
    gb = (src.numel() + out.numel()) / 1e9                 # what must move: every source byte once, every result byte once
    med = statistics.median(times)
    report("kernels device", shape, n, times, {"GB_in_out": round(gb, 3), "GB_s": round(gb / med, 1),
                                               "share_of_read_write_ceiling": round(gb / med / HBM_MIXED_GBS, 3), "equals_pillow": same})
    with ThreadPoolExecutor(threads) as pool:
        t = timed(lambda: list(pool.map(lambda k: pillow_resize(imgs[k], HW, 3), range(n_pillow))), reps)
    report("kernels pillow", shape, n_pillow, t, {"threads": threads})


def _pillow_bytes(path, HW):
    from PIL import Image
    b = io.BytesIO()
    with Image.open(path) as im:
        im.convert("RGB").resize((HW[1], HW[0]), 3).save(b, "JPEG", quality=95)
    return b.getvalue()


def leg_pipeline(shape, n, reps, threads, n_pillow, tmp):
    import torch
    from mspa import engine
    from mspa.ingest import read_color_frames_device
    (h, w), HW = shape
    paths = make_files(os.path.join(tmp, "src"), (h, w), n)
    files = {}

    def run():
        for d in range(0, n, DECODE_CHUNK):
            frames = read_color_frames_device(paths[d:d + DECODE_CHUNK], n_threads=min(16, threads))
            for c in range(0, len(frames), CHUNK):
                out, nb = engine.jpeg_encode_device(engine.resize_rgb_device(frames[c:c + CHUNK], HW, "bicubic"), 95, "4:2:0")
                sizes = nb.cpu().numpy()
                host = out[:, :int(sizes.max())].cpu().numpy()
                if c == 0 and d == 0:
                    files[0] = host[0, :int(sizes[0])].tobytes()
    times = timed(run, reps)
    report("pipeline device", shape, n, times, {"equals_pillow": files[0] == _pillow_bytes(paths[0], HW)})
    with ThreadPoolExecutor(threads) as pool:
        t = timed(lambda: list(pool.map(lambda p: _pillow_bytes(p, HW), paths[:n_pillow])), reps)
    report("pipeline pillow", shape, n_pillow, t, {"threads": threads})


def leg_tree(shape, n, reps, threads, n_pillow, tmp):
    from mspa import resize
    (h, w), HW = shape
    make_files(os.path.join(tmp, "src"), (h, w), n)
    make_files(os.path.join(tmp, "src_small"), (h, w), n_pillow)
    times = timed(lambda: resize.resize_tree(os.path.join(tmp, "src"), os.path.join(tmp, "device"), HW, backend="device"), reps)
    report("tree device", shape, n, times)
    t = timed(lambda: resize.resize_tree(os.path.join(tmp, "src_small"), os.path.join(tmp, "pillow"), HW, backend="pillow"), reps)
    same = all(open(os.path.join(tmp, "device", f"{k:05d}.jpg"), "rb").read() == open(os.path.join(tmp, "pillow", f"{k:05d}.jpg"), "rb").read()
               for k in range(0, n_pillow, max(1, n_pillow // 16)))
    report("tree pillow", shape, n_pillow, t, {"threads": threads, "device_files_equal": same})


LEGS = {"kernels": leg_kernels, "pipeline": leg_pipeline, "tree": leg_tree}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pillow-frames", type=int, default=256)
    ap.add_argument("--leg-timeout", type=int, default=420)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--shape", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:                                           # a child: one leg of one shape
        from mspa import hostinfo
        with tempfile.TemporaryDirectory(prefix="resize_bench_") as tmp:
            LEGS[args.leg](SHAPES[args.shape], args.frames, args.reps, max(1, hostinfo.effective_cpus()),
                           min(args.pillow_frames, args.frames), tmp)
        return 0
    for s in range(len(SHAPES)):
        for leg in LEGS:
            cmd = ["timeout", "-k", "10", str(args.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", leg, "--shape", str(s),
                   "--frames", str(args.frames), "--reps", str(args.reps), "--pillow-frames", str(args.pillow_frames)]
            run = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(run.stdout)
            sys.stdout.flush()
            if args.out:
                with open(args.out, "a") as f:
                    f.write(run.stdout)
            if run.returncode != 0:                        # a failed or timed-out GPU step: nothing more is started
                sys.stderr.write(run.stderr[-4000:])
                return run.returncode
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
