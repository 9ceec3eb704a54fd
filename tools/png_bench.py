"""Depth-PNG encode throughput: the device encoder (mspa_png_encode_device) against Pillow (``Image.fromarray(d).save``) on 16
host threads, over the same 1 024 frames of 640 x 480 per call.

    python tools/png_bench.py [--frames 1024] [--reps 5] [--threads 16] [--quick]

Prints one JSON line per content kind (smooth surfaces with sensor noise, planes with 30 % holes, uniform noise): device
frames/s (the encode call only: depth resident, files left on the device, timed between synchronisations), Pillow frames/s,
and the summed file size against Pillow's.  The per-kernel split comes from a separate
``rocprofv3 --kernel-trace --stats -- python tools/png_bench.py --quick``."""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-spatialmllm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def frames_of(kind: str, n: int) -> np.ndarray:
    from png_encode_util import content
    base = [content(kind, 480, 640, seed=s) for s in range(8)]
    out = np.empty((n, 480, 640), dtype=np.uint16)
    for i in range(n):
        out[i] = np.roll(base[i % 8], (i * 7) % 480, axis=0)
    return out


def pillow_bytes(d: np.ndarray) -> int:
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(d).save(buf, format="PNG")
    return buf.tell()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--quick", action="store_true", help="one kind, two reps, no Pillow: for a profiler run")
    a = ap.parse_args()
    import torch
    from mspa import engine
    kinds = ["smooth"] if a.quick else ["smooth", "planar", "noise"]
    for kind in kinds:
        frames = frames_of(kind, a.frames)
        d = torch.from_numpy(frames.view(np.int16)).cuda()
        out, nbytes = engine.png_encode_device(d)                       # warm-up (and the workspace's first allocation)
        torch.cuda.synchronize()
        times = []
        for _ in range(2 if a.quick else a.reps):
            t0 = time.perf_counter()
            engine.png_encode_device(d, out=out, nbytes=nbytes)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        dev_bytes = int(nbytes.sum())
        rec = {"kind": kind, "frames": a.frames, "hw": [480, 640], "device_fps": round(a.frames / min(times), 1),
               "device_ms_min": round(1e3 * min(times), 2), "device_ms_median": round(1e3 * float(np.median(times)), 2)}
        if not a.quick:
            with ThreadPoolExecutor(a.threads) as ex:
                list(ex.map(pillow_bytes, frames[:a.threads]))               # warm-up
                t0 = time.perf_counter()
                pil = list(ex.map(pillow_bytes, frames))
                dt = time.perf_counter() - t0
            rec.update(pillow_threads=a.threads, pillow_fps=round(a.frames / dt, 1), size_ratio=round(dev_bytes / sum(pil), 4),
                       speedup=round(rec["device_fps"] * dt / a.frames, 1))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
