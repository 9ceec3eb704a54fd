"""Colour-frame (JPEG) decode throughput: the device decoder (mspa_jpeg_decode_device) against Pillow (libjpeg-turbo) on
``hostinfo.effective_cpus()`` threads, over the same frames, at ScanNet's 1296 x 968.

    python tools/jpeg_bench.py [--frames 1024] [--reps 5] [--quick]

Prints one JSON line per configuration (quality 75 / 90 / 95, 4:2:0 / 4:4:4, with / without a restart marker per MCU row):
device frames/s and RGB GB/s (decode kernels only: payloads already resident, statuses read once per call), the wall time of
one call, and the host decode on the effective CPUs.  The IDCT / colour phases move (coefficients int16 + planes + RGB) bytes
that follow from the shapes; the entropy phase is a serial bit-stream walk per image and has no bandwidth bound.  The
per-phase kernel split comes from a separate ``rocprofv3 --kernel-trace --stats -- python tools/jpeg_bench.py --quick``."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-spatialmllm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="one configuration, for a profiler run")
    a = ap.parse_args()
    import torch
    from mspa import engine, hostinfo
    from jpeg_util import content, encode, pillow_rgb
    H, W = 968, 1296
    dev = "cuda:0"
    base = [content(H, W, s) for s in range(8)]
    cpus = hostinfo.effective_cpus()
    configs = [(q, sub, rst) for q in (75, 90, 95) for sub in (2, 0) for rst in (False, True)]
    if a.quick:
        configs = configs[:1]
    for q, sub, rst in configs:
        kw = dict(quality=q, subsampling=sub)
        if rst:
            kw["restart_marker_rows"] = 1
        uniq = [encode(b, **kw) for b in base]
        payloads = [uniq[k % len(uniq)] for k in range(a.frames)]
        offs = np.zeros(a.frames, np.int64)
        pos = 0
        for k, p in enumerate(payloads):
            offs[k] = pos
            pos += (len(p) + 15) // 16 * 16
        buf = np.zeros(pos + 16, np.uint8)
        for o, p in zip(offs, payloads):
            buf[o:o + len(p)] = np.frombuffer(p, np.uint8)
        desc, st = engine.jpeg_parse_host(payloads)
        src = torch.from_numpy(buf).to(dev)
        off_d = torch.from_numpy(offs).to(dev)
        nb_d = torch.tensor([len(p) for p in payloads], dtype=torch.int64, device=dev)
        desc_d = torch.from_numpy(desc).to(dev)
        out = torch.empty((a.frames, H, W, 3), dtype=torch.uint8, device=dev)
        out, status = engine.jpeg_decode_device(src, off_d, nb_d, desc_d, (H, W), out=out)
        torch.cuda.synchronize()
        ok = int((status == 0).sum())
        same = all(np.array_equal(out[k].cpu().numpy(), pillow_rgb(payloads[k])) for k in range(len(uniq)))
        times = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            engine.jpeg_decode_device(src, off_d, nb_d, desc_d, (H, W), out=out, status=status)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        t = float(np.median(times))
        n_host = min(a.frames, 32 * cpus)
        with ThreadPoolExecutor(cpus) as pool:
            t0 = time.perf_counter()
            list(pool.map(lambda k: pillow_rgb(payloads[k]), range(n_host)))
            th = time.perf_counter() - t0
        print(json.dumps({"quality": q, "subsampling": {2: "4:2:0", 0: "4:4:4"}[sub], "restart_rows": rst, "frames": a.frames,
                          "mean_payload_kb": round(float(np.mean([len(p) for p in uniq])) / 1024, 1), "status0": ok,
                          "equal_to_pillow": same, "device_call_ms": round(t * 1e3, 2), "device_fps": round(a.frames / t, 1),
                          "device_rgb_gbps": round(a.frames * H * W * 3 / t / 1e9, 2), "host_threads": cpus,
                          "host_fps": round(n_host / th, 1)}), flush=True)


if __name__ == "__main__":
    main()
