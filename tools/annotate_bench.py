#!/usr/bin/env python3
"""Annotated-image writes: the device JPEG encoder against Pillow, and DeviceAnnotator against PillowAnnotator, with every
output byte-compared.
    python tools/annotate_bench.py [--frames 1024] [--records 1000] [--sources 64]
Prints one JSON line per measurement: encoder frames/s and GB/s (RGB in + file out, and that traffic as a share of HBM peak)
for ScanNet-shaped frames at q95 4:2:0 and 4:4:4 against Pillow on effective_cpus() threads; then images/s of a VC_D-shaped
job (N records over M distinct source frames) for DeviceAnnotator, PillowAnnotator called serially, and PillowAnnotator on 16
threads."""
import argparse
import io
import json
import os
import shutil
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "multi-spatialmllm_amd"), os.path.join(ROOT, "tests")]

HW = (968, 1296)
HBM_PEAK_GBS = 8000.0


def pillow_encode(img, q, ss):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=q, subsampling=ss)
    return b.getvalue()


def bench_encoder(n, threads):
    import torch
    from jpeg_util import content
    from mspa import engine
    base = [content(*HW, s) for s in range(8)]
    imgs = np.stack([np.roll(base[k % 8], k // 8, axis=1) for k in range(n)])
    rgb = torch.from_numpy(imgs).cuda()
    for ss in ("4:2:0", "4:4:4"):
        out, nb = engine.jpeg_encode_device(rgb, 95, ss)                  # warm-up, and the buffers of the timed calls
        torch.cuda.synchronize()
        reps = 5
        t0 = time.perf_counter()
        for _ in range(reps):
            engine.jpeg_encode_device(rgb, 95, ss, out=out, nbytes=nb)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / reps
        sizes = nb.cpu().numpy()
        host = out[:, :int(sizes.max())].cpu().numpy()
        with ThreadPoolExecutor(threads) as pool:
            t0 = time.perf_counter()
            want = list(pool.map(lambda k: pillow_encode(imgs[k], 95, ss), range(n)))
            dt_host = time.perf_counter() - t0
        same = all(host[k, :sizes[k]].tobytes() == want[k] for k in range(n))
        gb = (imgs.nbytes + int(sizes.sum())) / 1e9
        print(json.dumps({"what": "encode", "subsampling": ss, "frames": n, "device_ms": round(dt * 1e3, 2),
                          "device_frames_s": round(n / dt, 1), "device_GB_s": round(gb / dt, 1),
                          "hbm_share": round(gb / dt / HBM_PEAK_GBS, 4), "pillow_threads": threads,
                          "pillow_frames_s": round(n / dt_host, 1), "bytes_equal": same}), flush=True)
        del out, nb


def bench_annotator(records, sources):
    d = tempfile.mkdtemp(prefix="annotate_bench_")
    try:
        _bench_annotator_in(d, records, sources)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def _bench_annotator_in(d, records, sources):
    import random
    from PIL import Image
    from jpeg_util import content
    from mspa.annotate import DeviceAnnotator, Mark, PillowAnnotator
    srcs = []
    for s in range(sources):
        p = os.path.join(d, "src", f"{s:05d}.jpg")
        os.makedirs(os.path.dirname(p), exist_ok=True)
        Image.fromarray(content(*HW, s)).save(p, quality=90)
        srcs.append(p)
    rng = random.Random(5)
    jobs = []
    for r in range(records):                                              # VC_D: one disc on image 1, four labelled discs on image 2
        a, b = rng.choice(srcs), rng.choice(srcs)
        col = lambda: (rng.randint(0, 255), rng.randint(0, 255), rng.randint(0, 255))        # noqa: E731
        jobs.append((a, f"{r}_img1.jpg", [Mark(rng.randint(0, HW[1] - 1), rng.randint(0, HW[0] - 1), 10, col())]))
        jobs.append((b, f"{r}_img2.jpg", [Mark(rng.randint(0, HW[1] - 1), rng.randint(0, HW[0] - 1), 10, col(), L, (15, 0))
                                          for L in "ABCD"]))
    res = {}
    for name in ("device", "pillow_serial", "pillow_16_threads"):
        out = os.path.join(d, name)
        t0 = time.perf_counter()
        if name == "device":
            with DeviceAnnotator() as ann:
                for src, dst, marks in jobs:
                    ann.annotate(src, os.path.join(out, dst), marks)
        elif name == "pillow_serial":
            ann = PillowAnnotator()
            for src, dst, marks in jobs:
                ann.annotate(src, os.path.join(out, dst), marks)
        else:
            ann = PillowAnnotator()
            with ThreadPoolExecutor(16) as pool:
                list(pool.map(lambda j: ann.annotate(j[0], os.path.join(out, j[1]), j[2]), jobs))
        res[name] = len(jobs) / (time.perf_counter() - t0)
    same = all(open(os.path.join(d, "device", j[1]), "rb").read() == open(os.path.join(d, "pillow_serial", j[1]), "rb").read()
               for j in jobs)
    print(json.dumps({"what": "annotate", "images": len(jobs), "distinct_sources": sources,
                      "images_per_source": round(len(jobs) / sources, 1), **{k + "_images_s": round(v, 1) for k, v in res.items()},
                      "bytes_equal": same}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--records", type=int, default=1000)
    ap.add_argument("--sources", type=int, default=64)
    a = ap.parse_args()
    from mspa import hostinfo
    threads = max(1, hostinfo.effective_cpus())
    bench_encoder(a.frames, threads)
    bench_annotator(a.records, a.sources)


if __name__ == "__main__":
    main()
