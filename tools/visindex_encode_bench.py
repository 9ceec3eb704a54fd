#!/usr/bin/env python3
"""Per-scene cost of turning K1's bit matrix into the visibility index's row group, host encode against device encode (K12).

    python tools/visindex_encode_bench.py [--frames 320] [--points 131072] [--scenes 7] [--visible 0.12]

One synthetic scene of the `--workload scenes` shape (each frame sees a few runs of neighbouring vertices, `--visible` of them in
all); per path the median over the warm scenes (the first one is dropped) of what one encoder thread spends on it:
``visindex.from_bits`` + ``VisibilityCSR.to_row_group``, i.e. CSR compaction, K10's text, the copies to the host and the parquet
encode.  Reported per scene: encoder-thread CPU (``time.thread_time``), wall, bytes copied device -> host, the values chunk's
size in the file, and -- device path -- the GPU time of the K12 call (pack, compress, compact and their prefix sums, between
two events on the stream).  Prints one JSON line."""
import argparse
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "multi-spatialmllm_amd"), ROOT]


def make_bits(frames, points, visible, seed=7):
    """[F, ceil(N / 64)] int64 on the device: every frame sees 48 runs of neighbouring vertices."""
    import numpy as np
    import torch
    rng = np.random.default_rng(seed)
    seen = np.zeros((frames, points), dtype=bool)
    run = max(1, int(points * visible / 48))
    for f in range(frames):
        for s in rng.integers(0, max(1, points - run), size=48):
            keep = rng.random(run) < 0.85                     # holes: occluded vertices inside a visible surface
            seen[f, s:s + run] |= keep
    pad = (-points) % 64
    packed = np.packbits(np.pad(seen, ((0, 0), (0, pad))), axis=1, bitorder="little")
    return torch.from_numpy(packed.view(np.int64).copy()).cuda(), float(seen.mean())


def d2h_bytes(csr, rows):
    total = 0
    for a in (csr.i2p_offsets, csr.i2p_indices, csr.p2i_offsets, csr.p2i_indices):
        total += 0 if a is None else a.nbytes
    for pair in (csr.i2p_text, csr.p2i_text):
        if pair is not None:
            total += pair[0].nbytes + pair[1].nbytes
    if csr.values_pages is not None:
        total += csr.values_pages["chunk"].nbytes + 4 * (rows + 1)          # the chunk, and the string offsets the page cuts read
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=320)
    ap.add_argument("--points", type=int, default=131072)
    ap.add_argument("--scenes", type=int, default=7, help="scenes per path; the first is the warm-up")
    ap.add_argument("--visible", type=float, default=0.12)
    a = ap.parse_args()
    import pyarrow.parquet as pq
    import torch
    from mspa import engine, visindex
    bits, density = make_bits(a.frames, a.points, a.visible)
    ids = [f"{5 * f:05d}" for f in range(a.frames)]
    rows = a.frames + a.points
    out = {"frames": a.frames, "vertices": a.points, "visible_fraction": round(density, 4), "warm_scenes": a.scenes - 1,
           "statistic": "median of the warm scenes", "paths": {}}
    tables = {}
    for path in ("host", "device"):
        cpu, wall, moved, chunk = [], [], [], []
        for k in range(a.scenes):
            torch.cuda.synchronize()
            c0, t0 = time.thread_time(), time.perf_counter()
            csr = visindex.from_bits(bits, ids, a.points, text=True, indices=False, pages=path == "device")
            blob = csr.to_row_group("scene0000_00")
            cpu.append(time.thread_time() - c0)
            wall.append(time.perf_counter() - t0)
            moved.append(d2h_bytes(csr, rows))
            chunk.append(pq.ParquetFile(io.BytesIO(blob)).metadata.row_group(0).column(1).total_compressed_size)
        tables[path] = pq.read_table(io.BytesIO(blob))
        out["paths"][path] = {"encoder_thread_cpu_ms": round(1e3 * statistics.median(cpu[1:]), 2),
                              "wall_ms": round(1e3 * statistics.median(wall[1:]), 2), "d2h_bytes": int(statistics.median(moved[1:])),
                              "values_chunk_bytes": int(statistics.median(chunk[1:])), "file_bytes": len(blob),
                              "cpu_ms_all": [round(1e3 * v, 1) for v in cpu], "wall_ms_all": [round(1e3 * v, 1) for v in wall]}
    out["tables_equal"] = bool(tables["host"].equals(tables["device"]))
    # K12 alone, on text that is already there
    o1, i1 = engine.bitset_csr(bits)
    t = engine.bits_transpose(bits)
    o2, i2 = engine.bitset_csr(t[:a.points].contiguous())
    t1 = engine.format_lists_device(o1, i1)
    t2 = engine.format_lists_device(o2, i2, visindex.VisibilityCSR(ids, a.points, None, None, None, None).quoted_image_ids())
    offsets, data = torch.cat([t1[1][:-1], t2[1] + t1[0].numel()]), torch.cat([t1[0], t2[0]])
    ms = []
    for _ in range(a.scenes):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        pages = engine.parquet_string_pages_device(offsets, data)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    out["k12"] = {"text_bytes": int(data.numel()), "pages": int(len(pages["compressed"])), "chunk_bytes": int(pages["chunk"].numel()),
                  "call_gpu_ms": round(statistics.median(ms[1:]), 3), "call_gpu_ms_all": [round(v, 2) for v in ms],
                  "note": "two events around engine.parquet_string_pages_device: the three kernels, torch's prefix sums and the "
                          "call's small read-backs"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
