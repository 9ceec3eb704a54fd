#!/usr/bin/env python3
"""What one sample of the pair table costs: the host line (``pd.read_parquet`` + ``sampling.sample_dataframe``: what the
camera-movement and visual-correspondence builders run per question type with ``MSPA_PAIRTABLE`` unset) against
``pairtable.PairTable.sample`` (the table decoded, classified and partitioned on the GPU, the draws on the host).

    python tools/pairtable_bench.py [--scenes 100 300] [--passes 5] [--samples 1000000] [--skip-host]

The table: ``--scenes`` scenes of 320 frames (51 040 pairs each: ScanNet's shape) in this project's layout -- a row group per scene
through ``parquet_splice.encode_row_group``, ids dictionary-coded, doubles PLAIN, Snappy -- about 60 % of the overlaps zero, the
others spread over (0, 100).  Per size: the host line's two stages, ``--passes`` warm passes each after one warm-up; the device
path's FIRST pass of a fresh ``PairTable`` (file read, H2D, decompress, columns, codes, partition, draws, row gather, id columns,
frame: each stage ended by a device synchronise) and ``--passes`` CACHED passes (the same table and parameter set again: draws,
row gather, id columns, frame).  Medians, with every pass listed.  Sample: (``--samples``, 0, 6, 35, 1), the camera-movement
builder's.  Prints one JSON line."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "multi-spatialmllm_amd"), ROOT]

FRAMES = 320


def write_table(path, scenes, seed=0):
    import numpy as np
    import pyarrow as pa
    from mspa import parquet_splice
    rng = np.random.default_rng(seed)
    a, b = np.triu_indices(FRAMES, 1)
    ids = pa.array([f"{k * 10:05d}" for k in range(FRAMES)], type=pa.string())
    id1, id2 = ids.take(pa.array(a)), ids.take(pa.array(b))
    n = len(a)
    with parquet_splice.SplicedParquetWriter(path) as w:
        for s in range(scenes):
            overlap = rng.uniform(0.0, 100.0, n)
            overlap[rng.random(n) < 0.6] = 0.0
            t = pa.table({"scene_id": pa.array([f"scene{s:04d}_00"] * n, type=pa.string()), "image_id1": id1, "image_id2": id2,
                          "overlap": overlap, "distance": rng.uniform(0.0, 9.0, n), "yaw": rng.uniform(-180.0, 180.0, n),
                          "pitch": rng.uniform(-90.0, 90.0, n)})
            w.append(parquet_splice.encode_row_group(t, use_dictionary=["scene_id", "image_id1", "image_id2"]))
    return scenes * n, os.path.getsize(path)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0


def summary(passes):
    return {"median_s": round(statistics.median(passes), 4), "passes_s": [round(p, 4) for p in passes]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, nargs="+", default=[100, 300])
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--samples", type=int, default=1000000)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import pandas as pd
    import torch
    from mspa import pairtable
    from mspa.sampling import sample_dataframe
    args = (a.samples, 0, 6, 35, 1)
    quiet = contextlib.redirect_stdout(io.StringIO())
    out = {"sample": list(args), "passes": a.passes, "sizes": []}
    with tempfile.TemporaryDirectory() as d:
        for scenes in a.scenes:
            path = os.path.join(d, f"pairs_{scenes}.parquet")
            rows, nbytes = write_table(path, scenes)
            size = {"scenes": scenes, "rows": rows, "file_mb": round(nbytes / 1e6, 1)}
            want = None
            if not a.skip_host:
                read, sample = [], []
                for k in range(a.passes + 1):
                    df, t_read = timed(lambda: pd.read_parquet(path))
                    np.random.seed(1)
                    with quiet:
                        want, t_sample = timed(lambda: sample_dataframe(df, *args))
                    if k:
                        read.append(t_read)
                        sample.append(t_sample)
                    del df
                size["host"] = {"read_parquet": summary(read), "sample_dataframe": summary(sample),
                                "total_median_s": round(statistics.median(r + s for r, s in zip(read, sample)), 4)}
            # warm the allocator and the kernels on another table object, then the measured first pass on a fresh one
            with quiet:
                pairtable.PairTable(path, "cuda").sample(*args)
            t = pairtable.PairTable(path, "cuda")
            t.stage_times = {}
            np.random.seed(1)
            torch.cuda.synchronize()
            with quiet:
                got, t_first = timed(lambda: t.sample(*args))
            size["device_first"] = {"wall_s": round(t_first, 4), "stages_s": {k: round(v, 4) for k, v in t.stage_times.items()}}
            cached, stages = [], []
            for _ in range(a.passes):
                t.stage_times = {}
                np.random.seed(1)
                with quiet:
                    got, dt = timed(lambda: t.sample(*args))
                cached.append(dt)
                stages.append(dict(t.stage_times))
            size["device_cached"] = dict(summary(cached), stages_median_s={k: round(statistics.median(s[k] for s in stages), 4) for k in stages[0]})
            size["stats"] = dict(t.stats)
            size["declined"] = t.last_decline
            if want is not None:
                pd.testing.assert_frame_equal(got, want, check_exact=True)
                size["same_frame_as_host"] = True
                size["host_over_device_cached"] = round(size["host"]["total_median_s"] / size["device_cached"]["median_s"], 2)
                size["host_over_device_first"] = round(size["host"]["total_median_s"] / t_first, 2)
            size["sampled_rows"] = len(got)
            out["sizes"].append(size)
            del t, got, want
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
