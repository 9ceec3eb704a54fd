"""Rigid-body track grouping: the SciPy path (K7, download of the [P, P] matrix, linkage + fcluster on one host thread) against
the device path (engine.track_rigid_groups: K7 + K7b, download of the labels), on one TAPVid-sized block (T = 300) of P = 256
and of P = 1024 points, and a batch of 64 equal blocks through one K7 launch + one K7b launch against 64 trips through the SciPy
path.  Every timing is a host clock around work that ends in a download (a synchronise); warm launches, medians of --repeats
runs, the two paths alternating.  Prints one JSON line; the device's current clock is noted in it.

    python tools/linkage_bench.py [--repeats 7] [--batch 64]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "multi-spatialmllm_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def scipy_groups(engine, dev_tracks):
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.spatial.distance import squareform
    loss = engine.track_rigidity_loss(dev_tracks).cpu().numpy()
    labels = fcluster(linkage(squareform(loss, checks=False), method="average"), 0.1, criterion="distance")
    return [np.where(labels == i)[0].tolist() for i in range(1, max(labels) + 1)]


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main(argv=None):
    import torch
    from mspa import _lib, engine, synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=64)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("linkage_bench needs the GPU: a CPU run gives no time")
    dev = "cuda:0"
    result = {"device": _lib.device_info(0), "repeats": args.repeats, "T": 300, "single": {}, "batch": {}}
    for P in (256, 1024):
        tr = synth.make_tracks(900 + P, T=300, P=P, n_groups=8)
        tracks = torch.from_numpy(np.ascontiguousarray(tr.tracks_XYZ, dtype=np.float64)).to(dev)
        assert scipy_groups(engine, tracks) == engine.track_rigid_groups(tracks)                 # warm-up, and the same answer
        host_ms, dev_ms, k7_ms, k7b_ms = [], [], [], []
        for _ in range(args.repeats):
            host_ms.append(timed(lambda: scipy_groups(engine, tracks))[0])
            dev_ms.append(timed(lambda: engine.track_rigid_groups(tracks))[0])
            ms, loss = timed(lambda: (engine.track_rigidity_loss(tracks), torch.cuda.synchronize())[0])
            k7_ms.append(ms)
            k7b_ms.append(timed(lambda: (engine.track_linkage(loss), torch.cuda.synchronize())[0])[0])
        result["single"][str(P)] = {"scipy_path_ms": round(statistics.median(host_ms), 3),
                                    "device_path_ms": round(statistics.median(dev_ms), 3),
                                    "k7_ms": round(statistics.median(k7_ms), 3), "k7b_ms": round(statistics.median(k7b_ms), 3),
                                    "download_bytes": {"scipy_path": 8 * P * P, "device_path": 4 * P + 4}}
    P, B = 256, args.batch
    blocks = [np.ascontiguousarray(synth.make_tracks(2000 + b, T=300, P=P, n_groups=8).tracks_XYZ, dtype=np.float64) for b in range(B)]
    singles = [torch.from_numpy(x).to(dev) for x in blocks]
    stacked = torch.from_numpy(np.stack(blocks)).to(dev)

    def batched():
        _, labels, status = engine.track_linkage(engine.track_rigidity_loss_batch(stacked))
        labels, status = labels.cpu().numpy(), status.cpu().numpy()
        assert not status.any()
        return [[np.where(row == i)[0].tolist() for i in range(1, int(row.max()) + 1)] for row in labels]

    assert batched() == [scipy_groups(engine, x) for x in singles]
    host_ms, dev_ms = [], []
    for _ in range(args.repeats):
        host_ms.append(timed(lambda: [scipy_groups(engine, x) for x in singles])[0])
        dev_ms.append(timed(batched)[0])
    result["batch"] = {"blocks": B, "P": P, "scipy_path_ms": round(statistics.median(host_ms), 3),
                       "device_path_ms": round(statistics.median(dev_ms), 3)}
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
