"""The two device paths of handler/ops.py against a host line over the same inputs, one JSON line per configuration.

    python tools/handler_ops_bench.py [--frames 1024] [--reps 5] [--sizes 20000 307200 1000000] [--skip sharpness|outliers]

Sharpness: ``--frames`` ScanNet-shaped (968 x 1296, 4:2:0) JPEG payloads of two kinds (a noisy frame at quality 90, some
730 KB; a smoother one at quality 75, some 270 KB: the size of a ScanNet colour frame) already resident on the device ->
grey decode (mspa_jpeg_decode_luma_device) + Laplacian moments + the download of the partial sums, against Pillow draft-L +
NumPy (the oracle's stencil and ``.var()``) on ``hostinfo.effective_cpus()`` threads.  The file reads and the H2D copy of the
compressed bytes are timed apart (``ingest.image_sharpness`` from files on disk, end to end).

Outlier removal: N uniform points, and the same with 0.1 % of the points at 1 000x the extent, k = 20 ->
``engine.knn_mean_distance`` (box from a device sort, cells, stable sort, search; ends in a synchronise), its stages apart, and
``ops.remove_statistical_outliers`` from a NumPy cloud (upload and download included), against
``scipy.spatial.cKDTree(xyz).query(xyz, k, workers=16)`` with the build of the tree timed apart.  Open3D, the reference's own
means, is not a dependency and is not measured."""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-spatialmllm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)


def _median(fn, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), [round(t, 4) for t in times]


def sharpness(a):
    for name in ("mixed-q90", "smooth-q75"):
        sharpness_of(a, name)


def sharpness_of(a, name):
    import torch
    import handler_ops_util as HU
    from jpeg_util import content, encode
    from mspa import engine, hostinfo, ingest
    H, W = 968, 1296
    dev = "cuda:0"
    if name == "mixed-q90":                  # tests/jpeg_util.py's frame: edges, texture and noise of sigma 18 -- a heavy bit stream
        uniq = [encode(content(H, W, s), quality=90, subsampling=2) for s in range(8)]
    else:                                    # low-frequency content with noise of sigma 8: the size of a ScanNet colour frame
        uniq = [encode(HU.smooth_image(H, W, s), quality=75, subsampling=2) for s in range(8)]
    payloads = [uniq[k % len(uniq)] for k in range(a.frames)]
    sizes = np.array([len(p) for p in payloads], dtype=np.int64)
    offs = np.zeros(a.frames, np.int64)
    offs[1:] = np.cumsum((sizes[:-1] + 15) // 16 * 16)
    buf = np.zeros(int(offs[-1] + sizes[-1] + 31) // 16 * 16, np.uint8)
    for o, p in zip(offs, payloads):
        buf[o:o + len(p)] = np.frombuffer(p, np.uint8)
    desc, st = engine.jpeg_parse_host(payloads)
    assert (st == 0).all()
    src, off_d, nb_d, desc_d = (torch.from_numpy(x).to(dev) for x in (buf, offs, sizes, desc))
    luma = torch.empty((a.frames, H, W), dtype=torch.uint8, device=dev)
    status = torch.empty((a.frames,), dtype=torch.int32, device=dev)
    result = {}

    def device_pass():
        engine.jpeg_decode_luma_device(src, off_d, nb_d, desc_d, (H, W), out=luma, status=status)
        result["var"] = engine.laplacian_variance(engine.laplacian_moments(luma), H * W)      # (.cpu(): synchronises)

    def decode_only():
        engine.jpeg_decode_luma_device(src, off_d, nb_d, desc_d, (H, W), out=luma, status=status)
        torch.cuda.synchronize()

    def moments_only():
        engine.laplacian_moments(luma)
        torch.cuda.synchronize()

    device_pass()
    assert int((status != 0).sum()) == 0
    want = [HU.variance_numpy(HU.pillow_luma(p)) for p in uniq]
    same = all(abs(result["var"][k] - want[k % len(uniq)]) <= 1e-12 * want[k % len(uniq)] for k in range(a.frames))
    t_dev, all_dev = _median(device_pass, a.reps)
    t_dec, _ = _median(decode_only, a.reps)
    t_mom, _ = _median(moments_only, a.reps)
    cpus = hostinfo.effective_cpus()
    n_host = min(a.frames, 8 * cpus)
    with ThreadPoolExecutor(cpus) as pool:
        t0 = time.perf_counter()
        list(pool.map(lambda k: HU.variance_numpy(HU.pillow_luma(payloads[k])), range(n_host)))
        t_host = (time.perf_counter() - t0) / n_host * a.frames
        t0 = time.perf_counter()
        list(pool.map(lambda k: HU.pillow_luma(payloads[k]), range(n_host)))
        t_host_decode = (time.perf_counter() - t0) / n_host * a.frames
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for k, p in enumerate(payloads):
            paths.append(os.path.join(tmp, f"{k}.jpg"))
            with open(paths[-1], "wb") as f:
                f.write(p)
        ingest.image_sharpness(paths[:16])
        t_files, all_files = _median(lambda: ingest.image_sharpness(paths, n_threads=cpus), max(1, a.reps // 2))
    print(json.dumps({"what": "sharpness", "content": name, "frames": a.frames, "hw": [H, W], "mean_payload_kb": round(float(sizes.mean()) / 1024, 1),
                      "scores_within_1e-12_of_numpy": bool(same), "device_resident_s": round(t_dev, 4), "device_resident_passes_s": all_dev,
                      "decode_luma_s": round(t_dec, 4), "moments_s": round(t_mom, 4),
                      "moments_luma_gbps": round(a.frames * H * W / t_mom / 1e9, 1), "from_files_s": round(t_files, 4),
                      "from_files_passes_s": all_files, "host_threads": cpus, "host_frames_timed": n_host,
                      "host_s_scaled_to_frames": round(t_host, 4), "host_decode_only_s_scaled": round(t_host_decode, 4),
                      "host_over_device_resident": round(t_host / t_dev, 2), "host_over_from_files": round(t_host / t_files, 2)}), flush=True)


def outliers(a):
    import torch
    from scipy.spatial import cKDTree
    import handler_ops_util as HU
    from mspa import _lib, engine
    from spatial_engine.utils.scannet_utils.handler import ops
    k = 20
    dev = "cuda:0"
    for n in a.sizes:
        for far in (False, True):
            rng = np.random.default_rng(n + far)
            xyz = rng.random((n, 3))
            if far:
                idx = rng.choice(n, size=n // 1000, replace=False)
                xyz[idx] = (rng.random((len(idx), 3)) - 0.5) * 2000.0
            x_d = torch.from_numpy(xyz).to(dev)
            mean, evals = engine.knn_mean_distance(x_d, k, want_evals=True)
            torch.cuda.synchronize()

            def device_pass():
                engine.knn_mean_distance(x_d, k)
                torch.cuda.synchronize()
            t_dev, all_dev = _median(device_pass, a.reps)
            # the stages apart, each ending in a synchronise
            lib = _lib.load()
            stage = {}
            t0 = time.perf_counter()
            r = n // 100
            box = np.ascontiguousarray(torch.sort(x_d, dim=0).values[[r, n - 1 - r]].cpu().numpy())
            stage["box_sort_s"] = time.perf_counter() - t0
            grid = np.zeros((_lib.KNN_GRID_BYTES,), dtype=np.uint8)
            _lib.check(lib.mspa_knn_grid_host(box[0].ctypes.data, box[1].ctypes.data, n, k, grid.ctypes.data))
            cells = torch.empty((n,), dtype=torch.int32, device=dev)
            t0 = time.perf_counter()
            _lib.check(lib.mspa_knn_cells_device(x_d.data_ptr(), n, grid.ctypes.data, cells.data_ptr(), engine._stream_ptr()))
            order = torch.sort(cells, stable=True).indices
            torch.cuda.synchronize()
            stage["cells_and_sort_s"] = time.perf_counter() - t0
            work = engine._workspace(int(lib.mspa_knn_workspace_bytes(n, k)), x_d.device)
            out = torch.empty((n,), dtype=torch.float64, device=dev)
            t0 = time.perf_counter()
            _lib.check(lib.mspa_knn_mean_distance_device(x_d.data_ptr(), n, k, grid.ctypes.data, order.data_ptr(), out.data_ptr(), None,
                                                         work.data_ptr(), int(work.numel()), engine._stream_ptr()))
            torch.cuda.synchronize()
            stage["search_s"] = time.perf_counter() - t0
            assert torch.equal(out, mean)
            t_ops, all_ops = _median(lambda: ops.remove_statistical_outliers(xyz, k, 1.0), a.reps)
            kept = len(ops.remove_statistical_outliers(xyz, k, 1.0))
            t0 = time.perf_counter()
            tree = cKDTree(xyz)
            t_build = time.perf_counter() - t0
            t0 = time.perf_counter()
            d, _ = tree.query(xyz, k=k, workers=16)
            t_query = time.perf_counter() - t0
            want = HU.knn_mean_oracle(xyz, k) if n <= 400000 else None
            ok = None if want is None else bool((np.abs(mean.cpu().numpy() - want) <= HU.knn_tolerance(k) * want).all())
            print(json.dumps({"what": "outliers", "n": n, "far_points": int(n // 1000) if far else 0, "k": k,
                              "within_tolerance_of_ckdtree": ok, "evaluations_per_point": round(float(evals.sum(dtype=torch.int64)) / n, 1),
                              "max_evaluations": int(evals.max()), "knn_mean_distance_s": round(t_dev, 4), "knn_passes_s": all_dev,
                              **{key: round(v, 4) for key, v in stage.items()},
                              "remove_statistical_outliers_numpy_in_out_s": round(t_ops, 4), "ops_passes_s": all_ops, "kept": kept,
                              "ckdtree_build_s": round(t_build, 4), "ckdtree_query_16_workers_s": round(t_query, 4),
                              "ckdtree_over_knn_mean_distance": round((t_build + t_query) / t_dev, 2),
                              "ckdtree_over_ops": round((t_build + t_query) / t_ops, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=[20000, 307200, 1000000])
    ap.add_argument("--skip", choices=("sharpness", "outliers"), default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this benchmark measures the device path: it needs the GPU"
    if a.skip != "sharpness":
        sharpness(a)
    if a.skip != "outliers":
        outliers(a)


if __name__ == "__main__":
    main()
