#!/usr/bin/env python3
"""Per-object clouds from instance masks: ``SceneInfoHandler.instance_clouds`` against the per-object composition
``get_instance_mask`` + ``project_image_to_3d_with_mask``, and its stages alone.  Prints markdown (profiles/instance_clouds_device.md).

    python tools/instance_clouds_bench.py [--passes 7] [--frames 64] [--objects 30] [--decode-counts 64,1024] [--stages abc]

(a) 8-bit mask decode: Pillow-written 1296 x 968 label images, ``ingest.read_label_frames_device`` against ``_images.read_depth`` on
    16 host threads (8 distinct files, hard-linked under the other names: every name is opened, read and decoded on its own);
(b) the whole path from files: one scene of ``--frames`` frames at ScanNet's shape (colour grid 1296 x 968, depth 640 x 480) with
    about ``--objects`` objects per frame; first compared for equality over every (image, object), then timed alternately;
(c) the split alone on the K3 outputs of 16 frames, in GB/s of the bytes it reads and writes.
One warm-up pass, then the median of the timed passes, all listed; a device synchronise on both sides of every timed region."""
import argparse
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "multi-spatialmllm_amd"), ROOT]
HW, DHW = (968, 1296), (480, 640)


def label_map(rng, n_objects):
    """[968, 1296] uint8: about n_objects rectangles over label 0, as an instance-filt image looks."""
    H, W = HW
    a = np.zeros(HW, np.uint8)
    for v in rng.permutation(np.arange(1, n_objects + 1)):
        h, w = int(rng.integers(60, 360)), int(rng.integers(60, 420))
        y, x = int(rng.integers(0, H - 40)), int(rng.integers(0, W - 40))
        a[y:y + h, x:x + w] = v
    return a


def fmt(xs):
    return ", ".join(f"{x * 1e3:.1f}" for x in xs)


def timed(fn, passes, torch):
    out = []
    for k in range(passes + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k:
            out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--objects", type=int, default=30)
    ap.add_argument("--decode-counts", default="64,1024")
    ap.add_argument("--stages", default="abc")
    args = ap.parse_args()
    import torch
    from PIL import Image
    from mspa import engine, ingest, instances, synth
    from spatial_engine.utils.scannet_utils.handler import _images
    from spatial_engine.utils.scannet_utils.handler.info_handler import SceneInfoHandler
    rng = np.random.default_rng(30)
    root = tempfile.mkdtemp(prefix="instance_clouds_bench_")
    distinct = 8
    maps = [label_map(rng, args.objects) for _ in range(distinct)]
    seeds = os.path.join(root, "seed")
    os.makedirs(seeds)
    for k, m in enumerate(maps):
        Image.fromarray(m, mode="L").save(os.path.join(seeds, f"{k}.png"))
    print("# Per-object clouds from instance masks: `instance_clouds` against the per-object composition\n")
    print(f"`python tools/instance_clouds_bench.py --passes {args.passes} --frames {args.frames} --objects {args.objects} "
          f"--decode-counts {args.decode_counts} --stages {args.stages}` on one MI355X, one process.  One warm-up pass, then the median of "
          "the timed passes (all listed, ms); a device synchronise on both sides of every timed region.\n")

    if "a" in args.stages:
        print("## (a) 8-bit mask decode, 1296 x 968 label images written by Pillow\n")
        print("| images | device path, median (ms) | passes (ms) | 16 host threads, median (ms) | passes (ms) | host / device |")
        print("|---|---|---|---|---|---|")
        for n in [int(x) for x in args.decode_counts.split(",") if x]:
            d = os.path.join(root, f"decode{n}")
            os.makedirs(d)
            paths = []
            for k in range(n):
                paths.append(os.path.join(d, f"{k}.png"))
                os.link(os.path.join(seeds, f"{k % distinct}.png"), paths[-1])
            got = ingest.read_label_frames_device(paths, "cuda", 16)
            assert all(np.array_equal(got[k].cpu().numpy(), maps[k % distinct]) for k in range(min(n, 2 * distinct)))
            del got

            def host():
                with ThreadPoolExecutor(max_workers=16) as ex:
                    return list(ex.map(_images.read_depth, paths))
            dev_t = timed(lambda: ingest.read_label_frames_device(paths, "cuda", 16), args.passes, torch)
            host_t = timed(host, args.passes, torch)
            print(f"| {n} | **{statistics.median(dev_t) * 1e3:.1f}** | {fmt(dev_t)} | **{statistics.median(host_t) * 1e3:.1f}** | {fmt(host_t)} | "
                  f"{statistics.median(host_t) / statistics.median(dev_t):.2f} x |")
        print()

    if "b" in args.stages or "c" in args.stages:
        sc = synth.make_scene(77, n_points=1024, n_frames=distinct, color_hw=HW, depth_hw=DHW, invalid_pose_frac=0.0, with_color=False,
                              scene_id="scene0977_00")
        base = sc.image_ids
        ids = [f"{k:05d}" for k in range(args.frames)]
        sc.E = {i: sc.E[base[k % distinct]] for k, i in enumerate(ids)}
        sc.depth = {i: sc.depth[base[k % distinct]] for k, i in enumerate(ids)}
        where = synth.write_scannet_layout([sc], root, link_identical=True)
        scans = os.path.join(root, "scans")
        os.makedirs(os.path.join(scans, sc.scene_id, "instance-filt"))
        for k, i in enumerate(ids):
            os.link(os.path.join(seeds, f"{k % distinct}.png"), os.path.join(scans, sc.scene_id, "instance-filt", f"{int(i)}.png"))
        import pickle
        handler = SceneInfoHandler(pickle.load(open(where["info_path"], "rb")), posed_images_root=where["posed_images_root"],
                                   instance_data_root=where["instance_data_root"], mask_image_root=scans)
        present = [[int(v) - 1 for v in np.unique(maps[k % distinct]) if v] for k in range(args.frames)]

    if "b" in args.stages:
        def composition():
            out = {}
            for k, i in enumerate(ids):
                for t in present[k]:
                    out[i, t] = handler.project_image_to_3d_with_mask(sc.scene_id, i, handler.get_instance_mask(sc.scene_id, i, t), False)
            return out
        torch.cuda.synchronize()
        want = composition()                                  # the composition's warm-up pass is the equality reference
        clouds = handler.instance_clouds(sc.scene_id, num_workers=16)
        assert instances.LAST_INSTANCE_CLOUDS["path"] == "device", instances.LAST_INSTANCE_CLOUDS
        rows = 0
        for (i, t), w in want.items():
            got = clouds.cloud(i, t).cpu().numpy()
            assert got.shape == w.shape and got.tobytes() == w.tobytes(), (i, t)
            rows += len(w)
        del clouds
        new_t, old_t = [], []
        for _ in range(args.passes):                          # alternately, in one process
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            handler.instance_clouds(sc.scene_id, num_workers=16)
            torch.cuda.synchronize()
            new_t.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            composition()
            torch.cuda.synchronize()
            old_t.append(time.perf_counter() - t0)
        n_obj = sum(len(p) for p in present)
        print(f"## (b) the whole path from files: {args.frames} frames, {n_obj} (image, object) clouds, {rows:,} rows\n")
        print("Every (image, object) cloud was first compared with the composition's, byte for byte.\n")
        print("| line | median (ms) | passes (ms) |")
        print("|---|---|---|")
        print(f"| composition: `get_instance_mask` + `project_image_to_3d_with_mask` per (image, object), NumPy out | "
              f"**{statistics.median(old_t) * 1e3:.0f}** | {fmt(old_t)} |")
        print(f"| `instance_clouds` (device tensors out) | **{statistics.median(new_t) * 1e3:.1f}** | {fmt(new_t)} |")
        print(f"\nComposition over `instance_clouds`: **{statistics.median(old_t) / statistics.median(new_t):.1f} x**.\n")
        # the stages of instance_clouds, each with a synchronise behind it
        depth_paths = [handler.get_depth_image_path(sc.scene_id, i) for i in ids]
        mask_paths = [os.path.join(scans, sc.scene_id, "instance-filt", f"{int(i)}.png") for i in ids]
        st = {}
        st["depth decode"] = timed(lambda: ingest.read_depth_frames_device(depth_paths, "cuda", 16), args.passes, torch)
        st["mask decode"] = timed(lambda: ingest.read_label_frames_device(mask_paths, "cuda", 16), args.passes, torch)
        per = max(1, (1 << 30) // (HW[0] * HW[1] * 24))
        chunk = ids[:per]
        depth = ingest.read_depth_frames_device(depth_paths[:len(chunk)], "cuda", 16)
        labels = ingest.read_label_frames_device(mask_paths[:len(chunk)], "cuda", 16)
        mats = torch.from_numpy(engine.frame_matrices(sc.K, sc.A, [sc.E[i] for i in chunk])).cuda()
        pairs = torch.arange(len(chunk), dtype=torch.int32, device="cuda")[:, None].repeat(1, 2).contiguous()
        out = engine.alloc_pair_outputs(len(chunk), HW, ("xyz_f64", "valid_u8"), "cuda")
        st[f"K3 exact, {len(chunk)} frames (one chunk)"] = timed(lambda: engine.pair_reproject(depth, mats, pairs, HW, out), args.passes, torch)
        st[f"split, {len(chunk)} frames (one chunk)"] = timed(lambda: engine.instance_split(labels, out["valid_u8"], out["xyz_f64"]), args.passes, torch)
        print(f"Stages of `instance_clouds`, each alone with a synchronise behind it (the run above takes {args.frames} frames in chunks of {per}):\n")
        print("| stage | median (ms) | passes (ms) |")
        print("|---|---|---|")
        for k, v in st.items():
            print(f"| {k} | {statistics.median(v) * 1e3:.1f} | {fmt(v)} |")
        print()
        del depth, labels, out

    if "c" in args.stages:
        n = min(16, args.frames)
        depth = ingest.read_depth_frames_device([handler.get_depth_image_path(sc.scene_id, i) for i in ids[:n]], "cuda", 16)
        labels = torch.from_numpy(np.stack([maps[k % distinct] for k in range(n)])).cuda()
        mats = torch.from_numpy(engine.frame_matrices(sc.K, sc.A, [sc.E[i] for i in ids[:n]])).cuda()
        pairs = torch.arange(n, dtype=torch.int32, device="cuda")[:, None].repeat(1, 2).contiguous()
        out = engine.alloc_pair_outputs(n, HW, ("xyz_f64", "valid_u8"), "cuda")
        engine.pair_reproject(depth, mats, pairs, HW, out)
        total = int(engine.instance_split(labels, out["valid_u8"], out["xyz_f64"])[1][-1])
        t = timed(lambda: engine.instance_split(labels, out["valid_u8"], out["xyz_f64"]), args.passes, torch)
        P = HW[0] * HW[1]
        # count: labels + valid; scatter: labels + valid, the selected rows read and written, their pixel index; extents: the rows again
        nbytes = n * P * 2 * 2 + total * (24 + 24 + 4 + 24)
        print(f"## (c) the split alone: {n} frames, {total:,} selected pixels of {n * P:,}\n")
        print(f"`engine.instance_split` (count, the counts' download, scatter, extents): median **{statistics.median(t) * 1e3:.2f} ms** "
              f"({fmt(t)}); {nbytes / 1e6:,.0f} MB read and written -> **{nbytes / statistics.median(t) / 1e9:,.0f} GB/s**.\n")


if __name__ == "__main__":
    main()
