#!/usr/bin/env python3
"""Per-scene cost of reading the visibility index back into bitsets: the host path (``scene_dict`` -> ``json.loads`` ->
``pack_index_lists`` -> upload: the code every consumer runs with ``MSPA_VISINDEX_DECODE`` unset) against
``visindex.SceneRowGroups.scene_bits`` (the pages decompressed, walked, parsed and packed on the GPU).

    python tools/visindex_decode_bench.py [--frames 320] [--points 131072] [--scenes 16] [--passes 6] [--host-scenes 4]

The file: ``--scenes`` scenes of the `--workload scenes` shape (tools/visindex_encode_bench.py's ``make_bits``), each one row
group written the way ``make_visibility_info.run_split`` writes it -- ``visindex.from_bits(...).to_row_group`` spliced by
``parquet_splice.SplicedParquetWriter`` -- once with pyarrow's pages (``--layout host``, the default) and once with K12's
(``--layout device``).  A pass reads every scene's bitsets (the host path: the first ``--host-scenes`` scenes) through a fresh
``SceneRowGroups``; the first pass is the warm-up, the median is over the others, all passes are listed.  Reported per scene:
wall, the process's CPU time (``time.process_time``: all threads, what a CPU quota counts), the bytes uploaded, and the device
path's stages (each ended by a device synchronise, so their sum exceeds the unsplit wall a little).  The device path runs twice
(``--route both``): with the Snappy decode by 64 KiB blocks, which is what ``scene_bits`` does, and with the one-wave kernel
for every page (``SceneRowGroups.decode_by_blocks = False``: the paths named ``device_one_wave``) -- both in this process, beside
the host path.  Then the decode calls alone, between two events on the stream: one scene's pages in one call, and 8 scenes' pages
in one call, by either route.  Prints one JSON line.  Kernel-by-kernel times (scan, block decode and last pass apart) come from
a separate ``rocprofv3 --kernel-trace --stats`` run of this tool with ``--device-only --route blocks``.

``--layout pandas``: the same scenes as ONE table written the reference's way, ``DataFrame.to_parquet(path, index=False)`` --
pyarrow's defaults: dictionary encoding on, row groups of 1 Mi rows that mix scenes, a dictionary page and one RLE_DICTIONARY
page in front of the PLAIN pages of every row group.  The device path then runs with ``page_kinds = "plain"`` (dictionary-coded
pages decline the scene to the host path: the paths named ``device_plain``) and with ``"any"`` (``device_any``); every path
reports its declined scenes, and each scene's wall of the last pass is listed (``scene_ms_last_pass``) beside the pages it
needed.  The host path of such a file reads a whole row group for its first scene and keeps it (``scene_dict``).

``--lists``: the rows as LISTS, the depth builders' route -- ``scene_lists`` and one ``pick`` of one position per image, per scene
-- twice in turn with ``scene_bits`` (``page_kinds = "any"``) on the same file in this process, and the builders' access with the
switch unset: ``json.loads`` of each image's text, ``len`` and one element, the texts already in memory.  Reports
``lists_over_bits`` and ``host_access_over_lists``; nothing else runs."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "multi-spatialmllm_amd"), ROOT, os.path.dirname(os.path.abspath(__file__))]


def write_index(path, bits, ids, points, scenes, layout):
    from mspa import parquet_splice, visindex
    with parquet_splice.SplicedParquetWriter(path) as w:
        for k in range(scenes):
            csr = visindex.from_bits(bits, ids, points, text=True, indices=False, pages=layout == "device")
            w.append(csr.to_row_group(f"scene{k:04d}_00"))
    return os.path.getsize(path)


def write_pandas_index(path, bits, ids, points, scenes):
    """All scenes as one DataFrame -> ``to_parquet(index=False)``, as make_visibility_info.py:71 does."""
    import pyarrow as pa
    from mspa import visindex
    csr = visindex.from_bits(bits, ids, points, text=True, indices=False)
    df = pa.concat_tables([csr.to_arrow(f"scene{k:04d}_00") for k in range(scenes)]).to_pandas()
    df.to_parquet(path, index=False)
    return os.path.getsize(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=320)
    ap.add_argument("--points", type=int, default=131072)
    ap.add_argument("--scenes", type=int, default=16)
    ap.add_argument("--passes", type=int, default=6, help="passes per path; the first is the warm-up")
    ap.add_argument("--host-scenes", type=int, default=4, help="scenes of a host-path pass")
    ap.add_argument("--visible", type=float, default=0.12)
    ap.add_argument("--layout", choices=("host", "device", "pandas"), default="host")
    ap.add_argument("--device-only", action="store_true", help="skip the host path and the kernel-alone timings (for a profiler run)")
    ap.add_argument("--route", choices=("both", "blocks", "one-wave"), default="both",
                    help="the device path's Snappy decode: one wave per 64 KiB block, the one-wave kernel for every page, or both in turn")
    ap.add_argument("--lists", action="store_true",
                    help="time scene_lists + one pick per image (the depth builders' route) beside scene_bits and beside the builders' host access")
    a = ap.parse_args()
    import numpy as np
    import torch
    from mspa import engine, visindex
    from visindex_encode_bench import make_bits
    bits, density = make_bits(a.frames, a.points, a.visible)
    ids = [f"{5 * f:05d}" for f in range(a.frames)]
    scene_ids = [f"scene{k:04d}_00" for k in range(a.scenes)]
    tmp = tempfile.mkdtemp(prefix="visindex_decode_bench_")
    path = os.path.join(tmp, "vis.parquet")
    file_bytes = (write_pandas_index(path, bits, ids, a.points, a.scenes) if a.layout == "pandas"
                  else write_index(path, bits, ids, a.points, a.scenes, a.layout))
    print(f"index written: {file_bytes} bytes", file=sys.stderr, flush=True)
    out = {"frames": a.frames, "vertices": a.points, "visible_fraction": round(density, 4), "scenes": a.scenes, "layout": a.layout,
           "file_bytes": file_bytes, "warm_passes": a.passes - 1, "statistic": "median of the warm passes, per scene", "paths": {}}
    want = bits.cpu().numpy()

    def run(path_name, scenes, stages, by_blocks=True, page_kinds="plain"):
        wall, cpu, h2d, st_all = [], [], [], []
        for _ in range(a.passes):
            index = visindex.SceneRowGroups(path)
            index.decode_by_blocks = by_blocks
            index.page_kinds = page_kinds
            each = []
            if stages:
                index.stage_times = {}
            torch.cuda.synchronize()
            c0, t0 = time.process_time(), time.perf_counter()
            for s in scenes:
                t1 = time.perf_counter()
                if path_name == "host":
                    present, got = index._scene_bits_host(s, ids, a.points, "cuda")
                else:
                    present, got = index.scene_bits(s, ids, a.points)
                if a.layout == "pandas":
                    torch.cuda.synchronize()
                    each.append(round(1e3 * (time.perf_counter() - t1), 2))
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) / len(scenes))
            cpu.append((time.process_time() - c0) / len(scenes))
            h2d.append(index.decode_stats["h2d_bytes"] // len(scenes))
            st_all.append({k: round(1e3 * v / len(scenes), 3) for k, v in (index.stage_times or {}).items()})
            assert present == ids and np.array_equal(got.cpu().numpy(), want)
            print(f"{path_name}{' staged' if stages else ''}: pass of {len(scenes)} scenes, {1e3 * wall[-1]:.1f} ms per scene", file=sys.stderr, flush=True)
            assert path_name == "host" or index.decode_stats["rows_declined"] == 0
            assert path_name == "host" or a.layout == "pandas" or index.decode_stats["scenes_declined"] == 0
        res = {"scenes_per_pass": len(scenes), "wall_ms": round(1e3 * statistics.median(wall[1:]), 2),
               "process_cpu_ms": round(1e3 * statistics.median(cpu[1:]), 2), "wall_ms_all": [round(1e3 * v, 2) for v in wall],
               "process_cpu_ms_all": [round(1e3 * v, 2) for v in cpu]}
        if path_name != "host":
            res["h2d_bytes"] = int(statistics.median(h2d[1:]))
            res["blocks_per_scene"] = index.decode_stats["blocks"] // len(scenes)
            res["serial_streams_per_scene"] = index.decode_stats["serial_streams"] // len(scenes)
            res["scenes_declined"] = index.decode_stats["scenes_declined"]
            res["dict_pages"], res["v2_pages"] = index.decode_stats["dict_pages"], index.decode_stats["v2_pages"]
        if a.layout == "pandas":
            res["scene_ms_last_pass"] = each
        if stages:
            res["stages_ms"] = {k: round(statistics.median([p[k] for p in st_all[1:]]), 3) for k in st_all[-1]}
            res["stages_ms_all"] = st_all
        return res

    def run_lists(scenes):
        """``scene_lists`` and one ``pick`` of one position per image (what a depth builder asks of a scene it draws every image
        of), per scene; the picks read back."""
        rng = np.random.default_rng(7)
        wall, cpu = [], []
        for _ in range(a.passes):
            index = visindex.SceneRowGroups(path)
            index.page_kinds = "any"
            torch.cuda.synchronize()
            c0, t0 = time.process_time(), time.perf_counter()
            for s in scenes:
                lists = index.scene_lists(s, ids)
                samples = [(i, int(rng.integers(0, n))) for i, n in zip(lists.present, lists.counts.tolist())]
                picked = lists.pick(samples, a.points).cpu()
            wall.append((time.perf_counter() - t0) / len(scenes))
            cpu.append((time.process_time() - c0) / len(scenes))
            assert lists.present == ids and index.decode_stats["rows_declined"] == 0 and index.decode_stats["scenes_declined"] == 0
            assert lists.counts.tolist() == want_counts and picked.tolist() == [want_lists[k][j] for k, (_, j) in enumerate(samples)]
            print(f"lists: pass of {len(scenes)} scenes, {1e3 * wall[-1]:.1f} ms per scene", file=sys.stderr, flush=True)
        return {"scenes_per_pass": len(scenes), "wall_ms": round(1e3 * statistics.median(wall[1:]), 2),
                "process_cpu_ms": round(1e3 * statistics.median(cpu[1:]), 2), "wall_ms_all": [round(1e3 * v, 2) for v in wall],
                "process_cpu_ms_all": [round(1e3 * v, 2) for v in cpu]}

    def run_host_access(scenes):
        """The builders' access with the switch unset, per scene: ``json.loads`` of every image's text, its ``len`` and one element.
        The texts are in memory already (``VisibilityInfoHandler`` holds the whole file as a dict): reading them (``scene_dict``) is
        timed apart."""
        rng = np.random.default_rng(7)
        wall, cpu, read = [], [], []
        index = visindex.SceneRowGroups(path)
        for _ in range(a.passes):
            for s in scenes:
                t0 = time.perf_counter()
                texts = index.scene_dict(s)
                read.append(time.perf_counter() - t0)
                c0, t0 = time.process_time(), time.perf_counter()
                got = []
                for i in ids:
                    seen = json.loads(texts[f"{s}:image_to_points:{i}"])
                    got.append((len(seen), int(seen[int(rng.integers(0, len(seen)))])))
                wall.append(time.perf_counter() - t0)
                cpu.append(time.process_time() - c0)
            assert [n for n, _ in got] == want_counts
            print(f"host access: pass of {len(scenes)} scenes, {1e3 * wall[-1]:.1f} ms per scene", file=sys.stderr, flush=True)
        warm = len(scenes)                                       # the first pass is the warm-up
        return {"scenes_per_pass": len(scenes), "wall_ms": round(1e3 * statistics.median(wall[warm:]), 2),
                "process_cpu_ms": round(1e3 * statistics.median(cpu[warm:]), 2), "scene_dict_read_ms": round(1e3 * statistics.median(read[warm:]), 2),
                "wall_ms_all": [round(1e3 * v, 2) for v in wall]}

    if a.lists:
        # the rows as lists (the depth builders' route) beside scene_bits on the same file in this process, and beside the host access
        want_lists = [np.nonzero(np.unpackbits(row.view(np.uint8), bitorder="little")[:a.points])[0].tolist() for row in want]
        want_counts = [len(v) for v in want_lists]
        for turn in ("first", "second"):                         # bits, lists, bits, lists: drift of the box shows between the turns
            out["paths"][f"scene_bits_{turn}"] = run("device", scene_ids, False, page_kinds="any")
            out["paths"][f"scene_lists_pick_{turn}"] = run_lists(scene_ids)
        out["paths"]["host_access"] = run_host_access(scene_ids[:a.host_scenes])
        bits_ms = statistics.median([out["paths"][f"scene_bits_{t}"]["wall_ms"] for t in ("first", "second")])
        lists_ms = statistics.median([out["paths"][f"scene_lists_pick_{t}"]["wall_ms"] for t in ("first", "second")])
        out["lists_over_bits"] = round(lists_ms / bits_ms, 3)
        out["host_access_over_lists"] = round(out["paths"]["host_access"]["wall_ms"] / lists_ms, 2)
        print(json.dumps(out))
        return
    if not a.device_only:
        out["paths"]["host"] = run("host", scene_ids[:a.host_scenes], False)
    if a.layout == "pandas":
        index = visindex.SceneRowGroups(path)
        index.page_kinds = "any"
        out["row_groups"] = index.file.metadata.num_row_groups
        out["scene_pages"] = []                    # per scene: (kind, compressed, uncompressed, values) of the pages it needs
        for s in scene_ids:
            pages, why = index._plan_pages(sorted(set(index.image_rows(s, ids).values())))
            out["scene_pages"].append(why or [(p.kind, p.compressed, p.uncompressed, p.num_values) for p in pages])
        if not a.device_only:
            out["paths"]["device_plain"] = run("device", scene_ids, False)
        out["paths"]["device_any"] = run("device", scene_ids, False, page_kinds="any")
        out["paths"]["device_any_staged"] = run("device", scene_ids, True, page_kinds="any")
        print(json.dumps(out))
        return
    if a.route != "one-wave":
        out["paths"]["device"] = run("device", scene_ids, False)
        out["paths"]["device_staged"] = run("device", scene_ids, True)
    if a.route != "blocks":
        out["paths"]["device_one_wave"] = run("device", scene_ids, False, by_blocks=False)
        out["paths"]["device_one_wave_staged"] = run("device", scene_ids, True, by_blocks=False)
    if a.device_only:
        print(json.dumps(out))
        return

    # the decode kernel alone: the needed pages of 1 and of 8 scenes, one launch each
    index = visindex.SceneRowGroups(path)
    parts, sizes = [], []
    many = min(8, a.scenes)
    for s in scene_ids[:many]:
        found = index.image_rows(s, ids)
        g = next(iter(found.values()))[0]
        table, page, reason = index.needed_pages(g, [r for _, r in found.values()])
        assert reason is None and table["codec"] == "SNAPPY"
        for pg in np.unique(page):
            pos, comp = int(table["pos"][pg]), int(table["compressed"][pg])
            parts.append(np.frombuffer(table["chunk"][pos:pos + comp], dtype=np.uint8))
            sizes.append((comp, int(table["uncompressed"][pg])))
    per_scene = len(parts) // many
    out["decode_kernel"] = {}
    for label, n in (("one_scene", per_scene), (f"{many}_scenes", len(parts))):
        src = torch.from_numpy(np.concatenate(parts[:n])).cuda()
        comp = torch.tensor([c for c, _ in sizes[:n]], dtype=torch.int64, device="cuda")
        offs = torch.cumsum(comp, 0) - comp
        unc = torch.tensor([u for _, u in sizes[:n]], dtype=torch.int64, device="cuda")
        entry = {"pages": n, "compressed_bytes": int(comp.sum().item()), "uncompressed_bytes": int(unc.sum().item()),
                 "note": "two events around the engine call: the kernels, the prefix sums and one read-back"}
        for route, call in (("blocks", engine.snappy_decompress_blocks_device), ("one_wave", engine.snappy_decompress_device)):
            ms = []
            for _ in range(8):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                status = call(src, offs, comp, unc)[2]
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            assert int(status.abs().sum().item()) == 0
            entry[f"{route}_call_gpu_ms"] = round(statistics.median(ms[1:]), 3)
            entry[f"{route}_call_gpu_ms_all"] = [round(v, 3) for v in ms]
        out["decode_kernel"][label] = entry
    print(json.dumps(out))


if __name__ == "__main__":
    main()
