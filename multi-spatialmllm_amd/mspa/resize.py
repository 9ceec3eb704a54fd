"""Resize image trees to the training shape (the reference's README: "All images should be resized to H*W=1296*968").

The definition is one Pillow line per file::

    Image.open(src).convert("RGB").resize((W, H), resample).save(dst, quality=95)

``resize_tree(backend="pillow")`` runs exactly that on a thread pool.  ``backend="device"`` writes the same bytes from the
MI355X: files are grouped by source shape (header-only reads), decoded by ``ingest.read_color_frames_device`` (baseline JPEG
on the device; its host reader takes what the device declines, a PNG for instance), resampled by
``engine.resize_rgb_device`` (bit-identical to ``Image.resize``) and encoded by ``engine.jpeg_encode_device``
(byte-identical to Pillow's save) in chunks, while a thread pool writes the previous chunk's files.  The decode runs over up to
``DECODE_CHUNK`` files per call (its entropy walk is one lane per image), resize and encode over ``CHUNK`` frames.

What the device backend hands to the Pillow line as a whole, so that the bytes stay the definition's:
  * a shape whose per-axis factor lies outside 1/8 .. 8 (the kernels decline it);
  * a JPEG destination whose source carries a comment, a PNG destination whose source carries an ICC profile or a
    transparency entry (Pillow's save copies those from the opened image).
A destination keeps its source's relative path and extension; one that is not .jpg / .jpeg is resized on the device and saved
by Pillow.  A file that already has the target shape is still decoded and re-encoded, as the Pillow line would; with
``skip_same_shape`` both backends copy its bytes instead.

Under a one-process-per-GPU launch (``shard.context_from_env``) the sorted file list is dealt to the ranks by index; no
collective is needed, every rank writes its own files.
"""
from __future__ import annotations

import os
import shutil
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Tuple

IMAGE_EXTENSIONS = (".jpg", ".jpeg", ".png")
TRAINING_HW = (968, 1296)
DECODE_CHUNK = 1024                         # images per decode call: the entropy decode is one lane per image, so it wants many
CHUNK = 128                                 # images per resize / encode call: bounds the device buffers


def list_images(src_root: str) -> List[str]:
    """Relative paths of the *.jpg / *.jpeg / *.png files under ``src_root``, sorted."""
    found = []
    for base, dirs, names in os.walk(src_root):
        dirs.sort()
        for name in names:
            if name.lower().endswith(IMAGE_EXTENSIONS):
                found.append(os.path.relpath(os.path.join(base, name), src_root))
    return sorted(found)


def pillow_resize_file(src: str, dst: str, hw: Tuple[int, int] = TRAINING_HW, resample="bicubic", quality: int = 95) -> None:
    """The definition, for one file."""
    from PIL import Image
    from .engine import _resize_filter
    os.makedirs(os.path.dirname(dst) or ".", exist_ok=True)
    with Image.open(src) as im:
        im.convert("RGB").resize((int(hw[1]), int(hw[0])), _resize_filter(resample)).save(dst, quality=int(quality))


def _header(path: str):
    """(h, w, carries metadata that Pillow's save would copy into a file of this extension): a header-only read."""
    from PIL import Image
    with Image.open(path) as im:
        w, h = im.size
        if path.lower().endswith(".png"):
            sticky = "icc_profile" in im.info or "transparency" in im.info
        else:
            sticky = im.info.get("comment") is not None
    return h, w, sticky


def _is_jpeg(path: str) -> bool:
    return path.lower().endswith((".jpg", ".jpeg"))


def resize_tree(src_root: str, dst_root: str, hw: Tuple[int, int] = TRAINING_HW, resample="bicubic", quality: int = 95,
                device="cuda", n_threads: Optional[int] = None, backend: str = "device", skip_same_shape: bool = False,
                ctx=None) -> Dict[str, int]:
    """Resize every image under ``src_root`` to ``hw`` = (H, W) into the same relative path under ``dst_root`` (see the module
    text).  Returns this rank's counts: ``files``; ``copied`` (``skip_same_shape``); ``device_decoded`` / ``host_decoded``;
    ``device_resized`` / ``host_resized``; ``device_encoded`` / ``host_encoded``.  A file the Pillow line handled as a whole
    counts as host decoded, resized and encoded."""
    from . import hostinfo
    if backend not in ("device", "pillow"):
        raise ValueError("backend: 'device' or 'pillow'")
    H, W = int(hw[0]), int(hw[1])
    if H < 1 or W < 1:
        raise ValueError("hw: positive sizes")
    n_threads = int(n_threads) if n_threads else max(1, hostinfo.effective_cpus())
    files = list_images(src_root)
    if ctx is None and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        from . import shard
        ctx = shard.context_from_env()
    if ctx is not None:
        files = files[ctx.rank::ctx.world]
        if getattr(ctx, "device", None) is not None and ctx.device.type == "cuda":
            device = ctx.device
    counts = dict.fromkeys(("files", "copied", "device_decoded", "host_decoded", "device_resized", "host_resized",
                            "device_encoded", "host_encoded"), 0)
    counts["files"] = len(files)
    if not files:
        return counts

    def src_of(rel):
        return os.path.join(src_root, rel)

    def dst_of(rel):
        return os.path.join(dst_root, rel)

    def whole_file(rel):
        pillow_resize_file(src_of(rel), dst_of(rel), (H, W), resample, quality)

    def copy_file(rel):
        os.makedirs(os.path.dirname(dst_of(rel)) or ".", exist_ok=True)
        shutil.copy(src_of(rel), dst_of(rel))

    with ThreadPoolExecutor(max_workers=n_threads) as pool:
        headers = list(pool.map(lambda rel: _header(src_of(rel)), files))
        same = [skip_same_shape and (h, w) == (H, W) for h, w, _ in headers]
        list(pool.map(copy_file, [rel for rel, s in zip(files, same) if s]))
        counts["copied"] = sum(same)
        todo = [(rel, hd) for rel, hd, s in zip(files, headers, same) if not s]
        if backend == "pillow":
            list(pool.map(whole_file, [rel for rel, _ in todo]))
            counts["host_decoded"] = counts["host_resized"] = counts["host_encoded"] = len(todo)
            return counts
        _device_backend(todo, src_of, dst_of, whole_file, (H, W), resample, quality, device, n_threads, pool, counts)
    return counts


def _device_backend(todo, src_of, dst_of, whole_file, hw, resample, quality, device, n_threads, pool, counts):
    import numpy as np
    import torch
    from PIL import Image
    from . import _lib, engine
    from .ingest import _pillow_rgb, read_color_frames_device

    def count_whole(rels):
        counts["host_decoded"] += len(rels)
        counts["host_resized"] += len(rels)
        counts["host_encoded"] += len(rels)
        return [pool.submit(whole_file, rel) for rel in rels]

    def write(dst, data):
        os.makedirs(os.path.dirname(dst) or ".", exist_ok=True)
        with open(dst, "wb") as f:
            f.write(memoryview(data))

    def save(dst, rgb):
        os.makedirs(os.path.dirname(dst) or ".", exist_ok=True)
        Image.fromarray(rgb).save(dst, quality=int(quality))

    pending = count_whole([rel for rel, (_, _, sticky) in todo if sticky])
    by_shape: Dict[Tuple[int, int], List[str]] = {}
    for rel, (h, w, sticky) in todo:
        if not sticky:
            by_shape.setdefault((h, w), []).append(rel)
    host_reads = [0]

    def host_reader(path):
        host_reads[0] += 1
        return _pillow_rgb(path)

    for shape, rels in by_shape.items():
        declined = False
        for d in range(0, len(rels), DECODE_CHUNK):
            batch = rels[d:d + DECODE_CHUNK]
            reads_before = host_reads[0]
            decoded = read_color_frames_device([src_of(r) for r in batch], device=device, n_threads=min(16, n_threads),
                                               general_reader=host_reader)
            for c in range(0, len(batch), CHUNK):
                chunk = batch[c:c + CHUNK]
                try:
                    resized = engine.resize_rgb_device(decoded[c:c + CHUNK], hw, resample, fallback=False)
                except _lib.MspaError as e:
                    if e.code != _lib.MSPA_EUNSUPPORTED:
                        raise
                    host_reads[0] = reads_before        # the shape is declined: the Pillow line takes all of its files
                    pending += count_whole(rels)
                    declined = True
                    break
                counts["device_resized"] += len(chunk)
                jpegs = [i for i, r in enumerate(chunk) if _is_jpeg(r)]
                others = [i for i, r in enumerate(chunk) if not _is_jpeg(r)]
                if jpegs:
                    pick = resized if len(jpegs) == len(chunk) else resized[torch.tensor(jpegs, device=resized.device)]
                    out, nbytes = engine.jpeg_encode_device(pick.contiguous(), quality=int(quality), subsampling="4:2:0")
                    nb = nbytes.cpu().numpy()
                    host = out[:, :int(nb.max())].cpu().numpy()
                    pending += [pool.submit(write, dst_of(chunk[i]), host[k, :int(nb[k])]) for k, i in enumerate(jpegs)]
                    counts["device_encoded"] += len(jpegs)
                    del out, pick
                if others:
                    rgb = resized[torch.tensor(others, device=resized.device)].cpu().numpy()
                    pending += [pool.submit(save, dst_of(chunk[i]), np.ascontiguousarray(rgb[k])) for k, i in enumerate(others)]
                    counts["host_encoded"] += len(others)
                del resized
            del decoded
            if declined:                                # (the first resize of a shape declines or none does)
                break
    decoded = counts["device_resized"]
    counts["host_decoded"] += min(host_reads[0], decoded)
    counts["device_decoded"] += decoded - min(host_reads[0], decoded)
    for f in pending:
        f.result()                                      # the first failed write raises here


def _parse_size(text: str) -> Tuple[int, int]:
    w, _, h = text.lower().partition("x")
    return int(h), int(w)


def main(argv=None) -> int:
    import argparse
    import json
    ap = argparse.ArgumentParser(prog="python -m mspa.resize", description=__doc__.split("\n\n")[0])
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("--size", default="1296x968", help="target WIDTHxHEIGHT (default 1296x968)")
    ap.add_argument("--resample", default="bicubic", choices=("bicubic", "bilinear"))
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--backend", default="device", choices=("device", "pillow"))
    ap.add_argument("--skip-same-shape", action="store_true", help="copy a file that already has the target shape instead of re-encoding it")
    ap.add_argument("--threads", type=int, default=None)
    args = ap.parse_args(argv)
    counts = resize_tree(args.src, args.dst, _parse_size(args.size), args.resample, args.quality, n_threads=args.threads,
                         backend=args.backend, skip_same_shape=args.skip_same_shape)
    print(json.dumps(counts))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
