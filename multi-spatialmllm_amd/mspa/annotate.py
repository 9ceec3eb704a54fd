"""Annotated images of the "dot" task variants: filled discs and letter labels on a copy of a colour frame.

Reference: the cv2.circle / cv2.putText calls of depth_estimation_dot_engine.py:158-168, depth_comparison_dot_engine.py
:332-346, visual_correspondence_qa_engine_dot_2_multichoice.py:362-397, single_object_movement_engine_dot.py:328-339.
This is file I/O around the geometry path, not part of it: the marks (pixel, radius, colour, label) are computed by the
heads; drawing and JPEG encoding run on the host.  The filled disc is OpenCV's own integer rasteriser restated
(``filled_circle_spans``: cv2.circle(img, c, r, color, -1) with the default LINE_8 and shift 0 takes the midpoint loop of
modules/imgproc/src/drawing.cpp ``Circle(..., fill=true)``, no anti-aliasing), so the disc's pixels are the ones OpenCV
sets; the Hershey-font label and the JPEG bytes are Pillow's and are NOT claimed identical (cv2 is not installable here:
nothing could pin them) -- the records never depend on the pixels.
"""
from __future__ import annotations

import dataclasses
import os
import shutil
from typing import List, Optional, Sequence, Tuple


@dataclasses.dataclass
class Mark:
    x: int
    y: int
    radius: int
    color: Tuple[int, int, int]              # as drawn by upstream: a BGR triple handed to cv2 on a BGR image
    label: Optional[str] = None
    label_offset: Tuple[int, int] = (15, 0)


def generate_distinct_colors(n: int, rng, max_retries: int = 10) -> List[Tuple[int, int, int]]:
    """Up to ``max_retries`` random colours kept when far (L1 > 300) from those already kept, topped up from five fixed
    ones (DE_D:23-35 and its copies in the other dot scripts): same draws from ``rng`` in the same order."""
    colors: List[Tuple[int, int, int]] = []
    retries = 0
    while len(colors) < n and retries < max_retries:
        color = (rng.randint(0, 255), rng.randint(0, 255), rng.randint(0, 255))
        if all(sum(abs(a - b) for a, b in zip(color, other)) > 300 for other in colors):
            colors.append(color)
        retries += 1
    if len(colors) < n:
        fixed = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (0, 0, 0), (255, 255, 255)]
        colors += rng.sample(fixed, n - len(colors))
    return colors


def filled_circle_spans(cx: int, cy: int, radius: int, width: int, height: int) -> List[Tuple[int, int, int]]:
    """Horizontal spans (y, x_first, x_last), inclusive and clipped to the image, that OpenCV's non-anti-aliased filled circle
    sets -- the integer midpoint loop of ``Circle()`` in modules/imgproc/src/drawing.cpp (the path cv2.circle takes for
    thickness < 0, LINE_8, shift 0): error term ``err``, odd increments ``plus`` / ``minus``, a row pair at +-dy with
    half-width dx and a row pair at +-dx with half-width dy per step.  Spans may repeat a row (as upstream's do)."""
    spans: List[Tuple[int, int, int]] = []

    def hline(y, x0, x1):
        if 0 <= y < height:
            x0, x1 = max(x0, 0), min(x1, width - 1)
            if x0 <= x1:
                spans.append((y, x0, x1))

    err, dx, dy, plus, minus = 0, int(radius), 0, 1, (int(radius) << 1) - 1
    while dx >= dy:
        hline(cy - dy, cx - dx, cx + dx)
        hline(cy + dy, cx - dx, cx + dx)
        hline(cy - dx, cx - dy, cx + dy)
        hline(cy + dx, cx - dy, cx + dy)
        dy += 1
        err += plus
        plus += 2
        if err > 0:                         # mask = (err <= 0) - 1: all ones exactly when err > 0
            err -= minus
            dx -= 1
            minus -= 2
    return spans


def draw_filled_circle(image, center: Tuple[int, int], radius: int, color) -> None:
    """cv2.circle(image, center, radius, color, -1) on an [H, W, C] array, in place."""
    h, w = image.shape[:2]
    for y, x0, x1 in filled_circle_spans(int(center[0]), int(center[1]), int(radius), w, h):
        image[y, x0:x1 + 1] = color


class PillowAnnotator:
    """Draw marks on ``src`` and save to ``dst`` (JPEG).  Colours arrive in upstream's channel order (BGR) and are
    flipped for Pillow's RGB canvas, so the saved picture shows what OpenCV would have shown.  ``output_size`` = (H, W): the
    painted picture is resized (``Image.resize``, bicubic) before it is saved, e.g. to the training shape (968, 1296)."""

    def __init__(self, output_size: Optional[Tuple[int, int]] = None):
        self.output_size = (int(output_size[0]), int(output_size[1])) if output_size else None

    def annotate(self, src: str, dst: str, marks: Sequence[Mark]):
        from PIL import Image, ImageDraw
        os.makedirs(os.path.dirname(dst) or ".", exist_ok=True)
        with Image.open(src) as im:
            im = im.convert("RGB")
        import numpy as np
        canvas = np.array(im)                         # [H, W, 3] RGB, writable copy
        for m in marks:                               # discs first, pixel for pixel as OpenCV rasterises them
            draw_filled_circle(canvas, (m.x, m.y), m.radius, (m.color[2], m.color[1], m.color[0]))
        im = Image.fromarray(canvas)
        draw = ImageDraw.Draw(im)
        for m in marks:
            if m.label:
                rgb = (m.color[2], m.color[1], m.color[0])
                draw.text((m.x + m.label_offset[0], m.y + m.label_offset[1] - 22), m.label, fill=rgb, font=self._font())
        if self.output_size:
            im = im.resize((self.output_size[1], self.output_size[0]))
        im.save(dst, quality=95)

    def copy(self, src: str, dst: str):
        os.makedirs(os.path.dirname(dst) or ".", exist_ok=True)
        shutil.copy(src, dst)

    _cached_font = None

    @classmethod
    def _font(cls):
        if cls._cached_font is None:
            from PIL import ImageFont
            try:
                cls._cached_font = ImageFont.load_default(size=28)
            except TypeError:
                cls._cached_font = ImageFont.load_default()
        return cls._cached_font


class RecordingAnnotator:
    """Collects the jobs instead of touching images (tests, dry runs)."""

    def __init__(self):
        self.jobs: List[tuple] = []

    def annotate(self, src, dst, marks):
        self.jobs.append(("annotate", src, dst, [dataclasses.astuple(m) for m in marks]))

    def copy(self, src, dst):
        self.jobs.append(("copy", src, dst))


def default_annotator():
    """The heads' annotator: ``PillowAnnotator()``, or ``DeviceAnnotator()`` when the environment sets MSPA_ANNOTATE=device."""
    if os.environ.get("MSPA_ANNOTATE", "") == "device":
        return DeviceAnnotator()
    return PillowAnnotator()


def flush_annotator(annotator) -> None:
    """Make every file an annotator was asked for exist with its final bytes (a no-op for annotators without ``flush``)."""
    flush = getattr(annotator, "flush", None)
    if flush is not None:
        flush()


def pack_spans(spans_per_image) -> "np.ndarray":
    """[(image, [(y, x0, x1, 0xRRGGBB), ...]), ...] in paint order -> int32 [S, 5] (image, y, x0, x1, rgb) grouped by (image, y),
    paint order kept inside a group: the record layout of mspa_draw_spans_device."""
    import numpy as np
    rows = [(i, y, x0, x1, rgb) for i, spans in spans_per_image for (y, x0, x1, rgb) in spans]
    if not rows:
        return np.zeros((0, 5), np.int32)
    a = np.array(rows, dtype=np.int64)
    order = np.lexsort((a[:, 1], a[:, 0]))              # stable: paint order survives inside an (image, y) group
    return np.ascontiguousarray(a[order].astype(np.int32))


def rgb24(color_bgr) -> int:
    """A BGR mark colour as 0xRRGGBB."""
    return (int(color_bgr[2]) << 16) | (int(color_bgr[1]) << 8) | int(color_bgr[0])


class LabelMasks:
    """Pillow's glyph masks of the label texts, rendered once per text: drawing a text with fill 255 on a zero "L" canvas
    leaves exactly the 8-bit mask ``ImageDraw.text`` blends with the ink, and with integer coordinates mask and offset depend
    on the text alone.  ``get(text)`` -> (mask [h, w] uint8, dx, dy): the mask's top-left corner is at (x + dx, y + dy) for a
    text drawn at (x, y)."""

    def __init__(self, font=None):
        self.font = font
        self._cache = {}

    def get(self, text: str):
        hit = self._cache.get(text)
        if hit is not None:
            return hit
        import numpy as np
        from PIL import Image, ImageDraw
        font = self.font if self.font is not None else PillowAnnotator._font()
        l, t, r, b = ImageDraw.Draw(Image.new("L", (1, 1))).textbbox((0, 0), text, font=font)
        ox, oy = 4 - min(l, 0), 4 - min(t, 0)
        canvas = Image.new("L", (max(r, 0) + ox + 4, max(b, 0) + oy + 4), 0)
        ImageDraw.Draw(canvas).text((ox, oy), text, fill=255, font=font)
        a = np.asarray(canvas)
        ys, xs = np.nonzero(a)
        if len(ys) == 0:
            hit = (np.zeros((0, 0), np.uint8), 0, 0)
        else:
            y0, y1, x0, x1 = ys.min(), ys.max() + 1, xs.min(), xs.max() + 1
            hit = (np.ascontiguousarray(a[y0:y1, x0:x1]), int(x0 - ox), int(y0 - oy))
        self._cache[text] = hit
        return hit


def blend_mask_numpy(image, mask, x: int, y: int, rgb) -> None:
    """Pillow's ink-through-mask blend (``ImageDraw.text`` on an RGB image), in place and clipped at the borders:
    t = ink * m + px * (255 - m) + 128, px' = ((t >> 8) + t) >> 8 -- the NumPy statement of mspa_blend_masks_device."""
    import numpy as np
    h, w = image.shape[:2]
    mh, mw = mask.shape
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + mw, w), min(y + mh, h)
    if x0 >= x1 or y0 >= y1:
        return
    m = mask[y0 - y:y1 - y, x0 - x:x1 - x].astype(np.int32)[..., None]
    px = image[y0:y1, x0:x1].astype(np.int32)
    t = np.asarray(rgb, dtype=np.int32)[None, None] * m + px * (255 - m) + 128
    image[y0:y1, x0:x1] = (((t >> 8) + t) >> 8).astype(np.uint8)


class DeviceAnnotator:
    """``PillowAnnotator`` on the MI355X, byte for byte: the same ``annotate(src, dst, marks)`` / ``copy(src, dst)`` calls,
    queued and run in batches.  A batch decodes each distinct source once (``ingest.read_color_frames_device``; Pillow for
    what the device declines) and keeps a bounded LRU of decoded frames across batches, paints the discs
    (mspa_draw_spans_device) and then the labels (mspa_blend_masks_device) on per-job copies, encodes them at quality 95 4:2:0
    (mspa_jpeg_encode_device) and writes the files from a thread pool.  A later job for the same ``dst`` replaces an earlier
    pending one; a destination that is not .jpg / .jpeg goes through ``PillowAnnotator`` at once.  Writes and reads of one file
    keep their call order: a job whose source is a pending destination, and a job (or host write) whose destination is the
    source of a pending job, first flush the queue, and a destination leaves the frame cache.  Paths are compared as given.
    ``flush()`` finishes every pending job (errors raise); ``pending(dst)`` says whether ``dst`` is queued.  A context manager
    flushes on exit.  Device memory: one batch's distinct frames, their per-job copies in chunks of ``ENCODE_CHUNK``, and
    ``cache_frames`` frames of their own (copied out of the decode batch, so a cached frame never keeps a batch alive).
    ``output_size`` = (H, W): painted frames are resized (``engine.resize_rgb_device``, bicubic, bit-identical to Pillow's
    ``Image.resize``) before the encode, as ``PillowAnnotator(output_size)`` does; copies stay copies."""

    ENCODE_CHUNK = 128                      # images per encode call: bounds the device output buffer and workspace

    def __init__(self, batch_size: int = 1024, cache_frames: int = 256, device="cuda", n_threads: Optional[int] = None,
                 output_size: Optional[Tuple[int, int]] = None):
        from collections import OrderedDict
        from . import hostinfo
        self.batch_size = max(1, int(batch_size))
        self.cache_frames = max(0, int(cache_frames))
        self.device = device
        self.n_threads = int(n_threads) if n_threads else max(1, hostinfo.effective_cpus())
        self._jobs = OrderedDict()          # dst -> ("annotate", src, marks) | ("copy", src)
        self._reads = {}                    # src -> number of pending jobs that read it
        self._frames = OrderedDict()        # src -> [H, W, 3] uint8 device tensor (LRU)
        self._labels = LabelMasks()
        self.output_size = (int(output_size[0]), int(output_size[1])) if output_size else None
        self._host = PillowAnnotator(self.output_size)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if exc[0] is None:
            self.flush()
        return False

    def pending(self, dst: str) -> bool:
        return dst in self._jobs

    def _order(self, src, dst):
        """Keep the call order of reads and writes of one file before ``dst`` is written from ``src``."""
        if src in self._jobs or dst in self._reads:    # reads a pending output / overwrites a pending job's source
            self.flush()
        self._frames.pop(dst, None)                    # the cached decode of an overwritten file is stale

    def _queue(self, dst, job):
        self._order(job[1], dst)
        old = self._jobs.pop(dst, None)
        if old is not None:
            self._unread(old[1])
        self._jobs[dst] = job
        self._reads[job[1]] = self._reads.get(job[1], 0) + 1
        if len(self._jobs) >= self.batch_size:
            self.flush()

    def _unread(self, src):
        n = self._reads.pop(src) - 1
        if n:
            self._reads[src] = n

    def annotate(self, src: str, dst: str, marks: Sequence[Mark]):
        if not dst.lower().endswith((".jpg", ".jpeg")):
            self._order(src, dst)
            self._host.annotate(src, dst, marks)
            return
        self._queue(dst, ("annotate", src, list(marks)))

    def copy(self, src: str, dst: str):
        self._queue(dst, ("copy", src))

    def flush(self):
        jobs, self._jobs = list(self._jobs.items()), type(self._jobs)()
        self._reads = {}
        for i in range(0, len(jobs), self.batch_size):
            self._run(jobs[i:i + self.batch_size])

    # -- one batch --------------------------------------------------------------------------------------------------------
    def _frames_for(self, srcs):
        """Device frames of the distinct ``srcs``: cached ones reused, the others decoded in one call per image size."""
        from PIL import Image
        from .ingest import read_color_frames_device
        got = {}
        missing = []
        for s in srcs:
            if s in self._frames:
                self._frames.move_to_end(s)
                got[s] = self._frames[s]
            else:
                missing.append(s)
        by_size = {}
        for s in missing:
            with Image.open(s) as im:
                by_size.setdefault(im.size, []).append(s)
        for group in by_size.values():
            frames = read_color_frames_device(group, device=self.device, n_threads=min(16, self.n_threads))
            for s, f in zip(group, frames):
                if self.cache_frames:
                    f = f.clone()                      # its own storage: the decode batch is freed after this loop
                    self._frames[s] = f
                    self._frames.move_to_end(s)
                got[s] = f
            del frames
        while len(self._frames) > self.cache_frames:
            self._frames.popitem(last=False)
        return got

    def _run(self, jobs):
        import numpy as np
        import torch
        from concurrent.futures import ThreadPoolExecutor
        from . import engine
        draws = [(dst, job) for dst, job in jobs if job[0] == "annotate"]
        frames = self._frames_for(list(dict.fromkeys(job[1] for _, job in draws)))
        by_shape = {}
        for dst, job in draws:
            by_shape.setdefault(tuple(frames[job[1]].shape), []).append((dst, job))
        outputs = []                        # (dst, bytes-like)
        for (H, W, _), group in by_shape.items():
            for c in range(0, len(group), self.ENCODE_CHUNK):
                chunk = group[c:c + self.ENCODE_CHUNK]
                canvas = torch.stack([frames[job[1]] for _, job in chunk]).contiguous()
                spans, labels, masks, moff = [], [], [], 0
                for i, (_, job) in enumerate(chunk):
                    spans.append((i, [(y, x0, x1, rgb24(m.color)) for m in job[2]
                                      for (y, x0, x1) in filled_circle_spans(int(m.x), int(m.y), int(m.radius), W, H)]))
                    for m in job[2]:
                        if m.label:
                            mask, dx, dy = self._labels.get(m.label)
                            if mask.size == 0:
                                continue
                            labels.append((i, int(m.x + m.label_offset[0]) + dx, int(m.y + m.label_offset[1] - 22) + dy,
                                           mask.shape[1], mask.shape[0], rgb24(m.color), moff, 0))
                            masks.append(mask.ravel())
                            moff += mask.size
                dev = canvas.device
                packed = pack_spans(spans)
                if len(packed):
                    engine.draw_spans_device(canvas, torch.from_numpy(packed).to(dev))
                if labels:
                    engine.blend_masks_device(canvas, torch.from_numpy(np.array(labels, dtype=np.int64)).to(dev),
                                              torch.from_numpy(np.concatenate(masks)).to(dev))
                if self.output_size:
                    canvas = engine.resize_rgb_device(canvas, self.output_size)
                out, nbytes = engine.jpeg_encode_device(canvas, quality=95, subsampling="4:2:0")
                nb = nbytes.cpu().numpy()
                host = out[:, :int(nb.max())].cpu().numpy()
                outputs += [(dst, host[i, :int(nb[i])]) for i, (dst, _) in enumerate(chunk)]
                del canvas, out

        def write(item):
            dst, data = item
            os.makedirs(os.path.dirname(dst) or ".", exist_ok=True)
            if isinstance(data, str):
                shutil.copy(data, dst)
            else:
                with open(dst, "wb") as f:
                    f.write(memoryview(data))
        outputs += [(dst, job[1]) for dst, job in jobs if job[0] == "copy"]
        with ThreadPoolExecutor(max_workers=self.n_threads) as pool:
            list(pool.map(write, outputs))          # list(): the first exception raises here
