"""Run an op with a watched strip of memory on both sides of every buffer it touches.

tests/poison_util.py asks whether a result depends on bytes nothing wrote INSIDE an op's allocations.  This module asks the
complementary questions: does the op write OUTSIDE a buffer (one element, one row, one 32-bit word past the end of an output or a
workspace; a back-reference or a reflected index before the start; ``status[n]`` of a status array of n), does it write into an
input, and does its result depend on the bytes that happen to lie beyond an input's last byte (a dword or int4 load whose tail is
not masked).  On the GPU such an access lands in the caching allocator's next block or in its rounding slack, and nothing fails.

``fenced_allocations(mode)`` replaces every factory the package allocates with (``FACTORIES``) for its duration.  A result that
lives on a watched device and has elements is moved into one flat uint8 buffer

    [ front fence | payload | back fence ]

and handed on as a view of the payload with the result's dtype, shape and strides.  The payload starts ``width`` bytes -- a
multiple of 512, the alignment torch's allocator gives anyway -- behind the buffer's base, so an alignment check sees what it sees
without the fences (tests/skew_util.py asks ``rehome`` for a ``skew`` on top of that, on purpose); it ends at its exact last byte,
and the back fence begins at the next one.  ``width`` is the payload size rounded up to 512, at least 4 KiB and at most 1 MiB: an error of one row, one tile or one segment still lands in it.  Host tensors,
pinned ones included, pass through untouched, and so do tensors of no elements.

The fences hold poison_util's fill, viewed in the payload's dtype, mode "a" or "b".  Those values are small on purpose: a stray
read that is used as an index or a count stays inside a small case's buffers and shows as a wrong number, never as a GPU fault.
The int32 fill is 1 / 2, so a stray store of 1 hides under "a" and shows under "b": run both.

``fenced_copy(inputs, mode)`` re-homes the device tensors of a nesting of dicts, lists and tuples between fences of the same kind.

Nothing here reads or writes outside an allocation: the fences are the harness's own memory.
"""
from __future__ import annotations

import contextlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from poison_util import fill_poison, poison_value  # noqa: E402

MODES = ("a", "b")
ALIGN = 512
MIN_FENCE, MAX_FENCE = 4 << 10, 1 << 20

# (owner, name): every factory mspa/*.py allocates with
FACTORIES = tuple((torch, n) for n in ("empty", "empty_like", "zeros", "zeros_like", "full", "full_like", "ones")) + \
    tuple((torch.Tensor, n) for n in ("new_empty", "new_zeros"))

_HERE = os.path.abspath(__file__)
_ROOT = os.path.dirname(os.path.dirname(_HERE))
PACKAGE_DIR = os.path.join(_ROOT, "multi-spatialmllm_amd") + os.sep
_REAL_EMPTY = torch.empty                                # (the module is imported outside any patch)
HARNESS = {_HERE}                                        # files whose frames are no call site (tests/skew_util.py adds itself)


def fence_width(payload_bytes: int) -> int:
    """Bytes of fence on each side of a payload: its size rounded up to 512, at least 4 KiB, at most 1 MiB."""
    return min(max((int(payload_bytes) + ALIGN - 1) // ALIGN * ALIGN, MIN_FENCE), MAX_FENCE)


def call_site() -> str:
    """'file:line function' of the first stack frame inside the package; without one (a case's own allocation, a test), of the first
    frame outside this module."""
    f = sys._getframe(1)
    outside = None
    while f is not None:
        path = os.path.abspath(f.f_code.co_filename)
        if path.startswith(PACKAGE_DIR):
            return f"{os.path.relpath(path, _ROOT)}:{f.f_lineno} {f.f_code.co_name}"
        if outside is None and path not in HARNESS and "contextlib" not in path:
            outside = f"{os.path.basename(path)}:{f.f_lineno} {f.f_code.co_name}"
        f = f.f_back
    return outside or "?"


def _span(t: torch.Tensor) -> int:
    """Elements of storage from ``t``'s first element to its last (strides are non-negative in torch)."""
    return 1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride()))


class Fences:
    """The fenced buffers of one context, kept alive, each with the site that allocated it."""

    def __init__(self, mode: str):
        if mode not in MODES:
            raise ValueError(f"fence mode {mode!r}: choose from {MODES}")
        poison_value(torch.int32, mode)
        self.mode = mode
        self.records = []                                # (site, dtype, shape, flat buffer, width, payload bytes)
        self.skews = []                                  # per record: the bytes its payload starts behind ``width`` (tests/skew_util.py)
        self.empty_sites = []                            # sites of the zero-length tensors that passed through: the early returns taken
        self._expected = {}

    def __len__(self):
        return len(self.records)

    def rehome(self, t: torch.Tensor, site: str, skew: int = 0) -> torch.Tensor:
        """An equal tensor (dtype, shape, strides, and every byte of the storage range ``t`` spans) between two fences.  ``skew``
        (bytes, a multiple of the element size) moves the payload that far behind its 512-aligned place: the front fence grows by
        it, the payload still ends at its exact last byte and the back fence begins at the next one."""
        span, size = _span(t), t.element_size()
        if skew < 0 or skew % size:
            raise ValueError(f"skew {skew}: a non-negative multiple of the element size {size}")
        nbytes = span * size
        width = fence_width(nbytes)
        front = width + skew
        buf = _REAL_EMPTY((front + nbytes + width,), dtype=torch.uint8, device=t.device)
        fill_poison(buf[:front].view(t.dtype), self.mode)
        fill_poison(buf[front + nbytes:].view(t.dtype), self.mode)
        payload = buf[front:front + nbytes].view(t.dtype)
        payload.copy_(t.detach().as_strided((span,), (1,)))
        self.records.append((site, t.dtype, tuple(t.shape), buf, width, nbytes))
        self.skews.append(skew)
        return payload.as_strided(t.shape, t.stride())

    def _fill(self, dtype, width):
        key = (dtype, width)
        if key not in self._expected:
            self._expected[key] = fill_poison(_REAL_EMPTY((width,), dtype=torch.uint8).view(dtype), self.mode).view(torch.uint8).numpy()
        return self._expected[key]

    def check_fences(self):
        """Synchronise, then compare every fence with its fill -> [(call site, dtype, shape, "before" | "after", byte distance
        from the payload of the nearest damaged byte, bytes damaged)], empty when no fence was touched."""
        if any(r[3].is_cuda for r in self.records):
            torch.cuda.synchronize()
        found = []
        for (site, dtype, shape, buf, back, nbytes), skew in zip(self.records, self.skews):
            for side, fence in (("before", buf[:back + skew]), ("after", buf[back + skew + nbytes:])):
                width = fence.numel()
                want = self._fill(dtype, width)
                if fence.is_cuda:                        # compare where the bytes are; only a damaged fence comes to the host
                    key = (dtype, width, fence.device)
                    if key not in self._expected:
                        self._expected[key] = torch.from_numpy(want).to(fence.device)
                    if torch.equal(fence, self._expected[key]):
                        continue
                bad = np.nonzero(fence.cpu().numpy() != want)[0]
                if len(bad):
                    nearest = int(bad[0]) if side == "after" else width - 1 - int(bad[-1])
                    found.append((site, dtype, shape, side, nearest, int(len(bad))))
        return found


@contextlib.contextmanager
def fenced_allocations(mode: str, devices=("cuda",)):
    """Every factory of ``FACTORIES`` returns its result between two fences, where that result lives on one of ``devices`` and has
    elements; until the block ends (also when it raises).  Yields the ``Fences`` of the block: ``check_fences()``, ``len()``."""
    fences = Fences(mode)
    devices = tuple(devices)
    saved = [(owner, name, name in vars(owner), getattr(owner, name)) for owner, name in FACTORIES]

    def wrap(real):
        def factory(*args, **kwargs):
            t = real(*args, **kwargs)
            if not isinstance(t, torch.Tensor) or t.device.type not in devices:
                return t
            if t.numel() == 0:
                fences.empty_sites.append(call_site())
                return t
            return fences.rehome(t, call_site())
        factory.__name__ = getattr(real, "__name__", "factory")
        return factory

    for owner, name, _own, real in saved:
        setattr(owner, name, wrap(real))
    try:
        yield fences
    finally:
        for owner, name, own, real in saved:
            if own:
                setattr(owner, name, real)
            else:
                delattr(owner, name)                     # the inherited method shows through again


def _walk(x, path, visit):
    if isinstance(x, dict):
        return {k: _walk(v, f"{path}/{k}" if path else str(k), visit) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        items = [_walk(v, f"{path}/{i}" if path else str(i), visit) for i, v in enumerate(x)]
        return type(x)(*items) if hasattr(x, "_fields") else type(x)(items)          # a namedtuple takes its fields one by one
    return visit(path, x)


def _span_bytes(t: torch.Tensor) -> np.ndarray:
    return t.detach().as_strided((_span(t),), (1,)).contiguous().view(torch.uint8).cpu().numpy().copy()


class FencedInputs(Fences):
    """``Fences`` of re-homed inputs, with the bytes each held when it was re-homed."""

    def __init__(self, mode):
        super().__init__(mode)
        self.tensors = {}                                # path -> the re-homed tensor
        self.snapshot = {}                               # path -> uint8 array: the storage range it spans

    def changed_inputs(self, writes=()):
        """Paths of re-homed inputs whose bytes differ from the snapshot -> [(path, first differing byte, bytes changed)]; a path
        listed in ``writes`` (or below one) is not compared."""
        writes = tuple(writes)
        unknown = [w for w in writes if not any(p == w or p.startswith(w + "/") for p in self.tensors)]
        if unknown:
            raise KeyError(f"writes names no re-homed input: {unknown} (has {sorted(self.tensors)})")
        found = []
        for path, t in self.tensors.items():
            if any(path == w or path.startswith(w + "/") for w in writes):
                continue
            bad = np.nonzero(_span_bytes(t) != self.snapshot[path])[0]
            if len(bad):
                found.append((path, int(bad[0]), int(len(bad))))
        return found


def fenced_copy(inputs, mode: str, devices=("cuda",)):
    """``inputs`` with every tensor on one of ``devices`` (and with elements) replaced by an equal one whose storage range sits
    between fences: shape, dtype and strides kept.  The same tensor object met twice is re-homed once.  Everything else is passed
    through.  -> (the copy, the ``FencedInputs`` -- ``check_fences()``, ``changed_inputs(writes)`` --, its snapshot: path -> the
    bytes of the storage range that input spans, as re-homed)."""
    handle = FencedInputs(mode)
    devices = tuple(devices)
    memo = {}

    def visit(path, x):
        if not isinstance(x, torch.Tensor) or x.device.type not in devices or x.numel() == 0:
            return x
        if id(x) not in memo:
            memo[id(x)] = (handle.rehome(x, f"input {path}"), x)         # (x kept: its id stays its own)
        t = memo[id(x)][0]
        handle.tensors[path] = t
        handle.snapshot[path] = _span_bytes(t)
        return t

    return _walk(inputs, "", visit), handle, handle.snapshot
