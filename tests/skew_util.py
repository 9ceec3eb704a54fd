"""Run an op with every buffer its CALLER owns at the least alignment the documents allow.

tests/fence_util.py hands every kernel a payload whose first byte is a multiple of 512, and a case's own inputs come straight
from torch's allocator, which aligns as generously.  The public contract is looser: ``engine._check`` passes any contiguous device
tensor of the right dtype and shape, and a view such as ``slot[1:1 + n]`` is aligned to its element size and to nothing else.
The kernels do look at the absolute address -- words loaded from an address rounded down, a wide store behind an alignment test,
a whole route chosen by ``pointer & 15`` -- and each such place is a second code path that runs as soon as a caller passes a view.

This module is fence_util with one more number, the ``skew`` of ``Fences.rehome``: the payload starts ``width + skew`` bytes behind
the 512-aligned base and still ends at its exact last byte, between the same two fences.  Two modes (``MODES``), which are the
fences' poison modes as well:

    "a"   the tensor starts ONE unit past the boundary        uint8 at 1 mod 4, int16 at 2 mod 4, 4-byte types at 4 mod 16,
                                                              8-byte types at 8 mod 16
    "b"   the tensor starts THREE units past the boundary     uint8 at 3 mod 4, int16 at 6 mod 8, 4-byte types at 12 mod 16

The unit is the element size -- what ``_check`` lets through, and what "any alignment" and "needs no more than the 2-byte
alignment of uint16" promise -- or, where include/mspa.h or the wrapper's docstring demands more for that argument, the
documented alignment A (``aligned``: path -> (A, the sentence), tests/poison_cases.py ``Case.aligned``); then the tensor
sits at A mod 2A in both modes.  Either way ``data_ptr() % (2 * unit) == unit``, which ``assert_skewed`` holds every re-homed
tensor to before a run.

An aligned-down read of an input's first word now reads the front fence, so the comparison of the plain, the "a" and the "b" run
catches a result that depends on the bytes IN FRONT of an input; a wide store that covers bytes in front of an output damages
that fence.

``skewed_copy(inputs, mode, aligned)`` re-homes the device tensors of a case's inputs; ``skewed_allocations(mode, aligned)``
patches fence_util's ``FACTORIES`` and skews a result only when the allocation was made OUTSIDE the package (a case's own ``out=``
buffers, slot buffers and status arrays: the caller's).  What ``mspa/*.py`` allocates for itself is fenced but not skewed:
``engine._workspace`` and the wrappers' outputs may rely on the allocator's alignment, and they say so.

``refusal_copy(inputs, aligned, path)`` is the other half of a documented alignment: the one argument ``path`` at A / 2 past a
boundary, everything else where the documents want it -- the call must be refused.

Nothing here reads or writes outside an allocation: the fences are the harness's own memory.
"""
from __future__ import annotations

import contextlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fence_util  # noqa: E402
from fence_util import FACTORIES, FencedInputs, Fences, _span_bytes, _walk, call_site  # noqa: E402

fence_util.HARNESS.add(os.path.abspath(__file__))      # the patched factories live here: no frame of this file is a call site

MODES = ("a", "b")
UNITS_PAST = {"a": 1, "b": 3}


def entry_for(aligned, path):
    """The (A, sentence) of ``aligned`` that covers ``path`` -- the path itself or a nesting above it -- or None."""
    for key, entry in (aligned or {}).items():
        if path == key or path.startswith(key + "/"):
            return entry
    return None


def unit_of(element_size: int, documented: int = 0) -> int:
    """The unit a tensor is skewed by: its element size, or the documented alignment where that asks for more."""
    return max(int(element_size), int(documented or 0))


def skew_of(element_size: int, mode: str, documented: int = 0) -> int:
    """Bytes past the 512-byte boundary: one ("a") or three ("b") element sizes; a documented alignment A > element size: A."""
    if mode not in MODES:
        raise ValueError(f"skew mode {mode!r}: choose from {MODES}")
    unit = unit_of(element_size, documented)
    if unit & (unit - 1) or unit % element_size or 2 * unit > fence_util.ALIGN:
        raise ValueError(f"a unit of {unit} bytes for elements of {element_size}: a power of two, a multiple of the element, at most 256")
    return unit if unit > element_size else unit * UNITS_PAST[mode]


class SkewedInputs(FencedInputs):
    """``FencedInputs`` whose payloads are skewed; ``units``: path -> the unit each was skewed by."""

    def __init__(self, mode):
        super().__init__(mode)
        self.units = {}


def assert_skewed(handle_or_pairs):
    """Every re-homed tensor starts where the module says: ``data_ptr() % (2 * unit) == unit``.  Takes a ``SkewedInputs`` /
    ``SkewedFences`` or (name, tensor, unit) triples; -> the number of tensors looked at."""
    triples = handle_or_pairs.skewed() if hasattr(handle_or_pairs, "skewed") else list(handle_or_pairs)
    for name, t, unit in triples:
        assert t.data_ptr() % (2 * unit) == unit, f"{name}: {str(t.dtype)[6:]} {list(t.shape)} at {t.data_ptr() % 512} mod 512, unit {unit}"
    return len(triples)


def _skewed_inputs(self):
    return [(path, t, self.units[path]) for path, t in self.tensors.items()]


SkewedInputs.skewed = _skewed_inputs


def skewed_copy(inputs, mode: str, aligned=None, devices=("cuda",)):
    """``fence_util.fenced_copy`` with every re-homed tensor one / three units past the boundary (the module's docstring): shape,
    dtype and strides kept, the same tensor object met twice re-homed once.  -> (the copy, the ``SkewedInputs`` --
    ``check_fences()``, ``changed_inputs(writes)``, ``skewed()`` --, its snapshot)."""
    handle = SkewedInputs(mode)
    devices = tuple(devices)
    memo = {}

    def visit(path, x):
        if not isinstance(x, torch.Tensor) or x.device.type not in devices or x.numel() == 0:
            return x
        if id(x) not in memo:
            entry = entry_for(aligned, path)
            documented = entry[0] if entry else 0
            skew = skew_of(x.element_size(), mode, documented)
            memo[id(x)] = (handle.rehome(x, f"input {path}", skew=skew), x, unit_of(x.element_size(), documented))
        t, _x, unit = memo[id(x)]
        handle.tensors[path] = t
        handle.units[path] = unit
        handle.snapshot[path] = _span_bytes(t)
        return t

    return _walk(inputs, "", visit), handle, handle.snapshot


def refusal_copy(inputs, aligned, path: str, mode: str = "a", devices=("cuda",)):
    """The inputs re-homed between fences with every tensor where the allocator would put it (skew 0), except the one(s) under
    ``path``: A / 2 past a boundary, A its documented alignment -- the largest alignment that is still too small.
    -> (the copy, the ``SkewedInputs``, the number of tensors put there)."""
    A = entry_for(aligned, path)[0]
    handle = SkewedInputs(mode)
    devices = tuple(devices)
    memo, moved = {}, []

    def visit(p, x):
        if not isinstance(x, torch.Tensor) or x.device.type not in devices or x.numel() == 0:
            return x
        if id(x) not in memo:
            here = p == path or p.startswith(path + "/")
            if here and (A // 2) % x.element_size():
                raise ValueError(f"{p}: A / 2 = {A // 2} is no multiple of the element size {x.element_size()}")
            memo[id(x)] = (handle.rehome(x, f"input {p}", skew=A // 2 if here else 0), x)
            if here:
                moved.append(p)
                assert memo[id(x)][0].data_ptr() % A == A // 2
        t = memo[id(x)][0]
        handle.tensors[p] = t
        handle.units[p] = x.element_size()
        handle.snapshot[p] = _span_bytes(t)
        return t

    return _walk(inputs, "", visit), handle, len(moved)


class SkewedFences(Fences):
    """The ``Fences`` of ``skewed_allocations``: ``caller`` lists (name, tensor, unit) of the results that were skewed, ``named``
    the buffers that came through ``caller_buffer`` (name -> [tensor]), ``filled`` those of a refusal run with the fill they got."""

    def __init__(self, mode):
        super().__init__(mode)
        self.caller = []
        self.named = {}
        self.filled = []

    def skewed(self):
        return list(self.caller)

    def written(self):
        """Names of the caller's buffers of a refusal run that no longer hold their fill (synchronises)."""
        if any(t.is_cuda for _n, t, _w in self.filled):
            torch.cuda.synchronize()
        return [name for name, t, want in self.filled if not torch.equal(t.contiguous().view(torch.uint8).cpu(), want)]


_NAMED = [None]                                           # the name of the buffer ``caller_buffer`` is allocating right now
_ACTIVE = [None]                                          # the mode of the ``skewed_allocations`` block that is open (not a refusal run)


def active_mode():
    """"a" / "b" inside a ``skewed_allocations`` block that skews (every tensor of the caller's is then where the module's table
    says, and a case may assert the residue its branch needs); None outside one and in a refusal run."""
    return _ACTIVE[0]


def caller_buffer(name: str, shape, dtype, device):
    """``torch.zeros`` for a buffer the CALLER of an op owns (a case's ``out=``, a status array, a workspace it passes): under
    ``skewed_allocations`` it is placed by the entry "own/<name>" of ``aligned``; outside the patch it is a plain allocation.
    Zeros, so that what an op is documented to leave as it was compares equal between the runs (unwritten outputs are
    tests/test_gpu_poisoned_memory.py's subject, not this harness's)."""
    _NAMED[0] = str(name)
    try:
        return torch.zeros(shape, dtype=dtype, device=device)
    finally:
        _NAMED[0] = None


def _outside_the_package(site: str) -> bool:
    """``fence_util.call_site()`` names the first frame inside the package as a path relative to the repository; without one it
    names a bare file."""
    return not site.startswith(os.path.relpath(fence_util.PACKAGE_DIR, fence_util._ROOT) + os.sep)


@contextlib.contextmanager
def skewed_allocations(mode: str, aligned=None, devices=("cuda",), misplace=None):
    """``fence_util.fenced_allocations`` in which a result allocated OUTSIDE the package -- ``fence_util.call_site()`` finds no
    frame of ``mspa/*.py`` -- is skewed as well: by its element size, or, a ``caller_buffer`` named N, by the alignment that
    ``aligned["own/N"]`` documents.  ``misplace`` ("own/N") makes it the refusal run: that buffer goes A / 2 past a boundary, every
    other caller's allocation stays where the allocator puts it, and every ``caller_buffer`` is filled with the mode's poison
    (``written()`` says which of them an op has touched).  Yields the ``SkewedFences``."""
    fences = SkewedFences(mode)
    devices = tuple(devices)
    saved = [(owner, name, name in vars(owner), getattr(owner, name)) for owner, name in FACTORIES]

    def wrap(real):
        def factory(*args, **kwargs):
            name, _NAMED[0] = _NAMED[0], None
            t = real(*args, **kwargs)
            if not isinstance(t, torch.Tensor) or t.device.type not in devices:
                return t
            site = call_site()
            if t.numel() == 0:
                fences.empty_sites.append(site)
                return t
            if name is None and not _outside_the_package(site):
                return fences.rehome(t, site)
            key = None if name is None else f"own/{name}"
            entry = entry_for(aligned, key) if key else None
            documented = entry[0] if entry else 0
            if misplace is not None:
                out = fences.rehome(t, site, skew=entry_for(aligned, misplace)[0] // 2 if key == misplace else 0)
                if name is not None:
                    fence_util.fill_poison(out, mode)
                    fences.filled.append((name, out, out.contiguous().view(torch.uint8).cpu().clone()))
            else:
                out = fences.rehome(t, site, skew=skew_of(t.element_size(), mode, documented))
                fences.caller.append((key or site, out, unit_of(t.element_size(), documented)))
                assert_skewed(fences.caller[-1:])        # before the op that it is allocated for sees it
            if name is not None:
                fences.named.setdefault(name, []).append(out)
            return out
        factory.__name__ = getattr(real, "__name__", "factory")
        return factory

    for owner, name, _own, real in saved:
        setattr(owner, name, wrap(real))
    previous, _ACTIVE[0] = _ACTIVE[0], mode if misplace is None else None
    try:
        yield fences
    finally:
        _ACTIVE[0] = previous
        for owner, name, own, real in saved:
            if own:
                setattr(owner, name, real)
            else:
                delattr(owner, name)                     # the inherited method shows through again
