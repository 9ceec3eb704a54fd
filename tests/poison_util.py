"""Run an op on memory that is not what a fresh allocation happens to hold.

Every byte of device memory the package touches comes from ``torch.empty`` (or ``empty_like`` / ``new_empty``).
``poisoned_allocations(mode)`` replaces those three for its duration with versions that fill the new tensor, host or device,
on the current stream.  An op whose result depends on memory it never wrote then gives different results under different
modes, and ``compare_runs`` names the output and the first element where they part.

The modes:

    "zero"   all zero -- the clean run, the one that is checked against the op's reference
    "a"/"b"  two poisons that differ from zero and from each other in every element:

        dtype               "a"                   "b"
        int32, int16        1                     2
        int64               0x0000000100000001    0x0000000200000002
        uint8, bool         0x5A                  0xA5
        float32, float64    NaN                   1.5

    (other integer types take 1 / 2, other floating types NaN / 1.5.)

The values are small on purpose: a stray read that is used as an index, a count or a pixel coordinate stays inside any
buffer of a small case, so that a read-before-write shows as a wrong number and not as a GPU fault.  The int64 patterns
repeat the int32 ones, so a workspace allocated as int64 and read as int32 lanes also reads 1 or 2.

Known limit: a kernel that reads the single bytes 1..3 of a stale 32-bit lane of an int-typed workspace sees zero under
all three modes.  Sensitivity there was given up for the no-fault property.
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch

MODES = ("zero", "a", "b")

_INT64 = {"a": 0x0000000100000001, "b": 0x0000000200000002}
_SMALL = {"a": 1, "b": 2}
_BYTE = {"a": 0x5A, "b": 0xA5}
_FLOAT = {"a": float("nan"), "b": 1.5}

_UNSIGNED_AS = {2: torch.int16, 4: torch.int32, 8: torch.int64}      # torch fills few unsigned types: fill their signed twin


def poison_value(dtype: torch.dtype, mode: str):
    """The fill of ``dtype`` under ``mode`` (the table of the module's docstring)."""
    if mode not in MODES:
        raise ValueError(f"poison mode {mode!r}: choose from {MODES}")
    if mode == "zero":
        return 0
    if dtype in (torch.uint8, torch.bool, torch.int8):
        return _BYTE[mode]
    if dtype == torch.int64 or dtype == getattr(torch, "uint64", None):
        return _INT64[mode]
    if dtype.is_floating_point or dtype.is_complex:
        return _FLOAT[mode]
    return _SMALL[mode]


def fill_poison(t: torch.Tensor, mode: str) -> torch.Tensor:
    """Fill ``t`` in place (on the current stream where it is a device tensor) and return it."""
    if t.numel() == 0:
        return t
    value = poison_value(t.dtype, mode)
    if t.dtype in (torch.bool, torch.int8):
        t.view(torch.uint8).fill_(value)                 # the byte pattern itself, not True / a wrapped negative
    elif not (t.dtype.is_floating_point or t.dtype.is_complex or t.dtype.is_signed or t.dtype == torch.uint8):
        t.view(_UNSIGNED_AS[t.element_size()]).fill_(value)
    else:
        t.fill_(value)
    return t


@contextlib.contextmanager
def poisoned_allocations(mode: str):
    """``torch.empty``, ``torch.empty_like`` and ``torch.Tensor.new_empty`` fill what they return, until the block ends
    (also when it raises)."""
    poison_value(torch.int32, mode)                      # an unknown mode fails before anything is replaced
    real_empty, real_empty_like = torch.empty, torch.empty_like
    own_new_empty = "new_empty" in vars(torch.Tensor)
    real_new_empty = torch.Tensor.new_empty

    def empty(*args, **kwargs):
        return fill_poison(real_empty(*args, **kwargs), mode)

    def empty_like(*args, **kwargs):
        return fill_poison(real_empty_like(*args, **kwargs), mode)

    def new_empty(self, *args, **kwargs):
        return fill_poison(real_new_empty(self, *args, **kwargs), mode)

    torch.empty, torch.empty_like, torch.Tensor.new_empty = empty, empty_like, new_empty
    try:
        yield
    finally:
        torch.empty, torch.empty_like = real_empty, real_empty_like
        if own_new_empty:
            torch.Tensor.new_empty = real_new_empty
        else:
            del torch.Tensor.new_empty                   # the inherited method shows through again


def _leaves(x, path=""):
    """(path, leaf) of a nesting of dicts, tuples and lists; ``None`` leaves are kept (an output that was not asked for)."""
    if isinstance(x, dict):
        for k in x:
            yield from _leaves(x[k], f"{path}/{k}" if path else str(k))
    elif isinstance(x, (tuple, list)) or (isinstance(x, np.ndarray) and x.dtype.hasobject):      # an object array: a list of things
        for i, v in enumerate(x.tolist() if isinstance(x, np.ndarray) else x):
            yield from _leaves(v, f"{path}/{i}" if path else str(i))
    else:
        yield path, x


def _bytes_of(x):
    """A tensor or array -> (shape, uint8 array [*shape, itemsize]); anything else -> None."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    if isinstance(x, np.ndarray):
        a = np.asarray(x, order="C")                  # (ascontiguousarray would turn a 0-d array into a 1-d one)
        return a.shape, a.reshape(-1).view(np.uint8).reshape(a.shape + (a.itemsize,))
    return None


def _mask_of(spec, zero_result, shape):
    """``defined[path]`` -> a boolean array of ``shape``: a mask as it is, or what a function of the zero run returns -- a mask,
    or an index (slice, tuple of slices, integer array) that selects the defined elements."""
    if callable(spec):
        spec = spec(zero_result)
    if isinstance(spec, torch.Tensor):
        spec = spec.detach().cpu().numpy()
    if isinstance(spec, np.ndarray) and spec.dtype == np.bool_:
        return np.broadcast_to(spec, shape)
    mask = np.zeros(shape, dtype=bool)
    mask[spec] = True
    return mask


def compare_runs(zero, a, b, defined=None):
    """The outputs of the three runs, bit for bit (NaN by its bit pattern) -> [(path, first differing index)], empty when the
    op is independent of what its allocations held.  ``defined`` maps a path to the elements that are specified (see
    ``_mask_of``); the others of that output are not compared.  A mask that leaves nothing of a non-empty output is an error."""
    defined = dict(defined or {})
    runs = [dict(_leaves(r)) for r in (zero, a, b)]
    found = []
    unknown = set(defined) - set(runs[0])
    if unknown:
        raise KeyError(f"defined names outputs the run does not return: {sorted(unknown)} (has {sorted(runs[0])})")
    for path, z in runs[0].items():
        if any(path not in r for r in runs[1:]):
            found.append((path, None))
            continue
        zb = _bytes_of(z)
        if zb is None:                                   # a Python value: a count, a name, None
            if any(type(r[path]) is not type(z) or r[path] != z for r in runs[1:]):
                found.append((path, None))
            continue
        shape, zbytes = zb
        mask = None
        if path in defined:
            mask = _mask_of(defined[path], zero, shape)
            if zbytes.size and not mask.any():
                raise ValueError(f"defined[{path!r}] masks the whole output out")
        first = None
        for r in runs[1:]:
            ob = _bytes_of(r[path])
            if ob is None or ob[0] != shape or ob[1].shape != zbytes.shape:
                first = ()
                break
            differs = (ob[1] != zbytes).any(axis=-1)
            if mask is not None:
                differs &= mask
            if differs.any():
                at = tuple(int(i) for i in np.unravel_index(int(np.argmax(differs.reshape(-1))), shape)) if shape else ()
                first = at if first is None or at < first else first
        if first is not None:
            found.append((path, first if len(first) != 1 else first[0]))
    return found


def n_masked(defined) -> int:
    return len(defined or {})
