"""Run an op behind a delay on a side stream that the default stream can overtake.

tests/poison_util.py and tests/fence_util.py ask what an op reads and writes.  This module asks WHEN: every device op of
``mspa.engine`` takes ``torch.cuda.current_stream()`` and promises to run there, and the callers (upload.py's decode slots, the
sweep's encoder threads) rely on it with non-blocking streams that the null stream orders nothing against.  A kernel launched on
stream 0, a memset on the wrong stream or a missing ``wait_stream`` changes no result while everything runs on the default stream
and is followed by a device synchronisation, which is how the rest of the suite runs.

``delayed_runs`` runs an op once plainly and then twice under ``torch.cuda.stream(S)``, S a non-blocking stream of the project's
own (``_lib.own_stream``) that is PROVEN to be overtaken by the default stream (``overtakes``; two streams that share a hardware
queue serialise, which would blind the harness).  On S, in this order: a delay kernel; the restore of every input, which until
then holds poison; the op; a clone of every output; the poison again.  Work that did not wait for S reads the poison or is not in
the clone; a host synchronisation inside an op documented as enqueue-only shows as ``delay_done.query()`` after the call.

The input poison, by the tensor's own dtype ("a" / "b"):

    every integer type, int64 included      1 / 2
    uint8, int8, bool                       0x5A / 0xA5
    floating point (and complex)            NaN / 1.5

poison_util's int64 pattern is for allocations (two int32 lanes); as an INPUT -- an offset, a row number -- it is 4 GiB, so inputs
take the small numbers: an op that reads its inputs too early produces a wrong result, not a fault.

The delay is ``torch.cuda._sleep`` (one thread spinning on the device's clock; its unit is not documented on ROCm), calibrated once
per process with events at two sizes; no clock rate is assumed.  Where its time does not grow with its argument, a calibrated chain
of matrix products on the side stream takes its place (``Delay.kind`` says which).
"""
from __future__ import annotations

import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fence_util import _walk  # noqa: E402
from poison_util import compare_runs  # noqa: E402

MODES = ("a", "b")
ROLES = tuple(f"test-stream-order-{k}" for k in range(8))      # candidates for the test stream (and for the self-checks' second one)
CAP_MS = 2000.0                     # no delay is longer
PROBE_MS = 50.0                     # the independence probe's delay

# MEASURED_FLOOR_MS: the shortest delay at which test_gpu_stream_order.py's self-check (b) -- an op that computes on the default
# stream -- was caught in 20 of 20 tries on the MI355X, doubled: 0.25 ms was the shortest tried and was caught every time (DESIGN 2.1
# has the table).  That is what the GPU needs.  The host needs more: with a delay of half a millisecond one descheduling of the test's
# thread between the delay's launch and the op's return reads as "delay too short" or as a host wait inside an enqueue-only op.  So
# the floor in use is 40 times the measured one.  A longer delay can hide nothing: every delayed run asserts that its delay is still
# running when the op is called, work on a wrong stream has more time to overtake, and a host wait inside an op waits for the end
# of the delay however long it is.  It costs 2 x 20 ms a case.
MEASURED_FLOOR_MS = 0.5
FLOOR_MS = 40 * MEASURED_FLOOR_MS

_SMALL = {"a": 1, "b": 2}
_BYTE = {"a": 0x5A, "b": 0xA5}
_FLOAT = {"a": float("nan"), "b": 1.5}
_UNSIGNED_AS = {2: torch.int16, 4: torch.int32, 8: torch.int64}


class DelayTooShort(AssertionError):
    """The delay had ended before the op was called: the run shows nothing and is an error, never a pass."""


class NoIndependentStream(AssertionError):
    """No candidate stream is overtaken by the default stream: the harness cannot see, which is not a pass."""


# ---- input poison -------------------------------------------------------------------------------------------------------------------------

def input_poison_value(dtype: torch.dtype, mode: str):
    """The fill of an INPUT of ``dtype`` under ``mode`` (the table of the module's docstring)."""
    if mode not in MODES:
        raise ValueError(f"input poison mode {mode!r}: choose from {MODES}")
    if dtype in (torch.uint8, torch.bool, torch.int8):
        return _BYTE[mode]
    if dtype.is_floating_point or dtype.is_complex:
        return _FLOAT[mode]
    return _SMALL[mode]


def fill_input_poison(t: torch.Tensor, mode: str) -> torch.Tensor:
    """Fill ``t`` in place (on the current stream where it is a device tensor) and return it."""
    value = input_poison_value(t.dtype, mode)
    if t.numel() == 0:
        return t
    if t.dtype in (torch.bool, torch.int8):
        t.view(torch.uint8).fill_(value)                 # the byte pattern itself, not True / a wrapped negative
    elif not (t.dtype.is_floating_point or t.dtype.is_complex or t.dtype.is_signed or t.dtype == torch.uint8):
        t.view(_UNSIGNED_AS[t.element_size()]).fill_(value)
    else:
        t.fill_(value)
    return t


def tensor_leaves(x, devices=("cuda",)):
    """[(path, tensor)] of the tensors on one of ``devices`` in a nesting of dicts, tuples and lists, each tensor object once (under
    the first path it is met at); ``None``, NumPy arrays, host tensors and every other leaf are passed over."""
    found, seen = [], set()

    def visit(path, leaf):
        if isinstance(leaf, torch.Tensor) and leaf.device.type in devices and id(leaf) not in seen:
            seen.add(id(leaf))
            found.append((path, leaf))
        return leaf

    _walk(x, "", visit)
    return found


def clone_leaves(leaves):
    """path -> a clone of that leaf (on the current stream)."""
    return {path: t.detach().clone() for path, t in leaves}


def poison_leaves(leaves, mode: str) -> None:
    for _path, t in leaves:
        fill_input_poison(t.detach(), mode)


def restore_leaves(leaves, good) -> None:
    """Every leaf takes its clone's bytes back, in place (NaN payloads included: a copy of equal dtypes moves bytes)."""
    for path, t in leaves:
        t.detach().copy_(good[path])


def snapshot(x, devices=("cuda",)):
    """``x`` with every tensor on one of ``devices`` replaced by a clone made on the current stream; the rest as it is."""
    return _walk(x, "", lambda _path, leaf: leaf.detach().clone() if isinstance(leaf, torch.Tensor) and leaf.device.type in devices else leaf)


# ---- the delay ----------------------------------------------------------------------------------------------------------------------------

def _timed_ms(enqueue, units) -> float:
    """Milliseconds of ``enqueue(units)`` on the current stream, by events."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.current_stream().synchronize()
    start.record()
    enqueue(units)
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def _calibrate(enqueue, first_units: int, limit_units: int):
    """(units per millisecond, milliseconds of no units) of ``enqueue`` from two sizes -- the first at which it takes 5 ms and four
    times that -- or None where its time does not grow with its argument."""
    _timed_ms(enqueue, first_units)                      # the first launch pays for loading the kernel
    units = first_units
    t1 = _timed_ms(enqueue, units)
    while t1 < 5.0:
        units *= 4
        if units > limit_units:
            return None
        t1 = _timed_ms(enqueue, units)
    t2 = _timed_ms(enqueue, 4 * units)
    if not (2.0 * t1 <= t2 <= 8.0 * t1):                 # 4x the units: about 4x the time
        return None
    per_ms = 3 * units / (t2 - t1)
    return per_ms, max(t1 - units / per_ms, 0.0), (units, t1, 4 * units, t2)


class Delay:
    """A kernel (or a chain of them) that occupies the current stream for a known wall time."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.kind, fit = "torch.cuda._sleep", None
        if hasattr(torch.cuda, "_sleep"):
            fit = _calibrate(lambda n: torch.cuda._sleep(int(n)), 1 << 16, 1 << 40)
        if fit is None:                                  # _sleep's time does not follow its argument here: matrix products instead
            self.kind = "chain of 2048^3 float32 matrix products"
            self._m = torch.full((2048, 2048), 1.0 / 2048, dtype=torch.float32, device=self.device)
            self._out = torch.empty_like(self._m)
            fit = _calibrate(self._chain, 4, 1 << 16)
            assert fit is not None, "neither torch.cuda._sleep nor a chain of matrix products takes a time that follows its size"
        self.units_per_ms, self.overhead_ms, self.measured = fit

    def _chain(self, n):
        for _ in range(int(n)):
            torch.mm(self._m, self._m, out=self._out)

    def enqueue(self, ms: float) -> None:
        """Occupy the current stream for ``ms`` milliseconds (at most CAP_MS)."""
        units = max(int((min(ms, CAP_MS) - self.overhead_ms) * self.units_per_ms), 1)
        if self.kind == "torch.cuda._sleep":
            torch.cuda._sleep(units)
        else:
            self._chain(units)

    def describe(self) -> str:
        u1, t1, u2, t2 = self.measured
        return f"{self.kind}: {u1} units {t1:.2f} ms, {u2} units {t2:.2f} ms -> {self.units_per_ms:.0f} units / ms"


def overtakes(fast, slow, delay: Delay, ms: float = PROBE_MS) -> bool:
    """Work enqueued on ``fast`` AFTER a delay was enqueued on ``slow`` completes while that delay is still running: the two streams
    do not share a hardware queue (and ``fast`` is not ordered behind ``slow`` in any other way)."""
    torch.cuda.synchronize()
    delay_done, mark = torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(slow):
        delay.enqueue(ms)
        delay_done.record()
    with torch.cuda.stream(fast):
        x = torch.zeros((8,), dtype=torch.int32, device=delay.device)
        x.add_(1)
        mark.record()
    deadline = time.perf_counter() + 4 * ms / 1000.0
    while not mark.query() and not delay_done.query() and time.perf_counter() < deadline:
        pass                                             # (polling two events: nothing here waits a time limit out)
    seen = mark.query() and not delay_done.query()
    torch.cuda.synchronize()
    return bool(seen and x.sum().item() == 8)


class Harness:
    """The calibrated delay and the test stream of this process, chosen once, before any case runs."""

    def __init__(self, device="cuda"):
        from mspa import _lib
        self.device = torch.device(device)
        torch.cuda.synchronize()
        self.delay = Delay(self.device)
        self.tried = []
        self.role = self.stream = None
        default = torch.cuda.default_stream(self.device)
        for role in ROLES:
            candidate = _lib.own_stream(role, self.device)
            self.tried.append(role)
            if overtakes(default, candidate, self.delay):
                self.role, self.stream = role, candidate
                break
        if self.stream is None:
            raise NoIndependentStream(f"none of the {len(ROLES)} candidate streams {ROLES} is overtaken by the default stream: work on the "
                                      "default stream waited for a delay on each of them, so a delayed run could not tell a kernel launched "
                                      "on the wrong stream from one launched on the right one")
        self._second = None

    def second_stream(self):
        """Another own stream, one that overtakes the test stream (for the self-checks' ops that compute on a stream of their own)."""
        if self._second is None:
            from mspa import _lib
            for role in ROLES:
                if role == self.role:
                    continue
                candidate = _lib.own_stream(role, self.device)
                if overtakes(candidate, self.stream, self.delay):
                    self._second = (role, candidate)
                    break
            else:
                raise NoIndependentStream(f"no second candidate stream of {ROLES} overtakes the test stream {self.role!r}")
        return self._second[1]


_HARNESS = []


def harness() -> Harness:
    """This process's ``Harness``; the first call calibrates and probes (a failure there is raised again by every later call)."""
    if not _HARNESS:
        try:
            _HARNESS.append(Harness())
        except AssertionError as e:
            _HARNESS.append(e)
    if isinstance(_HARNESS[0], BaseException):
        raise _HARNESS[0]
    return _HARNESS[0]


# ---- the delayed run ----------------------------------------------------------------------------------------------------------------------

def delay_for(t_host_ms: float, floor_ms: float = None) -> float:
    """4 x the host time of the warm plain call (the x 4 covers host jitter), at least the floor (FLOOR_MS), at most CAP_MS."""
    return min(max(4.0 * t_host_ms, FLOOR_MS if floor_ms is None else floor_ms), CAP_MS)


def delayed_runs(build, run, defined=None, expect=None, enqueue_only=None, floor_ms: float = None, h: Harness = None):
    """The plain run (twice: held against ``expect``, then timed on the host) and the two delayed ones of an op ->
    (the inputs of the delayed run "a", restored; its outputs' clones; findings: a list of sentences; info: ``t_host_ms``,
    ``delay_ms``, ``returned_early`` per fill, ``capped``)."""
    h = h or harness()
    inputs = build()
    torch.cuda.synchronize()
    plain = run(inputs)
    torch.cuda.synchronize()
    if expect is not None:
        expect(inputs, plain)
    t0 = time.perf_counter()
    again = run(inputs)
    t_host_ms = (time.perf_counter() - t0) * 1000.0
    torch.cuda.synchronize()
    del again
    delay_ms = delay_for(t_host_ms, floor_ms)
    capped = 4.0 * t_host_ms > CAP_MS
    findings, snaps, homes, early = [], {}, {}, {}
    if capped and enqueue_only:
        findings.append(f"the warm plain call took {t_host_ms:.0f} ms on the host, though documented: {enqueue_only}")
    for mode in MODES:
        inputs = build()
        leaves = tensor_leaves(inputs)
        good = clone_leaves(leaves)
        poison_leaves(leaves, mode)
        torch.cuda.synchronize()
        delay_done = torch.cuda.Event()
        with torch.cuda.stream(h.stream):
            h.delay.enqueue(delay_ms)
            delay_done.record()
            restore_leaves(leaves, good)
            if delay_done.query():
                torch.cuda.synchronize()
                raise DelayTooShort(f"delay too short: {delay_ms:.1f} ms on stream {h.role!r} had ended before the op was called (fill {mode})")
            out = run(inputs)
            early[mode] = not delay_done.query()
            snaps[mode] = snapshot(out)
            poison_leaves(leaves, mode)                  # what the op left on a stream S does not wait for reads this, or lands behind the clone
        h.stream.synchronize()
        torch.cuda.synchronize()
        restore_leaves(leaves, good)                     # (for ``expect``, and for whatever a case caches between builds)
        torch.cuda.synchronize()
        homes[mode] = inputs
        del out
    for path, at in compare_runs(plain, snaps["a"], snaps["b"], defined):
        findings.append(f"output {path} differs when the op runs behind a delay on a side stream (plain run, fill a, fill b), first at {at}: "
                        "some of its work did not wait for the stream (or the stream did not wait for it)")
    if expect is not None:
        try:
            expect(homes["a"], snaps["a"])
        except AssertionError as e:
            findings.append(f"the delayed run differs from the op's reference: {e!r}")
    if enqueue_only and not capped:
        for mode in MODES:
            if not early[mode]:
                findings.append(f"fill {mode}: the call returned only after the {delay_ms:.0f} ms delay in front of it had ended: it synchronised "
                                f"the host, though documented: {enqueue_only}")
    info = {"t_host_ms": t_host_ms, "delay_ms": delay_ms, "returned_early": early, "capped": capped}
    return homes["a"], snaps["a"], findings, info
