"""``mspa.cloud_segments.upright_iou`` and ``upright_iou_matrix`` through the memory and stream harnesses the other device ops run
through (tests/poison_util.py, tests/fence_util.py, tests/stream_util.py, tests/skew_util.py), as cases of the shape of
tests/test_gpu_upright_segments_memory.py's:

  * poisoned allocations (zero, "a", "b"): the result does not depend on what the allocator handed over;
  * fences around a, b, out and parts: no store outside a buffer, no written input, no result that depends on the bytes behind an input;
  * skew: the caller's tensors one and three elements past a 512-byte boundary give the same bytes;
  * a delay on a side stream: nothing is launched on stream 0, nothing is left on a stream nobody waits for, and the call returns
    while the delay still runs; the host is synchronised ZERO times, counted with torch's own synchronisation warnings, at P and at
    twice P.

The pairs are the first 1 100 of ``upright_iou_util.batch()`` (every named pair, the refused ones included; nine workgroups, the last
one partly filled); the matrix is the 70 boxes of ``matrix_boxes()`` against themselves."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_util as SU  # noqa: E402
import upright_iou_util as U  # noqa: E402
from poison_util import MODES, compare_runs, poisoned_allocations  # noqa: E402

pytestmark = pytest.mark.gpu
ENQUEUE_ONLY = "Enqueue only: one launch on the current stream and nothing is read back."
PAIRS = 1100


def _np(t):
    return t.detach().cpu().numpy()


def _case(function):
    class Case:
        name, syncs = function, 0

        @staticmethod
        def build(pairs=PAIRS):
            if function == "upright_iou_matrix":
                boxes = U.matrix_boxes()
                return {"a": torch.from_numpy(boxes.copy()).cuda(), "b": torch.from_numpy(boxes.copy()).cuda()}
            a, b, _names = U.batch()
            return {"a": torch.from_numpy(a[:pairs].copy()).cuda(), "b": torch.from_numpy(b[:pairs].copy()).cuda()}

        @staticmethod
        def run(i):
            from mspa import cloud_segments as CS
            out, parts = getattr(CS, function)(i["a"], i["b"], want_parts=True)
            return {"out": out, "parts": parts}

        @staticmethod
        def expect(i, z):
            want, want_parts = U.matrix_twin() if function == "upright_iou_matrix" else U.batch_twin()
            n = len(_np(z["out"]))
            assert _np(z["out"]).tobytes() == want[:n].tobytes() and _np(z["parts"]).tobytes() == want_parts[:n].tobytes(), Case.name
    Case.function = function
    return Case


CASES = [_case("upright_iou"), _case("upright_iou_matrix")]
ids = [c.name for c in CASES]


def test_the_enqueue_only_sentence_is_the_docstrings():
    from mspa import cloud_segments as CS
    for case in CASES:
        assert ENQUEUE_ONLY in " ".join(getattr(CS, case.function).__doc__.split())
    assert "Enqueue only." in " ".join(CS.upright_of_aabb.__doc__.split())


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_the_result_does_not_depend_on_what_the_allocator_handed_over(case):
    runs = {}
    for mode in MODES:
        inputs = case.build()                                                # outside the patch: inputs are never poisoned
        torch.cuda.synchronize()
        with poisoned_allocations(mode):
            runs[mode] = case.run(inputs)
            torch.cuda.synchronize()
    case.expect(inputs, runs["zero"])
    found = compare_runs(runs["zero"], runs["a"], runs["b"])
    assert found == [], f"{case.name}: outputs that depend on unwritten memory (path, first element): {found}"


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_nothing_is_written_outside_a_buffer_and_nothing_beyond_an_input_reaches_the_result(case):
    from test_gpu_fenced_memory import fenced_runs
    fenced_inputs, run_a, findings, fences = fenced_runs(case.build, case.run, (), None, case.expect)
    assert sum(len(f) for f in fences[0::2]) >= 4                            # a and b were fenced, in both modes,
    assert sum(len(f) for f in fences[1::2]) >= 4                            # and so were out and parts
    assert findings == [], f"{case.name}: " + "; ".join(findings)
    case.expect(fenced_inputs, run_a)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_the_result_is_the_same_wherever_the_callers_boxes_start(case):
    from test_gpu_skewed_memory import skewed_runs
    skewed_inputs, run_a, findings, _handles = skewed_runs(case.build, case.run, (), None, case.expect, None)
    assert findings == [], f"{case.name}: " + "; ".join(findings)
    case.expect(skewed_inputs, run_a)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_nothing_jumps_the_queue_and_the_call_returns_before_the_work_in_front_of_it(case):
    inputs, snap_a, findings, info = SU.delayed_runs(case.build, case.run, None, case.expect, ENQUEUE_ONLY)
    assert findings == [], f"{case.name} (host {info['t_host_ms']:.1f} ms, delay {info['delay_ms']:.0f} ms): " + "; ".join(findings)
    case.expect(inputs, snap_a)
    assert info["capped"] or info["returned_early"] == {"a": True, "b": True}, info


@pytest.mark.parametrize("case", CASES[:1], ids=ids[:1])
def test_the_host_never_waits(case):
    """torch warns at every call that synchronises the host (``set_sync_debug_mode``).  The count per call is zero, at P pairs and at
    twice P, and for ``upright_of_aabb`` in front of it."""
    from mspa import cloud_segments as CS

    def count(inputs):
        case.run(inputs)                                                     # warm: the library is loaded, the kernel is resident
        torch.cuda.synchronize()
        previous = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                case.run(inputs)
                CS.upright_iou_matrix(inputs["a"][:70], inputs["b"][:33])
                CS.upright_iou(CS.upright_of_aabb(inputs["a"][:, :6]), inputs["b"])
        finally:
            torch.cuda.set_sync_debug_mode(previous)
        torch.cuda.synchronize()
        return [str(w.message) for w in seen if "synchroniz" in str(w.message)]
    assert count(case.build(PAIRS)) == []
    assert count(case.build(2 * PAIRS)) == []
    assert len(U.batch()[0]) >= 2 * PAIRS
