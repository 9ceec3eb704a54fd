"""``mspa.cloud_segments.upright_boxes_segments`` and ``footprint_hull_segments`` through the memory and stream harnesses the other
device ops run through (tests/poison_util.py, tests/fence_util.py, tests/stream_util.py, tests/skew_util.py), as cases of the shape
of tests/test_gpu_dbscan_segments_memory.py's:

  * poisoned allocations (zero, "a", "b"): the result does not depend on what the allocator handed over;
  * fences: no store outside a buffer, no written input, no result that depends on the bytes behind an input;
  * skew: the caller's tensors one and three elements past a 512-byte boundary give the same values;
  * a delay on a side stream: nothing is launched on stream 0 and nothing is left on a stream nobody waits for; each op is held to
    the two read-backs its docstring names, counted with torch's own synchronisation warnings, at S and at twice S.

The batch is ``upright_box_util.memory_batch()``: the empty segments, n = 1, the three tiny segments of one wave, the Kettner grid,
the lattice with every point eight times and the 5 000-point circle (more survivors than one compaction tile, the longest chains,
twenty edge tiles)."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_util as SU  # noqa: E402
import upright_box_util as B  # noqa: E402
from poison_util import MODES, compare_runs, poisoned_allocations  # noqa: E402

pytestmark = pytest.mark.gpu
READ_BACK = "At most two read-backs per call, whatever S is: the survivor counts with the flag word, and the hull counts with the flag word."

_REFERENCE = {}


def _np(t):
    return t.detach().cpu().numpy()


def _case(function):
    class Case:
        name, syncs = function, 2

        @staticmethod
        def build():
            rows, off = B.memory_batch()
            return {"rows": torch.from_numpy(rows.copy()).cuda(), "offsets": off}

        @staticmethod
        def run(i):
            from mspa import cloud_segments as CS
            if function == "footprint_hull_segments":
                index, hull_offsets = CS.footprint_hull_segments(i["rows"], i["offsets"])
                return {"index": index, "hull_offsets": hull_offsets}
            boxes, index, hull_offsets, edges = CS.upright_boxes_segments(i["rows"], i["offsets"], want_hull=True, want_edges=True)
            return {"boxes": boxes, "index": index, "hull_offsets": hull_offsets, "edges": edges}

        @staticmethod
        def expect(i, z):
            from mspa import cloud_segments as CS
            if "twin" not in _REFERENCE:
                _REFERENCE["twin"] = CS.upright_boxes_segments_host(*B.memory_batch(), want_hull=True, want_edges=True)
            boxes, index, hull_offsets, edges = _REFERENCE["twin"]
            assert np.array_equal(_np(z["index"]), index) and np.array_equal(z["hull_offsets"], hull_offsets), Case.name
            if function == "upright_boxes_segments":
                assert _np(z["boxes"]).tobytes() == boxes.tobytes() and np.array_equal(_np(z["edges"]), edges), Case.name
    Case.function = function
    return Case


CASES = [_case("upright_boxes_segments"), _case("footprint_hull_segments")]
ids = [c.name for c in CASES]


def test_the_read_back_sentence_is_the_docstrings():
    from mspa import cloud_segments as CS
    for case in CASES:
        assert READ_BACK in " ".join(getattr(CS, case.function).__doc__.split())


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
    assert sum(len(f) for f in fences[1::2]) >= 4                            # the outputs and the workspaces were fenced
    assert findings == [], f"{case.name}: " + "; ".join(findings)
    case.expect(fenced_inputs, run_a)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_the_result_is_the_same_wherever_the_callers_rows_start(case):
    from test_gpu_skewed_memory import skewed_runs
    skewed_inputs, run_a, findings, _handles = skewed_runs(case.build, case.run, (), None, case.expect, None)
    assert findings == [], f"{case.name}: " + "; ".join(findings)
    case.expect(skewed_inputs, run_a)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_nothing_jumps_the_queue_and_the_read_backs_wait_for_the_work_in_front_of_them(case):
    inputs, snap_a, findings, info = SU.delayed_runs(case.build, case.run, None, case.expect, None)
    assert findings == [], f"{case.name} (host {info['t_host_ms']:.1f} ms, delay {info['delay_ms']:.0f} ms): " + "; ".join(findings)
    case.expect(inputs, snap_a)
    assert info["returned_early"] == {"a": False, "b": False}, info         # the documented read-backs wait for the delay


@pytest.mark.parametrize("case", CASES[:1], ids=ids[:1])
def test_the_host_waits_as_often_as_the_docstring_says(case):
    """torch warns at every call that synchronises the host (``set_sync_debug_mode``).  The count per call is the docstring's two
    read-backs, and does not grow with the number of segments."""
    def count(inputs):
        case.run(inputs)                                                     # warm: the library is loaded, the kernels are resident
        torch.cuda.synchronize()
        previous = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                case.run(inputs)
        finally:
            torch.cuda.set_sync_debug_mode(previous)
        torch.cuda.synchronize()
        return [str(w.message) for w in seen if "synchroniz" in str(w.message)]
    inputs = case.build()
    found = count(inputs)
    assert len(found) == case.syncs, (case.name, found)
    off = inputs["offsets"]                                                  # twice the segments (every segment split in two)
    finer = np.unique(np.concatenate([off, (off[:-1] + off[1:]) // 2]))
    assert len(finer) > len(off)
    assert len(count({**inputs, "offsets": finer})) == case.syncs
