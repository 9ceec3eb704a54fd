"""``mspa.cloud_segments.voxel_down_sample_segments`` through the memory and stream harnesses the other device ops run through
(tests/poison_util.py, tests/fence_util.py, tests/stream_util.py, tests/skew_util.py), as cases of the shape of
tests/test_gpu_cloud_segments_memory.py's:

  * poisoned allocations (zero, "a", "b"): the result does not depend on what the allocator handed over;
  * fences: no store outside a buffer, no written input, no result that depends on the bytes behind an input;
  * skew: the caller's tensors one and three elements past a 512-byte boundary give the same bits;
  * a delay on a side stream: nothing is launched on stream 0 and nothing is left on a stream nobody waits for; the op is held to the
    one read-back its docstring names, counted with torch's own synchronisation warnings, at S and at twice S.

The batch is the first 15 segments of tests/voxel_segments_util.py's (4 909 rows; empty segments first and in the middle, rows of
three segments in one wave), its lattice (half the rows on a voxel face), its identical points and an empty segment at the end; the
cases are the three sum regimes: every run short (size 0.01), both (0.25), a voxel that swallows a segment (100), the last two with
colour columns."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_segments_util as V  # noqa: E402
import stream_util as SU  # noqa: E402
from poison_util import MODES, compare_runs, poisoned_allocations  # noqa: E402

pytestmark = pytest.mark.gpu
ONE_READ_BACK = "One read-back per call, whatever S is: the per-segment voxel counts together with the flag word."


def _batch(columns):
    rows, offsets, names = V.batch(columns)
    cut = [(0, int(offsets[15]))] + [(int(offsets[names.index(n)]), int(offsets[names.index(n) + 1])) for n in ("lattice-3000", "identical-200")]
    lengths = list(np.diff(offsets[:16])) + [3000, 200, 0]
    off = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=off[1:])
    return np.ascontiguousarray(np.concatenate([rows[a:b] for a, b in cut])), off


_REFERENCE = {}


def _np(t):
    return t.detach().cpu().numpy()


def _case(size, columns):
    class Case:
        name, syncs = f"voxel_down_sample_segments-{size}-{columns}cols", 1

        @staticmethod
        def build():
            rows, off = _batch(columns)
            return {"rows": torch.from_numpy(rows).cuda(), "offsets": off}

        @staticmethod
        def run(i):
            from mspa import cloud_segments as CS
            rows, offsets, counts = CS.voxel_down_sample_segments(i["rows"], i["offsets"], size)
            return {"rows": rows, "offsets": offsets, "counts": counts}

        @staticmethod
        def expect(i, z):
            from mspa import cloud_segments as CS
            if (size, columns) not in _REFERENCE:
                _REFERENCE[(size, columns)] = CS.voxel_down_sample_segments_host(*_batch(columns), size)
            V.assert_same((_np(z["rows"]), z["offsets"], _np(z["counts"])), _REFERENCE[(size, columns)], Case.name)
    return Case


CASES = [_case(0.01, 3), _case(0.25, 6), _case(100.0, 6)]
ids = [c.name for c in CASES]


def test_the_read_back_sentence_is_the_docstrings():
    from mspa import cloud_segments as CS
    assert ONE_READ_BACK in " ".join(CS.voxel_down_sample_segments.__doc__.split())


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
    assert sum(len(f) for f in fences[1::2]) >= 4                            # the outputs and the workspace were fenced
    assert findings == [], f"{case.name}: " + "; ".join(findings)
    case.expect(fenced_inputs, run_a)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_the_result_is_the_same_bits_wherever_the_callers_rows_start(case):
    from test_gpu_skewed_memory import skewed_runs
    skewed_inputs, run_a, findings, _handles = skewed_runs(case.build, case.run, (), None, case.expect, None)
    assert findings == [], f"{case.name}: " + "; ".join(findings)
    case.expect(skewed_inputs, run_a)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_nothing_jumps_the_queue_and_the_read_back_waits_for_the_work_in_front_of_it(case):
    inputs, snap_a, findings, info = SU.delayed_runs(case.build, case.run, None, case.expect, None)
    assert findings == [], f"{case.name} (host {info['t_host_ms']:.1f} ms, delay {info['delay_ms']:.0f} ms): " + "; ".join(findings)
    case.expect(inputs, snap_a)
    assert info["returned_early"] == {"a": False, "b": False}, info         # the documented read-back waits for the delay


@pytest.mark.parametrize("case", CASES[:2], ids=ids[:2])
def test_the_host_waits_as_often_as_the_docstring_says(case):
    """torch warns at every call that synchronises the host (``set_sync_debug_mode``).  The count per call is the docstring's one
    read-back, and does not grow with the number of segments."""
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
