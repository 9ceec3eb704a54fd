"""The three ops of ``mspa.cloud_segments`` through the memory and stream harnesses the ops of ``mspa.engine`` run through
(tests/poison_util.py, tests/fence_util.py, tests/stream_util.py), as cases of the same shape as tests/poison_cases.py's:

  * poisoned allocations (zero, "a", "b"): the result does not depend on what the allocator handed over;
  * fences: no store outside a buffer, no written input, no result that depends on the bytes behind an input;
  * a delay on a side stream: nothing is launched on stream 0 and nothing is left on a stream nobody waits for;
    ``outlier_stats_segments`` is held to its "Enqueue only" sentence, and the other two to the read-backs their docstrings name,
    counted with torch's own synchronisation warnings.

The batch is the first 15 segments of tests/cloud_segments_util.py's (4 909 rows; empty segments first and in the middle, rows of
three segments in one wave) followed by its line and its identical points and an empty segment at the end."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_segments_util as U  # noqa: E402
import stream_util as SU  # noqa: E402
from poison_util import MODES, compare_runs, poisoned_allocations  # noqa: E402

pytestmark = pytest.mark.gpu
K, RATIO = 20, 1.0
ENQUEUE_ONLY = "Enqueue only: the offsets go up through pinned memory and nothing is read back."


def _batch():
    xyz, offsets, names = U.batch()
    parts = [xyz[:offsets[15]], xyz[offsets[names.index("line-500")]:offsets[names.index("line-500") + 1]],
             xyz[offsets[names.index("identical-200")]:offsets[names.index("identical-200") + 1]]]
    lengths = list(np.diff(offsets[:16])) + [500, 200, 0]
    off = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=off[1:])
    return np.ascontiguousarray(np.concatenate(parts)), off


def _host_reference():
    from mspa import cloud_segments as CS
    if not _REFERENCE:
        xyz, off = _batch()
        avg, evals = CS.knn_mean_distance_segments_host(xyz, off, K, want_evals=True)
        _REFERENCE.update(avg=avg, evals=evals, stats=CS.outlier_stats_segments_host(avg, off, RATIO, xyz))
    return _REFERENCE


_REFERENCE = {}


def _np(t):
    return t.detach().cpu().numpy()


class Search:
    name, enqueue_only, syncs = "knn_mean_distance_segments", None, 1        # "One read-back per call, whatever S is"

    @staticmethod
    def build():
        xyz, off = _batch()
        return {"xyz": torch.from_numpy(xyz).cuda(), "offsets": off}

    @staticmethod
    def run(i):
        from mspa import cloud_segments as CS
        avg, evals = CS.knn_mean_distance_segments(i["xyz"], i["offsets"], K, want_evals=True)
        return {"avg": avg, "evals": evals}

    @staticmethod
    def expect(i, z):
        ref = _host_reference()
        assert np.array_equal(U.bits(_np(z["avg"])), U.bits(ref["avg"])) and np.array_equal(_np(z["evals"]), ref["evals"])


class Stats:
    name, enqueue_only, syncs = "outlier_stats_segments", ENQUEUE_ONLY, 0

    @staticmethod
    def build():
        xyz, off = _batch()
        return {"avg": torch.from_numpy(_host_reference()["avg"].copy()).cuda(), "xyz": torch.from_numpy(xyz).cuda(), "offsets": off}

    @staticmethod
    def run(i):
        from mspa import cloud_segments as CS
        return CS.outlier_stats_segments(i["avg"], i["offsets"], RATIO, i["xyz"])

    @staticmethod
    def expect(i, z):
        want = _host_reference()["stats"]
        assert np.array_equal(_np(z["keep"]), want["keep"]) and np.array_equal(_np(z["kept"]), want["kept"])
        for key in ("mean", "sd", "thr", "lo", "hi"):
            assert np.array_equal(U.bits(_np(z[key])), U.bits(want[key])), key


class Clean:
    name, enqueue_only, syncs = "remove_statistical_outliers_segments", None, 2    # "Two read-backs per call, whatever S is"

    @staticmethod
    def build():
        xyz, off = _batch()
        rows = np.concatenate([xyz, np.arange(len(xyz), dtype=np.float64)[:, None]], axis=1)
        return {"rows": torch.from_numpy(rows).cuda(), "offsets": off}

    @staticmethod
    def run(i):
        from mspa import cloud_segments as CS
        kept, kept_offsets, lo, hi = CS.remove_statistical_outliers_segments(i["rows"], i["offsets"], K, RATIO)
        return {"rows": kept, "offsets": kept_offsets, "lo": lo, "hi": hi}

    @staticmethod
    def expect(i, z):
        want = _host_reference()["stats"]
        xyz, _off = _batch()
        index = np.nonzero(want["keep"])[0]
        assert np.array_equal(_np(z["rows"]), np.concatenate([xyz[index], index.astype(np.float64)[:, None]], axis=1))
        assert np.array_equal(np.diff(z["offsets"]), want["kept"])
        assert np.array_equal(U.bits(_np(z["lo"])), U.bits(want["lo"])) and np.array_equal(U.bits(_np(z["hi"])), U.bits(want["hi"]))


CASES = [Search, Stats, Clean]
ids = [c.name for c in CASES]


def test_the_enqueue_only_sentence_is_the_docstrings():
    from mspa import cloud_segments as CS
    fold = lambda text: " ".join(text.split())                               # noqa: E731
    assert ENQUEUE_ONLY in fold(CS.outlier_stats_segments.__doc__)
    assert "One read-back per call, whatever S is" in fold(CS.knn_mean_distance_segments.__doc__)
    assert "Two read-backs per call, whatever S is" in fold(CS.remove_statistical_outliers_segments.__doc__)


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
def test_nothing_jumps_the_queue_and_the_enqueue_only_op_returns_before_the_work_in_front_of_it(case):
    inputs, snap_a, findings, info = SU.delayed_runs(case.build, case.run, None, case.expect, case.enqueue_only)
    assert findings == [], f"{case.name} (host {info['t_host_ms']:.1f} ms, delay {info['delay_ms']:.0f} ms): " + "; ".join(findings)
    case.expect(inputs, snap_a)
    if case.enqueue_only is None:                                            # a documented read-back waits for the delay
        assert info["returned_early"] == {"a": False, "b": False}, info


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_the_host_waits_as_often_as_the_docstring_says(case):
    """torch warns at every call that synchronises the host (``set_sync_debug_mode``): a device-to-host copy, ``nonzero``,
    ``item``.  The count per call is the docstring's number of read-backs, and does not grow with the number of segments."""
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
    # twice the segments (every segment split in two): the same number of host waits
    off = inputs["offsets"]
    finer = np.unique(np.concatenate([off, (off[:-1] + off[1:]) // 2]))
    assert len(finer) > len(off)
    assert len(count({**inputs, "offsets": finer})) == case.syncs
