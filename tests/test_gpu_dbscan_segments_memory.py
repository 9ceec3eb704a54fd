"""``mspa.cloud_segments.dbscan_segments`` and ``largest_cluster_segments`` through the memory and stream harnesses the other device
ops run through (tests/poison_util.py, tests/fence_util.py, tests/stream_util.py, tests/skew_util.py), as cases of the shape of
tests/test_gpu_voxel_segments_memory.py's:

  * poisoned allocations (zero, "a", "b"): the result does not depend on what the allocator handed over;
  * fences: no store outside a buffer, no written input, no result that depends on the bytes behind an input;
  * skew: the caller's tensors one and three elements past a 512-byte boundary give the same values;
  * a delay on a side stream: nothing is launched on stream 0 and nothing is left on a stream nobody waits for; each op is held to
    the one read-back its docstring names, counted with torch's own synchronisation warnings, at S and at twice S.

The batch is the first 17 segments of tests/dbscan_segments_util.py's (4 909 rows; empty segments first and in the middle, rows of
three segments in one wave), its chain, its duplicated points, its small lattice, the two shared-border segments and an empty
segment at the end; the cases are labels at (0.05, 4) -- noise, border rows and many clusters -- and at (0.125, 1) -- every row
core, the chain one cluster -- and the largest cluster at (0.05, 4)."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dbscan_segments_util as D  # noqa: E402
import stream_util as SU  # noqa: E402
from poison_util import MODES, compare_runs, poisoned_allocations  # noqa: E402

pytestmark = pytest.mark.gpu
READ_BACKS = {"dbscan_segments": "One read-back per call, whatever S is: the per-segment cluster counts together with the flag word.",
              "largest_cluster_segments": "One read-back per call, whatever S is: the kept counts with the flag word."}


def _batch():
    rows, offsets, names, _eps = D.batch()
    picked = ["chain-3000", "dup8", "lattice-eighths", "shared-border", "shared-border-swapped", "end-empty"]
    cut = [(0, int(offsets[17]))] + [(int(offsets[names.index(n)]), int(offsets[names.index(n) + 1])) for n in picked]
    lengths = list(np.diff(offsets[:18])) + [b - a for a, b in cut[1:]]
    off = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=off[1:])
    return np.ascontiguousarray(np.concatenate([rows[a:b] for a, b in cut])), off


_REFERENCE = {}


def _np(t):
    return t.detach().cpu().numpy()


def _case(function, eps, min_points):
    class Case:
        name, syncs = f"{function}-{eps}-{min_points}", 1

        @staticmethod
        def build():
            rows, off = _batch()
            return {"rows": torch.from_numpy(rows).cuda(), "offsets": off}

        @staticmethod
        def run(i):
            from mspa import cloud_segments as CS
            if function == "dbscan_segments":
                labels, clusters = CS.dbscan_segments(i["rows"], i["offsets"], eps, min_points)
                return {"labels": labels, "clusters": clusters}
            kept, kept_offsets, lo, hi, index = CS.largest_cluster_segments(i["rows"], i["offsets"], eps, min_points)
            return {"rows": kept, "offsets": kept_offsets, "lo": lo, "hi": hi, "index": index}

        @staticmethod
        def expect(i, z):
            from mspa import cloud_segments as CS
            if Case.name not in _REFERENCE:
                _REFERENCE[Case.name] = getattr(CS, function + "_host")(*_batch(), eps, min_points)
            want = _REFERENCE[Case.name]
            if function == "dbscan_segments":
                assert np.array_equal(_np(z["labels"]), want[0]) and np.array_equal(z["clusters"], want[1]), Case.name
            else:
                got = (_np(z["rows"]), z["offsets"], _np(z["lo"]), _np(z["hi"]), _np(z["index"]))
                assert all(np.array_equal(a, b) for a, b in zip(got, want)), Case.name
    Case.function = function
    return Case


CASES = [_case("dbscan_segments", 0.05, 4), _case("dbscan_segments", 0.125, 1), _case("largest_cluster_segments", 0.05, 4)]
ids = [c.name for c in CASES]


def test_the_read_back_sentences_are_the_docstrings():
    from mspa import cloud_segments as CS
    for name, sentence in READ_BACKS.items():
        assert sentence in " ".join(getattr(CS, name).__doc__.split())


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
def test_nothing_jumps_the_queue_and_the_read_back_waits_for_the_work_in_front_of_it(case):
    inputs, snap_a, findings, info = SU.delayed_runs(case.build, case.run, None, case.expect, None)
    assert findings == [], f"{case.name} (host {info['t_host_ms']:.1f} ms, delay {info['delay_ms']:.0f} ms): " + "; ".join(findings)
    case.expect(inputs, snap_a)
    assert info["returned_early"] == {"a": False, "b": False}, info         # the documented read-back waits for the delay


@pytest.mark.parametrize("case", CASES[::2], ids=ids[::2])
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
