"""``TargetIndex.nearest`` + ``fit_segments`` and ``target_index`` (``mspa.cloud_segments``) through the memory and stream harnesses the
other device ops run through (tests/poison_util.py, tests/fence_util.py, tests/stream_util.py, tests/skew_util.py), as cases of the
shape of tests/test_gpu_upright_iou_memory.py's:

  * poisoned allocations (zero, "a", "b"): the result does not depend on what the allocator handed over;
  * fences around the queries, the index's sorted points, order and starts, and every output: no store outside a buffer, no written
    input, no result that depends on the bytes behind an input;
  * skew: the caller's tensors one and three elements past a 512-byte boundary give the same bytes;
  * a delay on a side stream: nothing is launched on stream 0, nothing is left on a stream nobody waits for; ``nearest`` and
    ``fit_segments`` return while the delay still runs and synchronise the host ZERO times, ``target_index`` waits for its one
    read-back and synchronises ONCE -- counted with torch's own synchronisation warnings, at the batch and at twice the batch.

The batch is ``cloud_distance_util.batch()`` with its pair table; the index's grid records and offsets stay outside the harnesses'
reach (a skewed grid record is a misaligned one, which the entry point refuses), its three large tables are inside it."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_distance_util as U  # noqa: E402
import stream_util as SU  # noqa: E402
from poison_util import MODES, compare_runs, poisoned_allocations  # noqa: E402

pytestmark = pytest.mark.gpu
ENQUEUE_ONLY = "Enqueue only: "
READ_BACK = "One read-back per call, whatever S is"


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def _twice(xyz, off):
    return np.concatenate([xyz, xyz]), np.concatenate([off, off[1:] + off[-1]])


class _Held:
    """What the harnesses pass over: not a tensor, a dict, a tuple or a list."""

    def __init__(self, index):
        self.index = index


class Nearest:
    name, syncs, sentence = "nearest+fit_segments", 0, ENQUEUE_ONLY

    @staticmethod
    def build(twice=False):
        from mspa import cloud_segments as CS
        t, t_off, q, q_off, pairs = U.batch()
        if twice:
            (t, t_off), (q, q_off) = _twice(t, t_off), _twice(q, q_off)
            pairs = np.concatenate([pairs, pairs + 13])
        ix = CS.target_index(_dev(t), t_off)
        return {"queries": _dev(q), "q_offsets": q_off, "pairs": pairs, "pts": ix.pts, "order": ix.order, "starts": ix.starts, "held": _Held(ix)}

    @staticmethod
    def run(i):
        from mspa import cloud_segments as CS
        ix = i["held"].index
        view = CS.TargetIndex(ix.offsets, ix.grid_k, ix.grids, ix.off_dev, ix.grids_dev, ix.base_dev, i["pts"], i["order"], i["starts"], ix.device)
        out = view.nearest(i["queries"], i["q_offsets"], i["pairs"], want_evals=True)
        capped = view.nearest(i["queries"], i["q_offsets"], i["pairs"], max_distance=0.05)
        ordered = view.nearest(i["queries"], i["q_offsets"], i["pairs"], want_evals=True, _ordered=not CS.ORDER_QUERIES)      # the other lane order
        return {"nearest": out, "fit": CS.fit_segments(out["distance"], out["offsets"], U.TAU), "capped": capped, "ordered": ordered}

    @staticmethod
    def expect(i, z):
        from mspa import cloud_segments as CS
        twin = U.batch_twin()
        M, P = len(twin["distance"]), len(twin["offsets"]) - 1
        for key in ("distance", "index", "evals"):
            assert _np(z["nearest"][key])[:M].tobytes() == twin[key].tobytes(), key
            assert _np(z["ordered"][key])[:M].tobytes() == twin[key].tobytes(), key
        for key in CS.FIT_KEYS:
            assert _np(z["fit"][key])[:P].tobytes() == twin["fit"][key].tobytes(), key
        t, t_off, q, q_off, pairs = U.batch()
        assert _np(z["capped"]["distance"])[:M].tobytes() == U.oracle(t, t_off, q, q_off, pairs, 0.05)[0].tobytes()


class Index:
    name, syncs, sentence = "target_index", 1, None

    @staticmethod
    def build(twice=False):
        t, t_off, _q, _q_off, _pairs = U.batch()
        if twice:
            t, t_off = _twice(t, t_off)
        return {"targets": _dev(t), "offsets": t_off}

    @staticmethod
    def run(i):
        from mspa import cloud_segments as CS
        ix = CS.target_index(i["targets"], i["offsets"])
        return {"pts": ix.pts, "order": ix.order, "starts": ix.starts, "grids": ix.grids_dev, "cell_base": ix.base_dev, "offsets": ix.off_dev}

    @staticmethod
    def expect(i, z):
        from mspa import cloud_segments as CS
        t, t_off, q, q_off, pairs = U.batch()
        order = _np(z["order"])
        assert np.array_equal(np.sort(order), np.arange(len(order))) and _np(z["pts"]).tobytes() == _np(i["targets"])[order].tobytes()
        ix = CS.TargetIndex(t_off, CS._lib.CLOUD_DISTANCE_GRID_K, _np(z["grids"])[:13].copy(), _dev(t_off), z["grids"][:13].contiguous(), z["cell_base"][:14].contiguous(),
                            z["pts"], z["order"], z["starts"], z["pts"].device)
        if len(order) == len(t):                                             # the index answers as the twin does
            out = ix.nearest(_dev(q), q_off, pairs)
            assert _np(out["distance"]).tobytes() == U.batch_twin()["distance"].tobytes()
            assert _np(out["index"]).tobytes() == U.batch_twin()["index"].tobytes()


CASES = [Nearest, Index]
ids = [c.name for c in CASES]


def test_the_sentences_are_the_docstrings():
    from mspa import cloud_segments as CS
    fold = lambda text: " ".join(text.split())                               # noqa: E731
    assert ENQUEUE_ONLY in fold(CS.TargetIndex.nearest.__doc__) and ENQUEUE_ONLY in fold(CS.fit_segments.__doc__)
    assert "nothing is read back" in fold(CS.TargetIndex.nearest.__doc__) and "nothing is read back" in fold(CS.fit_segments.__doc__)
    assert READ_BACK in fold(CS.target_index.__doc__)


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
    assert sum(len(f) for f in fences[0::2]) >= 2                            # the caller's tensors were fenced, in both modes,
    assert sum(len(f) for f in fences[1::2]) >= 4                            # and so was what the op allocated
    assert findings == [], f"{case.name}: " + "; ".join(findings)
    case.expect(fenced_inputs, run_a)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_the_result_is_the_same_wherever_the_callers_rows_start(case):
    from test_gpu_skewed_memory import skewed_runs
    skewed_inputs, run_a, findings, _handles = skewed_runs(case.build, case.run, (), None, case.expect, None)
    assert findings == [], f"{case.name}: " + "; ".join(findings)
    case.expect(skewed_inputs, run_a)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_nothing_jumps_the_queue_and_only_a_documented_read_back_waits(case):
    inputs, snap_a, findings, info = SU.delayed_runs(case.build, case.run, None, case.expect, case.sentence)
    assert findings == [], f"{case.name} (host {info['t_host_ms']:.1f} ms, delay {info['delay_ms']:.0f} ms): " + "; ".join(findings)
    case.expect(inputs, snap_a)
    early = case.syncs == 0
    assert info["capped"] or info["returned_early"] == {"a": early, "b": early}, info


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_the_host_waits_as_often_as_the_docstring_says(case):
    """torch warns at every call that synchronises the host (``set_sync_debug_mode``): zero times for ``nearest`` and ``fit_segments``,
    once for ``target_index``, at the batch and at twice the batch."""
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
    assert len(count(case.build())) == case.syncs
    assert len(count(case.build(twice=True))) == case.syncs
