"""``TargetIndex.register`` and ``rigid_fit_segments`` + ``transform_segments`` (``mspa.cloud_segments``) through the memory and stream
harnesses the other device ops run through (tests/poison_util.py, tests/fence_util.py, tests/stream_util.py, tests/skew_util.py), as
cases of the shape of tests/test_gpu_cloud_distance_memory.py's:

  * poisoned allocations (zero, "a", "b"): the result does not depend on what the allocator handed over;
  * fences around the queries, the targets, the index table, the index's sorted points, order and starts, and every output: no store
    outside a buffer, no written input, no result that depends on the bytes behind an input;
  * skew: the caller's tensors one and three elements past a 512-byte boundary give the same bytes;
  * a delay on a side stream: nothing is launched on stream 0, nothing is left on a stream nobody waits for; ``register`` (30
    iterations, 31 searches), ``rigid_fit_segments`` and ``transform_segments`` return while the delay still runs and synchronise the
    host ZERO times -- counted with torch's own synchronisation warnings, at the batch and at twice the batch.  With ``sync_every=5``
    and 12 iterations ``register`` reads ``converged_at`` back after iterations 5, 10 and 12 at most, ceil(12 / 5) = 3 times; on this
    batch every pair has converged by iteration 5 (the NumPy ICP's own fixed point is below 5), so it synchronises exactly ONCE.

The batches are ``cloud_align_util``'s; the index's grid records and offsets stay outside the harnesses' reach (a skewed grid record is
a misaligned one, which the entry point refuses), its three large tables are inside it."""
import math
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_align_util as U  # noqa: E402
import stream_util as SU  # noqa: E402
from poison_util import MODES, compare_runs, poisoned_allocations  # noqa: E402

pytestmark = pytest.mark.gpu
ENQUEUE_ONLY = "Enqueue only: "
CAP = U.CAPS[U.HARD]
REG_KEYS = ("R", "t", "status", "used", "converged_at", "fitness", "inlier_rmse")


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


def _register_twin(**kw):
    from mspa import cloud_segments as CS
    q, q_off, t, t_off, _truth = U.icp()
    return CS.register_segments_host(q, q_off, t, t_off, max_distance=CAP, **kw)


class Register:
    name, syncs, sentence, kw = "register", 0, ENQUEUE_ONLY, {"iterations": 30, "want_history": True}

    @classmethod
    def build(cls, twice=False):
        from mspa import cloud_segments as CS
        q, q_off, t, t_off, _truth = U.icp()
        if twice:
            (t, t_off), (q, q_off) = _twice(t, t_off), _twice(q, q_off)
        ix = CS.target_index(_dev(t), t_off)
        return {"queries": _dev(q), "q_offsets": q_off, "targets": ix.targets(), "pts": ix.pts, "order": ix.order, "starts": ix.starts, "held": _Held(ix)}

    @classmethod
    def run(cls, i):
        from mspa import cloud_segments as CS
        ix = i["held"].index
        view = CS.TargetIndex(ix.offsets, ix.grid_k, ix.grids, ix.off_dev, ix.grids_dev, ix.base_dev, i["pts"], i["order"], i["starts"], ix.device)
        view.xyz = i["targets"]
        out = view.register(i["queries"], i["q_offsets"], max_distance=CAP, **cls.kw)
        return {k: v for k, v in out.items() if isinstance(v, torch.Tensor)}

    @classmethod
    def expect(cls, i, z):
        twin = _register_twin(**cls.kw)
        P = len(twin["used"])
        for key in REG_KEYS:
            assert np.ascontiguousarray(_np(z[key])[:P]).tobytes() == np.ascontiguousarray(twin[key]).tobytes(), key
        for key in ("history_used", "history_rmse"):
            if key in z:
                assert np.ascontiguousarray(_np(z[key])[:, :P]).tobytes() == twin[key].tobytes(), key


class RegisterSynced(Register):
    name, sentence, kw = "register(sync_every=5)", None, {"iterations": 12, "sync_every": 5}
    at_most = math.ceil(12 / 5)
    syncs = 1                                                                # every pair's fixed point lies below iteration 5


class FitAndTransform:
    name, syncs, sentence = "rigid_fit_segments+transform_segments", 0, ENQUEUE_ONLY

    @staticmethod
    def build(twice=False):
        q, q_off, p, pairs, index, _out = U.kabsch_variant()
        if twice:
            S = len(q_off) - 1
            index = np.concatenate([index, np.where(index >= 0, index + len(p), -1)])
            (q, q_off), p, pairs = _twice(q, q_off), np.concatenate([p, p]), np.concatenate([pairs, pairs + S])
        return {"queries": _dev(q), "q_offsets": q_off, "targets": _dev(p), "index": _dev(index), "pairs": pairs}

    @staticmethod
    def run(i):
        from mspa import cloud_segments as CS
        fit = CS.rigid_fit_segments(i["queries"], i["q_offsets"], i["targets"], i["index"], i["pairs"], want_parts=True)
        moved = CS.transform_segments(i["queries"], i["q_offsets"], fit["R"], fit["t"], i["pairs"])
        return {"fit": {k: v for k, v in fit.items() if isinstance(v, torch.Tensor)}, "moved": moved["xyz"]}

    @staticmethod
    def expect(i, z):
        from mspa import cloud_segments as CS
        q, q_off, p, pairs, index, out = U.kabsch_variant()
        twin = CS.rigid_fit_segments_host(q, q_off, p, index, pairs, want_parts=True)
        P = len(pairs)
        for key in ("R", "t", "used", "status", "eigen"):
            assert np.ascontiguousarray(_np(z["fit"][key])[:P]).tobytes() == np.ascontiguousarray(twin[key]).tobytes(), key
        assert _np(z["moved"])[:out[-1]].tobytes() == CS.transform_segments_host(q, q_off, twin["R"], twin["t"], pairs)["xyz"].tobytes()


CASES = [Register, FitAndTransform]
ids = [c.name for c in CASES]


def test_the_sentences_are_the_docstrings():
    from mspa import cloud_segments as CS
    fold = lambda text: " ".join(text.split())                               # noqa: E731
    for doc in (CS.TargetIndex.register.__doc__, CS.rigid_fit_segments.__doc__, CS.transform_segments.__doc__):
        assert ENQUEUE_ONLY in fold(doc) and "nothing is read back" in fold(doc)
    assert "zero host synchronisations" in fold(CS.TargetIndex.register.__doc__)
    assert "ceil(iterations / n) read-backs at most" in fold(CS.TargetIndex.register.__doc__)


def test_the_reference_alone_says_every_pair_is_at_its_fixed_point_before_the_first_read_back():
    assert all(ref["fixed_at"] < 5 for ref in U.icp_references().values())


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
def test_nothing_jumps_the_queue_and_nothing_waits(case):
    inputs, snap_a, findings, info = SU.delayed_runs(case.build, case.run, None, case.expect, case.sentence)
    assert findings == [], f"{case.name} (host {info['t_host_ms']:.1f} ms, delay {info['delay_ms']:.0f} ms): " + "; ".join(findings)
    case.expect(inputs, snap_a)
    assert info["capped"] or info["returned_early"] == {"a": True, "b": True}, info


@pytest.mark.parametrize("case", CASES + [RegisterSynced], ids=ids + [RegisterSynced.name])
def test_the_host_waits_as_often_as_the_docstring_says(case):
    """torch warns at every call that synchronises the host (``set_sync_debug_mode``): zero times for ``register``, ``rigid_fit_segments``
    and ``transform_segments``; with ``sync_every=5`` and 12 iterations at most ceil(12 / 5) = 3 times, and once here, where the loop
    ends at its first read-back -- at the batch and at twice the batch."""
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
    for twice in (False, True):
        n = len(count(case.build(twice=twice)))
        assert n == case.syncs and n <= getattr(case, "at_most", 0), (twice, n)
