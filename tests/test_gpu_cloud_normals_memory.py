"""``normals_segments`` (``mspa.cloud_segments``) through the memory and stream harnesses the other device ops run through
(tests/poison_util.py, tests/fence_util.py, tests/stream_util.py, tests/skew_util.py), as a case of the shape of
tests/test_gpu_cloud_distance_memory.py's:

  * poisoned allocations (zero, "a", "b"): the result does not depend on what the allocator handed over;
  * fences around the rows, the viewpoints and every output and table the op allocates: no store outside a buffer, no written input,
    no result that depends on the bytes behind an input;
  * skew: the caller's tensors one and three elements past a 512-byte boundary give the same bytes;
  * a delay on a side stream: nothing is launched on stream 0, nothing is left on a stream nobody waits for; the op waits for the one
    read-back of its search tables and synchronises the host ONCE -- counted with torch's own synchronisation warnings, at the batch
    and at twice the batch.

The batch is ``cloud_normals_util.batch()`` with its viewpoints on the device; one run takes the normals with the neighbour table,
the capped normals without it and ``knn_segments``."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_normals_util as U  # noqa: E402
import stream_util as SU  # noqa: E402
from poison_util import MODES, compare_runs, poisoned_allocations  # noqa: E402

pytestmark = pytest.mark.gpu
READ_BACK = "One read-back per call, whatever S is"
KEYS = ("normal", "curvature", "used", "status", "index", "distance")


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


class Normals:
    name, syncs, sentence = "normals_segments", 1, None

    @staticmethod
    def build(twice=False):
        xyz, off, _names = U.batch()
        views = U.viewpoints()
        if twice:
            xyz, off, views = np.concatenate([xyz, xyz]), np.concatenate([off, off[1:] + off[-1]]), np.concatenate([views, views])
        return {"rows": _dev(xyz), "offsets": off, "viewpoints": _dev(views)}

    @staticmethod
    def run(i):
        from mspa import cloud_segments as CS
        return CS.normals_segments(i["rows"], i["offsets"], U.K, None, i["viewpoints"], want_neighbours=True)

    @staticmethod
    def expect(i, z):
        from mspa import cloud_segments as CS
        xyz, off, _names = U.batch()
        twin = CS.normals_segments_host(xyz, off, U.K, None, U.viewpoints(), want_neighbours=True)
        for key in KEYS:
            assert _np(z[key])[:len(xyz)].tobytes() == twin[key].tobytes(), key


class Capped:
    name, syncs, sentence = "normals_segments, capped + knn_segments", 2, None

    build = Normals.build

    @staticmethod
    def run(i):
        from mspa import cloud_segments as CS
        index, distance = CS.knn_segments(i["rows"], i["offsets"], 3)
        return {"capped": CS.normals_segments(i["rows"], i["offsets"], U.K, U.CAP, i["viewpoints"]), "index": index, "distance": distance}

    @staticmethod
    def expect(i, z):
        from mspa import cloud_segments as CS
        xyz, off, _names = U.batch()
        twin = CS.normals_segments_host(xyz, off, U.K, U.CAP, U.viewpoints())
        for key in KEYS[:4]:
            assert _np(z["capped"][key])[:len(xyz)].tobytes() == twin[key].tobytes(), key
        index, distance = CS.knn_segments_host(xyz, off, 3)
        assert _np(z["index"])[:len(xyz)].tobytes() == index.tobytes() and _np(z["distance"])[:len(xyz)].tobytes() == distance.tobytes()


class _Held:
    """What the harnesses pass over: not a tensor, a dict, a tuple or a list."""

    def __init__(self, index):
        self.index = index


class PlaneLoop:
    name, syncs, sentence = "register, point_to_plane", 0, "Enqueue only: "

    @staticmethod
    def build(twice=False):
        from mspa import cloud_segments as CS
        q, q_off, t, t_off, _truth, normals = U.plane_batch()
        if twice:
            q, q_off = np.concatenate([q, q]), np.concatenate([q_off, q_off[1:] + q_off[-1]])
            t, t_off, normals = np.concatenate([t, t]), np.concatenate([t_off, t_off[1:] + t_off[-1]]), np.concatenate([normals, normals])
        ix = CS.target_index(_dev(t), t_off)
        ix.targets()                                                         # scattered back once, outside the runs
        return {"queries": _dev(q), "q_offsets": q_off, "normals": _dev(normals), "pts": ix.pts, "order": ix.order, "starts": ix.starts, "held": _Held(ix)}

    @staticmethod
    def run(i):
        from mspa import cloud_segments as CS
        ix = i["held"].index
        view = CS.TargetIndex(ix.offsets, ix.grid_k, ix.grids, ix.off_dev, ix.grids_dev, ix.base_dev, i["pts"], i["order"], i["starts"], ix.device)
        reg = view.register(i["queries"], i["q_offsets"], max_distance=0.05, iterations=4, estimation="point_to_plane", normals=i["normals"])
        return {k: v for k, v in reg.items() if k != "offsets"}

    @staticmethod
    def expect(i, z):
        from mspa import cloud_segments as CS
        q, q_off, t, t_off, _truth, normals = U.plane_batch()
        twin = CS.register_segments_host(q, q_off, t, t_off, max_distance=0.05, iterations=4, estimation="point_to_plane", normals=normals)
        for key in ("R", "t", "status", "used", "converged_at", "fitness", "inlier_rmse"):
            assert np.ascontiguousarray(_np(z[key])[:5]).tobytes() == np.ascontiguousarray(twin[key]).tobytes(), key


CASES = [Normals, Capped, PlaneLoop]
ids = [c.name for c in CASES]


def test_the_sentences_are_the_docstrings():
    from mspa import cloud_segments as CS
    fold = lambda text: " ".join(text.split())                               # noqa: E731
    assert READ_BACK in fold(CS.normals_segments.__doc__) and READ_BACK in fold(CS.knn_segments.__doc__)


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
    """torch warns at every call that synchronises the host (``set_sync_debug_mode``): once per call of ``normals_segments`` or
    ``knn_segments`` -- the read-back of the search tables -- at the batch and at twice the batch."""
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
