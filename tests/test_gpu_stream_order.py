"""Every device op behind a delay on a busy side stream (tests/stream_util.py, tests/poison_cases.py): each case runs plainly on
the default stream -- the reference run, held against the op's plain reference, and timed on the host -- and twice under
``torch.cuda.stream(S)``, S a non-blocking stream of the project's own that the default stream is proven to overtake.  On S a delay
kernel runs first and the inputs, poisoned until then, are restored behind it; behind the op every output is cloned and the inputs
are poisoned again.  Then, together:

  * the three results are bit-identical wherever the op's documents specify them: a kernel, a memset or a copy that went to
    stream 0 (or to any stream that does not wait for S) read the poison, and work that S does not wait for is not in the clone;
  * the delayed run equals the op's reference as well;
  * where the documents promise that the op only enqueues (``Case.enqueue_only``), the call returned while the delay in front of
    it was still running.

Every delayed run asserts that its delay has not ended when the op is called ("delay too short" is an error, never a pass), and a
process in which no candidate stream is overtaken by the default stream fails every test here: a harness that cannot see is not a
pass.  The poison is small (1 / 2, 0x5A / 0xA5, NaN / 1.5), so an op that reads its inputs too early gives a wrong number."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poison_cases  # noqa: E402
import stream_util as SU  # noqa: E402

pytestmark = pytest.mark.gpu

SEEN = {}                                                # family -> {"cases", "enqueue_only", "early": [names], "slowest": (ms, name)} in this process


@pytest.mark.parametrize("case", poison_cases.CASES, ids=[f"{c.family}-{c.name}" for c in poison_cases.CASES])
def test_nothing_jumps_the_queue_and_an_enqueue_only_op_returns_before_the_work_in_front_of_it(case):
    inputs, snap_a, findings, info = SU.delayed_runs(case.build, case.run, case.defined, case.expect, case.enqueue_only)
    seen = SEEN.setdefault(case.family, {"cases": 0, "enqueue_only": 0, "early": [], "slowest": (0.0, "")})
    seen["cases"] += 1
    seen["enqueue_only"] += case.enqueue_only is not None
    if case.enqueue_only is None and all(info["returned_early"].values()):
        seen["early"].append(case.name)
    seen["slowest"] = max(seen["slowest"], (info["delay_ms"], case.name))
    if findings:
        pytest.fail(f"{case.name} (host {info['t_host_ms']:.1f} ms, delay {info['delay_ms']:.0f} ms): " + "; ".join(findings))
    case.expect(inputs, snap_a)


class _Kept:
    """A holder the leaf walk passes over: its tensor is neither poisoned nor restored, so the verdict that rides on it stays."""
    def __init__(self, t):
        self.t = t


@pytest.mark.parametrize("case", [c for c in poison_cases.CASES if c.covers == ("pair_reproject",)], ids=lambda c: c.name)
def test_pair_reproject_only_enqueues_on_a_table_it_has_seen(case):
    """The registry's K3 cases build a new frame table every time, and MSPA_PAIR_FAST reads a new table's pinhole verdict back.
    Here the verdict is known before the op is called, as it is for every launch but a scene's first: the same runs, held against
    the same references, now have to return while the delay in front of them is still running."""
    from mspa import engine

    def build():
        i = case.build()
        engine._require_pinhole(i["mats"])
        i["table"] = _Kept(i.pop("mats"))
        return i

    def run(i):
        return case.run({**i, "mats": i["table"].t})

    inputs, snap_a, findings, info = SU.delayed_runs(build, run, case.defined, case.expect, poison_cases.PAIR_REPROJECT_SEEN_TABLE)
    if findings:
        pytest.fail(f"{case.name} (host {info['t_host_ms']:.1f} ms, delay {info['delay_ms']:.0f} ms): " + "; ".join(findings))
    case.expect(inputs, snap_a)


# ---- the harness on itself: "ops" of a few torch calls on the test's own 37-element tensors ------------------------------------------------

N = 37
SENTENCE = "Only enqueues (a toy op of this file)."


def _build():
    return {"x": torch.arange(N, dtype=torch.int32, device="cuda") + 10, "scale": torch.full((N,), 3, dtype=torch.int32, device="cuda")}


def _expect(i, z):
    assert z["out"].tolist() == [(k + 10) * 3 for k in range(N)]


def _sound_op(i):
    out = torch.empty((N,), dtype=torch.int32, device="cuda")
    out.copy_(i["x"] * i["scale"])
    return {"out": out}


def _computes_on_the_default_stream(i):
    with torch.cuda.stream(torch.cuda.default_stream()):     # a kernel launched on stream 0: it reads what the inputs hold NOW
        return _sound_op(i)


def _on_another_stream(wait_before: bool, wait_after: bool, own_delay_ms: float = 0.0):
    def op(i):
        h = SU.harness()
        current, other = torch.cuda.current_stream(), h.second_stream()
        out = torch.zeros((N,), dtype=torch.int32, device="cuda")
        if wait_before:
            other.wait_stream(current)
        with torch.cuda.stream(other):
            if own_delay_ms:
                h.delay.enqueue(own_delay_ms)
            out.copy_(i["x"] * i["scale"])
        if wait_after:
            current.wait_stream(other)
        return {"out": out}
    return op


def _synchronises(i):
    out = _sound_op(i)
    torch.cuda.current_stream().synchronize()
    return out


def _differs(findings):
    return [f for f in findings if f.startswith("output out differs when the op runs behind a delay on a side stream")]


def _synchronised(findings):
    return [f for f in findings if "synchronised the host, though documented: " + SENTENCE in f]


def test_a_sound_op_has_no_finding_and_returns_while_the_delay_runs():
    _i, snap, findings, info = SU.delayed_runs(_build, _sound_op, expect=_expect, enqueue_only=SENTENCE)
    assert findings == [] and info["returned_early"] == {"a": True, "b": True} and info["delay_ms"] >= SU.FLOOR_MS
    _expect(None, snap)


def test_an_op_that_computes_on_the_default_stream_is_named():
    findings = SU.delayed_runs(_build, _computes_on_the_default_stream, expect=_expect)[2]
    assert len(_differs(findings)) == 1 and "first at 0" in _differs(findings)[0], findings
    assert any(f.startswith("the delayed run differs from the op's reference") for f in findings), findings


def test_an_op_on_a_stream_of_its_own_that_does_not_wait_for_the_current_one_is_named():
    findings = SU.delayed_runs(_build, _on_another_stream(wait_before=False, wait_after=True), expect=_expect)[2]
    assert len(_differs(findings)) == 1, findings


def test_an_op_that_leaves_work_on_a_stream_the_current_one_does_not_wait_for_is_named():
    """The op's own delay makes its work slower than the clone that follows: the clone was taken early."""
    findings = SU.delayed_runs(_build, _on_another_stream(wait_before=True, wait_after=False, own_delay_ms=SU.FLOOR_MS), expect=_expect)[2]
    assert len(_differs(findings)) == 1, findings


def test_an_op_that_synchronises_has_no_output_finding_but_breaks_an_enqueue_only_promise():
    _i, _snap, findings, info = SU.delayed_runs(_build, _synchronises, expect=_expect)
    assert findings == [] and info["returned_early"] == {"a": False, "b": False}
    findings = SU.delayed_runs(_build, _synchronises, expect=_expect, enqueue_only=SENTENCE)[2]
    assert len(findings) == 2 and len(_synchronised(findings)) == 2 and not _differs(findings), findings


def test_an_op_on_a_stream_of_its_own_with_both_waits_passes():
    _i, _snap, findings, info = SU.delayed_runs(_build, _on_another_stream(wait_before=True, wait_after=True), expect=_expect, enqueue_only=SENTENCE)
    assert findings == [] and info["returned_early"] == {"a": True, "b": True}


def test_summary_of_delayed_runs(capsys):
    """Last in the file: prints what the cases above ran behind (those that ran in this process)."""
    h = SU.harness()
    cases = poison_cases.CASES
    with capsys.disabled():
        print(f"\nstream order: {len(cases)} cases, {sum(c.enqueue_only is not None for c in cases)} documented as enqueue-only; test stream "
              f"{h.role!r} (tried {len(h.tried)}), delay floor {SU.FLOOR_MS:.0f} ms (measured: {SU.MEASURED_FLOOR_MS} ms), {h.delay.describe()}; per family, of the cases run in this "
              "process: " + "; ".join(f"{fam}: {s['cases']} cases, {s['enqueue_only']} enqueue-only, returned early without a promise: "
                                      f"{', '.join(s['early']) or 'none'}, longest delay {s['slowest'][0]:.0f} ms ({s['slowest'][1]})"
                                      for fam, s in SEEN.items()))
    assert len({c.name for c in cases}) == len(cases)
    assert 0 < sum(c.enqueue_only is not None for c in cases) < len(cases)
