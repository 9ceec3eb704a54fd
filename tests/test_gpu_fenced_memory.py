"""Every device op between fences (tests/fence_util.py, tests/poison_cases.py): each case runs once plainly -- the reference run,
held against the op's plain reference -- and twice with every input re-homed between two fences and every allocation of the
package fenced, the fences filled with poison "a" and with poison "b".  Then, together:

  * no fence is damaged -- a store before or behind an input, an output, a workspace, a status array;
  * no input has changed, except those the op is documented to write (``Case.writes``);
  * the three results are bit-identical wherever the op's documents specify them -- whether the bytes beyond an input's end are
    poison "a", poison "b" or whatever the allocator held: a dword or int4 load whose tail is not masked shows here;
  * the fenced run equals the op's reference as well.

The fences are the harness's own memory and their fills are small: a stray access of one element, one row or one tile lands in
them and shows as a wrong byte or a wrong number, never as a GPU fault."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poison_cases  # noqa: E402
from fence_util import MODES, fenced_allocations, fenced_copy  # noqa: E402
from poison_util import compare_runs  # noqa: E402
from test_fence_util_cpu import ZERO_LENGTH_PATHS  # noqa: E402

pytestmark = pytest.mark.gpu

SEEN = {}                                                # family -> [cases run, fenced allocations, fenced inputs] in this process


def fenced_runs(build, run, writes=(), defined=None, expect=None):
    """The plain run (held against ``expect`` before anything is fenced: the case is sound on this machine) and the two fenced
    ones of an op -> (fenced inputs and result of mode "a", findings: a list of sentences, the fences: inputs', allocations', per mode)."""
    inputs = build()
    torch.cuda.synchronize()
    plain = run(inputs)
    torch.cuda.synchronize()
    if expect is not None:
        expect(inputs, plain)
    findings, runs, homes, all_fences = [], {}, {}, []
    for mode in MODES:
        homes[mode], on_inputs, _snapshot = fenced_copy(build(), mode)
        with fenced_allocations(mode) as fences:
            runs[mode] = run(homes[mode])
            torch.cuda.synchronize()
        for site, dtype, shape, side, distance, n_bytes in on_inputs.check_fences() + fences.check_fences():
            findings.append(f"mode {mode}: fence damaged {side} {str(dtype)[6:]} {list(shape)} of [{site}]: {n_bytes} bytes, the nearest "
                            f"{distance} bytes from the payload")
        for path, first, n_bytes in on_inputs.changed_inputs(writes):
            findings.append(f"mode {mode}: input {path} was written: {n_bytes} bytes differ, the first at byte {first}")
        all_fences += [on_inputs, fences]
    for path, at in compare_runs(plain, runs["a"], runs["b"], defined):
        findings.append(f"output {path} depends on the fences (plain run, fence a, fence b differ), first at {at}")
    return homes["a"], runs["a"], findings, all_fences


@pytest.mark.parametrize("case", poison_cases.CASES, ids=[f"{c.family}-{c.name}" for c in poison_cases.CASES])
def test_nothing_is_written_outside_a_buffer_and_nothing_beyond_an_input_reaches_the_result(case):
    fenced_inputs, run_a, findings, fences = fenced_runs(case.build, case.run, case.writes, case.defined, case.expect)
    seen = SEEN.setdefault(case.family, [0, 0, 0])
    seen[0] += 1
    seen[1] += sum(len(f) for f in fences[1::2])
    seen[2] += sum(len(f) for f in fences[0::2])
    for function, where in ZERO_LENGTH_PATHS.items():        # the early returns this case is named for: it did take them
        if where == case.name:
            sites = [s for f in fences[1::2] for s in f.empty_sites]
            if not any(s.endswith(" " + function) for s in sites):
                findings.append(f"no zero-length allocation of {function} was seen (zero-length ones: {sorted(set(sites))})")
    if findings:
        try:
            case.expect(fenced_inputs, run_a)
            clean = "the fenced run equals the reference"
        except AssertionError as e:
            clean = f"the fenced run differs from the reference as well: {e!r}"
        pytest.fail(f"{case.name}: " + "; ".join(findings) + f"; {clean}")
    case.expect(fenced_inputs, run_a)


# ---- the harness on itself: an "op" of torch calls whose three stray accesses all lie inside the harness's own flat buffers ----------------

N = 37


def _build():
    return {"x": torch.arange(N, dtype=torch.int32, device="cuda") + 10, "scale": torch.full((N,), 3, dtype=torch.int32, device="cuda")}


def _sound_op(i):
    out = torch.empty((N,), dtype=torch.int32, device="cuda")
    out.copy_(i["x"] * i["scale"])
    return {"out": out}


def _writes_one_past_the_end(i):
    out = torch.zeros((N,), dtype=torch.int32, device="cuda")
    out.copy_(i["x"] * i["scale"])
    if out.storage_offset():                                 # fenced: one element longer is the back fence's first
        out.as_strided((N + 1,), (1,))[N] = -7
    return {"out": out}


def _writes_one_before_the_start(i):
    out = torch.zeros((N,), dtype=torch.int32, device="cuda")
    out.copy_(i["x"] * i["scale"])
    if out.storage_offset():                                 # fenced: one element early is the front fence's last
        out.as_strided((1,), (1,), out.storage_offset() - 1)[0] = -7
    return {"out": out}


def _reads_one_past_an_input(i):
    out = torch.empty((N,), dtype=torch.int32, device="cuda")
    out.copy_(i["x"] * i["scale"])
    if i["x"].storage_offset():                              # fenced: the element behind the input's last is the fence's
        out[N - 1] += i["x"].as_strided((1,), (1,), i["x"].storage_offset() + N)[0]
    return {"out": out}


def _writes_an_input(i):
    out = torch.empty((N,), dtype=torch.int32, device="cuda")
    out.copy_(i["x"] * i["scale"])
    i["scale"][5] = 4
    return {"out": out}


def test_the_harness_names_a_write_past_the_end_a_write_before_the_start_a_read_past_an_input_and_a_written_input():
    assert fenced_runs(_build, _sound_op)[2] == []
    found = fenced_runs(_build, _writes_one_past_the_end)[2]
    assert len(found) == 2 and all("fence damaged after int32 [37]" in f and "_writes_one_past_the_end" in f and "the nearest 0 bytes" in f
                                   and ": 4 bytes" in f for f in found), found
    found = fenced_runs(_build, _writes_one_before_the_start)[2]
    assert len(found) == 2 and all("fence damaged before int32 [37]" in f and "_writes_one_before_the_start" in f and "the nearest 0 bytes" in f
                                   for f in found), found
    found = fenced_runs(_build, _reads_one_past_an_input)[2]
    assert found == [f"output out depends on the fences (plain run, fence a, fence b differ), first at {N - 1}"], found
    found = fenced_runs(_build, _writes_an_input)[2]
    assert len(found) == 2 and all("input scale was written: 1 bytes differ, the first at byte 20" in f for f in found), found
    assert fenced_runs(_build, _writes_an_input, writes=("scale",))[2] == []


def test_a_stray_store_of_the_fill_itself_hides_in_one_mode_and_shows_in_the_other():
    def stores_a_one(i):
        out = torch.zeros((N,), dtype=torch.int32, device="cuda")
        if out.storage_offset():
            out.as_strided((N + 1,), (1,))[N] = 1             # the int32 fill of mode "a"
        return {"out": out}
    found = fenced_runs(_build, stores_a_one)[2]
    assert len(found) == 1 and found[0].startswith("mode b: fence damaged after"), found


def test_summary_of_fenced_allocations_and_documented_writes(capsys):
    """Last in the file: prints what the cases above fenced (those that ran in this process)."""
    cases = poison_cases.CASES
    writes = [(c.name, path) for c in cases for path in c.writes]
    with capsys.disabled():
        print(f"\nfenced memory: {len(cases)} cases; fenced allocations (both modes) per family, of the cases run in this process: "
              + ", ".join(f"{fam}: {n_alloc} allocations and {n_in} inputs in {n} cases" for fam, (n, n_alloc, n_in) in SEEN.items())
              + f"; total {sum(v[1] for v in SEEN.values())} allocations, {sum(v[2] for v in SEEN.values())} inputs"
              + "; documented writes: " + (", ".join(f"{n}:{p}" for n, p in writes) or "none"))
    assert len({c.name for c in cases}) == len(cases)
    assert len({c.name for c in cases if c.writes}) < len([c for c in cases if not c.writes])
