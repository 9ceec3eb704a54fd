"""Every device op on buffers at their least documented alignment (tests/skew_util.py, tests/poison_cases.py): each case runs once
plainly -- the reference run, held against the op's plain reference -- and twice with every tensor its CALLER owns re-homed between
two fences one ("a") and three ("b") units past a 512-byte boundary: the inputs, and whatever the case allocates itself
(``poison_cases.own``: ``out=`` buffers, status arrays, a workspace).  The unit is the element's size, or the alignment the
documents demand for that argument (``Case.aligned``, each entry with its sentence).  What ``mspa/*.py`` allocates is fenced and
stays where the allocator puts it.  Then, together:

  * every re-homed tensor did start at ``unit`` mod ``2 * unit`` (asserted before the op sees it);
  * no fence is damaged -- a 32-bit store that covers bytes in front of an output shows here;
  * no input has changed, except those the op is documented to write (``Case.writes``);
  * the three results are bit-identical wherever the op's documents specify them: an aligned-down read of an input's first word
    reads the front fence, poison "a" or "b", and a route taken for an address must give what the aligned route gives;
  * the run of mode "a" equals the op's reference as well.

And for every entry of ``Case.aligned`` one more call with that ONE argument at A / 2 past a boundary and everything else where the
allocator puts it: it is refused (``MspaError`` MSPA_EINVAL, or the wrapper's ``ValueError``), no fence is damaged, no input has
changed and every buffer of the caller's still holds its fill -- nothing was enqueued.

The fences are the harness's own memory: a stray access of a word or a row lands in them and shows as a wrong byte or a wrong
number, never as a GPU fault.  Every wide access to a caller's pointer that these runs reach was read beforehand."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poison_cases  # noqa: E402
from mspa import _lib  # noqa: E402
from poison_util import compare_runs  # noqa: E402
from skew_util import MODES, assert_skewed, refusal_copy, skewed_allocations, skewed_copy  # noqa: E402

pytestmark = pytest.mark.gpu

SEEN = {}                                                # family -> [cases run, re-homed inputs, skewed caller allocations, fenced allocations]


def skewed_runs(build, run, writes=(), defined=None, expect=None, aligned=None):
    """The plain run (held against ``expect`` before anything moves) and the two skewed ones of an op -> (skewed inputs and result
    of mode "a", findings: a list of sentences, [inputs' handle, allocations' fences] per mode)."""
    inputs = build()
    torch.cuda.synchronize()
    plain = run(inputs)
    torch.cuda.synchronize()
    if expect is not None:
        expect(inputs, plain)
    findings, runs, homes, handles = [], {}, {}, []
    for mode in MODES:
        homes[mode], on_inputs, _snapshot = skewed_copy(build(), mode, aligned)
        assert_skewed(on_inputs)                         # (the caller's allocations are asserted where they are made)
        with skewed_allocations(mode, aligned) as fences:
            runs[mode] = run(homes[mode])
            torch.cuda.synchronize()
        for site, dtype, shape, side, distance, n_bytes in on_inputs.check_fences() + fences.check_fences():
            findings.append(f"mode {mode}: fence damaged {side} {str(dtype)[6:]} {list(shape)} of [{site}]: {n_bytes} bytes, the nearest "
                            f"{distance} bytes from the payload")
        for path, first, n_bytes in on_inputs.changed_inputs(writes):
            findings.append(f"mode {mode}: input {path} was written: {n_bytes} bytes differ, the first at byte {first}")
        handles += [on_inputs, fences]
    for path, at in compare_runs(plain, runs["a"], runs["b"], defined):
        findings.append(f"output {path} depends on where its buffers start or on the bytes in front of them (plain run, skew a, skew b differ), "
                        f"first at {at}")
    return homes["a"], runs["a"], findings, handles


@pytest.mark.parametrize("case", poison_cases.CASES, ids=[f"{c.family}-{c.name}" for c in poison_cases.CASES])
def test_the_result_is_the_same_bits_wherever_the_callers_buffers_start(case):
    skewed_inputs, run_a, findings, handles = skewed_runs(case.build, case.run, case.writes, case.defined, case.expect, case.aligned)
    seen = SEEN.setdefault(case.family, [0, 0, 0, 0])
    seen[0] += 1
    seen[1] += sum(len(h) for h in handles[0::2])
    seen[2] += sum(len(h.skewed()) for h in handles[1::2])
    seen[3] += sum(len(h) for h in handles[1::2])
    for name in case.own_buffers:                            # the buffers the case says it owns: it did allocate them, through ``own``
        if not all(name in h.named for h in handles[1::2]):
            findings.append(f"no buffer named {name!r} was allocated through own()")
    if findings:
        try:
            case.expect(skewed_inputs, run_a)
            clean = "the skewed run equals the reference"
        except AssertionError as e:
            clean = f"the skewed run differs from the reference as well: {e!r}"
        pytest.fail(f"{case.name}: " + "; ".join(findings) + f"; {clean}")
    case.expect(skewed_inputs, run_a)


REFUSALS = [(c, path) for c in poison_cases.CASES for path in (c.aligned or {})]


@pytest.mark.parametrize("case,path", REFUSALS, ids=[f"{c.family}-{c.name}-{path.replace('/', '.')}" for c, path in REFUSALS])
def test_an_argument_below_its_documented_alignment_is_refused_before_anything_is_enqueued(case, path):
    A, sentence = case.aligned[path]
    inputs, on_inputs, moved = refusal_copy(case.build(), case.aligned, path)
    assert moved >= 1 or path.startswith("own/"), f"{case.name}: no input under {path!r}"
    torch.cuda.synchronize()
    with skewed_allocations("a", case.aligned, misplace=path) as fences:
        with pytest.raises((_lib.MspaError, ValueError)) as refused:
            case.run(inputs)
        torch.cuda.synchronize()
    if isinstance(refused.value, _lib.MspaError):
        assert refused.value.code == _lib.MSPA_EINVAL, refused.value
    assert case.refused_by is None or case.refused_by in str(refused.value), refused.value       # the entry point the case means to reach
    if path.startswith("own/"):
        placed = fences.named.get(path[4:], [])
        assert placed and all(t.data_ptr() % A == A // 2 for t in placed), f"{case.name}: {path} was not where the refusal run puts it"
    assert on_inputs.check_fences() + fences.check_fences() == [], f"a fence was damaged although the call was refused ({sentence})"
    assert on_inputs.changed_inputs() == [] and fences.written() == [], f"something was written although the call was refused ({sentence})"


# ---- the harness on itself: "ops" of torch calls whose stray accesses all lie inside the harness's own flat buffers ------------------------

N = 37


def _build():
    return {"x": torch.arange(N, dtype=torch.int32, device="cuda") + 10, "scale": torch.full((N,), 3, dtype=torch.int32, device="cuda")}


def _sound_op(i):
    out = torch.empty((N,), dtype=torch.int32, device="cuda")
    out.copy_(i["x"] * i["scale"])
    return {"out": out}


def _wrong_on_the_odd_branch(i):
    """A route on the address: the "wide" one where x is 16-byte aligned, an "element" one elsewhere that drops the last element."""
    out = torch.zeros((N,), dtype=torch.int32, device="cuda")
    if i["x"].data_ptr() % 16 == 0:
        out.copy_(i["x"] * i["scale"])
    else:
        out[:N - 1].copy_(i["x"][:N - 1] * i["scale"][:N - 1])
    return {"out": out}


def _folds_in_the_element_in_front(i):
    """What a load from the address rounded down does when the bytes it should not use are not masked out."""
    out = torch.empty((N,), dtype=torch.int32, device="cuda")
    out.copy_(i["x"] * i["scale"])
    if i["x"].storage_offset():                              # re-homed: the element in front of the input's first is the fence's
        out[0] += i["x"].as_strided((1,), (1,), i["x"].storage_offset() - 1)[0]
    return {"out": out}


def _stores_a_word_over_the_front(i):
    """What a 64-bit store at the address rounded down to 8 does to an int32 output at 4 mod 8."""
    out = torch.empty((N,), dtype=torch.int32, device="cuda")
    out.copy_(i["x"] * i["scale"])
    if out.storage_offset() and out.data_ptr() % 8:
        out.as_strided((1,), (1,), out.storage_offset() - 1)[0] = -7
    return {"out": out}


def test_the_harness_passes_a_sound_op_and_names_a_wrong_route_a_read_in_front_of_an_input_and_a_store_in_front_of_an_output():
    assert skewed_runs(_build, _sound_op)[2] == []
    found = skewed_runs(_build, _wrong_on_the_odd_branch)[2]
    assert found == [f"output out depends on where its buffers start or on the bytes in front of them (plain run, skew a, skew b differ), "
                     f"first at {N - 1}"], found
    found = skewed_runs(_build, _folds_in_the_element_in_front)[2]
    assert len(found) == 1 and found[0].endswith("first at 0") and found[0].startswith("output out depends"), found
    found = skewed_runs(_build, _stores_a_word_over_the_front)[2]
    assert len(found) == 2 and all("fence damaged before int32 [37]" in f and "_stores_a_word_over_the_front" in f and "the nearest 0 bytes" in f
                                   for f in found), found


def test_the_harness_puts_inputs_and_the_callers_allocations_where_it_says_and_leaves_the_packages_alone():
    aligned = {"x": (256, "two hundred and fifty-six"), "own/slot": (16, "sixteen")}
    for mode in MODES:
        copy, handle, _ = skewed_copy(_build(), mode, aligned)
        assert copy["x"].data_ptr() % 512 == 256 and copy["scale"].data_ptr() % 512 == {"a": 4, "b": 12}[mode] and assert_skewed(handle) == 2
        with skewed_allocations(mode, aligned) as fences:
            mine = torch.empty((N,), dtype=torch.int16, device="cuda")
            slot = poison_cases.own("slot", (3, 5), torch.float64)
            theirs = poison_cases.engine.all_pairs(5, "cuda")                   # allocates inside the package (or not at all)
        assert mine.data_ptr() % 512 == {"a": 2, "b": 6}[mode] and slot.data_ptr() % 32 == 16 and theirs.data_ptr() % 256 == 0
        assert len(fences.skewed()) == 2 and fences.check_fences() + handle.check_fences() == []
    copy, handle, moved = refusal_copy(_build(), aligned, "x")
    assert moved == 1 and copy["x"].data_ptr() % 256 == 128 and copy["scale"].data_ptr() % 512 == 0


def test_summary_of_skewed_runs(capsys):
    """Last in the file: prints what the cases above moved (those that ran in this process)."""
    cases = poison_cases.CASES
    with capsys.disabled():
        print(f"\nskewed memory: {len(cases)} cases, {len(MODES)} modes, {len(REFUSALS)} refusals; per family, of the cases run in this process: "
              + ", ".join(f"{fam}: {n} cases, {n_in} re-homed inputs, {n_own} skewed buffers of the caller's among {n_alloc} fenced allocations"
                          for fam, (n, n_in, n_own, n_alloc) in SEEN.items())
              + f"; total {sum(v[1] + v[2] for v in SEEN.values())} re-homed tensors")
    assert len({c.name for c in cases}) == len(cases) and len(REFUSALS) >= 10
