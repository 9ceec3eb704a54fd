"""Every device op on poisoned memory (tests/poison_util.py, tests/poison_cases.py): each case runs three times -- with every
``torch.empty`` / ``empty_like`` / ``new_empty`` filled with zeros, with poison "a" and with poison "b" -- and the three results
must be bit-identical wherever the op's documents specify them; the zero run must also equal the op's plain reference.  A
difference means a kernel read, or left for a reader, memory that nothing had written: in a long-running process the caching
allocator hands such memory over still holding the previous scene's data."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poison_cases  # noqa: E402
from poison_util import MODES, compare_runs, poisoned_allocations  # noqa: E402

pytestmark = pytest.mark.gpu


def test_masked_outputs_are_few_and_named(capsys):
    masked = [(c.name, path) for c in poison_cases.CASES for path in (c.defined or {})]
    with capsys.disabled():
        print(f"\npoisoned memory: {len(poison_cases.CASES)} cases, {len(masked)} outputs carry a defined-mask: "
              + ", ".join(f"{n}:{p}" for n, p in masked))
    assert len({c.name for c in poison_cases.CASES}) == len(poison_cases.CASES)
    assert len(masked) < len(poison_cases.CASES)


@pytest.mark.parametrize("case", poison_cases.CASES, ids=[f"{c.family}-{c.name}" for c in poison_cases.CASES])
def test_result_does_not_depend_on_what_the_allocator_handed_over(case):
    inputs = case.build()                                   # outside the patch: inputs are never poisoned
    torch.cuda.synchronize()
    runs = {}
    for mode in MODES:
        with poisoned_allocations(mode):
            runs[mode] = case.run(inputs)
            torch.cuda.synchronize()
    different = compare_runs(runs["zero"], runs["a"], runs["b"], case.defined)
    if different:                                           # say both things at once: what differs, and whether the clean run is right
        try:
            case.expect(inputs, runs["zero"])
            clean = "the zero run equals the reference"
        except AssertionError as e:
            clean = f"the zero run differs from the reference as well: {e!r}"
        pytest.fail(f"{case.name}: outputs (path, first differing index) that depend on unwritten memory: {different}; {clean}")
    case.expect(inputs, runs["zero"])
