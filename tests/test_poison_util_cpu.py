"""tests/poison_util.py on host tensors: the patterns, the restore, the comparison's teeth (on fake ops: no kernel is broken to
show them), and the completeness of tests/poison_cases.py over ``mspa.engine``'s allocating functions.  No GPU."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poison_util as PU  # noqa: E402

I64 = {"a": 0x0000000100000001, "b": 0x0000000200000002}
TABLE = {torch.int32: {"a": 1, "b": 2}, torch.int64: I64, torch.int16: {"a": 1, "b": 2}, torch.uint8: {"a": 0x5A, "b": 0xA5},
         torch.bool: {"a": 0x5A, "b": 0xA5}, torch.float32: {"a": float("nan"), "b": 1.5}, torch.float64: {"a": float("nan"), "b": 1.5}}


def raw(t):
    return t.reshape(-1).view(torch.uint8).numpy()


def pattern(dtype, mode, n):
    """n elements of the table's value as raw bytes, written down independently of poison_util."""
    if mode == "zero":
        return np.zeros(n * torch.empty((), dtype=dtype).element_size(), dtype=np.uint8)
    v = TABLE[dtype][mode]
    np_dtype = {torch.int32: np.int32, torch.int64: np.int64, torch.int16: np.int16, torch.uint8: np.uint8, torch.bool: np.uint8,
                torch.float32: np.float32, torch.float64: np.float64}[dtype]
    return np.full(n, v, dtype=np_dtype).view(np.uint8)


@pytest.mark.parametrize("mode", PU.MODES)
@pytest.mark.parametrize("dtype", list(TABLE), ids=lambda d: str(d)[6:])
def test_every_allocator_holds_exactly_the_pattern(dtype, mode):
    like = torch.zeros((3, 5), dtype=dtype)
    with PU.poisoned_allocations(mode):
        got = [torch.empty((3, 5), dtype=dtype), torch.empty(15, dtype=dtype), torch.empty_like(like), like.new_empty((3, 5)),
               torch.empty((0,), dtype=dtype), torch.empty((4, 6), dtype=dtype).t()]
    want = pattern(dtype, mode, 15)
    for t in got[:4]:
        assert t.dtype == dtype and np.array_equal(raw(t), want)
    assert got[4].numel() == 0 and np.array_equal(raw(got[5].t()), pattern(dtype, mode, 24))
    if mode != "zero" and dtype.is_floating_point:
        assert bool(torch.isnan(got[0]).all()) == (mode == "a")


def test_poisons_differ_from_zero_and_from_each_other_in_every_element_and_int64_reads_as_int32_lanes():
    for dtype in TABLE:
        with PU.poisoned_allocations("a"):
            a = torch.empty((7,), dtype=dtype)
        with PU.poisoned_allocations("b"):
            b = torch.empty((7,), dtype=dtype)
        width = a.element_size()
        ra, rb = raw(a).reshape(7, width), raw(b).reshape(7, width)
        assert ra.any(axis=1).all() and rb.any(axis=1).all() and (ra != rb).any(axis=1).all()
    with PU.poisoned_allocations("a"):
        assert torch.empty((4,), dtype=torch.int64).view(torch.int32).tolist() == [1] * 8
    with PU.poisoned_allocations("b"):
        assert torch.empty((4,), dtype=torch.int64).view(torch.int32).tolist() == [2] * 8


def test_the_originals_are_back_after_exit_and_after_an_exception():
    before = (torch.empty, torch.empty_like, torch.Tensor.new_empty, "new_empty" in vars(torch.Tensor))
    with PU.poisoned_allocations("a"):
        assert torch.empty is not before[0] and torch.empty_like is not before[1] and torch.Tensor.new_empty is not before[2]
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty, "new_empty" in vars(torch.Tensor)) == before
    with pytest.raises(RuntimeError, match="inside"):
        with PU.poisoned_allocations("b"):
            raise RuntimeError("inside")
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty, "new_empty" in vars(torch.Tensor)) == before
    with pytest.raises(ValueError):
        with PU.poisoned_allocations("c"):
            pass
    assert torch.empty is before[0]
    assert torch.zeros(3).new_empty((2,)).shape == (2,)


def three_runs(op):
    runs = []
    for mode in PU.MODES:
        with PU.poisoned_allocations(mode):
            runs.append(op())
    return runs


N = 37


def writes_all_but_the_last():
    out = torch.empty((N,), dtype=torch.int32)
    out[:N - 1] = torch.arange(N - 1, dtype=torch.int32)
    return {"out": out, "n": N}


def test_an_unwritten_element_is_reported_at_its_index():
    assert PU.compare_runs(*three_runs(writes_all_but_the_last)) == [("out", N - 1)]


def test_a_defined_mask_takes_the_element_out():
    mask = np.arange(N) < N - 1
    for defined in ({"out": mask}, {"out": torch.from_numpy(mask)}, {"out": lambda zero: np.arange(zero["n"]) < zero["n"] - 1},
                    {"out": lambda zero: slice(0, zero["n"] - 1)}, {"out": slice(0, N - 1)}):
        assert PU.compare_runs(*three_runs(writes_all_but_the_last), defined=defined) == []
    assert PU.compare_runs(*three_runs(writes_all_but_the_last), defined={"out": np.arange(N) > 3}) == [("out", N - 1)]
    with pytest.raises(ValueError, match="whole output"):
        PU.compare_runs(*three_runs(writes_all_but_the_last), defined={"out": np.zeros(N, dtype=bool)})
    with pytest.raises(KeyError):
        PU.compare_runs(*three_runs(writes_all_but_the_last), defined={"nothing": mask})


def test_an_accumulation_into_empty_is_reported():
    x = torch.arange(12, dtype=torch.float64).reshape(3, 4)

    def accumulates():
        out = torch.empty_like(x)
        out += x
        return [out, (x.numpy().copy(), None)]

    assert PU.compare_runs(*three_runs(accumulates)) == [("0", (0, 0))]


def test_nan_compares_by_bit_pattern_and_nesting_gives_paths():
    quiet, other = np.array([np.nan, 1.0]), np.array([np.nan, 1.0])
    other.view(np.uint64)[0] ^= 1                                       # another NaN payload
    assert PU.compare_runs({"x": quiet}, {"x": quiet.copy()}, {"x": quiet.copy()}) == []
    assert PU.compare_runs({"x": quiet}, {"x": quiet.copy()}, {"x": other}) == [("x", 0)]
    z = {"a": (torch.zeros(2, 3), [np.zeros(4, dtype=np.uint8)]), "n": 5}
    b = {"a": (torch.zeros(2, 3), [np.array([0, 0, 9, 0], dtype=np.uint8)]), "n": 6}
    assert PU.compare_runs(z, z, b) == [("a/1/0", 2), ("n", None)]
    assert PU.compare_runs(z, z, {"a": (torch.zeros(2, 2), [np.zeros(4, dtype=np.uint8)]), "n": 5}) == [("a/0", ())]
    assert PU.compare_runs(torch.tensor(-0.0), torch.tensor(-0.0), torch.tensor(0.0)) == [("", ())]


# ---- completeness: every allocating public function of mspa.engine has a case, or a reason ---------------------------------------------

ALLOCATES = re.compile(r"\b(?:torch\.empty|torch\.empty_like|new_empty)\s*\(")
CALLS_PRIVATE = re.compile(r"\b(_[a-z]\w*)\s*\(")


def allocating_public_functions(module):
    """Public functions defined in ``module`` whose body -- or a private helper of the module it calls, transitively -- allocates
    through torch.empty / empty_like / new_empty."""
    functions = {name: f for name, f in vars(module).items() if inspect.isfunction(f) and f.__module__ == module.__name__}
    source = {name: inspect.getsource(f) for name, f in functions.items()}

    def allocates(name, seen):
        if name in seen:
            return False
        seen.add(name)
        if ALLOCATES.search(source[name]):
            return True
        return any(allocates(callee, seen) for callee in CALLS_PRIVATE.findall(source[name]) if callee in source and callee != name)

    return sorted(name for name in functions if not name.startswith("_") and allocates(name, set()))


def test_the_collector_sees_direct_and_indirect_allocations(tmp_path):
    import importlib.util
    path = tmp_path / "fake_engine.py"
    path.write_text("import torch\n"
                    "def _scratch(n):\n    return torch.empty((n,))\n"
                    "def _middle(n):\n    return _scratch(n)\n"
                    "def direct(n):\n    return torch.empty_like(torch.zeros(n))\n"
                    "def indirect(n):\n    return _middle(n)\n"
                    "def method(t):\n    return t.new_empty((3,))\n"
                    "def clean(n):\n    return torch.zeros(n)\n")
    spec = importlib.util.spec_from_file_location("fake_engine", path)
    fake = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fake)
    assert allocating_public_functions(fake) == ["direct", "indirect", "method"]


def test_every_allocating_engine_function_has_a_case_or_a_reason():
    import poison_cases
    from mspa import engine
    allocating = allocating_public_functions(engine)
    assert len(allocating) > 50, allocating
    covered = {name for c in poison_cases.CASES for name in c.covers}
    assert all(hasattr(engine, name) for name in covered | set(poison_cases.NOT_COVERED)), "a case names a function the engine does not have"
    assert all(isinstance(r, str) and len(r.split()) >= 4 for r in poison_cases.NOT_COVERED.values()), "NOT_COVERED: a one-line reason each"
    stale = set(poison_cases.NOT_COVERED) - set(allocating)
    assert not stale, f"NOT_COVERED excuses functions that do not allocate (any more): {sorted(stale)}"
    both = covered & set(poison_cases.NOT_COVERED)
    assert not both, f"covered and excused at once: {sorted(both)}"
    missing = [name for name in allocating if name not in covered and name not in poison_cases.NOT_COVERED]
    assert not missing, f"mspa.engine functions that allocate with torch.empty and have neither a case in tests/poison_cases.py nor a reason in NOT_COVERED: {missing}"
    assert len({c.name for c in poison_cases.CASES}) == len(poison_cases.CASES)
    for c in poison_cases.CASES:
        assert c.covers and c.family and callable(c.build) and callable(c.run) and callable(c.expect), c.name
