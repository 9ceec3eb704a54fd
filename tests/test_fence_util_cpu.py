"""tests/fence_util.py on host tensors (``devices=("cpu",)``): what each patched factory returns, what a stray write looks like in
``check_fences``, what ``fenced_copy`` keeps and reports, the restore; and the completeness of tests/poison_cases.py over every
``mspa.engine`` function that allocates through any of the patched factories, early returns of zero-length tensors included.
No GPU."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fence_util as FU  # noqa: E402

CPU = ("cpu",)


def raw(t):
    return t.contiguous().reshape(-1).view(torch.uint8).numpy()


def factories_state():
    return tuple((getattr(owner, name), name in vars(owner)) for owner, name in FU.FACTORIES)


# ---- the payload is what the real factory returns ------------------------------------------------------------------------------------------

def make_all():
    like = torch.arange(15, dtype=torch.int16).reshape(3, 5)
    return {"empty": torch.empty((3, 5), dtype=torch.int32), "empty_like": torch.empty_like(like), "new_empty": like.new_empty((4,)),
            "zeros": torch.zeros((3, 5), dtype=torch.float64), "zeros_like": torch.zeros_like(like), "new_zeros": like.new_zeros((2, 3)),
            "full": torch.full((7,), -3, dtype=torch.int64), "full_f": torch.full((2, 2), 2.5), "full_like": torch.full_like(like, 9),
            "ones": torch.ones((5,), dtype=torch.uint8), "bool": torch.full((9,), True, dtype=torch.bool),
            "int8": torch.full((9,), -2, dtype=torch.int8), "scalar": torch.zeros((), dtype=torch.bool),
            "none": torch.zeros((0, 3), dtype=torch.int64), "none_e": torch.empty((0,), dtype=torch.uint8),
            "transposed_like": torch.zeros_like(like.t())}


@pytest.mark.parametrize("mode", FU.MODES)
def test_every_factory_returns_what_the_real_one_returns_between_two_clean_fences(mode):
    want = make_all()
    with FU.fenced_allocations(mode, devices=CPU) as fences:
        got = make_all()
        assert fences.check_fences() == []
    assert list(got) == list(want)
    for name, w in want.items():
        g = got[name]
        assert g.dtype == w.dtype and g.shape == w.shape and g.stride() == w.stride() and g.is_contiguous() == w.is_contiguous(), name
        if not name.startswith(("empty", "new_empty")):
            assert np.array_equal(raw(g), raw(w)), name                      # byte patterns: True is 1, -2 is 0xFE
        if g.numel():
            assert g.storage_offset() * g.element_size() % FU.ALIGN == 0, name  # the payload starts on a multiple of 512 bytes
        else:
            assert g.storage_offset() == 0, name                             # 0 elements: passed through
    assert not got["zeros"].any() and (got["full"] == -3).all() and (got["full_f"] == 2.5).all() and raw(got["bool"]).tolist() == [1] * 9
    assert raw(got["int8"]).tolist() == [0xFE] * 9
    n_fenced = sum(1 for t in want.values() if t.numel())
    assert len(fences) == n_fenced and len(fences.empty_sites) == 2
    assert all(site.startswith("test_fence_util_cpu.py:") and site.endswith(" make_all") for site, *_ in fences.records)


def test_host_tensors_pass_through_when_only_the_gpu_is_watched():
    with FU.fenced_allocations("a") as fences:               # devices=("cuda",): the default
        t = torch.zeros((5,), dtype=torch.int32)
    assert t.storage_offset() == 0 and len(fences) == 0


def test_the_fence_width_and_the_fill():
    assert [FU.fence_width(n) for n in (1, 4096, 4097, 5000, (1 << 20) - 1, 1 << 20, 50 << 20)] == \
        [4096, 4096, 4608, 5120, 1 << 20, 1 << 20, 1 << 20]
    for mode, (i32, byte) in (("a", (1, 0x5A)), ("b", (2, 0xA5))):
        with FU.fenced_allocations(mode, devices=CPU) as fences:
            torch.zeros((10,), dtype=torch.int32)
            torch.zeros((3,), dtype=torch.bool)
            torch.zeros((3,), dtype=torch.float64)
        (_s, _d, _sh, buf, width, nbytes), (_s2, _d2, _sh2, buf2, width2, nbytes2), (_s3, _d3, _sh3, buf3, width3, nbytes3) = fences.records
        assert width == 4096 and nbytes == 40 and buf.numel() == 2 * 4096 + 40           # the back fence begins at the payload's next byte
        assert buf[:width].view(torch.int32).tolist() == [i32] * 1024 and buf[width + nbytes:].view(torch.int32).tolist() == [i32] * 1024
        assert nbytes2 == 3 and buf2[width2 + 3:].tolist() == [byte] * 4096 and buf2[:width2].tolist() == [byte] * 4096
        back = buf3[width3 + nbytes3:].view(torch.float64)
        assert bool(torch.isnan(back).all()) if mode == "a" else (back == 1.5).all()
    with pytest.raises(ValueError):
        with FU.fenced_allocations("zero", devices=CPU):
            pass


# ---- writes --------------------------------------------------------------------------------------------------------------------------------

def test_stray_writes_are_found_and_named_and_sound_ones_are_not():
    with FU.fenced_allocations("b", devices=CPU) as fences:
        clean = torch.empty((37,), dtype=torch.int32)
        clean[:] = 5                                                         # in bounds, first to last
        past = torch.zeros((3, 5), dtype=torch.int16)
        past.as_strided((16,), (1,))[15] = 7                                 # one element past the end
        early = torch.full((11,), 0.5, dtype=torch.float64)
        early.as_strided((1,), (1,), early.storage_offset() - 1)[0] = -0.25  # one element before the start
        far = torch.empty((100,), dtype=torch.uint8)
        far.as_strided((1,), (1,), far.storage_offset() + 100 + 3 * 1024)[0] = 0   # 3 KiB past the end: still inside the 4 KiB fence
        found = fences.check_fences()
    assert len(fences) == 4
    here = "test_fence_util_cpu.py:"
    assert [(f[0][:len(here)], f[0].split()[-1]) + f[1:] for f in found] == [
        (here, "test_stray_writes_are_found_and_named_and_sound_ones_are_not", torch.int16, (3, 5), "after", 0, 1),      # 7, 0: one byte differs from 2, 0
        (here, "test_stray_writes_are_found_and_named_and_sound_ones_are_not", torch.float64, (11,), "before", 0, 2),    # -0.25 against 1.5: two bytes
        (here, "test_stray_writes_are_found_and_named_and_sound_ones_are_not", torch.uint8, (100,), "after", 3072, 1)]
    assert fences.check_fences() == found                                    # checking changes nothing


def test_a_stray_store_of_the_fill_hides_in_its_own_mode_only():
    found = {}
    for mode in FU.MODES:
        with FU.fenced_allocations(mode, devices=CPU) as fences:
            status = torch.zeros((8,), dtype=torch.int32)
            status.as_strided((9,), (1,))[8] = 1                             # status[n] of a status array of n
        found[mode] = fences.check_fences()
    assert found["a"] == [] and [f[3:] for f in found["b"]] == [("after", 0, 1)]


def test_the_call_site_is_the_first_frame_inside_the_package():
    from mspa import engine
    source, first = inspect.getsourcelines(engine._workspace)
    with FU.fenced_allocations("a", devices=CPU) as fences:
        ws = engine._workspace(100, "cpu")
    assert ws.dtype == torch.uint8 and ws.numel() == 112 and ws.data_ptr() % 16 == 0
    (site, dtype, shape, _buf, width, nbytes), = fences.records
    assert site.startswith(os.path.join("multi-spatialmllm_amd", "mspa", "engine.py") + ":") and site.endswith(" _workspace")
    assert first <= int(site.split(":")[1].split()[0]) < first + len(source) and (dtype, shape, nbytes, width) == (torch.int64, (14,), 112, 4096)


# ---- fenced_copy -----------------------------------------------------------------------------------------------------------------------------

def some_inputs():
    soa = torch.arange(30, dtype=torch.float64).reshape(3, 10).t()          # [10, 3] with strides (1, 10): xyz_soa's layout
    shared = torch.arange(6, dtype=torch.int32)
    return {"soa": soa, "pair": (shared, [shared, torch.zeros((0,), dtype=torch.int64)]), "n": 5, "text": "x", "array": np.arange(3),
            "row": torch.arange(40, dtype=torch.int16).reshape(4, 10)[1:3, 2:7], "nothing": None}


def test_fenced_copy_keeps_values_shapes_strides_and_everything_else():
    inputs = some_inputs()
    copy, handle, snapshot = FU.fenced_copy(inputs, "a", devices=CPU)
    assert list(copy) == list(inputs) and copy["n"] == 5 and copy["text"] == "x" and copy["array"] is inputs["array"] and copy["nothing"] is None
    assert isinstance(copy["pair"], tuple) and isinstance(copy["pair"][1], list) and copy["pair"][1][1] is inputs["pair"][1][1]   # 0 elements
    for got, want in ((copy["soa"], inputs["soa"]), (copy["pair"][0], inputs["pair"][0]), (copy["row"], inputs["row"])):
        assert got is not want and got.dtype == want.dtype and got.shape == want.shape and got.stride() == want.stride() and torch.equal(got, want)
        assert got.data_ptr() != want.data_ptr() and got.storage_offset() * got.element_size() % FU.ALIGN == 0
    assert copy["pair"][0] is copy["pair"][1][0]                             # one tensor met twice: re-homed once
    assert sorted(snapshot) == ["pair/0", "pair/1/0", "row", "soa"] and len(handle) == 3
    assert handle.records[[r[0] for r in handle.records].index("input row")][5] == 2 * (10 + 5)      # the span of rows 1..2, columns 2..6
    assert handle.check_fences() == [] and handle.changed_inputs() == []
    assert not any(t is c for t, c in ((inputs["soa"], copy["soa"]), (inputs["row"], copy["row"])))
    inputs["soa"][0, 0] = -1.0                                               # the original is another tensor
    assert copy["soa"][0, 0] == 0.0


def test_a_written_input_is_reported_by_its_path_unless_it_is_listed_and_a_write_behind_it_damages_its_fence():
    copy, handle, _snapshot = FU.fenced_copy(some_inputs(), "b", devices=CPU)
    copy["soa"][9, 2] = 0.5                                                  # the last element of the span
    copy["pair"][0][1] = 77
    differ = np.nonzero(np.array([29.0]).view(np.uint8) != np.array([0.5]).view(np.uint8))[0]
    soa = ("soa", 29 * 8 + int(differ[0]), len(differ))                     # element [9, 2] lies 9 * 1 + 2 * 10 elements into the span
    assert handle.changed_inputs() == [soa, ("pair/0", 4, 1), ("pair/1/0", 4, 1)]
    assert handle.changed_inputs(writes=("pair",)) == [soa]
    assert handle.changed_inputs(writes=("soa", "pair/0", "pair/1")) == []
    with pytest.raises(KeyError):
        handle.changed_inputs(writes=("sao",))
    assert handle.check_fences() == []
    row = copy["row"]
    row.as_strided((1,), (1,), row.storage_offset() + 15)[0] = 9             # one element behind the span
    assert [(f[0], f[3], f[4]) for f in handle.check_fences()] == [("input row", "after", 0)]


# ---- restore -----------------------------------------------------------------------------------------------------------------------------------

def test_the_factories_are_the_originals_after_exit_and_after_an_exception():
    before = factories_state()
    assert [own for _f, own in before[-2:]] == ["new_empty" in vars(torch.Tensor), "new_zeros" in vars(torch.Tensor)]
    with FU.fenced_allocations("a", devices=CPU):
        assert all(now is not was for (now, _), (was, _) in zip(factories_state(), before))
    assert factories_state() == before
    with pytest.raises(RuntimeError, match="inside"):
        with FU.fenced_allocations("b", devices=CPU):
            raise RuntimeError("inside")
    assert factories_state() == before
    with pytest.raises(ValueError):
        with FU.fenced_allocations("c", devices=CPU):
            pass
    assert factories_state() == before
    assert torch.zeros(3).new_zeros((2,)).storage_offset() == 0 and torch.zeros(3).new_empty((2,)).shape == (2,)


def test_the_fence_patch_and_the_poison_patch_nest_and_unwind():
    import poison_util as PU
    before = factories_state()
    with PU.poisoned_allocations("a"):
        with FU.fenced_allocations("b", devices=CPU) as fences:
            t = torch.empty((4,), dtype=torch.int32)
        assert t.tolist() == [1] * 4 and t.storage_offset() and fences.check_fences() == []      # the payload: the poisoned tensor's bytes
    assert factories_state() == before


# ---- completeness: every engine function that allocates through ANY patched factory has a case, or a reason --------------------------------

FACTORY_CALL = r"(?:torch\.(?:empty|empty_like|zeros|zeros_like|full|full_like|ones)|\.new_empty|\.new_zeros)\s*\("
ALLOCATES = re.compile(FACTORY_CALL)
ZERO_LENGTH = re.compile(FACTORY_CALL + r"\(\s*0\s*[,)]")                  # torch.zeros((0,), ...), torch.empty((0, n), ...)
CALLS = re.compile(r"(?<![\w.])([A-Za-z_]\w*)\s*\(")

# Public functions of mspa.engine that reach a patched factory and have no case, each with its reason (tests/poison_cases.py's
# NOT_COVERED holds the two the narrower collector of tests/test_poison_util_cpu.py finds; they are repeated, not replaced).
NOT_COVERED = {
    "alloc_pair_outputs": "a pure allocator; its consumer pair_reproject is covered with outputs allocated by it under the patch",
    "alloc_pair_correspondences": "a pure allocator; pair_correspondences calls it under the patch",
    "parse_int_lists": "a dispatcher: the host parser for device=None, else parse_int_lists_device, which is covered",
}

# Functions of mspa.engine (private ones included: the site is named by its function) that allocate a ZERO-LENGTH device tensor --
# an early return, or the empty form of an output -- and the case of tests/poison_cases.py that takes that path;
# tests/test_gpu_fenced_memory.py holds the case to it: a zero-length allocation of that function must be seen in its fenced runs.
ZERO_LENGTH_PATHS = {
    "bitset_csr": "bitset_empty",
    "_snappy_compress": "empty_batches",
    "parquet_string_pages_device": "index_text_and_pages",
    "snappy_decompress_device": "empty_batches",
    "snappy_decompress_blocks_device": "empty_batches",
    "rle_hybrid_runs_device": "rle_hybrid",
    "_spans_to_lists": "parquet_spans_to_bits_and_lists",
    "index_spans_to_lists": "empty_batches",
    "index_spans_to_bits": "parquet_spans_to_bits_and_lists",
    "parse_int_lists_device": "parse_int_lists_device",
}


def module_functions(module):
    functions = {name: f for name, f in vars(module).items() if inspect.isfunction(f) and f.__module__ == module.__name__}
    return {name: inspect.getsource(f) for name, f in functions.items()}


def allocating_public_functions(module):
    """tests/test_poison_util_cpu.py's collector over the wider factory list, and through every function of the module a function
    calls, public ones too (a public wrapper over a public op allocates as well): the public functions of ``module`` whose body, or
    a function of the module it calls, transitively, calls one of fence_util.FACTORIES."""
    source = module_functions(module)

    def allocates(name, seen):
        if name in seen:
            return False
        seen.add(name)
        if ALLOCATES.search(source[name]):
            return True
        return any(allocates(callee, seen) for callee in CALLS.findall(source[name]) if callee in source and callee != name)

    return sorted(name for name in source if not name.startswith("_") and allocates(name, set()))


def zero_length_functions(module):
    """Functions of ``module`` that call a patched factory with a shape whose first extent is the literal 0."""
    return sorted(name for name, text in module_functions(module).items() if ZERO_LENGTH.search(text))


def test_the_wider_collector_sees_every_factory_public_callees_and_zero_length_returns(tmp_path):
    import importlib.util
    path = tmp_path / "fake_engine.py"
    path.write_text("import torch\n"
                    "def _scratch(n):\n    return torch.empty((n,))\n"
                    "def _status(n):\n    return torch.zeros((n,), dtype=torch.int32)\n"
                    "def direct(n):\n    return torch.empty_like(torch.arange(n))\n"
                    "def indirect(n):\n    return _scratch(n)\n"
                    "def status_only(n):\n    return _status(n)\n"
                    "def filled(n):\n    return torch.full((n,), -1)\n"
                    "def filled_like(t):\n    return torch.full_like(t, 3), torch.zeros_like(t), torch.ones(3)\n"
                    "def methods(t):\n    return t.new_empty((3,)), t.new_zeros((3,))\n"
                    "def over_public(n):\n    return filled(n)\n"
                    "def early_out(n):\n    if n == 0:\n        return torch.zeros((0,), dtype=torch.int32)\n    return torch.arange(n)\n"
                    "def early_out_2d(n):\n    return torch.empty(( 0, n))\n"
                    "def clean(n):\n    return torch.arange(n), zeros(n), torch.zeros_(n)\n")
    spec = importlib.util.spec_from_file_location("fake_engine", path)
    fake = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fake)
    assert allocating_public_functions(fake) == ["direct", "early_out", "early_out_2d", "filled", "filled_like", "indirect", "methods",
                                                 "over_public", "status_only"]
    assert zero_length_functions(fake) == ["early_out", "early_out_2d"]
    from test_poison_util_cpu import allocating_public_functions as narrow
    assert set(narrow(fake)) < set(allocating_public_functions(fake))         # the old collector's, and more


def test_every_engine_function_that_reaches_a_patched_factory_has_a_case_or_a_reason():
    import poison_cases
    from mspa import engine
    from test_poison_util_cpu import allocating_public_functions as narrow
    allocating = allocating_public_functions(engine)
    assert set(narrow(engine)) <= set(allocating) and len(allocating) > len(narrow(engine)) > 50, allocating
    public = [name for name in module_functions(engine) if not name.startswith("_")]
    covered = {name for c in poison_cases.CASES for name in c.covers}
    assert all(hasattr(engine, name) for name in covered | set(NOT_COVERED)), "a case names a function the engine does not have"
    assert all(isinstance(r, str) and len(r.split()) >= 4 for r in NOT_COVERED.values()), "NOT_COVERED: a one-line reason each"
    assert set(poison_cases.NOT_COVERED) <= set(NOT_COVERED)
    stale = set(NOT_COVERED) - set(allocating)
    assert not stale, f"NOT_COVERED excuses functions that do not allocate (any more): {sorted(stale)}"
    both = covered & set(NOT_COVERED)
    assert not both, f"covered and excused at once: {sorted(both)}"
    missing = [name for name in allocating if name not in covered and name not in NOT_COVERED]
    assert not missing, f"mspa.engine functions that allocate device memory through a patched factory and have neither a case in tests/poison_cases.py nor a reason in NOT_COVERED: {missing}"
    # the device surface: every op with a case; what is left of the public functions is host-side code and pure allocators
    assert len(covered) >= 62 and covered <= set(public)
    for c in poison_cases.CASES:
        assert isinstance(c.writes, tuple) and all(isinstance(p, str) and p for p in c.writes), c.name


def test_every_zero_length_return_is_reached_by_a_named_case():
    import poison_cases
    from mspa import engine
    found = zero_length_functions(engine)
    assert found == sorted(ZERO_LENGTH_PATHS), f"zero-length allocations in {sorted(set(found) ^ set(ZERO_LENGTH_PATHS))}: name the case that reaches each"
    source = module_functions(engine)
    cases = {c.name: c for c in poison_cases.CASES}
    for function, name in ZERO_LENGTH_PATHS.items():
        assert name in cases, (function, name)
        reached = set(cases[name].covers)                                    # the case covers the function, or a public one that calls it
        assert function in reached or any(re.search(r"(?<![\w.])" + function + r"\s*\(", source[f]) for f in reached), (function, name)
