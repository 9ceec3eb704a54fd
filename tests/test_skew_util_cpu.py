"""tests/skew_util.py on host tensors (``devices=("cpu",)``): where a re-homed tensor starts in both modes and under a documented
alignment, what is kept, what a store one element in front looks like, who is skewed and who is not; ``rehome(..., skew=0)`` is
what it was; and tests/poison_cases.py's ``Case.aligned`` against the documents it quotes.  No GPU.

Host memory of torch's is 64-byte aligned, so addresses are held modulo 4, 8, 16, 32 and 64 here; the 512 of the device allocator
(and with it an alignment of 256) is tests/test_gpu_skewed_memory.py's."""
import importlib.util
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fence_util as FU  # noqa: E402
import poison_cases  # noqa: E402
import skew_util as SK  # noqa: E402
from test_stream_util_cpu import _folded  # noqa: E402

CPU = ("cpu",)
# every dtype of a device tensor in tests/poison_cases.py (bool and int8 ride along: one byte, like uint8)
DTYPES = (torch.uint8, torch.bool, torch.int8, torch.int16, torch.int32, torch.float32, torch.int64, torch.float64)
# mode -> element size -> {modulus: residue}: the module's table
WHERE = {"a": {1: {4: 1}, 2: {4: 2}, 4: {16: 4}, 8: {16: 8}},
         "b": {1: {4: 3}, 2: {8: 6}, 4: {16: 12}, 8: {16: 8}}}


def raw(t):
    return t.contiguous().reshape(-1).view(torch.uint8).numpy()


def _inputs():
    shared = torch.arange(12, dtype=torch.int32)
    base = torch.arange(40, dtype=torch.int16).reshape(5, 8)
    return {"per_dtype": {str(d)[6:]: (torch.arange(11) % 2).to(d) for d in DTYPES}, "shared": shared, "again": [shared, None, "text", 3],
            "view": base[1:4, 2:7], "transposed": torch.arange(6, dtype=torch.float64).reshape(2, 3).t(), "empty": torch.zeros((0,), dtype=torch.int64),
            "np": np.arange(3)}


@pytest.mark.parametrize("mode", SK.MODES)
def test_a_rehomed_tensor_starts_one_or_three_elements_past_the_boundary_and_keeps_shape_strides_and_bytes(mode):
    inputs = _inputs()
    copy, handle, snapshot = SK.skewed_copy(inputs, mode, devices=CPU)
    assert SK.assert_skewed(handle) == len(handle.tensors) == len(DTYPES) + 4            # shared is met twice: two paths, ...
    assert len(handle) == len(DTYPES) + 3 and copy["again"][0] is copy["shared"]          # ... one buffer
    for d in DTYPES:
        t, src = copy["per_dtype"][str(d)[6:]], inputs["per_dtype"][str(d)[6:]]
        size = t.element_size()
        for modulus, residue in WHERE[mode][size].items():
            assert t.data_ptr() % modulus == residue, (d, mode, t.data_ptr() % 64)
        assert t.data_ptr() % (2 * size) == size and t.data_ptr() % 64 == size * SK.UNITS_PAST[mode]
        assert t.dtype == src.dtype and t.shape == src.shape and t.stride() == src.stride() and np.array_equal(raw(t), raw(src))
    for key in ("view", "transposed"):
        t, src = copy[key], inputs[key]
        assert t.shape == src.shape and t.stride() == src.stride() and t.is_contiguous() == src.is_contiguous() and torch.equal(t, src), key
        assert np.array_equal(snapshot[key], FU._span_bytes(src)), key                    # every byte of the storage range it spans
    assert copy["empty"] is inputs["empty"] and copy["np"] is inputs["np"] and copy["again"][1:] == [None, "text", 3]
    assert handle.check_fences() == [] and handle.changed_inputs() == []
    with pytest.raises(ValueError):
        SK.skewed_copy(inputs, "zero", devices=CPU)


@pytest.mark.parametrize("mode", SK.MODES)
@pytest.mark.parametrize("A", [16, 32])
def test_a_documented_alignment_puts_the_tensor_at_A_mod_2A_in_both_modes(mode, A):
    aligned = {"per_dtype/uint8": (A, "sixteen"), "shared": (A, "as well"), "per_dtype/float64": (4, "less than its element: the element rules")}
    copy, handle, _ = SK.skewed_copy(_inputs(), mode, aligned, devices=CPU)
    for t in (copy["per_dtype"]["uint8"], copy["shared"]):
        assert t.data_ptr() % (2 * A) == A
    assert handle.units["per_dtype/uint8"] == handle.units["shared"] == handle.units["again/0"] == A
    assert handle.units["per_dtype/float64"] == 8 and copy["per_dtype"]["float64"].data_ptr() % 16 == 8
    assert copy["per_dtype"]["int16"].data_ptr() % 64 == 2 * SK.UNITS_PAST[mode]           # no entry: its element
    assert SK.assert_skewed(handle) == len(handle.tensors)
    assert SK.entry_for(aligned, "shared/0") == aligned["shared"] and SK.entry_for(aligned, "shared_too") is None


def test_the_skew_table():
    assert [SK.skew_of(s, "a") for s in (1, 2, 4, 8)] == [1, 2, 4, 8] and [SK.skew_of(s, "b") for s in (1, 2, 4, 8)] == [3, 6, 12, 24]
    assert SK.skew_of(1, "a", 256) == SK.skew_of(1, "b", 256) == 256 and SK.skew_of(2, "b", 4) == 4 and SK.skew_of(8, "b", 8) == 24
    assert SK.unit_of(2, 4) == 4 and SK.unit_of(8, 4) == 8 and SK.unit_of(1) == 1
    for bad in ((1, "a", 512), (1, "a", 24), (4, "c", 0)):
        with pytest.raises(ValueError):
            SK.skew_of(*bad)
    with pytest.raises(AssertionError):
        SK.assert_skewed([("x", torch.zeros(4, dtype=torch.int32), 4)])                 # the allocator's own: at 0 mod 64


def test_rehome_without_a_skew_is_what_it_was():
    t = torch.arange(15, dtype=torch.int16).reshape(3, 5)[:, 1:4]
    for mode in FU.MODES:
        old, new = FU.Fences(mode), FU.Fences(mode)
        a, b = old.rehome(t, "site"), new.rehome(t, "site", skew=0)
        (_s, dtype, shape, buf_a, width, nbytes), (_s2, _d, _sh, buf_b, width_b, nbytes_b) = old.records[0], new.records[0]
        assert (width, nbytes) == (width_b, nbytes_b) == (FU.MIN_FENCE, 2 * 13) and buf_a.numel() == buf_b.numel() == 2 * width + nbytes
        assert a.storage_offset() == b.storage_offset() == width // 2 and a.stride() == b.stride() == t.stride() and torch.equal(a, b)
        assert np.array_equal(buf_a.numpy(), buf_b.numpy()) and old.skews == new.skews == [0] and new.check_fences() == []
    fenced, handle, _ = FU.fenced_copy({"t": t}, "a", devices=CPU)
    assert handle.skews == [0] and fenced["t"].storage_offset() * 2 % FU.ALIGN == 0
    skewed = FU.Fences("a")
    c = skewed.rehome(t, "site", skew=6)
    assert c.storage_offset() == (FU.MIN_FENCE + 6) // 2 and skewed.records[0][3].numel() == 2 * FU.MIN_FENCE + 6 + 26 and torch.equal(c, t)
    assert skewed.check_fences() == []                                                 # the longer front fence is filled and checked whole
    for bad in (3, -2):
        with pytest.raises(ValueError):
            FU.Fences("a").rehome(t, "site", skew=bad)


def _sound_op(i, out):
    out.copy_(i["x"] * 3)


def _stores_one_element_in_front(i, out):
    out.copy_(i["x"] * 3)
    out.as_strided((1,), (1,), out.storage_offset() - 1)[0] = -7


def _stores_a_word_over_the_first_bytes(i, out):
    """What a dword store at the address rounded down to 4 does to an int16 buffer at 2 mod 4: two bytes of the fence go with it."""
    out.copy_(i["x"] * 3)
    flat = out.as_strided((out.numel() + 1,), (1,), out.storage_offset() - 1)
    flat[:2] = flat[1].item()


@pytest.mark.parametrize("mode", SK.MODES)
def test_the_fences_are_intact_after_a_sound_op_and_damaged_by_a_store_in_front(mode):
    def run(op):
        inputs, on_inputs, _ = SK.skewed_copy({"x": torch.arange(37, dtype=torch.int16)}, mode, devices=CPU)
        with SK.skewed_allocations(mode, devices=CPU) as fences:
            out = torch.empty((37,), dtype=torch.int16)
            SK.assert_skewed(fences)
            op(inputs, out)
        assert out.data_ptr() % 4 == 2 and len(fences) == 1 and [u for _n, _t, u in fences.skewed()] == [2]
        assert out.tolist() == [3 * k for k in range(37)] and on_inputs.check_fences() == [] and on_inputs.changed_inputs() == []
        return fences.check_fences()
    assert run(_sound_op) == []
    (site, dtype, shape, side, distance, n_bytes), = run(_stores_one_element_in_front)
    assert (dtype, shape, side, distance) == (torch.int16, (37,), "before", 0) and 1 <= n_bytes <= 2 and site.endswith(" run")
    (_site, _dtype, _shape, side, distance, n_bytes), = run(_stores_a_word_over_the_first_bytes)
    assert side == "before" and distance <= 1 and 1 <= n_bytes <= 2          # (the copied element is 0: under fill 1 only its low byte differs)


STUB = '''
import torch


def allocate(n):
    """What a wrapper does: its own scratch and its own output."""
    return torch.empty((n,), dtype=torch.int64).view(torch.uint8), torch.zeros((n,), dtype=torch.int16)


def allocate_through(callback, n):
    return callback(n)
'''


def test_only_what_is_allocated_outside_the_package_is_skewed(tmp_path, monkeypatch):
    package = tmp_path / "multi-spatialmllm_amd" / "mspa"
    package.mkdir(parents=True)
    (package / "stub_wrappers.py").write_text(STUB)
    spec = importlib.util.spec_from_file_location("stub_wrappers", str(package / "stub_wrappers.py"))
    stub = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(stub)
    monkeypatch.setattr(FU, "PACKAGE_DIR", str(tmp_path / "multi-spatialmllm_amd") + os.sep)
    before = tuple((getattr(owner, name), name in vars(owner)) for owner, name in FU.FACTORIES)
    aligned = {"own/slot": (32, "a slot buffer's documented alignment")}
    for mode in SK.MODES:
        with SK.skewed_allocations(mode, aligned, devices=CPU) as fences:
            scratch, output = stub.allocate(24)                                         # the package's own: fenced, at the allocator's place
            mine = torch.zeros((24,), dtype=torch.int32)                                # the caller's: skewed by its element
            slot = SK.caller_buffer("slot", (5, 7), torch.uint8, "cpu")                 # the caller's, with a documented alignment
            # a caller's allocation made in a callback the package calls is the package's: a frame of it is on the stack
            inner = stub.allocate_through(lambda n: torch.empty((n,), dtype=torch.int32), 8)
            none = torch.empty((0,), dtype=torch.int32)
        assert len(fences) == 5 and len(fences.empty_sites) == 1 and none.storage_offset() == 0
        for t in (scratch, output, inner):
            assert t.data_ptr() % 64 == 0 and (t.storage_offset() * t.element_size()) % FU.ALIGN == 0
        assert mine.data_ptr() % 64 == 4 * SK.UNITS_PAST[mode] and slot.data_ptr() % 64 == 32 and not slot.any() and slot.shape == (5, 7)
        assert [(n, u) for n, _t, u in fences.skewed()] == [(fences.records[2][0], 4), ("own/slot", 32)] and SK.assert_skewed(fences) == 2
        assert fences.records[0][0].endswith("stub_wrappers.py:7 allocate") and fences.records[2][0].startswith("test_skew_util_cpu.py:")
        assert list(fences.named) == ["slot"] and fences.named["slot"][0] is slot and fences.check_fences() == []
        assert tuple((getattr(owner, name), name in vars(owner)) for owner, name in FU.FACTORIES) == before      # restored
    assert SK.caller_buffer("slot", (3,), torch.int16, "cpu").tolist() == [0, 0, 0]     # outside the patch: a plain allocation


def test_the_refusal_run_moves_one_argument_and_fills_the_callers_buffers():
    aligned = {"src": (16, "sixteen"), "own/out": (32, "thirty-two")}
    inputs = {"src": torch.arange(40, dtype=torch.uint8), "table": torch.arange(5, dtype=torch.int64)}
    copy, handle, moved = SK.refusal_copy(inputs, aligned, "src", devices=CPU)
    assert moved == 1 and copy["src"].data_ptr() % 16 == 8 and copy["table"].data_ptr() % 64 == 0 and torch.equal(copy["src"], inputs["src"])
    assert handle.check_fences() == [] and handle.changed_inputs() == []
    with SK.skewed_allocations("b", aligned, devices=CPU, misplace="own/out") as fences:
        out = SK.caller_buffer("out", (9,), torch.int32, "cpu")
        status = SK.caller_buffer("status", (3,), torch.int32, "cpu")
        plain = torch.zeros((4,), dtype=torch.int16)
    assert out.data_ptr() % 32 == 16 and status.data_ptr() % 64 == 0 and plain.data_ptr() % 64 == 0
    assert out.tolist() == [2] * 9 and status.tolist() == [2] * 3 and not plain.any()     # the mode's poison, so that a write shows
    assert fences.written() == [] and fences.skewed() == []
    status[1] = 0
    assert fences.written() == ["status"]
    with pytest.raises(ValueError):
        SK.refusal_copy({"table": inputs["table"]}, {"table": (8, "half of it is no multiple of the element")}, "table", devices=CPU)


# ---- the registry's alignment table against the documents --------------------------------------------------------------------------------------

DOCUMENTS = ("include/mspa.h", "multi-spatialmllm_amd/mspa/engine.py")


def _entries():
    return [(c, path, A, sentence) for c in poison_cases.CASES for path, (A, sentence) in (c.aligned or {}).items()]


def test_every_sentence_of_every_alignment_table_stands_in_the_documents_word_for_word():
    text = {d: _folded(d) for d in DOCUMENTS}
    assert len(_entries()) >= 10
    for c, path, A, sentence in _entries():
        assert any(sentence in t for t in text.values()), (c.name, path, sentence)
        assert isinstance(A, int) and A & (A - 1) == 0 and 2 <= A <= 256, (c.name, path, A)
        assert re.search(rf"\b{A}(-byte| bytes)", sentence), (c.name, path, A, sentence)   # the sentence does speak of that many bytes
    for sentence, reason in list(poison_cases.ALIGN_WRAPPER_OWNED.items()) + list(poison_cases.ALIGN_ROUTES.items()):
        assert any(sentence in t for t in text.values()) and reason, sentence


def test_every_path_of_an_alignment_table_names_an_input_or_a_buffer_of_the_case():
    """``build()`` needs the GPU, so an input path is held against the dict literal ``build`` returns (its source text) and a buffer
    against ``Case.own_buffers``, the names ``run`` may pass to ``own``.  For those this is a reading of ``run``'s source and a loose
    one -- a factory's ``run`` builds its names (``own(name, ..)``, ``own(f".."``) --: that every listed buffer IS allocated through
    ``own`` is held by tests/test_gpu_skewed_memory.py, which finds each name among the allocations of both skewed runs."""
    for c in poison_cases.CASES:
        run_source = inspect.getsource(c.run)
        assert "own(" in run_source or not c.own_buffers, c.name
        for name in c.own_buffers:
            assert f'own("{name}"' in run_source or "own(name" in run_source or 'own(f"' in run_source, (c.name, name)
        for path in (c.aligned or {}):
            if path.startswith("own/"):
                assert path[4:] in c.own_buffers, (c.name, path)
            else:
                assert re.search(rf'"{re.escape(path.split("/")[0])}":', inspect.getsource(c.build)), (c.name, path)
    owners = [c.name for c in poison_cases.CASES if c.own_buffers]
    assert len(owners) >= 10 and len({c.name for c in poison_cases.CASES}) == len(poison_cases.CASES)


def test_every_alignment_the_header_speaks_of_is_in_a_table(capsys):
    """Every "N-byte aligned" / "N-byte," of include/mspa.h lies inside a sentence that some ``Case.aligned`` quotes, or that
    ``ALIGN_WRAPPER_OWNED`` / ``ALIGN_ROUTES`` name with the reason it needs no entry."""
    header = _folded("include/mspa.h")
    quoted = {s for _c, _p, _A, s in _entries()} | set(poison_cases.ALIGN_WRAPPER_OWNED) | set(poison_cases.ALIGN_ROUTES)
    spans = [(m.start(), m.end()) for s in quoted for m in re.finditer(re.escape(s), header)]
    loose = [header[max(0, m.start() - 60):m.end() + 20] for m in re.finditer(r"\b\d+-byte(?: aligned|,| and)", header)
             if not any(a <= m.start() and m.end() <= b for a, b in spans)]
    with capsys.disabled():
        print(f"\nalignment sentences: {len(_entries())} entries in {sum(1 for c in poison_cases.CASES if c.aligned)} cases, "
              f"{len(poison_cases.ALIGN_WRAPPER_OWNED)} about buffers the wrappers own, {len(poison_cases.ALIGN_ROUTES)} route offers")
    assert loose == [], loose
