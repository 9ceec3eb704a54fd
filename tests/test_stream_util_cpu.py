"""tests/stream_util.py without a GPU: the leaf walk, the input poison and the restore on host tensors; the registry's enqueue-only
sentences against the documents they quote; and a check of the stream argument of every launch and asynchronous copy in
``csrc/*.hip``.  The last one READS SOURCE TEXT ONLY: it compiles nothing and runs nothing, so it says what the text passes, not
what a kernel does -- tests/test_gpu_stream_order.py is the test of that."""
import collections
import glob
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poison_cases  # noqa: E402
import stream_util as SU  # noqa: E402
from mspa import engine  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = ("cpu",)

Pair = collections.namedtuple("Pair", "first second")


def _nest():
    shared = torch.arange(6, dtype=torch.int32)
    return {"a": torch.tensor([1.25, float("nan"), -0.0], dtype=torch.float64), "none": None, "np": np.arange(3), "text": "abc", "n": 7,
            "list": [torch.tensor([True, False]), (torch.arange(4, dtype=torch.int64), shared)], "again": shared,
            "pair": Pair(torch.arange(5, dtype=torch.uint8), torch.zeros((2, 3), dtype=torch.float32).t()),
            "deep": {"x": {"y": [torch.tensor([3], dtype=torch.int16)]}}, "empty": torch.zeros((0,), dtype=torch.int32)}


def test_every_tensor_leaf_is_found_once_in_dicts_tuples_and_lists_and_the_rest_is_passed_over():
    nest = _nest()
    leaves = SU.tensor_leaves(nest, CPU)
    assert [p for p, _t in leaves] == ["a", "list/0", "list/1/0", "list/1/1", "pair/0", "pair/1", "deep/x/y/0", "empty"]    # "again" is list/1/1
    assert all(isinstance(t, torch.Tensor) for _p, t in leaves) and leaves[3][1] is nest["again"]
    assert SU.tensor_leaves(nest, ("cuda",)) == []          # host tensors are no device leaves
    assert SU.tensor_leaves(None, CPU) == [] and SU.tensor_leaves([None, np.zeros(2), "x"], CPU) == []


@pytest.mark.parametrize("mode", SU.MODES)
def test_poison_fills_every_leaf_in_place_and_restore_is_bit_exact(mode):
    nest = _nest()
    leaves = SU.tensor_leaves(nest, CPU)
    before = {p: t.clone() for p, t in leaves}
    nan_bits = nest["a"].view(torch.int64).clone()
    good = SU.clone_leaves(leaves)
    SU.poison_leaves(leaves, mode)
    for path, t in leaves:
        want = SU.input_poison_value(t.dtype, mode)
        if t.dtype.is_floating_point:
            assert t.isnan().all() if mode == "a" else (t == 1.5).all(), path
        elif t.dtype == torch.bool:
            assert (t.view(torch.uint8) == want).all(), path
        else:
            assert (t == want).all(), path
    assert nest["np"].tolist() == [0, 1, 2] and nest["none"] is None and nest["n"] == 7          # passed over
    assert nest["pair"].second.shape == (3, 2) and not nest["pair"].second.is_contiguous()       # a strided view keeps its strides
    SU.restore_leaves(leaves, good)
    for path, t in leaves:
        assert torch.equal(t.contiguous().view(torch.uint8), before[path].contiguous().view(torch.uint8)), path
    assert torch.equal(nest["a"].view(torch.int64), nan_bits)                                     # NaN and -0.0 by their bits
    assert nest["again"] is nest["list"][1][1] and nest["again"].tolist() == list(range(6))


def test_the_input_poison_table():
    small = (torch.int16, torch.int32, torch.int64) + tuple(getattr(torch, n) for n in ("uint16", "uint32", "uint64") if hasattr(torch, n))
    for dtype in small:
        assert (SU.input_poison_value(dtype, "a"), SU.input_poison_value(dtype, "b")) == (1, 2), dtype
    for dtype in (torch.uint8, torch.int8, torch.bool):
        assert (SU.input_poison_value(dtype, "a"), SU.input_poison_value(dtype, "b")) == (0x5A, 0xA5), dtype
    for dtype in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
        assert np.isnan(SU.input_poison_value(dtype, "a")) and SU.input_poison_value(dtype, "b") == 1.5, dtype
    # an int64 input is an offset or a row number: 1 / 2, never poison_util's two-lane pattern (4 GiB as an offset)
    t = SU.fill_input_poison(torch.zeros((5,), dtype=torch.int64), "a")
    assert t.tolist() == [1] * 5 and SU.fill_input_poison(t, "b").tolist() == [2] * 5
    assert SU.fill_input_poison(torch.zeros((3,), dtype=torch.int8), "b").view(torch.uint8).tolist() == [0xA5] * 3
    assert SU.fill_input_poison(torch.zeros((3,), dtype=torch.bool), "a").view(torch.uint8).tolist() == [0x5A] * 3
    with pytest.raises(ValueError):
        SU.input_poison_value(torch.int32, "zero")


def test_snapshot_clones_the_tensors_and_keeps_the_rest():
    nest = _nest()
    snap = SU.snapshot(nest, CPU)
    assert snap["a"] is not nest["a"] and torch.equal(snap["a"].view(torch.int64), nest["a"].view(torch.int64))
    assert snap["np"] is nest["np"] and snap["none"] is None and isinstance(snap["pair"], Pair) and isinstance(snap["list"][1], tuple)
    nest["deep"]["x"]["y"][0].fill_(9)
    assert snap["deep"]["x"]["y"][0].tolist() == [3]


def test_the_delay_is_four_warm_host_times_between_the_floor_and_the_cap():
    assert SU.delay_for(0.1) == SU.FLOOR_MS and SU.delay_for(100.0) == 400.0 and SU.delay_for(900.0) == SU.CAP_MS == 2000.0
    assert SU.FLOOR_MS >= SU.MEASURED_FLOOR_MS > 0 and SU.delay_for(1.0, floor_ms=1.0) == 4.0 and len(SU.ROLES) == 8 and len(set(SU.ROLES)) == 8


# ---- the registry's sentences -----------------------------------------------------------------------------------------------------------------

def _folded(path):
    """A file's text with its line breaks (and a C comment's leading " * ") folded into single spaces."""
    with open(os.path.join(ROOT, path)) as f:
        return re.sub(r"[ \t]*\n[ \t]*(?:\*(?!/)[ \t]*)?", " ", f.read())


def test_every_enqueue_only_sentence_stands_in_the_documents_and_every_case_names_functions_that_exist():
    documents = {"engine": _folded("multi-spatialmllm_amd/mspa/engine.py"), "header": _folded("include/mspa.h")}
    assert poison_cases.C_ABI in documents["header"]
    for function, sentence in poison_cases.ENQUEUES.items():
        assert callable(getattr(engine, function, None)), function
        if sentence != poison_cases.C_ABI:                   # in ITS docstring, and so in the file
            assert sentence in re.sub(r"\s*\n\s*", " ", getattr(engine, function).__doc__) and sentence in documents["engine"], (function, sentence)
    for c in poison_cases.CASES:
        for function in c.covers:
            assert callable(getattr(engine, function, None)), (c.name, function)
        listed = all(f in poison_cases.ENQUEUES for f in c.covers)
        if c.enqueue_only is not None:
            assert listed, (c.name, [f for f in c.covers if f not in poison_cases.ENQUEUES])
            assert c.enqueue_only in [poison_cases.ENQUEUES[f] for f in c.covers], c.name
            assert any(c.enqueue_only in text for text in documents.values()), c.name
            assert c.name not in poison_cases.HOST_STEPS, c.name
        else:
            assert not listed or c.name in poison_cases.HOST_STEPS, f"{c.name}: every covered function only enqueues, and no host step is named"
    assert poison_cases.PAIR_REPROJECT_SEEN_TABLE in engine.pair_reproject.__doc__ and "pair_reproject" not in poison_cases.ENQUEUES
    assert set(poison_cases.HOST_STEPS) <= {c.name for c in poison_cases.CASES}
    assert sum(c.enqueue_only is not None for c in poison_cases.CASES) >= 20


# ---- the stream argument of every launch and asynchronous copy in csrc/*.hip: source text only ------------------------------------------------

# (file, function, reason): entry points that may use a synchronous copy / memset or wait for the device -- host-only ones and the
# ones that only report about the device.  None needs it today; an entry that nothing uses fails the test below.
SYNCHRONOUS_ALLOWED = (
)

NULL_STREAMS = {"0", "nullptr", "NULL", "hipStreamDefault", "hipStreamLegacy", "hipStreamPerThread"}
CALL = re.compile(r"\b(hipLaunchKernelGGL|hipMemsetAsync|hipMemset\w*Async|hipMemcpy\w*Async)\s*\(")
SYNCHRONOUS = re.compile(r"\b(hipMemcpy(?!\w*Async)\w*|hipMemset(?!\w*Async)\w*|hipDeviceSynchronize|hipStreamSynchronize)\s*\(")
DEFINITION = re.compile(r"^(?![ \t#/}])[^\n;(]*?\b(\w+)\s*\([^;{}]*?\)\s*(?:noexcept\s*)?\{", re.M | re.S)


def _strip_comments(text):
    """Comments and string literals blanked out, every other character (newlines included) where it was."""
    def blank(m):
        return re.sub(r"[^\n]", " ", m.group(0))
    return re.sub(r'//[^\n]*|/\*.*?\*/|"(?:\\.|[^"\\\n])*"', blank, text, flags=re.S)


def _arguments(text, open_paren):
    """The top-level arguments of the call whose "(" is at ``open_paren``; angle brackets nest only in the first one (a kernel's
    template arguments)."""
    args, depth, angle, start, k = [], 0, 0, open_paren + 1, open_paren
    while True:
        k += 1
        ch = text[k]
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            if depth == 0:
                args.append(text[start:k].strip())
                return args
            depth -= 1
        elif ch == "<" and not args and depth == 0:
            angle += 1
        elif ch == ">" and not args and depth == 0 and angle:
            angle -= 1
        elif ch == "," and depth == 0 and angle == 0:
            args.append(text[start:k].strip())
            start = k + 1


def _function_at(text, position):
    name = "?"
    for m in DEFINITION.finditer(text):
        if m.start() > position:
            break
        name = m.group(1)
    return name


def _sources():
    paths = sorted(glob.glob(os.path.join(ROOT, "multi-spatialmllm_amd", "csrc", "*.hip")))
    assert len(paths) >= 20
    for path in paths:
        with open(path) as f:
            yield os.path.basename(path), _strip_comments(f.read())


def test_the_argument_splitter_on_made_up_calls():
    text = _strip_comments('hipLaunchKernelGGL(ns::k<false, 3>, dim3((unsigned)(n + 1), 2), dim3(64), 0, (hipStream_t)stream, a, f(b, c)); // 0, 0\n'
                           'int mspa_x(void *stream)\n{\n    hipMemsetAsync(p, 0, (size_t)n * 4, st);\n}\n')
    first = CALL.search(text)
    assert _arguments(text, first.end() - 1) == ["ns::k<false, 3>", "dim3((unsigned)(n + 1), 2)", "dim3(64)", "0", "(hipStream_t)stream", "a", "f(b, c)"]
    second = CALL.search(text, first.end())
    assert _arguments(text, second.end() - 1)[-1] == "st" and _function_at(text, second.start()) == "mspa_x"
    assert SYNCHRONOUS.search("hipMemcpy(a, b, n, k)") and SYNCHRONOUS.search("hipMemset(a, 0, n)") and SYNCHRONOUS.search("hipMemcpy2D(a)")
    assert not SYNCHRONOUS.search("hipMemcpyAsync(a, b, n, k, st)") and not SYNCHRONOUS.search("hipMemcpy2DAsync(a)") and not SYNCHRONOUS.search("hipMemsetAsync(")


def test_every_launch_and_asynchronous_copy_in_csrc_passes_a_stream_and_no_entry_point_waits_for_the_device(capsys):
    """Source text only.  The stream of ``hipLaunchKernelGGL`` is its fifth argument, that of ``hipMemsetAsync`` / ``hipMemcpy*Async``
    the last; a literal 0 / nullptr (behind a cast or not) is the null stream, which the project's non-blocking streams do not
    order against."""
    launches, copies, wrong, waits = 0, 0, [], []
    for name, text in _sources():
        assert "<<<" not in text, f"{name}: a triple-chevron launch, which this check does not read"
        for m in CALL.finditer(text):
            args = _arguments(text, m.end() - 1)
            is_launch = m.group(1) == "hipLaunchKernelGGL"
            launches += is_launch
            copies += not is_launch
            assert len(args) >= (5 if is_launch else 4), (name, m.group(1), args)
            stream = re.sub(r"^\(\s*hipStream_t\s*\)\s*", "", args[4] if is_launch else args[-1]).strip()
            if stream in NULL_STREAMS or not re.search(r"[A-Za-z_]", stream):
                wrong.append((name, _function_at(text, m.start()), m.group(1), stream))
        for m in SYNCHRONOUS.finditer(text):
            waits.append((name, _function_at(text, m.start()), m.group(1)))
    allowed = {(f, fn) for f, fn, _reason in SYNCHRONOUS_ALLOWED}
    assert all(len(entry) == 3 and entry[2] for entry in SYNCHRONOUS_ALLOWED)
    with capsys.disabled():
        print(f"\ncsrc/*.hip (source text): {launches} hipLaunchKernelGGL and {copies} hipMemsetAsync / hipMemcpy*Async sites, each with a stream "
              f"of its caller's; {len(waits)} synchronous calls ({len(allowed)} allowed)")
    assert launches > 100 and copies >= 14, (launches, copies)
    assert wrong == [], f"launched or copied on the null stream: {wrong}"
    assert [w for w in waits if w[:2] not in allowed] == [], "a device entry point copies synchronously or waits for the device"
    assert allowed <= {w[:2] for w in waits}, f"allowed, but no longer there: {sorted(allowed - {w[:2] for w in waits})}"
