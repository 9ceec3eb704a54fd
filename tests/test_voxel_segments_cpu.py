"""The voxel down-sampling of a ragged batch without a GPU (csrc/voxel_grid_core.h through the library's host twin,
mspa_voxel_segments_host): the twin against the oracle of tests/voxel_segments_util.py, written from the rule's text alone, bit
for bit; the edge batches; the invariants; every argument error of the C entry points and of the Python functions;
``ops.voxel_down_sample`` on NumPy input; and the header once more as a stand-alone g++ program under AddressSanitizer + UBSan.
The rule restates Open3D's ``voxel_down_sample`` and is not checked against Open3D, which is not installed."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_segments_util as V  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-spatialmllm_amd", "csrc")


def _ops():
    for name in [m for m in sys.modules if m == "spatial_engine" or m.startswith("spatial_engine.")]:
        if not (getattr(sys.modules[name], "__file__", None) or "").startswith(ROOT):
            del sys.modules[name]                   # the reference's modules of the same names, left by another test
    from spatial_engine.utils.scannet_utils.handler import ops
    return ops


@pytest.mark.parametrize("columns", V.COLUMNS)
@pytest.mark.parametrize("size", V.SIZES)
def test_the_host_twin_equals_the_oracle_bit_for_bit(size, columns):
    want = V.batch_oracle(size, columns)
    V.assert_same(V.batch_twin(size, columns), want, (size, columns))
    counts = want[2]
    if size == 0.25:                                                         # both sum regimes, many times
        assert (counts > V.SEQUENTIAL).sum() >= 100 and (counts <= V.SEQUENTIAL).sum() >= 100 and ((counts > 1) & (counts <= 64)).sum() >= 100
    if size == 100.0:                                                        # voxels that swallow a segment
        assert counts.max() == 20000


def test_the_batch_is_what_its_docstring_says():
    rows, offsets, names = V.batch()
    assert len(rows) == offsets[-1] and len(names) == len(offsets) - 1 and np.diff(offsets)[0] == 0
    lengths = dict(zip(names, np.diff(offsets)))
    assert lengths["wave-20"] + lengths["wave-17"] + lengths["wave-9"] < 64
    idx = V.indices(rows, offsets, V.TOO_SMALL)
    assert idx[:, 1:].max() >= V.AXIS_LIMIT                                  # the ValueError case
    for size in V.SIZES:
        assert V.indices(rows, offsets, size)[:, 1:].max() < V.AXIS_LIMIT and V.indices(rows, offsets, size)[:, 1:].min() >= 0
    # the lattice at 0.25: every operand exact, the odd k on a face and in the UPPER voxel
    s = names.index("lattice-3000")
    p = rows[offsets[s]:offsets[s + 1]]
    k = np.rint(p * 8).astype(np.int64)
    assert np.array_equal(k / 8.0, p) and p.min() == 0.0 and ((k % 2) == 1).mean() > 0.4
    got = V.indices(rows, offsets, 0.25)[offsets[s]:offsets[s + 1], 1:]
    assert np.array_equal(got, (k + 1) // 2)
    # identical-200: one voxel of 200 rows at every size
    s = names.index("identical-200")
    for size in V.SIZES:
        out, out_offsets, counts, _vox = V.batch_oracle(size)
        assert out_offsets[s + 1] - out_offsets[s] == 1 and counts[out_offsets[s]] == 200


@pytest.mark.parametrize("name", ["S=1", "all-empty", "N=0", "n=1"])
def test_one_segment_only_empty_segments_no_rows_and_one_row(name):
    from mspa import cloud_segments as CS
    xyz, offsets = V.small_batches()[name]
    for size in (0.05, 10.0):
        got = CS.voxel_down_sample_segments_host(xyz, offsets, size)
        V.assert_same(got, V.oracle(xyz, offsets, size), (name, size))
        assert got[1].shape == offsets.shape and got[1][-1] == len(got[0])
    if name == "n=1":
        assert np.array_equal(V.bits(got[0]), V.bits(xyz)) and got[2].tolist() == [1] and got[1].tolist() == [0, 0, 1, 1]


def test_a_size_so_small_that_every_row_is_alone_permutes_the_input_by_key():
    from mspa import cloud_segments as CS
    rows, offsets, names = V.batch(6)
    a, b = names.index("uniform-257"), names.index("line-500") + 1        # identical-200 excluded: its rows share a voxel at every size
    sub, off = rows[offsets[a]:offsets[b]], offsets[a:b + 1] - offsets[a]
    size = 2.0 ** -20                                                        # extents of 1 (uniform, plane) and 2 (the line): below 2^21 cells
    idx = V.indices(sub, off, size)
    assert len(np.unique(idx, axis=0)) == len(sub) and idx[:, 1:].max() < V.AXIS_LIMIT
    out, out_offsets, counts = CS.voxel_down_sample_segments_host(sub, off, size)
    perm = np.lexsort((idx[:, 3], idx[:, 2], idx[:, 1], idx[:, 0]))
    assert np.array_equal(V.bits(out), V.bits(sub[perm])) and (counts == 1).all() and np.array_equal(out_offsets, off)


def test_a_size_larger_than_the_cloud_gives_one_row_per_non_empty_segment():
    from mspa import cloud_segments as CS
    rows, offsets, _names = V.batch()
    out, out_offsets, counts = CS.voxel_down_sample_segments_host(rows, offsets, 1e6)
    n = np.diff(offsets)
    assert np.array_equal(np.diff(out_offsets), (n > 0).astype(np.int64)) and np.array_equal(counts, n[n > 0]) and len(out) == (n > 0).sum()


@pytest.mark.parametrize("size", V.SIZES)
def test_counts_sum_to_each_segments_rows_and_every_mean_lies_in_its_cell(size):
    """The cell of voxel idx on an axis is [min_bound + idx * size, min_bound + (idx + 1) * size].  A row's idx is the floor of a
    ROUNDED quotient, so a row may lie outside its cell by the rounding of (p - min_bound) / size: at most 2^-52 of
    |p| + |min_bound| + (idx + 1) * size; a mean of such rows, itself rounded once per sum, by no more than m + 2 times that.  The
    tolerance is 2^-50 times that magnitude (m + 2 roundings would need runs of millions of rows to matter; the longest is 20 000
    and its rows span a fraction of the cell)."""
    rows, offsets, _names = V.batch()
    out, out_offsets, counts = V.batch_twin(size)
    voxels = V.batch_oracle(size)[3]
    for s in range(len(offsets) - 1):
        assert counts[out_offsets[s]:out_offsets[s + 1]].sum() == offsets[s + 1] - offsets[s]
        if offsets[s + 1] > offsets[s]:
            min_bound = rows[offsets[s]:offsets[s + 1], :3].min(axis=0) - size * 0.5
            idx = voxels[out_offsets[s]:out_offsets[s + 1], 1:].astype(np.float64)
            mean = out[out_offsets[s]:out_offsets[s + 1], :3]
            lower, upper = min_bound + idx * size, min_bound + (idx + 1) * size
            tol = 2.0 ** -50 * (np.abs(mean) + np.abs(min_bound) + (idx + 1) * size)
            assert (mean >= lower - tol).all() and (mean <= upper + tol).all(), s


def test_the_python_functions_refuse_bad_arguments():
    from mspa import cloud_segments as CS
    ops = _ops()
    rows, offsets, _names = V.batch()
    for size in (0, 0.0, -1, -1.0, float("nan"), float("inf"), None, "small"):
        with pytest.raises(RuntimeError, match="voxel_size"):
            CS.voxel_down_sample_segments_host(rows, offsets, size)
        with pytest.raises(RuntimeError, match="voxel_size"):
            ops.voxel_down_sample(rows, size)
    with pytest.raises(ValueError, match="voxel_size"):
        CS.voxel_down_sample_segments_host(rows, offsets, V.TOO_SMALL)
    for value in (np.nan, np.inf, -np.inf):
        bad = rows.copy()
        bad[5000, 1] = value
        with pytest.raises(ValueError, match="non-finite"):
            CS.voxel_down_sample_segments_host(bad, offsets, 0.25)
        with pytest.raises(ValueError, match="non-finite"):
            ops.voxel_down_sample(bad, 0.25)
    with pytest.raises(ValueError):
        CS.voxel_down_sample_segments_host(rows, offsets[:-1], 0.25)         # offsets that do not end at N
    with pytest.raises(ValueError):
        CS.voxel_down_sample_segments_host(rows, offsets[::-1], 0.25)        # descending
    with pytest.raises(ValueError):
        CS.voxel_down_sample_segments_host(rows[:, :2], offsets, 0.25)       # C < 3
    with pytest.raises(ValueError):
        CS.voxel_down_sample_segments_host(rows.reshape(-1), offsets, 0.25)
    with pytest.raises((ValueError, RuntimeError)):
        CS.voxel_down_sample_segments(rows, offsets, 0.25)                   # NumPy rows have no device: no quiet fallback


def test_the_c_entry_points_refuse_bad_arguments_before_anything_is_enqueued():
    """Every refusal below returns MSPA_EINVAL from the argument checks; none of the pointers is a device pointer, and none is ever
    dereferenced as one (the checks come before the first launch)."""
    from mspa import _lib
    lib = _lib.load()
    rows = np.random.default_rng(1).random((10, 4))
    good = np.array([0, 4, 4, 10], dtype=np.int64)
    S, C = 3, 4
    base = np.zeros(S + 1, dtype=np.int64)
    assert lib.mspa_voxel_segments_tables_host(good.ctypes.data, S, base.ctypes.data) == 0 and base.tolist() == [0, 1, 1, 2]
    big = np.array([0, 4096, 4097, 4097 + 8192], dtype=np.int64)
    assert lib.mspa_voxel_segments_tables_host(big.ctypes.data, S, base.ctypes.data) == 0 and base.tolist() == [0, 1, 2, 4]
    work_bytes = lib.mspa_voxel_segments_workspace_bytes(good.ctypes.data, S)
    assert work_bytes > 0 and work_bytes % 16 == 0
    work = np.zeros(work_bytes + 16, dtype=np.uint8)
    aligned = (work.ctypes.data + 15) // 16 * 16
    keys, order, segment = np.zeros(10, dtype=np.int64), np.arange(10, dtype=np.int64), np.zeros(10, dtype=np.int32)
    seg_voxels, out, counts = np.zeros(S + 1, dtype=np.int32), np.zeros((10, C)), np.zeros(10, dtype=np.int32)
    out_offsets, flags = np.zeros(S + 1, dtype=np.int64), np.zeros(1, dtype=np.int32)
    p = lambda a: a.ctypes.data                                              # noqa: E731
    descending = np.array([0, 5, 4, 10], dtype=np.int64)
    not_from_zero = np.array([1, 4, 4, 10], dtype=np.int64)
    too_long = np.array([0, (1 << 30) + 1], dtype=np.int64)
    many = (1 << 24) + 1

    def keys_call(off=good, n_seg=S, c=C, size=0.5, rows_p=p(rows), keys_p=p(keys), seg_p=p(segment), vox_p=p(seg_voxels), base_p=p(base),
                  w=aligned, w_bytes=work_bytes):
        return lib.mspa_voxel_segments_keys_device(rows_p, c, p(off), n_seg, size, p(off), base_p, keys_p, seg_p, vox_p, w, w_bytes, None)

    def heads_call(off=good, n_seg=S, keys_p=p(keys), order_p=p(order), vox_p=p(seg_voxels), w=aligned, w_bytes=work_bytes):
        return lib.mspa_voxel_segments_heads_device(p(off), n_seg, p(off), keys_p, order_p, vox_p, w, w_bytes, None)

    def means_call(off=good, n_seg=S, c=C, M=5, rows_p=p(rows), order_p=p(order), out_p=p(out), counts_p=p(counts), w=aligned,
                   w_bytes=work_bytes):
        return lib.mspa_voxel_segments_means_device(rows_p, c, p(off), n_seg, p(off), order_p, M, out_p, counts_p, w, w_bytes, None)

    def host_call(off=good, n_seg=S, c=C, size=0.5, rows_p=p(rows), out_p=p(out), off_p=p(out_offsets), flags_p=p(flags)):
        return lib.mspa_voxel_segments_host(rows_p, c, p(off), n_seg, size, out_p, off_p, p(counts), flags_p)

    refused = {}
    for name, call in (("keys", keys_call), ("heads", heads_call), ("means", means_call)):
        refused.update({
            f"{name}: descending offsets": call(off=descending), f"{name}: offsets[0] != 0": call(off=not_from_zero),
            f"{name}: N > 2^30": call(off=too_long, n_seg=1), f"{name}: negative S": call(n_seg=-1), f"{name}: S > 2^24": call(n_seg=many),
            f"{name}: null workspace": call(w=None), f"{name}: workspace too small": call(w_bytes=work_bytes - 16),
            f"{name}: workspace misaligned": call(w=aligned + 8)})
    refused.update({
        "keys: C = 2": keys_call(c=2), "keys: size 0": keys_call(size=0.0), "keys: size -1": keys_call(size=-1.0),
        "keys: size NaN": keys_call(size=float("nan")), "keys: size inf": keys_call(size=float("inf")), "keys: null rows": keys_call(rows_p=None),
        "keys: null keys": keys_call(keys_p=None), "keys: null segment": keys_call(seg_p=None), "keys: null seg_voxels": keys_call(vox_p=None),
        "keys: null tile_base": keys_call(base_p=None), "keys: keys at 4 mod 8": keys_call(keys_p=p(keys) + 4),
        "keys: segment at 2 mod 4": keys_call(seg_p=p(segment) + 2),
        "heads: null keys": heads_call(keys_p=None), "heads: null order": heads_call(order_p=None), "heads: null seg_voxels": heads_call(vox_p=None),
        "heads: order at 4 mod 8": heads_call(order_p=p(order) + 4),
        "means: C = 2": means_call(c=2), "means: M < 0": means_call(M=-1), "means: M > N": means_call(M=11), "means: null rows": means_call(rows_p=None),
        "means: null order": means_call(order_p=None), "means: null out": means_call(out_p=None), "means: null counts": means_call(counts_p=None),
        "means: out at 4 mod 8": means_call(out_p=p(out) + 4),
        "host: descending": host_call(off=descending), "host: C = 2": host_call(c=2), "host: size 0": host_call(size=0.0),
        "host: size NaN": host_call(size=float("nan")), "host: null rows": host_call(rows_p=None), "host: null out": host_call(out_p=None),
        "host: null offsets out": host_call(off_p=None), "host: null flags": host_call(flags_p=None), "host: N > 2^30": host_call(off=too_long, n_seg=1),
        "tables: descending": lib.mspa_voxel_segments_tables_host(p(descending), S, p(base.copy())),
        "tables: null out": lib.mspa_voxel_segments_tables_host(p(good), S, None),
    })
    assert {k: v for k, v in refused.items() if v != _lib.MSPA_EINVAL} == {}
    assert lib.mspa_voxel_segments_workspace_bytes(p(descending), S) == -1 and lib.mspa_voxel_segments_workspace_bytes(p(too_long), 1) == -1
    assert b"mspa_voxel_segments" in lib.mspa_last_error_string()
    assert host_call() == 0 and flags[0] == 0 and out_offsets[-1] >= 2       # the good arguments are good
    # the flag word: a NaN row and a size that is too small, clamped and reported, not refused by the C layer
    nan_rows = rows.copy()
    nan_rows[7, 2] = np.nan
    assert host_call(rows_p=p(nan_rows)) == 0 and flags[0] & 1
    assert host_call(size=1e-9) == 0 and flags[0] == 2


def test_ops_voxel_down_sample_on_numpy_input_is_the_one_segment_batch():
    import torch
    from mspa import cloud_segments as CS
    ops = _ops()
    assert "No reference counterpart" in " ".join(ops.voxel_down_sample.__doc__.split()) and "not checked against Open3D" in " ".join(
        ops.voxel_down_sample.__doc__.split())
    rows, offsets, names = V.batch(6)
    s = names.index("plane-3000")
    cloud = rows[offsets[s]:offsets[s + 1]]
    for size in (0.01, 0.25):
        got = ops.voxel_down_sample(cloud, size)
        want = CS.voxel_down_sample_segments_host(cloud, np.array([0, len(cloud)]), size)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and np.array_equal(V.bits(got), V.bits(want[0]))
        whole = V.batch_twin(size, 6)                                         # and it is that segment's part of the batch
        assert np.array_equal(V.bits(got), V.bits(whole[0][whole[1][s]:whole[1][s + 1]]))
    narrow = cloud.astype(np.float32)                                        # float32 in: widened exactly, float64 out
    assert np.array_equal(ops.voxel_down_sample(narrow, 0.25), ops.voxel_down_sample(narrow.astype(np.float64), 0.25))
    for C in (3, 6):
        empty = ops.voxel_down_sample(np.zeros((0, C), dtype=np.float32), 0.1)
        assert empty.shape == (0, C) and empty.dtype == np.float64
    on_host = ops.voxel_down_sample(torch.from_numpy(cloud.copy()), 0.25)    # a host tensor in gives a host tensor out
    assert isinstance(on_host, torch.Tensor) and np.array_equal(on_host.numpy(), ops.voxel_down_sample(cloud, 0.25))


def test_by_object_without_a_size_is_what_it_was_and_the_docstrings_keep_their_sentences():
    import torch
    from mspa import cloud_segments as CS
    from mspa.instances import InstanceClouds
    rng = np.random.default_rng(5)
    F, L = 3, 6
    counts = rng.integers(0, 5, size=(F, L))
    total = int(counts.sum())
    rows = torch.from_numpy(np.arange(total * 3, dtype=np.float64).reshape(total, 3))
    clouds = InstanceClouds([10, 11, 12], counts, rows, None, torch.zeros((F, L, 3), dtype=torch.float64), torch.zeros((F, L, 3), dtype=torch.float64))
    plain, with_none = clouds.by_object(), clouds.by_object(voxel_size=None)
    assert torch.equal(plain[0], with_none[0]) and np.array_equal(plain[1], with_none[1]) and np.array_equal(plain[2], with_none[2])
    fold = lambda text: " ".join(text.split())                               # noqa: E731
    assert "Enqueue only." in fold(InstanceClouds.by_object.__doc__)
    assert "One read-back per call, whatever S is: the per-segment voxel counts together with the flag word." in fold(
        CS.voxel_down_sample_segments.__doc__)
    assert "not checked against Open3D" in fold(CS.voxel_down_sample_segments.__doc__)


# One record: int64 S, int64 C, float64 size, (S + 1) int64 offsets, N * C float64 -> int32 flags, (S + 1) int64 out_offsets, M * C float64,
# M int32 counts.  Every buffer is a heap block of exactly its size.
DRIVER = r"""
#include "voxel_grid_core.h"
#include <cstdio>
#include <cstdlib>
template <typename T> static T *block(int64_t n) { return (T *)malloc((size_t)(n > 0 ? n : 1) * sizeof(T)); }
int main() {
    int64_t head[2];
    double size;
    while (fread(head, 8, 2, stdin) == 2) {
        const int64_t S = head[0], C = head[1];
        if (fread(&size, 8, 1, stdin) != 1) return 3;
        int64_t *offsets = block<int64_t>(S + 1), *out_offsets = block<int64_t>(S + 1);
        if (fread(offsets, 8, (size_t)(S + 1), stdin) != (size_t)(S + 1)) return 4;
        const int64_t N = mspa::segs::batch_rows(offsets, S);
        if (N < 0 || !mspa::voxel::size_ok(size)) return 5;
        double *rows = block<double>(N * C), *out = block<double>(N * C);
        int32_t *counts = block<int32_t>(N);
        if (fread(rows, 8, (size_t)(N * C), stdin) != (size_t)(N * C)) return 6;
        const int32_t flags = mspa::voxel::down_sample_all(rows, C, offsets, S, size, out, out_offsets, counts);
        const int64_t M = out_offsets[S];
        int64_t *tiles = block<int64_t>(S + 1);
        mspa::voxel::tile_table(offsets, S, tiles);
        if (tiles[S] < (N + mspa::voxel::kExtentTile - 1) / mspa::voxel::kExtentTile) return 7;
        fwrite(&flags, 4, 1, stdout);
        fwrite(out_offsets, 8, (size_t)(S + 1), stdout);
        fwrite(out, 8, (size_t)(M * C), stdout);
        fwrite(counts, 4, (size_t)M, stdout);
        void *all[] = {offsets, out_offsets, rows, out, counts, tiles};
        for (void *b : all) free(b);
    }
    return 0;
}
"""


def test_the_header_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    from mspa import cloud_segments as CS
    (tmp_path / "driver.cpp").write_text(DRIVER)
    exe = str(tmp_path / "driver")
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", CSRC, str(tmp_path / "driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    records = [(V.batch(c)[0], V.batch(c)[1], size) for c in V.COLUMNS for size in (0.01, 0.25, 100.0)]
    records += [(x, o, 0.05) for x, o in V.small_batches().values()]
    nan_rows = V.batch()[0].copy()
    nan_rows[123, 0] = np.nan
    records += [(V.batch()[0], V.batch()[1], V.TOO_SMALL), (nan_rows, V.batch()[1], 0.25)]      # the clamped keys index nothing outside a block
    inp = b"".join(struct.pack("<qqd", len(o) - 1, x.shape[1], s) + np.asarray(o, dtype="<i8").tobytes() + np.asarray(x, dtype="<f8").tobytes()
                   for x, o, s in records)
    run = subprocess.run([exe], input=inp, capture_output=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:].decode(errors="replace"))
    at = 0

    def take(dtype, count, shape=None):
        nonlocal at
        a = np.frombuffer(run.stdout, dtype=dtype, count=count, offset=at)
        at += a.nbytes
        return a if shape is None else a.reshape(shape)

    for n, (x, o, s) in enumerate(records):
        S, C = len(o) - 1, x.shape[1]
        flags = int(take("<i4", 1)[0])
        out_offsets = take("<i8", S + 1)
        M = int(out_offsets[-1])
        out, counts = take("<f8", M * C, (M, C)), take("<i4", M)
        assert flags == (2 if s == V.TOO_SMALL else 1 if np.isnan(x).any() else 0), (n, flags)
        if not flags:
            V.assert_same((out, out_offsets, counts), CS.voxel_down_sample_segments_host(x, o, s), n)
    assert at == len(run.stdout)
