"""bench.py --dump-outputs, host side: the sampled, unpacked float32 / float64 form of the pair outputs on CPU tensors."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import bench  # noqa: E402


def _pair_outputs(n, rng):
    vis = rng.random((n, bench.P)) < 0.3
    out = {"vis_bits": torch.from_numpy(np.packbits(vis, axis=1, bitorder="little").view(np.int64).copy()),
           "pix_i16": torch.from_numpy(rng.integers(-1, 640, (n, bench.P, 2)).astype(np.int16)),
           "xyz_f32": torch.from_numpy(rng.standard_normal((n, bench.P, 3)).astype(np.float32)),
           "rgba": torch.from_numpy(rng.integers(-2**31, 2**31 - 1, (n, bench.P)).astype(np.int32)),
           "counts": torch.from_numpy(rng.integers(0, 1000, (n, 2)).astype(np.int32))}
    return vis, out


def test_dense_outputs_sampled_exactly(tmp_path):
    rng = np.random.default_rng(1)
    n = 8
    vis, out = _pair_outputs(n, rng)
    r = bench.pair_outputs_for_dump(out, n)
    idx = r["pixel_sample_index"].astype(np.int64)
    assert idx.size == bench.DUMP_SAMPLE and np.all(np.diff(idx) > 0)
    assert np.array_equal(r["vis"], vis.reshape(-1)[idx].astype(np.float32))
    assert np.array_equal(r["pix_i16"], out["pix_i16"].numpy().reshape(-1, 2)[idx].astype(np.float32))
    assert np.array_equal(r["xyz_f32"], out["xyz_f32"].numpy().reshape(-1, 3)[idx])
    assert np.array_equal(r["rgba"], out["rgba"].numpy().reshape(-1)[idx].view(np.uint32).astype(np.float64))
    assert np.array_equal(r["counts"], out["counts"].numpy().astype(np.float64))
    again = bench.pair_outputs_for_dump(out, n)
    assert all(np.array_equal(r[k], again[k]) for k in r)
    bench.dump_outputs(str(tmp_path), r)
    files = sorted(os.listdir(tmp_path))
    assert files == sorted(f"{k}.npy" for k in r)
    assert sum(os.path.getsize(tmp_path / f) for f in files) <= bench.DUMP_BUDGET
    assert all(np.load(tmp_path / f).dtype in (np.float32, np.float64) for f in files)


def test_compact_entries_past_the_tile_count_are_minus_one():
    rng = np.random.default_rng(2)
    n, nt, cap = 4, 80, 3072
    vis, out = _pair_outputs(n, rng)
    cpix = torch.from_numpy(rng.integers(-5, 640, (n, nt, cap, 2)).astype(np.int16))
    tc = torch.from_numpy(rng.integers(0, cap, (n, nt)).astype(np.int32))
    r = bench.pair_outputs_for_dump({"vis_bits": out["vis_bits"], "cpix": cpix, "tile_counts": tc, "counts": out["counts"]}, n)
    e = r["cpix_sample_index"].astype(np.int64)
    want = cpix.numpy().reshape(-1, 2)[e].astype(np.float32)
    want[(e % cap) >= tc.numpy().reshape(-1)[e // cap]] = -1
    assert np.array_equal(r["cpix"], want)
    assert np.array_equal(r["tile_counts"], tc.numpy().astype(np.float64))


def test_large_whole_outputs_are_cut_to_a_seeded_row_sample():
    a = np.arange(6 << 20, dtype=np.float64).reshape(-1, 2)      # 96 MB
    s = bench._dump_rows(a)
    assert s.nbytes <= bench.DUMP_ARRAY_CAP and np.array_equal(s, bench._dump_rows(a))
    assert np.all(s[:, 1] == s[:, 0] + 1)
