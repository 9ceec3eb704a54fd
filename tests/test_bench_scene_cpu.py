"""bench.py's synthetic scene, host side: the column-wise ray cast it renders with gives mspa.synth.make_scene's scene bit for bit."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "multi-spatialmllm_amd"), ROOT]
import bench  # noqa: E402
from mspa import synth  # noqa: E402


def test_base_scene_equals_make_scene_bit_for_bit():
    args = argparse.Namespace(scene_points=4096, base_frames=12, walk_step=0.08, target_step=0.25)
    got = bench.make_base_scene(args, 0)
    assert synth.render_depth is not bench._render_depth_columns          # swapped back after the call
    want = synth.make_scene(1000, n_points=4096, n_frames=12, color_hw=(bench.H, bench.W), depth_hw=(bench.H, bench.W),
                            invalid_pose_frac=0.0, with_color=False, trajectory="sweep", walk_step=0.08, target_step=0.25)
    assert got.image_ids == want.image_ids and got.valid_image_ids == want.valid_image_ids
    assert np.array_equal(got.K, want.K) and np.array_equal(got.A, want.A) and np.array_equal(got.points, want.points)
    for i in want.image_ids:
        assert np.array_equal(got.E[i], want.E[i]), i
        assert got.depth[i].dtype == np.uint16 and np.array_equal(got.depth[i], want.depth[i]), i


def test_column_ray_cast_equals_render_depth_on_float_depth():
    """Before the millimetre rounding: the same float64 z for every pixel, at the bench's shape and at a small odd one."""
    sc = synth.make_scene(7, n_points=1024, n_frames=6, invalid_pose_frac=0.0, with_color=False, trajectory="sweep")
    for hw in ((bench.H, bench.W), (37, 53)):
        Kd = synth.intrinsics_for(hw)
        for i in sc.image_ids:
            E_al = sc.A @ sc.E[i]
            a = synth.render_depth(E_al, Kd, hw, sc.boxes)
            b = bench._render_depth_columns(E_al, Kd, hw, sc.boxes)
            assert a.shape == b.shape == hw
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (hw, i)
