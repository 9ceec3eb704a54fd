"""One launch per compiled K3 instantiation (the key array of csrc/pair_route.h, walked by pair_route_cases.WALK), each on the
smallest shape at which its family exists: the kernel family that ran is the one the route rules name, and masks, pixel
indices at visible pixels and counters equal the exact kernel's on the same inputs (the exact kernel's own two
instantiations: the NumPy oracle's).  One more case takes mspa_pair_correspondences' dense-table route, so that
compact_corr_kernel runs too.  tests/test_pair_route_cpu.py proves on the CPU that WALK covers every key exactly once."""
import functools

import numpy as np
import pytest
import torch

import pair_route_cases as C
from mspa import engine, synth, _lib
from oracle import np_oracle as O
from test_gpu_compact import poisoned_outputs
from test_gpu_guard import check_integers
from test_gpu_tight import launch, unpack_bits

DEV = "cuda"
PAIRS = [(0, 1), (1, 0), (2, 2)]          # two ordinary pairs and an identity pair (every depth test a tie: the cold loop)


@functools.lru_cache(maxsize=None)
def scene(hw, dhw):
    sc = synth.make_scene(5150, n_points=64, n_frames=3, color_hw=hw, depth_hw=dhw, invalid_pose_frac=0.0, with_color=True,
                          trajectory="sweep", walk_step=0.08)
    ids = sc.valid_image_ids
    depth = engine.depth_to_device(np.stack([sc.depth[i] for i in ids]), DEV)
    # the same table one int16 element into a larger buffer: 2-byte aligned only, which the tight kernel's LDS-DMA cannot take
    odd = torch.zeros(depth.numel() + 1, dtype=depth.dtype, device=DEV)[1:].view(depth.shape)
    odd.copy_(depth)
    assert depth.data_ptr() % 4 == 0 and odd.data_ptr() % 4 == 2
    mats = torch.from_numpy(engine.frame_matrices(sc.K, sc.A, [sc.E[i] for i in ids])).to(DEV)
    rgb = torch.from_numpy(np.stack([sc.color[i] for i in ids])).to(DEV)
    pairs = torch.tensor(PAIRS, dtype=torch.int32, device=DEV)
    return sc, ids, depth, odd, mats, rgb, pairs


@functools.lru_cache(maxsize=None)
def exact_outputs(hw, dhw, outputs):
    """The exact kernel's result for one (shape, output set), computed once; never modified."""
    sc, ids, depth, odd, mats, rgb, pairs = scene(hw, dhw)
    if outputs == "compact":
        out = poisoned_outputs(len(PAIRS), hw)
        engine.pair_correspondences(depth, mats, pairs, hw, out, flags=0)
        kern = _lib.load().mspa_pair_reproject_last_kernel()
        torch.cuda.synchronize()
        res = {k: v.cpu().numpy() for k, v in out.items()}
    else:
        res, kern = launch(depth, mats, rgb, pairs, hw, outputs, 0)
    assert kern == _lib.KERNEL_PAIR_EXACT
    assert int(res["counts"][:, 1].sum()) > 200, "the pairs must see something"
    return res


def visible(res, P):
    if "vis_bits" in res:
        return np.stack([unpack_bits(w, P) for w in res["vis_bits"]])
    return res["vis_u8"].astype(bool)


@pytest.mark.gpu
@pytest.mark.parametrize("case", C.WALK + [C.DENSE_ROUTE], ids=lambda c: c.name)
def test_every_instantiation_runs_where_the_route_says(case):
    hw, dhw = case.hw, case.dhw
    named = C.parent_route(*C.walk_route_inputs(case))
    assert named.err == 0 and named.key == case.key
    sc, ids, depth, odd, mats, rgb, pairs = scene(hw, dhw)
    d = odd if case.misaligned else depth
    P = hw[0] * hw[1]
    if case.outputs == "compact":
        out = poisoned_outputs(len(PAIRS), hw)
        engine.pair_correspondences(d, mats, pairs, hw, out, flags=case.flags)
        kern = _lib.load().mspa_pair_reproject_last_kernel()
        torch.cuda.synchronize()
        res = {k: v.cpu().numpy() for k, v in out.items()}
    else:
        res, kern = launch(d, mats, rgb, pairs, hw, case.outputs, case.flags)
    assert kern == named.family
    if case.key.kernel == C.K_EXACT:          # the reference of every other case: against the oracle
        for n, (a, b) in enumerate(PAIRS):
            check_integers(res, n, O.frame_pair(sc.depth[ids[a]], sc.depth[ids[b]], sc.K, sc.E[ids[a]], sc.E[ids[b]], sc.A, hw), hw)
        return
    ref = exact_outputs(hw, dhw, case.outputs)
    assert np.array_equal(res["counts"], ref["counts"])
    vis = visible(ref, P)
    assert np.array_equal(visible(res, P), vis)
    if "pix_i16" in res:
        assert np.array_equal(res["pix_i16"][vis], ref["pix_i16"][vis])
    if case.outputs == "compact":
        assert np.array_equal(res["tile_counts"], ref["tile_counts"])
        keep = np.arange(res["cpix"].shape[2])[None, None, :] < ref["tile_counts"][:, :, None]
        assert np.array_equal(res["cpix"][keep], ref["cpix"][keep])
