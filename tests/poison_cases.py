"""The device surface of ``mspa.engine`` as cases for tests/test_gpu_poisoned_memory.py, tests/test_gpu_fenced_memory.py and
tests/test_gpu_stream_order.py: one case per op, or per chain of ops that hand state to each other (a producer's unspecified
region then reaches its consumer still poisoned).

A case has a name, a family (one process per family on the GPU machine), the engine functions it covers, ``build()`` (the
inputs: real device tensors, built OUTSIDE the patch, so inputs are never poisoned), ``run(inputs)`` (calls the ops and returns
every tensor the wrappers return, padding included), an optional ``defined`` (poison_util.compare_runs) and
``expect(inputs, zero_result)``, which holds the clean run against the op's plain reference -- the oracles and ``*_util``
helpers the suite already has.

A region is masked out by ``defined`` only where include/mspa.h or the wrapper's docstring already calls it unspecified; the
sentence is quoted next to the mask.  ``writes`` names the inputs an op is documented to write (the fenced run takes every other
input to be unchanged afterwards), each with its sentence quoted the same way; no case needs one today.  ``enqueue_only`` holds
the sentence that promises that no covered function synchronises the host (tests/test_gpu_stream_order.py holds the case to
it); where it is None, a comment at the case quotes the read-back that the documents name instead.  Importing this module
touches no GPU (the completeness check reads ``CASES`` on the CPU).
"""
from __future__ import annotations

import functools
import os
import sys
from dataclasses import dataclass
from typing import Callable, Dict, Optional, Tuple

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mspa import _lib, engine, synth  # noqa: E402
from oracle import c_oracle as C  # noqa: E402
from oracle import np_oracle as O  # noqa: E402

DEV = "cuda"


@dataclass
class Case:
    name: str
    family: str
    covers: Tuple[str, ...]
    build: Callable[[], dict]
    run: Callable[[dict], object]
    expect: Callable[[dict, object], None]
    defined: Optional[Dict[str, object]] = None
    writes: Tuple[str, ...] = ()      # paths into ``inputs`` the op is documented to write (tests/test_gpu_fenced_memory.py), each with its sentence
    enqueue_only: Optional[str] = None    # the documents' promise that no covered function synchronises the host (tests/test_gpu_stream_order.py)
    # tests/test_gpu_skewed_memory.py: path into ``inputs`` (or "own/<name>": a buffer ``run`` allocates with ``own``) -> (the bytes of
    # alignment the documents demand for that argument, the sentence that demands them); every other caller-owned tensor is run at
    # the alignment of its element.  ``own_buffers``: the names ``run`` may pass to ``own`` (checked on the CPU).
    aligned: Optional[Dict[str, Tuple[int, str]]] = None
    own_buffers: Tuple[str, ...] = ()
    refused_by: Optional[str] = None      # where it matters WHICH entry point refuses: a piece of the error string of every refusal of the case


CASES = []

# Public functions of mspa.engine that allocate through torch.empty and have no case, each with its reason.
NOT_COVERED = {
    "alloc_pair_outputs": "a pure allocator; its consumer pair_reproject is covered with outputs allocated by it under the patch",
    "alloc_pair_correspondences": "a pure allocator; pair_correspondences calls it under the patch",
}


# The sentence with which mspa/engine.py (a wrapper's docstring) or include/mspa.h promises that a function only enqueues on the
# current stream: no read-back, no upload from pageable memory, no host synchronisation of any kind.  A wrapper without a sentence
# of its own that does nothing but check its arguments, allocate and call the C entry point stands under the header's general one.
# A function that is absent here documents a read-back instead (quoted at its cases).  ``Case.enqueue_only`` is set where every
# covered function is listed AND ``run`` itself does nothing else on the host (``HOST_STEPS`` names the cases where it does);
# tests/test_stream_util_cpu.py holds the three tables against each other and every sentence against the two files, word for word
# (line breaks folded).
C_ABI = "Calls enqueue work and return; they never synchronise."
ENQUEUES = {
    "vertex_visibility": "Enqueue K1.",
    "check_visibility": C_ABI,
    "pair_overlap": "Enqueue K2 on K1's bitsets.",
    "scene_overlap": "Enqueue the tiled K2 over ALL pairs i < j of a scene's bitsets",
    "overlap_matrix": "Enqueue the tiled K2 on a rectangle",
    "bits_transpose": C_ABI,
    "select_common_point": "Enqueue K6a.",
    "project_samples": "Enqueue K6b.",
    "object_extents": "Enqueue K8",
    "extract_yaw_pitch": C_ABI,
    "pair_pose": "Enqueue K4.",
    "track_to_world": "Enqueue K5a.",
    "track_displacement": "Enqueue K5b.",
    "track_rigidity_loss": "Enqueue K7",
    "track_rigidity_loss_batch": "Enqueue K7 for equal-shape track blocks in one launch",
    "track_linkage": "Enqueue only: the status is a device tensor like the rest.",
    "track_pair_stats": "Enqueue K5d's statistics.",
    "track_pair_bin_counts": "Enqueue K5d's second pass",
    "track_pair_sort": "Enqueue K5d's segmented sort on its own, in place",
    "track_pair_order": "Enqueue K5d's order",
    "inflate_blocks_device": "Only enqueues; read ``status`` after a synchronisation.",
    "png_unfilter_device": C_ABI,
    "png_unfilter8_device": C_ABI,
    "jpeg_decode_device": "Only enqueues; read ``status`` after a synchronisation.",
    "jpeg_decode_luma_device": "Same arguments, same (out, status) contract; only enqueues.",
    "laplacian_moments": "Only enqueues.",
    "resize_rgb_device": "Only enqueues on the current stream otherwise.",
    "draw_spans_device": C_ABI,
    "blend_masks_device": C_ABI,
    "jpeg_encode_device": "Only enqueues; read ``nbytes`` after a synchronisation.",
    "png_encode_device": "Runs on the current torch stream and only enqueues",
    "parquet_plain_spans_device": "Only enqueues.",
    "parquet_dict_spans_device": "Only enqueues.",
    "rle_hybrid_expand_device": "One lane per value; only enqueues.",
    "pair_bin_codes": "Only enqueues.",
    "pair_partition": "Only enqueues.",
    "index_lists_pick": "Only enqueues: the caller reads ``status`` before a vertex goes anywhere that indexes with it",
    "prep_labels": "Enqueue ``mspa_prep_labels``",
    "prep_align": "Enqueue ``mspa_prep_align``",
}

# pair_reproject's promise holds from a table's second launch on (its cases build a new table every time and so have no
# ``enqueue_only``); tests/test_gpu_stream_order.py runs them once more on a table whose verdict is known.
PAIR_REPROJECT_SEEN_TABLE = "Only enqueues, with one exception: under MSPA_PAIR_FAST the first launch"

# Cases whose covered functions all only enqueue, but whose ``run`` does more on the host than call them.
HOST_STEPS = {
    "heads_end_to_end": "the heads read samples, records and the visibility index back; the prefetcher uploads scenes",
    "prefetch_packed_scenes": "ScenePrefetcher packs on the host, uploads and hands each scene out after its slot's decode",
}


def case(name, family, covers, defined=None, writes=(), enqueue_only=None, aligned=None, own_buffers=(), refused_by=None):
    """Decorator of a class with static ``build`` / ``run`` / ``expect``: registers it as a Case."""
    def register(cls):
        CASES.append(Case(name, family, tuple(covers), cls.build, cls.run, cls.expect, defined, tuple(writes), enqueue_only,
                          dict(aligned) if aligned else None, tuple(own_buffers), refused_by))
        return cls
    return register


# The alignment sentences of include/mspa.h and of the wrappers' docstrings, word for word (tests/test_skew_util_cpu.py holds every
# one against the two files, line breaks folded).  An argument without a sentence is run at its element's alignment: what
# ``engine._check`` lets through.  Where the header offers a route instead of a refusal ("a table at an odd 2-byte offset takes the
# dense route as well", "a launch with one of them elsewhere takes the general kernel of its mode") the argument has no entry and
# is skewed fully: the result must not change.
ALIGN_INFLATE = "src_dev 16-byte, dst_dev and dst_pitch 256-byte aligned"
ALIGN_JPEG_SRC = "src_dev 4-byte aligned"
ALIGN_JPEG_DESC = "desc_dev, 16-byte aligned"
ALIGN_PIX = "out_pix_i16 must be 4-byte aligned (MSPA_EINVAL otherwise)"
ALIGN_CPIX = "out_cpix_i16 must be 16-byte aligned"
ALIGN_CORR_WORKSPACE = "`workspace` (caller-owned, 16-byte aligned, at least mspa_pair_correspondences_workspace_bytes(...) bytes"
ALIGN_PNG_ENCODE = "Alignment: depth_dev 2 bytes, out_dev 4 bytes, nbytes_dev 8 bytes, workspace 16 bytes"
# Sentences about buffers that no case can place, because the wrappers allocate them themselves (``engine._workspace``: "on a 16-byte
# boundary (allocated as int64 pairs)"; the un-filters' ``raw`` is inflate_blocks_device's own output in every chain): each with the
# test that exercises its refusal, or the reason there is none.
ALIGN_WRAPPER_OWNED = {
    "raw_dev 4-byte aligned (MSPA_EINVAL otherwise)": "tests/test_gpu_png_unfilter.py and tests/test_gpu_png_unfilter8.py: test_unaligned_layouts_are_refused",
    "workspace: caller-owned, 16-byte aligned": "engine._workspace allocates it in every wrapper but pair_correspondences (whose case pair_correspondences_own_workspace places one)",
    "bytes (4-byte aligned)": "mspa_overlap_workspace_bytes: an int32 tensor of the wrapper's, element alignment",
    "the workspace of both calls (4-byte aligned)": "mspa_instance_split_workspace_bytes: an int32 tensor of the wrapper's, element alignment",
    "mspa_knn_workspace_bytes(n, k), 16-byte aligned": "engine._workspace allocates it",
    "pix_i16 and out_cpix_i16 must be 4-byte aligned (MSPA_EINVAL otherwise)":
        "mspa_compact_correspondences on its own: no wrapper calls it; tests/test_gpu_compact.py holds its refusal",
    "mspa_knn_segments_workspace_bytes(), 16-byte aligned": "the wrapper of mspa/instances.py allocates it; no case of this registry reaches it",
}
# Sentences that offer a route instead of a refusal, each with the cases that take the other route: no entry, skewed fully.
ALIGN_ROUTES = {
    "`depth` 4-byte aligned (any allocator's base address is): a table at an odd 2-byte offset takes the dense route as well":
        "pair_correspondences_tight96x128 / _rect64x80: depth at 2 mod 4 (mode a) and 6 mod 8 (mode b); the wrapper allocates the workspace",
    "additionally want depth and out_vis_u8 4-byte, out_vis_bits 8-byte and out_pix_i16, out_xyz_f32 and out_rgba 16-byte aligned":
        "pair_reproject_tight96x128 (depth) and pair_reproject_own_* (one output pointer each): the general kernel of the mode runs; "
        "pair_reproject_kept_depth_*: all of them aligned, rgb / mats / pairs skewed, the tile kernels stay",
    "out_dev needs no more than the 2-byte alignment of uint16": "depth_png_own_17x34: the images at 2 mod 4 take the bytes route",
    "pitches in bytes, any alignment": "resize_rgb_device and resize_rgb_device_own: sources and destinations at 1 / 3 mod 4",
}


def skewed_mode():
    """"a" / "b" while tests/test_gpu_skewed_memory.py runs a case skewed, else None: where a case asserts the residue a branch needs."""
    import skew_util
    return skew_util.active_mode()


def own(name, shape, dtype):
    """A buffer the CALLER of an op allocates -- an ``out=``, a status array, a slot -- named so that ``Case.aligned`` can speak of it
    ("own/<name>") and tests/skew_util.py can place it."""
    import skew_util
    return skew_util.caller_buffer(name, shape, dtype, DEV)


def dev(a) -> torch.Tensor:
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(DEV)


def host(x):
    """Tensors of a nesting -> NumPy (the rest as it is)."""
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    if isinstance(x, dict):
        return {k: host(v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return type(x)(host(v) for v in x)
    return x


def pack_rows(masks: np.ndarray) -> np.ndarray:
    """bool [R, n_bits] -> int64 [R, ceil(n_bits / 64)], bit b of row r = masks[r, b] (K1's layout), padding bits zero."""
    R, n_bits = masks.shape
    padded = np.zeros((R, (n_bits + 63) // 64 * 64), dtype=bool)
    padded[:, :n_bits] = masks
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little").view(np.int64)).reshape(R, -1)


def unpack_rows(words: np.ndarray, n_bits: int) -> np.ndarray:
    words = np.ascontiguousarray(words)
    return np.unpackbits(words.view(np.uint8).reshape(words.shape[0], -1), axis=1, bitorder="little")[:, :n_bits].astype(bool)


def nan_equal_bits(a, b):
    """tests/test_gpu_parity.py's: bit-identical where finite / inf, NaN where NaN."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and \
        np.array_equal(np.where(na, 0.0, a).view(np.int64), np.where(nb, 0.0, b).view(np.int64))


def random_masks(R, n_bits, seed, empty_rows=()):
    rng = np.random.default_rng(seed)
    masks = rng.random((R, n_bits)) < rng.random((R, 1)) * 0.4
    for r in empty_rows:
        masks[r] = False
    return masks


# =====================================================================================================================
# K1 / K2 / K9 / K6 / K8
# =====================================================================================================================

@functools.lru_cache(maxsize=None)
def small_scene(hw=(61, 83), dhw=(37, 53), n_points=1000, n_frames=5, seed=4311):
    """61 x 83 colour over 37 x 53 depth, 1000 points, 5 frames: a ragged last wave everywhere, more than one workgroup; frame 3
    has no valid depth (an image that sees nothing)."""
    sc = synth.make_scene(seed, n_points=n_points, n_frames=n_frames, color_hw=hw, depth_hw=dhw, invalid_pose_frac=0.0, with_color=True)
    ids = sc.valid_image_ids
    sc.depth[ids[3]] = np.zeros_like(sc.depth[ids[3]])
    return sc, ids


def scene_on_device(sc, ids):
    return {"xyz": dev(sc.points[:, :3]), "xyz_soa": dev(sc.points[:, :3].T).t(),
            "cam": dev(engine.camera_matrices(sc.K, [sc.A @ sc.E[i] for i in ids])),
            "depth": engine.depth_to_device(np.stack([sc.depth[i] for i in ids]), DEV),
            "mats": dev(engine.frame_matrices(sc.K, sc.A, [sc.E[i] for i in ids])),
            "rgb": dev(np.stack([sc.color[i] for i in ids]))}


K1_WANTS = {"all": ("bits", "mask", "uv", "depth", "count"), "lists": ("bits", "mask", "count"), "bits": ("bits",), "count": ("count",)}


@case("vertex_visibility", "k1k2", ["vertex_visibility"], enqueue_only=ENQUEUES["vertex_visibility"])
class _VertexVisibility:
    @staticmethod
    def build():
        sc, ids = small_scene()
        return {"sc": sc, "ids": ids, **scene_on_device(sc, ids)}

    @staticmethod
    def run(i):
        out = {}
        for layout in ("xyz", "xyz_soa"):                # rows3 and soa; every output set: the reference-order and the compacted kernel
            for name, want in K1_WANTS.items():
                out[f"{layout}.{name}"] = engine.vertex_visibility(i[layout], i["cam"], i["depth"], i["sc"].color_hw, want)
        return out

    @staticmethod
    def expect(i, z):
        sc, ids = i["sc"], i["ids"]
        z = host(z)
        n = sc.points.shape[0]
        masks = O.scene_visibility_masks(sc.points[:, :3], sc.K, sc.A, sc.E, sc.depth, sc.color_hw)
        want = np.stack([masks[k] for k in ids])
        assert want[3].sum() == 0 and want.sum() > 100
        for key, res in z.items():
            if "mask" in res:
                assert np.array_equal(res["mask"].astype(bool), want), key
            if "bits" in res:
                assert np.array_equal(unpack_rows(res["bits"], res["bits"].shape[1] * 64)[:, :n], want), key
                assert not unpack_rows(res["bits"], res["bits"].shape[1] * 64)[:, n:].any(), key
            if "count" in res:
                assert np.array_equal(res["count"], want.sum(axis=1)), key
            if "uv" in res:
                for k, image_id in enumerate(ids):
                    _m, uvc, dc = C.vertex_visibility(sc.points[:, :3], sc.K, sc.A @ sc.E[image_id], sc.depth[image_id], sc.color_hw)
                    assert nan_equal_bits(res["uv"][k], uvc) and nan_equal_bits(res["depth"][k], dc), key


@case("check_visibility", "k1k2", ["check_visibility"], enqueue_only=ENQUEUES["check_visibility"])
class _CheckVisibility:
    @staticmethod
    def build():
        sc, ids = small_scene()
        uv, d = O.project_3d_point_to_image(sc.points[:, :3], sc.K, sc.A @ sc.E[ids[1]])
        return {"sc": sc, "uv_np": uv, "d_np": d, "image": sc.depth[ids[1]], "uv": dev(uv), "d": dev(d),
                "depth_image": engine.depth_to_device(sc.depth[ids[1]][None], DEV)[0]}

    @staticmethod
    def run(i):
        hw = i["sc"].color_hw
        return {"three": engine.check_visibility(i["uv"], i["d"], i["depth_image"], hw, ("in_bounds", "by_depth", "visible")),
                "one": engine.check_visibility(i["uv"], i["d"], i["depth_image"], hw),
                "bounds": engine.check_visibility(i["uv"], None, None, hw, ("in_bounds",))}

    @staticmethod
    def expect(i, z):
        z, hw = host(z), i["sc"].color_hw
        with np.errstate(invalid="ignore"):
            inb = O.check_point_in_image_boundary(i["uv_np"], hw)
            vis = O.check_point_visibility(i["uv_np"], i["d_np"], i["image"], hw)
        assert np.array_equal(z["three"]["in_bounds"].astype(bool), inb) and np.array_equal(z["bounds"]["in_bounds"].astype(bool), inb)
        assert np.array_equal(z["three"]["visible"].astype(bool), vis) and np.array_equal(z["one"]["visible"].astype(bool), vis)
        assert np.array_equal(z["three"]["by_depth"].astype(bool)[inb], vis[inb]) and 0 < vis.sum() < len(vis)


def overlap_reference(masks):
    gram = masks.astype(np.int64) @ masks.astype(np.int64).T
    i, j = np.triu_indices(len(masks), 1)                # all_pairs order (CFR:176-178)
    cnt = np.diag(gram)
    inter, uni = gram[i, j], cnt[i] + cnt[j] - gram[i, j]
    with np.errstate(invalid="ignore"):
        return inter, uni, inter.astype(np.float64) / uni.astype(np.float64) * 100.0, gram


def _overlap_case(name, F, n_bits, unaligned=False):
    """F rows of n_bits bits, rows 3 and F // 2 empty (their pair: an empty union, NaN).  An odd word count takes the popcount tile
    kernel, an even one in a 16-byte aligned table the matrix-core one; ``unaligned`` puts an even count 8 bytes past a boundary."""
    @case(name, "k1k2", ["pair_overlap", "scene_overlap", "overlap_matrix"], enqueue_only=ENQUEUES["pair_overlap"])
    class _Overlap:
        @staticmethod
        def build():
            masks = random_masks(F, n_bits, F * 1000 + n_bits, empty_rows=(3, F // 2))
            other = np.random.default_rng(n_bits).random((max(1, F // 3), n_bits)) < 0.3
            other[0] = False
            words = dev(pack_rows(masks))
            if unaligned:
                buf = torch.zeros((words.numel() + 1,), dtype=torch.int64, device=DEV)
                view = buf[1:].view(words.shape)
                view.copy_(words)
                assert view.data_ptr() % 16 == 8
                words = view
            return {"masks": masks, "other": other, "bits": words, "bits_b": dev(pack_rows(other)), "pairs": engine.all_pairs(F, DEV)}

        @staticmethod
        def run(i):
            return {"pair": engine.pair_overlap(i["bits"], i["pairs"], want_counts=True), "pair_ratio": engine.pair_overlap(i["bits"], i["pairs"]),
                    "scene": engine.scene_overlap(i["bits"], want_counts=True), "scene_ratio": engine.scene_overlap(i["bits"]),
                    "rect": engine.overlap_matrix(i["bits_b"], i["bits"]), "rect_t": engine.overlap_matrix(i["bits"], i["bits_b"]),
                    "sym": engine.overlap_matrix(i["bits"], i["bits"])}

        @staticmethod
        def expect(i, z):
            z = host(z)
            inter, uni, ratio, gram = overlap_reference(i["masks"])
            assert np.isnan(ratio).sum() >= 1                # rows 3 and F // 2: an empty union
            for key in ("pair", "scene"):
                assert nan_equal_bits(z[key][0], ratio) and np.array_equal(z[key][1], inter) and np.array_equal(z[key][2], uni), key
                assert nan_equal_bits(z[key + "_ratio"], ratio), key
            for p in (0, len(ratio) // 2, len(ratio) - 1):
                a, b = np.triu_indices(len(i["masks"]), 1)
                ref = O.calculate_camera_overlap(i["masks"][a[p]], i["masks"][b[p]])
                assert (np.isnan(ref) and np.isnan(ratio[p])) or ref == ratio[p]
            rect = i["other"].astype(np.int64) @ i["masks"].astype(np.int64).T
            assert np.array_equal(z["rect"], rect) and np.array_equal(z["rect_t"], rect.T) and np.array_equal(z["sym"], gram)
    return _Overlap


_overlap_case("overlap_odd_words_700", 33, 700)                         # 11 words: the popcount tile kernel; a ragged second row tile
_overlap_case("overlap_even_words_8320", 70, 8320)                      # 130 words in an aligned table: the matrix-core tiles, three row tiles
_overlap_case("overlap_even_words_unaligned", 33, 66 * 64, unaligned=True)   # an even count 8 bytes past a 16-byte boundary
# tests/test_gpu_skewed_memory.py puts every int64 table at 8 mod 16 (data_ptr() % 16 == 8, asserted there): pair_overlap_kernel's
# 16-byte pieces of an even-count row then sit at 8 mod 16 (csrc/pair_overlap.hip says why that stands), and launch_tiles'
# ``((uintptr_t)bits_a & 15u) == 0`` fails, so overlap_even_words_8320 takes the popcount tiles where its plain run took the matrix cores.


@case("overlap_no_words", "k1k2", ["scene_overlap", "overlap_matrix"], enqueue_only=ENQUEUES["scene_overlap"])
class _OverlapNoWords:
    """Bitsets of no points (n_words == 0): every union is empty -> NaN, every intersection 0.  No kernel has a word to read, so
    the wrappers have to write the results themselves (pair_overlap refuses such a table: it has no address)."""
    @staticmethod
    def build():
        return {"bits": torch.zeros((5, 0), dtype=torch.int64, device=DEV), "pairs": engine.all_pairs(5, DEV)}

    @staticmethod
    def run(i):
        return {"scene": engine.scene_overlap(i["bits"], want_counts=True), "scene_ratio": engine.scene_overlap(i["bits"]),
                "rect": engine.overlap_matrix(i["bits"][:2], i["bits"]), "no_rows": engine.overlap_matrix(i["bits"][:0], i["bits"])}

    @staticmethod
    def expect(i, z):
        z = host(z)
        assert np.isnan(z["scene"][0]).all() and z["scene"][0].shape == (10,) and not z["scene"][1].any() and not z["scene"][2].any()
        assert np.isnan(z["scene_ratio"]).all() and z["rect"].shape == (2, 5) and not z["rect"].any() and z["no_rows"].shape == (0, 5)


def _bitset_case(name, R, n_bits):
    @case(name, "k1k2", ["bitset_csr", "bits_transpose"])          # bitset_csr: "One small read-back (the number of set bits: the size to allocate)"
    class _Bitset:
        @staticmethod
        def build():
            masks = random_masks(R, n_bits, R * 7 + n_bits, empty_rows=(R // 2,))
            masks[0, :3] = True
            masks[-1, -1] = True
            return {"masks": masks, "bits": dev(pack_rows(masks))}

        @staticmethod
        def run(i):
            t = engine.bits_transpose(i["bits"])
            return {"csr": engine.bitset_csr(i["bits"]), "t": t, "csr_t": engine.bitset_csr(t)}       # the transpose WITH its padding rows

        @staticmethod
        def expect(i, z):
            z, masks = host(z), i["masks"]
            off, idx = z["csr"]
            assert off[0] == 0 and off[-1] == masks.sum() == len(idx)
            for r in range(R):
                assert np.array_equal(idx[off[r]:off[r + 1]], np.nonzero(masks[r])[0])
            n_words = (n_bits + 63) // 64
            assert z["t"].shape == (n_words * 64, (R + 63) // 64)
            tb = unpack_rows(z["t"], z["t"].shape[1] * 64)
            # "(padding bits zero)": bits_transpose's docstring -- compared above, asserted here
            assert np.array_equal(tb[:n_bits, :R], masks.T) and not tb[:, R:].any() and not tb[n_bits:].any()
            off2, idx2 = z["csr_t"]
            assert off2[-1] == masks.sum() and (np.diff(off2)[n_bits:] == 0).all()
            for v in range(0, n_bits, 37):
                assert np.array_equal(idx2[off2[v]:off2[v + 1]], np.nonzero(masks[:, v])[0])
    return _Bitset


_bitset_case("bitset_5x700", 5, 700)
_bitset_case("bitset_70x8320", 70, 8320)


@case("bitset_empty", "k1k2", ["bitset_csr", "bits_transpose"])          # bitset_csr's read-back of the number of set bits
class _BitsetEmpty:
    @staticmethod
    def build():
        return {"none": torch.zeros((0, 3), dtype=torch.int64, device=DEV), "zeros": torch.zeros((33, 11), dtype=torch.int64, device=DEV)}

    @staticmethod
    def run(i):
        return {"t_none": engine.bits_transpose(i["none"]), "csr_none": engine.bitset_csr(i["none"]),
                "t_zeros": engine.bits_transpose(i["zeros"]), "csr_zeros": engine.bitset_csr(i["zeros"])}

    @staticmethod
    def expect(i, z):
        z = host(z)
        assert z["t_none"].shape == (192, 0) and z["t_zeros"].shape == (704, 1) and not z["t_zeros"].any()
        assert z["csr_none"][0].tolist() == [0] and len(z["csr_none"][1]) == 0
        assert not z["csr_zeros"][0].any() and z["csr_zeros"][0].shape == (34,) and len(z["csr_zeros"][1]) == 0


def _common_point_case(name, F, n_bits):
    @case(name, "k1k2", ["select_common_point"], enqueue_only=ENQUEUES["select_common_point"])
    class _CommonPoint:
        @staticmethod
        def build():
            rng = np.random.default_rng(n_bits + F)
            masks = random_masks(F, n_bits, n_bits * 3 + F, empty_rows=(2,))
            masks[1] = rng.random(n_bits) < 0.9           # dense rows: their common list runs through every word a lane owns
            masks[4] = rng.random(n_bits) < 0.9
            sel, want = [], []
            for k in range(300):
                a, b = (1, 4) if k % 3 == 0 else rng.integers(0, F, 2)
                common = np.nonzero(masks[a] & masks[b])[0]           # np.intersect1d of the two visible lists
                j = int(rng.integers(0, len(common) + 3)) if k % 7 else max(len(common) - 1, 0)      # past the end; the very last
                sel.append([a, b, j])
                want.append(int(common[j]) if j < len(common) else -1)
            return {"bits": dev(pack_rows(masks)), "sel": dev(np.asarray(sel, dtype=np.int32)), "want": np.asarray(want, dtype=np.int32)}

        @staticmethod
        def run(i):
            return engine.select_common_point(i["bits"], i["sel"])

        @staticmethod
        def expect(i, z):
            got = host(z)
            assert np.array_equal(got, i["want"]) and (got >= 0).sum() > 100 and (got == -1).sum() > 10     # "-1 if out of range": compared
            assert got.max() > 0.95 * n_bits
    return _CommonPoint


_common_point_case("select_common_point_700", 9, 700)
_common_point_case("select_common_point_8320", 9, 8320)                # 130 words: a lane owns more than one word, with a carry


@case("project_samples", "k1k2", ["project_samples"], enqueue_only=ENQUEUES["project_samples"])
class _ProjectSamples:
    @staticmethod
    def build():
        sc, ids = small_scene()
        rng = np.random.default_rng(5)
        smp = np.stack([rng.integers(0, sc.points.shape[0], 333), rng.integers(0, len(ids), 333)], axis=1).astype(np.int32)
        return {"sc": sc, "ids": ids, "smp": smp, "samples": dev(smp), **scene_on_device(sc, ids)}

    @staticmethod
    def run(i):
        return {"rows": engine.project_samples(i["xyz"], i["cam"], i["depth"], i["sc"].color_hw, i["samples"]),
                "soa": engine.project_samples(i["xyz_soa"], i["cam"], i["depth"], i["sc"].color_hw, i["samples"])}

    @staticmethod
    def expect(i, z):
        sc, ids, z = i["sc"], i["ids"], host(z)
        uv, d, ok = z["rows"]
        for a, b in zip(z["rows"], z["soa"]):
            assert nan_equal_bits(a, b)
        per_image = [C.vertex_visibility(sc.points[:, :3], sc.K, sc.A @ sc.E[k], sc.depth[k], sc.color_hw) for k in ids]
        for n, (v, img) in enumerate(i["smp"]):
            m, uvc, dc = per_image[img]
            assert bool(ok[n]) == bool(m[v]) and nan_equal_bits(uv[n], uvc[v]) and nan_equal_bits(d[n], dc[v])
        assert 0 < ok.sum() < len(ok)


@case("object_extents", "k1k2", ["object_extents"], enqueue_only=ENQUEUES["object_extents"])
class _ObjectExtents:
    @staticmethod
    def build():
        rng = np.random.default_rng(12)
        V, F, n_obj = 1000, 33, 7
        pts = rng.normal(0, 2, (V, 3))
        label = rng.integers(-1, n_obj, V)
        objs = [np.where(label == o)[0] for o in range(n_obj)]
        objs[2] = objs[2][:0]                              # an object with no vertices
        objs[3] = objs[3][:1]                              # a one-vertex object
        objs[5] = rng.permutation(objs[5])
        seen = rng.random((F, V)) < rng.uniform(0.0, 0.3, (F, 1))
        seen[4] = False                                    # an image that sees nothing
        off = np.zeros(n_obj + 1, dtype=np.int32)
        np.cumsum([len(o) for o in objs], out=off[1:])
        return {"pts": pts, "objs": objs, "seen": seen, "bits": dev(pack_rows(seen)), "xyz": dev(pts), "off": dev(off),
                "verts": dev(np.concatenate(objs).astype(np.int32))}

    @staticmethod
    def run(i):
        return engine.object_extents(i["bits"], i["xyz"], i["off"], i["verts"])

    @staticmethod
    def expect(i, z):
        lo, hi, count = host(z)
        pts, seen = i["pts"], i["seen"]
        for o, idx in enumerate(i["objs"]):
            m = np.zeros(len(pts), dtype=bool)
            m[idx] = True
            for f in range(seen.shape[0]):
                both = seen[f] & m
                assert count[o, f] == both.sum()
                if not both.any():                         # promised values, compared between the runs as well: +inf / -inf
                    assert (lo[o, f] == np.inf).all() and (hi[o, f] == -np.inf).all()
                else:
                    assert np.array_equal(lo[o, f], pts[both].min(axis=0)) and np.array_equal(hi[o, f], pts[both].max(axis=0))
                    for axis in range(3):
                        assert hi[o, f, axis] - lo[o, f, axis] == O.compute_coverage(pts, both, axis)
        assert not count[2].any() and not count[:, 4].any() and count.sum() > 100


# =====================================================================================================================
# K3
# =====================================================================================================================

K3_SHAPES = {"tight96x128": ((96, 128), (96, 128)),        # whole tiles, colour grid == depth grid: the tight kernels
             "ragged61x83": ((61, 83), (37, 53)),          # nothing divides: the exact, the general fast and the linear fast kernel
             "rect64x80": ((64, 80), (32, 40))}            # rect_shape: the tight kernel's scaled form
# Skewed (tests/test_gpu_skewed_memory.py) the depth table of every K3 case sits at 2 mod 4 / 6 mod 8: pair_reproject_impl's
# ``((uintptr_t)depth & 3u) == 0`` fails, the whole-tile and rectangular-tile kernels are not taken (tight96x128, rect64x80: the
# general kernels run where the plain run took the tight ones), and mspa_pair_correspondences goes through the dense table.
K3_PAIRS = [(0, 1), (1, 0), (0, 4), (2, 2), (3, 0), (0, 3)]         # an identity pair; frame 3 has no valid depth
K3_EXACT = ("vis_bits", "vis_u8", "valid_u8", "pix_i16", "xyz_f32", "xyz_f64", "uv_f64", "depth_f64", "counts", "rgba")
K3_FAST_SETS = {"generic": ("vis_bits", "vis_u8", "valid_u8", "pix_i16", "xyz_f32", "counts"), "corr": ("vis_bits", "pix_i16", "counts"),
                "minimal": ("vis_bits", "counts"), "dense": ("vis_u8", "pix_i16", "xyz_f32", "rgba", "counts"),
                "dense_xyz": ("vis_u8", "pix_i16", "xyz_f32", "counts"), "bytes": ("vis_u8", "valid_u8", "pix_i16", "counts")}


def _k3_inputs(shape):
    hw, dhw = K3_SHAPES[shape]
    sc, ids = small_scene(hw, dhw, 64, 5, 1010)
    return {"sc": sc, "ids": ids, "hw": hw, "pairs": dev(np.asarray(K3_PAIRS, dtype=np.int32)), **scene_on_device(sc, ids)}


def _k3_references(i):
    sc, ids = i["sc"], i["ids"]
    return [(C.frame_pair(sc.depth[ids[a]], sc.depth[ids[b]], sc.K, sc.E[ids[a]], sc.E[ids[b]], sc.A, i["hw"]),
             O.frame_pair(sc.depth[ids[a]], sc.depth[ids[b]], sc.K, sc.E[ids[a]], sc.E[ids[b]], sc.A, i["hw"], sc.color[ids[a]]))
            for a, b in K3_PAIRS]


def _pair_reproject_case(shape):
    # pair_reproject: "under MSPA_PAIR_FAST the first launch on a ``mats`` tensor object [...] reads the pinhole verdict back" -- and
    # build() makes a new table every time
    @case(f"pair_reproject_{shape}", "k3", ["pair_reproject"])
    class _PairReproject:
        @staticmethod
        def build():
            return _k3_inputs(shape)

        @staticmethod
        def run(i):
            n = len(K3_PAIRS)                             # the outputs come from alloc_pair_outputs UNDER the patch
            out = {"exact": engine.pair_reproject(i["depth"], i["mats"], i["pairs"], i["hw"],
                                                  engine.alloc_pair_outputs(n, i["hw"], K3_EXACT, DEV), rgb=i["rgb"])}
            for name, outs in K3_FAST_SETS.items():
                for suffix, flags in (("", _lib.PAIR_FAST), ("_stream", _lib.PAIR_FAST | _lib.PAIR_STREAM)):
                    out[name + suffix] = engine.pair_reproject(i["depth"], i["mats"], i["pairs"], i["hw"], engine.alloc_pair_outputs(n, i["hw"], outs, DEV),
                                                               rgb=i["rgb"] if "rgba" in outs else None, flags=flags)
            return out

        @staticmethod
        def expect(i, z):
            from test_gpu_parity import check_pair_against
            z, refs = host(z), _k3_references(i)
            for n, ((a, _b), (ref_c, ref_np)) in enumerate(zip(K3_PAIRS, refs)):
                check_pair_against(z["exact"], n, ref_c, ref_np, i["hw"], i["sc"].color[i["ids"][a]])
                check_pair_against(z["generic"], n, ref_c, ref_np, i["hw"])
            assert sum(r["n_vis"] for _c, r in refs) > 100 and refs[4][1]["n_valid"] == 0
            for name, outs in [(n + sfx, o) for n, o in K3_FAST_SETS.items() for sfx in ("", "_stream")]:
                for k in outs:                            # the specialised sets: the exact kernel's integers, float32 points to ~1 ulp
                    if k != "xyz_f32":
                        assert np.array_equal(z[name][k], z["exact"][k]), (name, k)
                    else:
                        valid = z["exact"]["valid_u8"].astype(bool)
                        assert np.isnan(z[name][k][~valid]).all(), name
                        assert np.allclose(z[name][k][valid], z["exact"][k][valid], rtol=2e-7, atol=1e-7), name
    return _PairReproject


def _cpix_defined(which):
    # include/mspa.h, mspa_pair_correspondences: "the k-th set bit of the tile's part of the bitset <-> entry k; entries beyond the
    # tile's count are unspecified"
    def mask(zero):
        out = host(zero[which]["out"])
        cap = out["cpix"].shape[2]
        return np.broadcast_to((np.arange(cap)[None, None, :] < out["tile_counts"][:, :, None])[..., None], out["cpix"].shape)
    return mask


def _pair_correspondences_case(shape):
    # correspondences_rowmajor: torch.nonzero reads the number of visible pixels back ("torch indexing as plumbing")
    @case(f"pair_correspondences_{shape}", "k3", ["pair_correspondences", "correspondences_rowmajor"],
          defined={"fast/out/cpix": _cpix_defined("fast"), "reference_order/out/cpix": _cpix_defined("reference_order"),
                   "stream/out/cpix": _cpix_defined("stream")})
    class _PairCorrespondences:
        @staticmethod
        def build():
            return _k3_inputs(shape)

        @staticmethod
        def run(i):
            out = {}
            for name, flags in (("fast", _lib.PAIR_FAST), ("reference_order", 0), ("stream", _lib.PAIR_FAST | _lib.PAIR_STREAM)):
                # outputs AND workspace allocated by the wrapper
                res = engine.pair_correspondences(i["depth"], i["mats"], i["pairs"], i["hw"], flags=flags)
                out[name] = {"out": res, "rowmajor": [engine.correspondences_rowmajor(res, i["hw"], n) for n in range(len(K3_PAIRS))]}
            return out

        @staticmethod
        def expect(i, z):
            from test_gpu_compact import check_pair
            z, refs = host(z), _k3_references(i)
            for name in ("fast", "reference_order", "stream"):
                for n, (_c, ref) in enumerate(refs):
                    check_pair(z[name]["out"], n, ref, i["hw"])
                    pix, xi, yi = z[name]["rowmajor"][n]
                    nz = np.nonzero(ref["vis"])[0]
                    assert np.array_equal(pix, nz) and np.array_equal(xi, ref["xi"][nz]) and np.array_equal(yi, ref["yi"][nz]), (name, n)
    return _PairCorrespondences


for _shape in K3_SHAPES:
    _pair_reproject_case(_shape)
    _pair_correspondences_case(_shape)


class Kept:
    """An input that tests/skew_util.py and tests/fence_util.py leave where the allocator put it (they walk dicts, lists and tuples
    only): the depth table of the cases below, which are about ONE output pointer each -- a skewed depth table alone already takes the
    whole-tile kernel away (the K3 cases above, tests/pair_route_cases.py's ``misaligned``)."""
    def __init__(self, tensor):
        self.tensor = tensor


# csrc/pair_reproject.hip, pair_reproject_impl: "the tight kernel's LDS-DMA moves depth in 4-byte units and its 16-byte stores need
# aligned outputs" -- the alignment below which each pointer takes the whole-tile kernel away from a launch
K3_POINTER_NEEDS = {"pix_i16": 16, "vis_bits": 8, "cpix": 16, "xyz_f32": 16, "rgba": 16, "vis_u8": 4}


def _k3_check_some(res, n, ref_np, hw, color):
    """tests/test_gpu_parity.py's ``check_pair_against`` for whichever of the fast outputs ``res`` holds."""
    valid, vis = ref_np["valid"], ref_np["vis"]
    if "vis_u8" in res:
        assert np.array_equal(res["vis_u8"][n].astype(bool), vis)
    if "vis_bits" in res:
        assert np.array_equal(unpack_rows(res["vis_bits"][n:n + 1], hw[0] * hw[1])[0], vis)
    assert tuple(res["counts"][n]) == (ref_np["n_valid"], ref_np["n_vis"])
    if "pix_i16" in res:
        pix = res["pix_i16"][n]
        with np.errstate(invalid="ignore"):
            inview = valid & O.check_point_in_image_boundary(ref_np["uv2"], hw) & (ref_np["depth2"] > 0)
        assert np.array_equal(pix[inview, 0], ref_np["xi"][inview]) and np.array_equal(pix[inview, 1], ref_np["yi"][inview])
        assert (pix[~inview] == -1).all()
    if "rgba" in res:
        exp = color.reshape(-1, 3).astype(np.uint32)
        exp = exp[:, 0] | (exp[:, 1] << 8) | (exp[:, 2] << 16) | np.where(valid, 0xFF000000, 0).astype(np.uint32)
        assert np.array_equal(res["rgba"][n].view(np.uint32), exp)
    if "xyz_f32" in res:
        assert np.isnan(res["xyz_f32"][n][~valid]).all()
        assert np.allclose(res["xyz_f32"][n][valid], ref_np["xyz"][valid], rtol=2e-7, atol=1e-7)


def _k3_own_output_case(name, set_name):
    """A whole-tile MSPA_PAIR_FAST launch (96 x 128: tests/pair_route_cases.py's smallest) in which ONE output is the caller's own
    buffer and every other pointer, the depth table included, is the allocator's.  Skewed, that output sits one / three units past
    a boundary -- int16 pairs at 4 mod 8 (their documented 4 bytes), float32 and int32 at 4 / 12 mod 16, uint8 at 1 / 3 mod 4, int64
    at 8 mod 16 -- and route() (csrc/pair_route.h) sees ``aligned == false`` exactly when ``data_ptr() % K3_POINTER_NEEDS[name]``
    is not 0: the general whole-tile kernel (MSPA_KERNEL_PAIR_FAST) then runs instead of MSPA_KERNEL_PAIR_FAST_TIGHT, which ``run``
    asserts from the pointers it handed over; a bitset at 8 mod 16 keeps the tight kernel (it needs 8)."""
    outputs = K3_FAST_SETS[set_name]

    @case(f"pair_reproject_own_{name}", "k3", ["pair_reproject"], aligned={"own/pix_i16": (4, ALIGN_PIX)} if name == "pix_i16" else None,
          own_buffers=(name,))
    class _OwnOutput:
        @staticmethod
        def build():
            i = _k3_inputs("tight96x128")
            i["depth"] = Kept(i["depth"])
            return i

        @staticmethod
        def run(i):
            import pair_route_cases as R
            n, hw, depth = len(K3_PAIRS), i["hw"], i["depth"].tensor
            out = engine.alloc_pair_outputs(n, hw, outputs, DEV)
            out[name] = own(name, out[name].shape, out[name].dtype)
            engine.pair_reproject(depth, i["mats"], i["pairs"], hw, out, rgb=i["rgb"] if "rgba" in outputs else None, flags=_lib.PAIR_FAST)
            ran = _lib.load().mspa_pair_reproject_last_kernel()
            assert depth.data_ptr() % 4 == 0 and all(t.data_ptr() % K3_POINTER_NEEDS[k] == 0 for k, t in out.items() if k in K3_POINTER_NEEDS and k != name)
            aligned = out[name].data_ptr() % K3_POINTER_NEEDS[name] == 0
            want = R.parent_route(hw[0], hw[1], hw[0], hw[1], R.bits(outputs), aligned, R.FAST)
            assert want.err == 0 and want.family == (R.TIGHT_FAMILY if aligned else R.FAST_FAMILY) and ran == want.family, (name, aligned, ran, want)
            return out

        @staticmethod
        def expect(i, z):
            z = host(z)
            for n, ((a, _b), (_c, ref_np)) in enumerate(zip(K3_PAIRS, _k3_references(i))):
                _k3_check_some(z, n, ref_np, i["hw"], i["sc"].color[i["ids"][a]])
    return _OwnOutput


for _name, _set in (("pix_i16", "dense"), ("xyz_f32", "dense"), ("rgba", "dense"), ("vis_u8", "dense"), ("vis_bits", "corr")):
    _k3_own_output_case(_name, _set)


def _k3_kept_depth_case(shape, set_names, family):
    """MSPA_PAIR_FAST launches whose depth table and outputs are the allocator's, so that route() keeps the whole-tile (96 x 128)
    or the rectangular-tile (64 x 80 over 32 x 40) kernel while ``rgb``, ``mats`` and ``pairs`` are skewed -- ``run`` asserts the
    family that ran.  The whole-tile kernel's dense set reads a row's colour bytes with one 32-bit buffer load per lane at byte
    ``stripe * 192 + 3 * lane - 1`` of the row (lane 0: byte 0): (rgb + f1 * P * 3 + row * W * 3 + 3 * lane - 1) % 4 takes every
    residue in any run, wherever ``rgb`` starts, and no load begins in front of ``rgb``; there is no guard and none is needed (the
    rectangular kernel has no set with colour).  What moves with rgb % 4 = 1 / 3 is WHICH lanes load off a word."""
    @case(f"pair_reproject_kept_depth_{shape}", "k3", ["pair_reproject"])
    class _KeptDepth:
        @staticmethod
        def build():
            i = _k3_inputs(shape)
            i["depth"] = Kept(i["depth"])
            return i

        @staticmethod
        def run(i):
            import pair_route_cases as R
            n, hw, depth = len(K3_PAIRS), i["hw"], i["depth"].tensor
            dh, dw = depth.shape[1:]
            mode = skewed_mode()
            if mode:                                      # uint8 at 1 / 3 mod 4, float64 at 8 mod 16, int32 at 4 / 12 mod 16
                assert i["rgb"].data_ptr() % 4 == {"a": 1, "b": 3}[mode] and i["mats"].data_ptr() % 16 == 8
                assert i["pairs"].data_ptr() % 16 == {"a": 4, "b": 12}[mode] and depth.data_ptr() % 4 == 0
            out = {}
            for name in set_names:
                outputs = K3_FAST_SETS[name]
                for suffix, flags in (("", _lib.PAIR_FAST), ("_stream", _lib.PAIR_FAST | _lib.PAIR_STREAM)):
                    res = engine.alloc_pair_outputs(n, hw, outputs, DEV)
                    engine.pair_reproject(depth, i["mats"], i["pairs"], hw, res, rgb=i["rgb"] if "rgba" in outputs else None, flags=flags)
                    ran = _lib.load().mspa_pair_reproject_last_kernel()
                    want = R.parent_route(dh, dw, hw[0], hw[1], R.bits(outputs), True, flags)
                    assert want.err == 0 and ran == want.family == family, (shape, name, suffix, ran, want)
                    out[name + suffix] = res
            return out

        @staticmethod
        def expect(i, z):
            z = host(z)
            for n, ((a, _b), (_c, ref_np)) in enumerate(zip(K3_PAIRS, _k3_references(i))):
                for res in z.values():
                    _k3_check_some(res, n, ref_np, i["hw"], i["sc"].color[i["ids"][a]])
    return _KeptDepth


_k3_kept_depth_case("tight96x128", ("dense", "dense_xyz", "corr", "minimal"), 4)      # MSPA_KERNEL_PAIR_FAST_TIGHT
_k3_kept_depth_case("rect64x80", ("corr", "minimal"), 6)                               # MSPA_KERNEL_PAIR_FAST_RECT


def _corr_own_case(name, shape, sentence):
    """mspa_pair_correspondences with the caller's own ``cpix`` (the fused kernel, 96 x 128) or ``workspace`` (61 x 83: the dense
    route): both documented 16 bytes, so both sit at 16 mod 32 and nothing may change; 8 mod 16 is refused."""
    @case(f"pair_correspondences_own_{name}", "k3", ["pair_correspondences"], aligned={f"own/{name}": (16, sentence)}, own_buffers=(name,),
          defined={"cpix": lambda zero: np.broadcast_to((np.arange(host(zero["cpix"]).shape[2])[None, None, :] <
                                                         host(zero["tile_counts"])[:, :, None])[..., None], zero["cpix"].shape)})
    class _OwnCorr:
        @staticmethod
        def build():
            i = _k3_inputs(shape)
            i["depth"] = Kept(i["depth"])
            return i

        @staticmethod
        def run(i):
            n, hw, depth = len(K3_PAIRS), i["hw"], i["depth"].tensor
            out = engine.alloc_pair_correspondences(n, hw, DEV)
            workspace = None
            if name == "cpix":
                out["cpix"] = own("cpix", out["cpix"].shape, out["cpix"].dtype)
            else:
                workspace = own("workspace", (n * hw[0] * hw[1],), torch.int32)
            return engine.pair_correspondences(depth, i["mats"], i["pairs"], hw, out, flags=_lib.PAIR_FAST, workspace=workspace)

        @staticmethod
        def expect(i, z):
            from test_gpu_compact import check_pair
            z = host(z)
            for n, (_c, ref) in enumerate(_k3_references(i)):
                check_pair(z, n, ref, i["hw"])
    return _OwnCorr


_corr_own_case("cpix", "tight96x128", ALIGN_CPIX)
_corr_own_case("workspace", "ragged61x83", ALIGN_CORR_WORKSPACE)


# =====================================================================================================================
# K4 / K5 / K7
# =====================================================================================================================

def _f64_ok(a, b):
    from golden_util import close_f64, same_f64
    return same_f64(a, b) or close_f64(a, b, rtol=1e-12, scale=1e-9)


@case("extract_yaw_pitch", "tracks", ["extract_yaw_pitch"], enqueue_only=ENQUEUES["extract_yaw_pitch"])
class _YawPitch:
    @staticmethod
    def build():
        rng = np.random.default_rng(8)
        Ea = []
        for _ in range(70):
            q, _r = np.linalg.qr(rng.normal(size=(3, 3)))
            e = np.eye(4)
            e[:3, :3] = q
            Ea.append(e)
        up = np.eye(4)
        up[:3, :3] = [[1, 0, 0], [0, 0, -1], [0, 1, 0]]
        Ea.append(up)
        return {"Ea": Ea, "E": dev(np.stack(Ea).reshape(-1, 16))}

    @staticmethod
    def run(i):
        return engine.extract_yaw_pitch(i["E"])

    @staticmethod
    def expect(i, z):
        yaw, pitch = host(z)              # tests/test_gpu_parity.py::test_extract_yaw_pitch_device_vs_reference_values' bar: 1e-12 degrees
        yaw_h, pitch_h = engine.extract_yaw_pitch_host(i["Ea"])
        assert np.abs(yaw - yaw_h).max() < 1e-12 and np.abs(pitch - pitch_h).max() < 1e-12
        assert abs(yaw[-1] + 90.0) < 1e-12 and abs(pitch[-1]) < 1e-12


@case("pair_pose", "tracks", ["pair_pose"], enqueue_only=ENQUEUES["pair_pose"])
class _PairPose:
    @staticmethod
    def build():
        from golden_util import GoldenScene
        g = GoldenScene("scene_ident")
        Ea = [g.A @ g.E[k] for k in g.valid_image_ids]
        yaw, pitch = engine.extract_yaw_pitch_host(Ea)
        pairs = engine.all_pairs(len(Ea), DEV)
        return {"g": g, "E": dev(np.stack(Ea).reshape(-1, 16)), "Einv": dev(np.stack([np.linalg.inv(e) for e in Ea]).reshape(-1, 16)),
                "yaw": dev(yaw), "pitch": dev(pitch), "n": pairs.shape[0], "both": torch.cat([pairs, pairs.flip(1)], dim=0).contiguous()}

    @staticmethod
    def run(i):
        return engine.pair_pose(i["E"], i["Einv"], i["yaw"], i["pitch"], i["both"])

    @staticmethod
    def expect(i, z):
        import json
        from golden_util import same_f64
        out, g, n = host(z), i["g"], i["n"]          # tests/test_gpu_parity.py::test_pair_pose_golden
        ref = g["cfr_values"]
        assert _f64_ok(out[:n, 0], ref[:, 1]) and same_f64(out[:n, 1], ref[:, 2]) and same_f64(out[:n, 2], ref[:, 3])
        for p, (swap, ans) in enumerate(zip(g["cme_swap"], g["cme_answers_json"])):
            a = json.loads(str(ans))
            d = out[p + n, 3:6] if swap else out[p, 3:6]
            assert _f64_ok(d, a["displacement_vector"]) and [int(v * 1000) for v in d] == [a["x_value"], a["y_value"], a["z_value"]]


TRACK_T, TRACK_P = 40, 50


@functools.lru_cache(maxsize=None)
def small_tracks():
    tr = synth.make_tracks(910, T=TRACK_T, P=TRACK_P, n_groups=3)
    xyz = np.ascontiguousarray(tr.tracks_XYZ)
    xyz[5, 7] = [0.3, 0.2, -1.0]                  # behind the camera, outside the image, on the reference's epsilon, at the origin
    xyz[6, 7] = [50.0, 0.0, 1.0]
    xyz[7, 7] = [0.0, 0.0, -1e-8]
    xyz[8, 7] = [0.0, 0.0, 0.0]
    return tr, xyz


# track_pair_distances: "four small tables go up from pageable memory and the distances come back to the host"
@case("track_geometry", "tracks", ["track_to_world", "track_displacement", "track_pair_distances"])
class _TrackGeometry:
    """K5a -> K5b and K5c, which read K5a's world positions."""
    @staticmethod
    def build():
        tr, xyz = small_tracks()
        rng = np.random.default_rng(910)
        T, P = TRACK_T, TRACK_P
        trip = np.stack([rng.integers(0, T, 333), rng.integers(0, T, 333), rng.integers(0, P, 333)], 1).astype(np.int32)
        trip[:20, 1] = trip[:20, 0]
        trip[20:30, 2] = 7
        trip[20:30, 0] = np.arange(0, 10)
        vis = np.array(tr.visibility, dtype=bool)
        vis[:, 3] = False                            # a point visible in no frame, in one frame, in all T frames
        vis[:, 4] = False
        vis[11, 4] = True
        vis[:, 6] = True
        pts = [3, 4, 6] + rng.choice(np.arange(8, P), 9, replace=False).tolist()
        return {"tr": tr, "xyz": xyz, "trip": trip, "vis": vis, "pts": pts, "frames": [np.where(vis[:, p])[0] for p in pts],
                "tracks": dev(xyz), "c2w": dev(np.linalg.inv(tr.extrinsics_w2c).reshape(T, 16)),
                "w2c": dev(np.ascontiguousarray(tr.extrinsics_w2c).reshape(T, 16)), "triples": dev(trip)}

    @staticmethod
    def run(i):
        tr = i["tr"]
        res = engine.track_to_world(i["tracks"], i["c2w"], tr.fx_fy_cx_cy, tr.image_hw)
        return {"k5a": res, "k5a_camera": engine.track_to_world(i["tracks"], None, tr.fx_fy_cx_cy, tr.image_hw, want=("uvn", "ok")),
                "k5b": engine.track_displacement(res["world"], i["w2c"], i["c2w"], i["triples"]),
                "k5c": engine.track_pair_distances(res["world"], i["pts"], i["frames"])}

    @staticmethod
    def expect(i, z):
        from golden_util import same_f64
        tr, xyz, z = i["tr"], i["xyz"], host(z)          # tests/test_gpu_tracks_full.py at T = 40, P = 50
        H, W = tr.image_hw
        world = z["k5a"]["world"]
        assert _f64_ok(world, O.tracks_cam_to_world(xyz, tr.extrinsics_w2c))
        fx, fy, cx, cy = tr.fx_fy_cx_cy
        with np.errstate(divide="ignore", invalid="ignore"):
            un = ((fx * xyz[..., 0] / (xyz[..., 2] + 1e-8)) + cx) / W
            vn = ((fy * xyz[..., 1] / (xyz[..., 2] + 1e-8)) + cy) / H
        ok_ref = (0 <= un) & (un < 1) & (0 <= vn) & (vn < 1) & (xyz[..., 2] > 0)
        for key in ("k5a", "k5a_camera"):
            ok, uvn = z[key]["ok"].astype(bool), z[key]["uvn"]
            assert np.array_equal(ok, ok_ref) and not ok[5:9, 7].any()
            assert same_f64(uvn[ok][:, 0], un[ok]) and same_f64(uvn[ok][:, 1], vn[ok])
        ok = z["k5a"]["ok"].astype(bool)
        for p, d in zip(i["pts"], z["k5c"]):
            want, _f1, _f2 = O.point_pair_distances(world, i["vis"], p)
            assert d.shape == want.shape and np.array_equal(d, want)
        assert [len(d) for d in z["k5c"][:3]] == [0, 0, TRACK_T * (TRACK_T - 1) // 2]
        disp, flags = z["k5b"]
        n_checked = 0
        for k, (f1, f2, p) in enumerate(i["trip"].tolist()):
            o = O.object_displacement(world, xyz, tr.extrinsics_w2c, tr.fx_fy_cx_cy, (H, W), f1, f2, p)
            assert (o is None) == (not (ok[f1, p] and ok[f2, p]))
            assert flags[k, 0] == int(not (np.linalg.norm(world[f2, p] - world[f1, p]) < 0.01))
            if o is not None:
                assert flags[k, 0] == o["point_moving"] and flags[k, 1] == o["cam_moving"]
                assert _f64_ok(disp[k, 1:4], o["gt_vector"]) and int(disp[k, 0] * 1000) == o["gt_total_distance"]
                n_checked += 1
        assert n_checked > 150


# track_rigid_groups: "only the labels (4 P bytes) and the status come back"
@case("track_rigidity", "tracks", ["track_rigidity_loss", "track_rigidity_loss_batch", "track_linkage", "track_rigid_groups"])
class _TrackRigidity:
    """K7 (single and batched) -> K7b -> the groups: the loss matrix, the linkage workspace and the labels all stay on the device."""
    @staticmethod
    def build():
        blocks = np.stack([np.ascontiguousarray(synth.make_tracks(70 + b, T=TRACK_T, P=TRACK_P, n_groups=3).tracks_XYZ) for b in range(3)])
        import linkage_util as LU
        cut = LU.thresholds(O.rigidity_loss(blocks[0], 0.01))[-1]         # a height of block 0's own tree: a node exactly on the threshold
        return {"blocks": blocks, "cut": cut, "batch": dev(blocks), "one": dev(blocks[0]), "pair": dev(blocks[0][:, :2]),
                "single": dev(blocks[0][:, :1])}

    @staticmethod
    def run(i):
        loss, batch = engine.track_rigidity_loss(i["one"], 0.01), engine.track_rigidity_loss_batch(i["batch"], 0.01)
        return {"loss": loss, "loss_batch": batch, "linkage": engine.track_linkage(loss, i["cut"]), "linkage_batch": engine.track_linkage(batch, i["cut"]),
                "linkage_pair": engine.track_linkage(engine.track_rigidity_loss(i["pair"])),
                "linkage_single": engine.track_linkage(engine.track_rigidity_loss(i["single"])),
                "groups": engine.track_rigid_groups(i["one"], i["cut"], 0.01)}

    @staticmethod
    def expect(i, z):
        import linkage_util as LU
        z = host(z)
        for b in range(3):
            want = O.rigidity_loss(i["blocks"][b], 0.01)
            assert np.array_equal(z["loss_batch"][b], want) and (want > 0).any()
            wz, wl = LU.scipy_answer(want, i["cut"])
            Z, labels, status = (t[b] for t in z["linkage_batch"])
            assert status == 0 and Z.tobytes() == wz.tobytes() and np.array_equal(labels, wl)
        assert np.array_equal(z["loss"], z["loss_batch"][0])
        for a, b in zip(z["linkage"], z["linkage_batch"]):
            assert np.array_equal(a, b[0])
        assert z["groups"] == LU.groups_of(z["linkage"][1]) and len(z["groups"]) >= 2
        assert z["linkage_pair"][0].shape == (1, 4) and z["linkage_pair"][1].shape == (2,) and z["linkage_pair"][2] == 0
        assert z["linkage_single"][0].shape == (0, 4) and z["linkage_single"][1].tolist() == [1]


# =====================================================================================================================
# Track mining chain (K5d)
# =====================================================================================================================

def _first_v(name):
    # engine.track_pair_stats: "``frames`` [n,T] i32 and ``positions`` [n,T,3] f64 (a point's visible frames and its positions there:
    # the first V of a row)"
    def mask(zero):
        state = host(zero["state"])
        m = np.arange(state["frames"].shape[1])[None, :] < state["stats"][:, :1]
        return m if name == "frames" else np.broadcast_to(m[..., None], state["positions"].shape)
    return mask


# engine.track_pair_order: "row 0 holds every selected point's moving pairs [...] in ascending order, row 1 is the sort's scratch"
_ROW0 = (slice(0, 1),)


# track_pair_resolve: "The picks go up from pageable memory, which waits for the current stream" (and run() reads the statistics back
# between the calls, as heads._mine_pairs_device does)
@case("track_mining_chain", "mining", ["track_pair_stats", "track_pair_bin_counts", "track_pair_order", "track_pair_resolve", "track_pair_sort"],
      defined={"state/frames": _first_v("frames"), "state/positions": _first_v("positions"), "keys": _ROW0, "payload": _ROW0})
class _TrackMining:
    """track_pair_stats -> track_pair_bin_counts -> track_pair_order -> track_pair_resolve on one state; the host steps between them
    (edges, segment offsets, picks) are what heads._mine_pairs_device computes from the statistics."""
    POINTS = [7, 0, 3, 1, 2, 4, 9]            # moving, nearly static, two-valued AND visible in all T frames, visible in 0 / 1 frames, static

    @staticmethod
    def build():
        import track_mining_util as U
        world, vis, _ = U.make_block(4, TRACK_T)
        return {"world_np": world, "vis_np": vis, "world": dev(world), "vis": dev(vis.astype(np.uint8)),
                "points": dev(np.asarray(_TrackMining.POINTS, dtype=np.int32))}

    @staticmethod
    def run(i):
        import track_mining_util as U
        state = engine.track_pair_stats(i["world"], i["vis"], i["points"], 0.01, 1e8)
        stats = state["stats"].cpu().numpy()
        edges = np.stack([U.point_edges(r) for r in stats])
        counts = engine.track_pair_bin_counts(state, dev(edges), 0.01, 1e8)
        n = len(stats)
        rows = np.arange(n, dtype=np.int32)
        seg = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(stats[:, 2], out=seg[1:])
        classes = np.concatenate([counts.cpu().numpy(), stats[:, 1:2]], axis=1).astype(np.int32)
        picks = np.asarray([(s, c, r) for s in range(n) for c in range(11) for r in range(classes[s, c])], dtype=np.int32).reshape(-1, 3)
        rows_dev, seg_dev = dev(rows), dev(seg)
        keys, payload = engine.track_pair_order(state, rows_dev, seg_dev, int(seg[-1]))
        frames = engine.track_pair_resolve(state, counts, rows_dev, seg_dev, payload, picks, classes)
        sorted_keys, sorted_payload = keys.flip(1).contiguous(), payload.flip(1).contiguous()      # row 0 reversed, row 1 the poison
        engine.track_pair_sort(sorted_keys, sorted_payload, dev(np.array([0, seg[-1]], dtype=np.int64)))
        return {"state": state, "edges": edges, "counts": counts, "seg": seg, "classes": classes, "picks": picks, "keys": keys,
                "payload": payload, "frames": frames, "sorted_keys": sorted_keys, "sorted_payload": sorted_payload}

    @staticmethod
    def expect(i, z):
        import track_mining_util as U
        z, world, vis, points = host(z), i["world_np"], i["vis_np"], np.asarray(_TrackMining.POINTS)
        want = U.track_pair_stats(world, vis, points)
        stats = z["state"]["stats"]
        assert np.array_equal(stats, want["stats"]) and stats[:, 0].tolist()[2:5] == [TRACK_T, 0, 1]
        for r in range(len(points)):
            V = stats[r, 0]
            assert np.array_equal(z["state"]["frames"][r, :V], want["frames"][r, :V])
            assert np.array_equal(z["state"]["positions"][r, :V], world[want["frames"][r, :V], points[r]])
        counts = U.track_pair_bin_counts(want, z["edges"], 0.01, 1e8)
        assert np.array_equal(z["counts"], counts) and np.array_equal(counts.sum(axis=1), stats[:, 2])
        rows = np.arange(len(points), dtype=np.int32)
        want_keys, want_payload = U.track_pair_order(want, rows, z["seg"], int(z["seg"][-1]))
        assert np.array_equal(z["keys"][0], want_keys[0]) and np.array_equal(z["payload"][0], want_payload[0])
        frames = U.track_pair_resolve(want, counts, rows, z["seg"], want_payload, z["picks"], z["classes"])
        assert np.array_equal(z["frames"], frames) and (frames[:, 0] < frames[:, 1]).all() and len(frames) == stats[:, 1:3].sum() > 1000
        order = U.sorted_segment(want_keys[0][::-1], want_payload[0][::-1])                            # the sort alone: one segment
        assert np.array_equal(z["sorted_keys"][0], want_keys[0][::-1][order]) and np.array_equal(z["sorted_payload"][0], want_payload[0][::-1][order])


# =====================================================================================================================
# Ingest
# =====================================================================================================================

def upload_streams(streams, pad=0):
    """Byte streams at 16-byte aligned offsets of one device buffer (a multiple of 4 bytes long) -> (src, offsets, nbytes)."""
    offs, pos = [], 0
    for s in streams:
        offs.append(pos)
        pos += (len(s) + 15) // 16 * 16 + 16
    buf = np.full(pos + 16, pad, dtype=np.uint8)
    for o, s in zip(offs, streams):
        buf[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return dev(buf), dev(np.asarray(offs, dtype=np.int64)), dev(np.asarray([len(s) for s in streams], dtype=np.int64))


def _status_rows(path_of_status, ndim):
    # include/mspa.h, mspa_inflate_blocks_device: "A block with a non-zero status holds garbage"; mspa_png_unfilter_device: "Images
    # whose status_dev[k] is non-zero on entry are skipped"; mspa_png_unfilter8_device: "an image with a filter byte > 4 gets status 3
    # and is not written"; mspa_jpeg_decode_device: "A non-zero image's output is unspecified: decode that frame on the host."
    def mask(zero):
        st = zero
        for key in path_of_status:
            st = st[key]
        return (host(st) == 0).reshape((-1,) + (1,) * (ndim - 1))
    return mask


def _png_case(name, bits, h, w, caller=False):
    """inflate_blocks_device -> png_unfilter(8)_device: every filter kind, images taller than one 64-row band where h says so; one
    stream with a damaged trailer (declined by the inflate, skipped by the un-filter) and one image with a filter byte 5.
    ``caller``: the scanline blocks, the status array and the images are the caller's own buffers (``own``)."""
    row = w * (2 if bits == 16 else 1) + 1
    pitch = (h * row + 255) // 256 * 256
    owned = ("raw", "status", "images") if caller else ()

    @case(name, "ingest", ["inflate_blocks_device", "png_unfilter_device" if bits == 16 else "png_unfilter8_device"],
          defined={"raw": _status_rows(("status_inflate",), 2), "images": _status_rows(("status",), 3)}, enqueue_only=ENQUEUES["inflate_blocks_device"],
          aligned={"src": (16, ALIGN_INFLATE), "own/raw": (256, ALIGN_INFLATE)} if caller else {"src": (16, ALIGN_INFLATE)}, own_buffers=owned)
    class _Png:
        @staticmethod
        def build():
            import zlib
            import png8_raw
            import png_raw
            rng = np.random.default_rng(h * 1000 + w + bits)
            raws, wants = [], []
            for kind in png_raw.FILTER_KINDS:
                filters = png_raw.row_filters(kind, h, rng)
                raw = png_raw.scanlines(filters, w, "random", rng) if bits == 16 else png8_raw.scanlines8(filters, w, "random", rng)
                raws.append(raw)
                wants.append(png_raw.pillow_unfilter(raw, h, w) if bits == 16 else png8_raw.pillow_unfilter8(raw, h, w))
            streams = [zlib.compress(r, 1 + k % 9) for k, r in enumerate(raws)]
            streams[2] = streams[2][:-1] + bytes([streams[2][-1] ^ 1])          # wrong Adler-32: status 2
            bad = bytearray(raws[4])
            bad[(h - 1) * row] = 5                                               # a filter byte > 4 in the last row: status 3
            streams[4] = zlib.compress(bytes(bad), 6)
            src, off, nb = upload_streams(streams)
            return {"wants": wants, "src": src, "off": off, "nb": nb}

        @staticmethod
        def run(i):
            unfilter = engine.png_unfilter_device if bits == 16 else engine.png_unfilter8_device
            if caller:
                # the caller's blocks at 256 mod 512 (their documented 256), its status at 4 / 12 mod 16; its images one / three
                # elements past a boundary: int16 at 2 mod 4 -- png_unfilter_kernel's and png_unfilter_hard_kernel's word routes want
                # ``((uintptr_t)out & 3u) == 0`` (w is even here, so the pointer alone decides) and every image takes the bytes route --,
                # uint8 at 1 / 3 mod 4
                n = i["off"].shape[0]
                raw, status = engine.inflate_blocks_device(i["src"], i["off"], i["nb"], h * row, out=own("raw", (n, pitch), torch.uint8),
                                                           status=own("status", (n,), torch.int32))
                after_inflate = status.clone()
                images = unfilter(raw, h, w, status, out=own("images", (n, h, w), torch.int16 if bits == 16 else torch.uint8))
                if skewed_mode():                        # image k starts at images + k * h * w elements: h * w * 2 = 1156 is a multiple of 4
                    assert raw.data_ptr() % 512 == 256 and images.data_ptr() % 4 == (2 if bits == 16 else {"a": 1, "b": 3}[skewed_mode()])
                    assert bits != 16 or (w % 2 == 0 and (h * w * 2) % 4 == 0)      # so EVERY image fails ``(out & 3) == 0``, and for the address alone
                return {"raw": raw, "status_inflate": after_inflate, "images": images, "status": status}
            raw, status = engine.inflate_blocks_device(i["src"], i["off"], i["nb"], h * row)
            after_inflate = status.clone()
            return {"raw": raw, "status_inflate": after_inflate, "images": unfilter(raw, h, w, status), "status": status}

        @staticmethod
        def expect(i, z):
            z = host(z)
            want_status = [0] * len(i["wants"])
            want_status[2] = 2
            assert z["status_inflate"].tolist() == want_status
            want_status[4] = 3
            assert z["status"].tolist() == want_status
            assert z["raw"].shape[1] % 256 == 0 and not z["raw"][:, h * row:].any()      # "zeros behind ``block_bytes``": compared, and asserted
            for k, want in enumerate(i["wants"]):
                if want_status[k] == 0:
                    got = z["images"][k].view(np.uint16) if bits == 16 else z["images"][k]
                    assert np.array_equal(got, want), k
    return _Png


_png_case("depth_png_17x33", 16, 17, 33)
_png_case("depth_png_70x83", 16, 70, 83)                  # past one 64-row band
_png_case("mask_png_17x33", 8, 17, 33)
_png_case("mask_png_70x130", 8, 70, 130)
_png_case("depth_png_own_17x34", 16, 17, 34, caller=True)       # an even width: only the images' address keeps the word routes away
_png_case("mask_png_own_17x33", 8, 17, 33, caller=True)


def _jpeg_case(name, hw, caller=False):
    @case(name, "ingest", ["jpeg_decode_device", "jpeg_decode_luma_device"],
          defined={"rgb/0": _status_rows(("rgb", 1), 4), "luma/0": _status_rows(("luma", 1), 3)}, enqueue_only=ENQUEUES["jpeg_decode_device"],
          aligned={"src": (4, ALIGN_JPEG_SRC), "desc": (16, ALIGN_JPEG_DESC)}, own_buffers=("rgb", "luma", "status_rgb", "status_luma") if caller else (),
          refused_by="mspa_jpeg_decode_luma_device:" if caller else "mspa_jpeg_decode_device:")
    class _Jpeg:
        @staticmethod
        def build():
            from jpeg_util import content, encode
            h, w = hw
            payloads = []
            for k, (sub, q, rs) in enumerate([(0, 95, {}), (1, 75, {"restart_marker_blocks": 3}), (2, 50, {}), (2, 100, {"restart_marker_rows": 1}),
                                              ("L", 90, {}), (2, 95, {"optimize": True})]):
                img = content(h, w, 1000 * q + k)
                kw = dict(quality=q, **rs)
                if sub == "L":
                    img = img[..., 0]
                else:
                    kw["subsampling"] = sub
                payloads.append(encode(img, **kw))
            from jpeg_util import sos_end
            cut = payloads[2]
            payloads.append(cut[:(sos_end(cut) + len(cut)) // 2])                    # the entropy-coded data ends early: declined
            desc, parsed = engine.jpeg_parse_host(payloads)
            src, off, nb = upload_streams(payloads)
            return {"payloads": payloads, "parsed": parsed, "src": src, "off": off, "nb": nb, "desc": dev(desc)}

        @staticmethod
        def run(i):
            if caller:
                # the caller's pixels at 1 / 3 mod 4: color_kernel's ``((uintptr_t)o & 3u) == 0`` fails for every group of four
                # pixels (o = out + 12 * group keeps out's residue), so all of them take the byte stores
                n = i["off"].shape[0]
                rgb, luma = own("rgb", (n,) + tuple(hw) + (3,), torch.uint8), own("luma", (n,) + tuple(hw), torch.uint8)
                if skewed_mode():                        # (out + 12 * group) % 4 == out % 4 == 1 / 3: never 0
                    assert rgb.data_ptr() % 4 == luma.data_ptr() % 4 == {"a": 1, "b": 3}[skewed_mode()]
                # the grey decode FIRST: this case's refusal runs (src at 2 mod 4, desc at 8 mod 16) then stop in mspa_jpeg_decode_luma_device,
                # where jpeg_17x33's and jpeg_61x83's stop in mspa_jpeg_decode_device
                grey = engine.jpeg_decode_luma_device(i["src"], i["off"], i["nb"], i["desc"], hw, out=luma, status=own("status_luma", (n,), torch.int32))
                return {"rgb": engine.jpeg_decode_device(i["src"], i["off"], i["nb"], i["desc"], hw, out=rgb, status=own("status_rgb", (n,), torch.int32)),
                        "luma": grey}
            return {"rgb": engine.jpeg_decode_device(i["src"], i["off"], i["nb"], i["desc"], hw),
                    "luma": engine.jpeg_decode_luma_device(i["src"], i["off"], i["nb"], i["desc"], hw)}

        @staticmethod
        def expect(i, z):
            from handler_ops_util import pillow_luma
            from jpeg_util import pillow_rgb
            z = host(z)
            assert not i["parsed"].any()
            for key in ("rgb", "luma"):
                assert z[key][1][:-1].tolist() == [0] * (len(i["payloads"]) - 1) and z[key][1][-1] != 0, z[key][1]
            for k, p in enumerate(i["payloads"][:-1]):
                assert np.array_equal(z["rgb"][0][k], pillow_rgb(p)), k
                assert np.array_equal(z["luma"][0][k], pillow_luma(p)), k
    return _Jpeg


_jpeg_case("jpeg_17x33", (17, 33))
_jpeg_case("jpeg_61x83", (61, 83))
_jpeg_case("jpeg_own_17x33", (17, 33), caller=True)


@case("laplacian_moments", "ingest", ["laplacian_moments"], enqueue_only=ENQUEUES["laplacian_moments"])
class _Laplacian:
    @staticmethod
    def build():
        from handler_ops_util import smooth_image
        small = np.stack([smooth_image(17, 33, s, channels=1) for s in range(3)])
        small[1] = 0                                       # a flat image: every Laplacian 0
        large = np.stack([smooth_image(61, 83, 7 + s, channels=1) for s in range(2)])
        return {"small_np": small, "large_np": large, "small": dev(small), "large": dev(large)}

    @staticmethod
    def run(i):
        return {"small": engine.laplacian_moments(i["small"]), "large": engine.laplacian_moments(i["large"])}

    @staticmethod
    def expect(i, z):
        from handler_ops_util import moments, variance_numpy
        z = host(z)
        for key in ("small", "large"):
            imgs = i[key + "_np"]
            var = engine.laplacian_variance(z[key], imgs[0].size)
            for k, img in enumerate(imgs):
                assert tuple(int(v) for v in z[key][k].sum(axis=0)) == moments(img), (key, k)
                assert abs(var[k] - variance_numpy(img)) <= 1e-12 * max(variance_numpy(img), 1.0)
        assert not z["small"][1].any()


@case("instance_split", "ingest", ["instance_split"])          # "reading the counts is the call's one synchronisation"
class _InstanceSplit:
    @staticmethod
    def build():
        from instance_split_util import make_case
        out = {}
        labels, valid, xyz, rgb = make_case(3, 4097, "all_invalid", 3 * 1000 + 4097)      # label 5 has no valid pixel; labels 1..3 never occur
        valid[1] = 0                                                                       # a frame with no valid pixel
        out["ragged"] = (labels, valid, xyz, rgb)
        out["blocky"] = make_case(3, 65, "blocky", 3065)
        out["nothing"] = make_case(1, 65, "zero", 1065)                                    # total == 0
        return {"np": out, "dev": {k: tuple(dev(a) for a in v) for k, v in out.items()}}

    @staticmethod
    def run(i):
        out = {k: engine.instance_split(*v) for k, v in i["dev"].items()}
        out["no_rgb"] = engine.instance_split(*i["dev"]["ragged"][:3], None)
        return out

    @staticmethod
    def expect(i, z):
        from instance_split_util import assert_same, numpy_split
        z = host(z)
        for k, v in i["np"].items():
            assert_same(z[k], numpy_split(*v), k)          # lo / hi of an empty segment: +inf / -inf, promised and compared
        assert_same(z["no_rgb"], numpy_split(*i["np"]["ragged"][:3], None), "no_rgb")
        counts = z["ragged"][0]
        assert not counts[1].any() and not counts[:, 5].any() and counts[0, 4] > 0 and z["nothing"][1][-1] == 0


@case("knn_mean_distance", "ingest", ["knn_mean_distance"])          # "read back from a device sort: synchronises once"
class _Knn:
    CLOUDS = (("uniform", 65, 20), ("uniform", 1000, 20), ("clusters", 1000, 5), ("identical", 200, 20), ("uniform", 19, 20))

    @staticmethod
    def build():
        from handler_ops_util import cloud
        clouds = [cloud(kind, n) for kind, n, _k in _Knn.CLOUDS]
        return {"np": clouds, "dev": [dev(c) for c in clouds]}

    @staticmethod
    def run(i):
        return [engine.knn_mean_distance(c, k, want_evals=True) for c, (_kind, _n, k) in zip(i["dev"], _Knn.CLOUDS)] + \
            [engine.knn_mean_distance(i["dev"][0], 20)]

    @staticmethod
    def expect(i, z):
        from handler_ops_util import knn_mean_oracle, knn_tolerance
        z = host(z)
        for (mean, evals), xyz, (kind, _n, k) in zip(z[:-1], i["np"], _Knn.CLOUDS):
            want = knn_mean_oracle(xyz, k)                 # tests/test_gpu_handler_ops.py's bar, unchanged
            assert (np.abs(mean - want) <= knn_tolerance(k) * want).all(), kind
            host_mean, host_evals = engine.knn_mean_distance_host(xyz, k, want_evals=True)
            assert np.array_equal(mean, host_mean) and np.array_equal(evals, host_evals), kind
        assert np.array_equal(z[-1], z[0][0]) and (z[3][0] == 0).all()


@case("resize_rgb_device", "ingest", ["resize_rgb_device"], enqueue_only=ENQUEUES["resize_rgb_device"])
class _Resize:
    PAIRS = (((17, 33), (61, 83), "bicubic"), ((61, 83), (17, 33), "bicubic"), ((61, 83), (30, 83), "bilinear"), ((17, 33), (17, 70), "bilinear"),
             ((17, 33), (17, 33), "bicubic"))               # both passes (a workspace), one pass each way, a copy

    @staticmethod
    def build():
        from jpeg_util import content
        frames = {hw: np.stack([content(*hw, 40 + s) for s in range(3)]) for hw in ((17, 33), (61, 83))}
        return {"np": frames, "dev": {hw: dev(f) for hw, f in frames.items()}}

    @staticmethod
    def run(i):
        return [engine.resize_rgb_device(i["dev"][src], dst, f, fallback=False) for src, dst, f in _Resize.PAIRS]

    @staticmethod
    def expect(i, z):
        from resize_util import FILTERS, pillow_resize
        for got, (src, dst, f) in zip(host(z), _Resize.PAIRS):
            for k, img in enumerate(i["np"][src]):
                assert np.array_equal(got[k], pillow_resize(img, dst, FILTERS[f])), (src, dst, f, k)


@case("resize_rgb_device_own", "ingest", ["resize_rgb_device"], enqueue_only=ENQUEUES["resize_rgb_device"],
      own_buffers=tuple(f"resized{k}" for k in range(len(_Resize.PAIRS))))
class _ResizeOwn:
    """``_Resize`` into the caller's own ``out`` at 1 / 3 mod 4.  csrc/resize.hip's ``store4`` writes a 32-bit word where
    ``((uintptr_t)p & 3) == 0`` and bytes elsewhere; p = out + row * W * 3 + 12 * group, and no W * 3 here (249, 99, 210) is a
    multiple of 4, so which rows take which store moves with ``out % 4`` -- rows 0, 4, 8, .. take words in the plain run and bytes in
    both skewed ones.  The sources' skew (``stage_rows``' words from the address rounded down to 4, the vertical pass's ``skew0`` /
    ``skew_step``, the route switch on ``(src | row_pitch | image_pitch) & 3``) comes with the inputs, which are at 1 / 3 mod 4 too."""
    build = _Resize.build
    expect = _Resize.expect

    @staticmethod
    def run(i):
        outs = [own(f"resized{k}", (3,) + dst + (3,), torch.uint8) for k, (_src, dst, _f) in enumerate(_Resize.PAIRS)]
        if skewed_mode():
            r = {"a": 1, "b": 3}[skewed_mode()]
            assert all(o.data_ptr() % 4 == r for o in outs) and all(t.data_ptr() % 4 == r for t in i["dev"].values())
            for o in outs:                               # row y's stores go to (out + y * W * 3 + 12 * group + 4 * d): the row's residue
                pitch = o.shape[2] * 3                     # row 0 takes the byte stores now; with an odd pitch one of rows 1..3 takes words
                assert pitch % 4 and o.data_ptr() % 4 != 0 and (pitch % 2 == 0 or any((o.data_ptr() + y * pitch) % 4 == 0 for y in (1, 2, 3)))
        return [engine.resize_rgb_device(i["dev"][src], dst, f, out=outs[k], fallback=False) for k, (src, dst, f) in enumerate(_Resize.PAIRS)]


# =====================================================================================================================
# Export
# =====================================================================================================================

def _file_bytes(which, round_to=1):
    # engine.jpeg_encode_device: "row k holds image k's whole baseline JPEG file [...] its ``nbytes`` says how long it is";
    # include/mspa.h, mspa_png_encode_device: "Bytes [0, nbytes rounded up to 4) of a row are written (the padding bytes are 0); the
    # rest of the row is left as it was."
    def mask(zero):
        files, nbytes = host(zero[which])
        return np.arange(files.shape[1])[None, :] < ((nbytes + round_to - 1) // round_to * round_to)[:, None]
    return mask


@case("annotate_and_encode_jpeg", "export", ["draw_spans_device", "blend_masks_device", "jpeg_encode_device"],
      defined={"420/0": _file_bytes("420"), "444/0": _file_bytes("444"), "422/0": _file_bytes("422")}, enqueue_only=ENQUEUES["jpeg_encode_device"])
class _AnnotateJpeg:
    """draw_spans_device -> blend_masks_device on per-job copies (allocated under the patch, as DeviceAnnotator's are) ->
    jpeg_encode_device: the annotated-image export."""
    HW = (61, 83)

    @staticmethod
    def build():
        from jpeg_util import content
        from mspa import annotate
        H, W = _AnnotateJpeg.HW
        rng = np.random.default_rng(61)
        frames = np.stack([content(H, W, 300 + s) for s in range(3)])
        frames[2] = 128                                    # a flat image: EOB runs only
        spans, labels, masks, moff = [], [], [], 0
        for n in range(2):                                 # image 2 stays unpainted
            marks = [(int(rng.integers(-5, W + 5)), int(rng.integers(-5, H + 5)), int(rng.integers(1, 12)), int(rng.integers(0, 1 << 24))) for _ in range(4)]
            spans.append((n, [(y, x0, x1, rgb) for (cx, cy, r, rgb) in marks for (y, x0, x1) in annotate.filled_circle_spans(cx, cy, r, W, H)]))
            for (cx, cy, _r, rgb) in marks[:2]:
                mask = rng.integers(0, 256, (int(rng.integers(3, 20)), int(rng.integers(3, 30))), dtype=np.uint8)
                labels.append((n, cx - 6, cy - 9, mask.shape[1], mask.shape[0], rgb, moff, 0))
                masks.append(mask)
                moff += mask.size
        return {"frames_np": frames, "spans_np": spans, "labels_np": labels, "masks_np": masks, "frames": dev(frames),
                "spans": dev(annotate.pack_spans(spans)), "labels": dev(np.array(labels, dtype=np.int64)),
                "masks": dev(np.concatenate([m.ravel() for m in masks]))}

    @staticmethod
    def run(i):
        canvas = torch.empty_like(i["frames"])
        canvas.copy_(i["frames"])
        engine.draw_spans_device(canvas, i["spans"])
        engine.blend_masks_device(canvas, i["labels"], i["masks"])
        return {"canvas": canvas, "420": engine.jpeg_encode_device(canvas, 95, "4:2:0"), "444": engine.jpeg_encode_device(canvas, 50, "4:4:4"),
                "422": engine.jpeg_encode_device(canvas, 100, "4:2:2")}

    @staticmethod
    def expect(i, z):
        from jpeg_util import encode
        from mspa import annotate
        z = host(z)
        want = i["frames_np"].copy()
        for n, spans in i["spans_np"]:
            for (y, x0, x1, rgb) in spans:                 # "pixels x0..x1 (inclusive, clipped) of row y take the colour"
                want[n, y, x0:x1 + 1] = [(rgb >> 16) & 255, (rgb >> 8) & 255, rgb & 255]
        for (n, x, y, _w, _h, rgb, _off, _zero), mask in zip(i["labels_np"], i["masks_np"]):
            annotate.blend_mask_numpy(want[n], mask, x, y, [(rgb >> 16) & 255, (rgb >> 8) & 255, rgb & 255])
        assert np.array_equal(z["canvas"], want) and not np.array_equal(want[0], i["frames_np"][0])
        for key, q, sub in (("420", 95, 2), ("444", 50, 0), ("422", 100, 1)):
            files, nbytes = z[key]
            for n in range(3):
                assert files[n, :nbytes[n]].tobytes() == encode(want[n], quality=q, subsampling=sub), (key, n)


@case("png_encode_device", "export", ["png_encode_device"], defined={"small/0": _file_bytes("small", 4), "large/0": _file_bytes("large", 4)},
      enqueue_only=ENQUEUES["png_encode_device"])
class _PngEncode:
    @staticmethod
    def build():
        import png_encode_util as PU
        small = np.stack([PU.content(kind, 17, 33, 5) for kind in ("zeros", "ramp", "noise", "runs")]).astype(np.uint16)
        large = np.stack([PU.content(kind, 61, 83, 6) for kind in ("smooth", "planar", "alternate")]).astype(np.uint16)
        return {"small_np": small, "large_np": large, "small": dev(small.view(np.int16)), "large": dev(large.view(np.int16))}

    @staticmethod
    def run(i):
        return {"small": engine.png_encode_device(i["small"]), "large": engine.png_encode_device(i["large"])}

    @staticmethod
    def expect(i, z):
        import io
        import png_encode_util as PU
        from PIL import Image
        z = host(z)
        for key in ("small", "large"):
            files, nbytes = z[key]
            for k, frame in enumerate(i[key + "_np"]):
                data = files[k, :nbytes[k]].tobytes()
                h, w = frame.shape
                assert PU.strict_idat(data, h, w) == PU.strict_idat(PU.pillow_png(frame), h, w), (key, k)    # Pillow's filtered scanlines
                assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), frame), (key, k)
                assert not files[k, nbytes[k]:(nbytes[k] + 3) // 4 * 4].any()                              # "(the padding bytes are 0)"


@case("png_encode_device_own", "export", ["png_encode_device"], defined={"small/0": _file_bytes("small", 4)}, enqueue_only=ENQUEUES["png_encode_device"],
      aligned={"own/files": (4, ALIGN_PNG_ENCODE)}, own_buffers=("files", "nbytes"))
class _PngEncodeOwn:
    """``_PngEncode``'s small frames into the caller's own rows: ``out_dev 4 bytes`` -- copy_kernel stores whole 32-bit words at
    ``out + k * out_pitch + i``, i a multiple of 4 -- so the rows sit at 4 mod 8 and 2 mod 4 is refused; ``nbytes`` at 8 mod 16; the
    frames (``depth_dev 2 bytes``) come at 2 mod 4 / 6 mod 8 with the inputs."""
    @staticmethod
    def build():
        i = _PngEncode.build()
        return {"small_np": i["small_np"], "large_np": i["large_np"][:0], "small": i["small"]}

    @staticmethod
    def run(i):
        n, h, w = i["small"].shape
        pitch = (engine.png_encode_capacity((h, w)) + 3) // 4 * 4
        return {"small": engine.png_encode_device(i["small"], out=own("files", (n, pitch), torch.uint8), nbytes=own("nbytes", (n,), torch.int64))}

    @staticmethod
    def expect(i, z):
        _PngEncode.expect(i, {**z, "large": (z["small"][0][:0], z["small"][1][:0])})


# =====================================================================================================================
# Visibility index and pair table
# =====================================================================================================================

def _i64(a):
    return dev(np.asarray(a, dtype=np.int64))


# format_lists_device: "one small read-back: the size to allocate"; parquet_string_pages_device: "Synchronises the current stream."
@case("index_text_and_pages", "visindex", ["format_lists_device", "parquet_string_pages_device"])
class _IndexText:
    """format_lists_device (integers, then tokens) -> one string column -> parquet_string_pages_device (PLAIN pages, Snappy by the
    batched compressor): the encode chain of the visibility index."""
    F, N = 8, 1000

    @staticmethod
    def build():
        import json
        rng = np.random.default_rng(21)
        F, N = _IndexText.F, _IndexText.N
        seen = rng.random((F, N)) < 0.3
        seen[:, 777] = False                               # a vertex nobody sees: "[]"
        seen[5] = False                                    # an image that sees nothing
        ids = [f"{k * 10:05d}" for k in range(F)]

        def csr(m):
            return _i64(np.concatenate([[0], np.cumsum(m.sum(1))])), dev(np.nonzero(m)[1].astype(np.int32))
        return {"seen": seen, "ids": ids, "by_image": csr(seen), "by_point": csr(seen.T), "tokens": [json.dumps(i).encode() for i in ids],
                "no_lists": (_i64([0]), dev(np.zeros(0, np.int32))), "empty_lists": (_i64([0, 0, 0, 0]), dev(np.zeros(0, np.int32)))}

    @staticmethod
    def run(i):
        t1 = engine.format_lists_device(*i["by_image"])
        t2 = engine.format_lists_device(*i["by_point"], i["tokens"])
        offsets = torch.cat([t1[1][:-1], t2[1] + t1[0].numel()])
        data = torch.cat([t1[0], t2[0]])
        return {"images": t1, "points": t2, "no_lists": engine.format_lists_device(*i["no_lists"]),
                "empty_lists": engine.format_lists_device(*i["empty_lists"]), "offsets": offsets, "data": data,
                "pages_4k": engine.parquet_string_pages_device(offsets, data, 4096, return_payload=True),
                "pages_1m": engine.parquet_string_pages_device(offsets, data, 1 << 20, return_payload=True)}

    @staticmethod
    def expect(i, z):
        import json
        import snappy_util as SU
        z, seen, ids = host(z), i["seen"], i["ids"]

        def texts(pair):
            t, o = pair[0].tobytes(), pair[1]
            return [t[o[k]:o[k + 1]].decode() for k in range(len(o) - 1)]
        assert texts(z["images"]) == [json.dumps(np.nonzero(row)[0].tolist()) for row in seen]
        assert texts(z["points"]) == [json.dumps([ids[k] for k in np.nonzero(col)[0]]) for col in seen.T]
        assert texts(z["no_lists"]) == [] and z["no_lists"][1].tolist() == [0] and texts(z["empty_lists"]) == ["[]"] * 3
        lib = _lib.load()
        for key, page_bytes in (("pages_4k", 4096), ("pages_1m", 1 << 20)):
            got, want = z[key], SU.host_pages(lib, z["offsets"], z["data"], page_bytes)
            assert got["num_values"].tolist() == want["num_values"] and got["uncompressed"].tolist() == want["uncompressed"]
            assert got["payload"].tobytes() == want["payload"] and got["compressed"].tolist() == want["compressed"]
            assert got["chunk"].tobytes() == want["chunk"]
        assert len(z["pages_4k"]["compressed"]) > 5 and len(z["pages_1m"]["compressed"]) == 1


@case("snappy_compress_device", "visindex", ["snappy_compress_device"])          # "Three small read-backs (block count, total, the kernels' flag)"
class _SnappyCompress:
    @staticmethod
    def build():
        import snappy_util as SU
        cases = SU.streams()                                # lengths around a 64 KiB block, zero-length streams among them
        blob, offsets = bytearray(), []
        for _, d in cases:
            blob += b"\xEE" * 5
            offsets.append(len(blob))
            blob += d
        return {"cases": cases, "src": dev(np.frombuffer(bytes(blob), dtype=np.uint8)), "off": _i64(offsets), "nb": _i64([len(d) for _, d in cases])}

    @staticmethod
    def run(i):
        return engine.snappy_compress_device(i["src"], i["off"], i["nb"])

    @staticmethod
    def expect(i, z):
        import snappy_util as SU
        out, starts = host(z)
        lib, out = _lib.load(), out.tobytes()
        assert starts[0] == 0 and starts[-1] == len(out)
        for k, (name, d) in enumerate(i["cases"]):
            got = out[starts[k]:starts[k + 1]]
            assert got == SU.compress_host(lib, d), name
            SU.check_stream(name, d, got, lib.mspa_snappy_capacity(len(d)))


def _taken_bytes(which):
    # include/mspa.h, mspa_snappy_decompress_device: "A declined stream's output bytes are unspecified"
    def mask(zero):
        res = host(zero[which])
        out, out_offsets, status = res[0], res[1], res[2]
        m = np.zeros(out.shape, dtype=bool)
        for k in np.nonzero(status == 0)[0]:
            m[out_offsets[k]:out_offsets[k + 1]] = True
        return m
    return mask


# each of the three: "One small read-back (the size(s) to allocate)"
@case("snappy_decode", "visindex", ["snappy_decompress_device", "snappy_block_starts_device", "snappy_decompress_blocks_device"],
      defined={"serial/0": _taken_bytes("serial"), "blocks/0": _taken_bytes("blocks")})
class _SnappyDecode:
    """The one-wave decoder, the block-start scan and the decode by blocks on tests/test_gpu_snappy_blocks.py's stream set: both
    writers' streams, hand-built ones, segment seams, and every corrupt stream between two good ones."""
    @staticmethod
    def build():
        from test_gpu_snappy_blocks import _cases
        cases = _cases()
        buf, offs = bytearray(), []
        for k, (_n, s, _e, _kind) in enumerate(cases):
            buf += b"\x5a" * ((k % 4 - len(buf)) % 4 + 4 * (k % 3))
            offs.append(len(buf))
            buf += s
        return {"cases": cases, "src": dev(np.frombuffer(bytes(buf), dtype=np.uint8)), "off": _i64(offs), "nb": _i64([len(c[1]) for c in cases]),
                "sizes": _i64([c[2] for c in cases])}

    @staticmethod
    def run(i):
        args = (i["src"], i["off"], i["nb"], i["sizes"])
        return {"serial": engine.snappy_decompress_device(*args), "starts": engine.snappy_block_starts_device(*args),
                "blocks": engine.snappy_decompress_blocks_device(*args)}

    @staticmethod
    def expect(i, z):
        import snappy_blocks_util as BU
        import visindex_decode_util as VU
        from test_gpu_snappy_blocks import _host
        z, ref = host(z), _host()
        starts, block_prefix, route = z["starts"]
        taken = 0
        for k, ((name, _s, e, kind), (rc, data, brc, want_starts)) in enumerate(zip(i["cases"], ref)):
            if brc > 0:
                assert route[k] == brc == BU.block_count(e) and starts[block_prefix[k] + k:block_prefix[k + 1] + k + 1].tolist() == want_starts, name
                taken += 1
            else:
                assert route[k] == 0, name
            for key in ("serial", "blocks"):
                out, out_offsets, status = z[key][:3]
                got = out[out_offsets[k]:out_offsets[k + 1]].tobytes()
                if rc < 0:
                    assert kind == "corrupt" and status[k] == rc, (key, name, int(status[k]), rc)
                elif name == VU.FAR_NAME and key == "serial":            # reaches back more than 64 KiB: equal, or declined
                    assert status[k] != 0 or got == data, name
                else:
                    assert status[k] == 0 and got == data, (key, name, int(status[k]))
            blocks, routed = BU.block_count(e), z["blocks"][3][k]
            if rc < 0 or brc == BU.NOT_BLOCKWISE or blocks < 2:
                assert routed == 0, (name, int(routed))                      # by the one-wave kernel
            elif kind in ("writer", "neighbour") or brc == blocks:
                assert routed == blocks, (name, int(routed), blocks)
        assert taken > 100


def small_snappy_stream():
    """A hand-made stream of 31 bytes -> 42: a literal SHORTER than a word first, a copy (1-byte offset form) that reaches back to
    output byte 0, a 20-byte literal, a copy (2-byte offset form) that reaches back to output byte 0 again.  -> (stream, output)."""
    out, s = bytearray(b"abc"), bytearray([42])                  # the preamble: varint(42)
    s += bytes([(3 - 1) << 2]) + b"abc"
    s += bytes([((9 - 4) << 2) | 1, 3])                          # 9 bytes from 3 back
    for _ in range(9):
        out.append(out[-3])
    lit = bytes(range(100, 120))
    s += bytes([(20 - 1) << 2]) + lit
    out += lit
    s += bytes([((10 - 1) << 2) | 2, 32, 0])                     # 10 bytes from 32 back
    for _ in range(10):
        out.append(out[-32])
    assert len(s) == 31 and len(out) == 42
    return bytes(s), bytes(out)


# each of the two: "One small read-back (the size(s) to allocate)"
@case("snappy_decode_every_residue", "visindex", ["snappy_decompress_device", "snappy_decompress_blocks_device"])
class _SnappyResidues:
    """``small_snappy_stream`` four times in one ``src``, at offsets 0, 33, 66 and 99: whatever ``src % 4`` is, one copy starts at
    each of 0, 1, 2 and 3 mod 4 (asserted in ``run``).  csrc/snappy_decode_loop.inc: ``mis = sp & 3``; ``wbase = p - ((p + mis) & 3)``
    is negative for the three that start off a word (-1, -2, -3), and lane 0's ``fetch(wbase)`` takes the byte loop that reads the
    bytes in front of the stream as zero; the last copy ends at ``src``'s last byte, so the window's last words take that loop too."""
    OFFSETS = (0, 33, 66, 99)

    @staticmethod
    def build():
        stream, want = small_snappy_stream()
        buf = bytearray(b"\xee" * (_SnappyResidues.OFFSETS[-1] + len(stream)))
        for o in _SnappyResidues.OFFSETS:
            buf[o:o + len(stream)] = stream
        return {"want": want, "src": dev(np.frombuffer(bytes(buf), dtype=np.uint8)), "off": _i64(_SnappyResidues.OFFSETS),
                "nb": _i64([len(stream)] * 4), "sizes": _i64([len(want)] * 4)}

    @staticmethod
    def run(i):
        assert sorted((i["src"].data_ptr() + o) % 4 for o in _SnappyResidues.OFFSETS) == [0, 1, 2, 3]
        args = (i["src"], i["off"], i["nb"], i["sizes"])
        return {"serial": engine.snappy_decompress_device(*args), "blocks": engine.snappy_decompress_blocks_device(*args)}

    @staticmethod
    def expect(i, z):
        z = host(z)
        for key in ("serial", "blocks"):
            out, out_offsets, status = z[key][:3]
            assert status.tolist() == [0] * 4 and out_offsets.tolist() == [0, 42, 84, 126, 168], (key, status, out_offsets)
            assert out.tobytes() == i["want"] * 4, key


# the early returns read nothing back, but the functions document read-backs (snappy_*: above; index_spans_to_lists: "Synchronises")
@case("empty_batches", "visindex", ["snappy_compress_device", "snappy_decompress_device", "snappy_block_starts_device",
                                    "snappy_decompress_blocks_device", "index_spans_to_lists"])
class _EmptyBatches:
    """Tables of no streams and of no rows: the wrappers' early returns, which no other case reaches -- zero-length outputs and the
    one-element prefix arrays, allocated and returned without a kernel."""
    @staticmethod
    def build():
        return {"src": dev(np.frombuffer(b"no stream is cut out of this", dtype=np.uint8)), "none": _i64([])}

    @staticmethod
    def run(i):
        src, none = i["src"], i["none"]
        return {"compress": engine.snappy_compress_device(src, none, none), "serial": engine.snappy_decompress_device(src, none, none, none),
                "starts": engine.snappy_block_starts_device(src, none, none, none),
                "blocks": engine.snappy_decompress_blocks_device(src, none, none, none), "lists": engine.index_spans_to_lists(src, none, none)}

    @staticmethod
    def expect(i, z):
        z = host(z)
        assert z["compress"][0].shape == (0,) and z["compress"][1].tolist() == [0]
        for key, n_outputs in (("serial", 3), ("blocks", 4)):
            assert len(z[key]) == n_outputs and z[key][0].shape == (0,) and z[key][1].tolist() == [0], key
            assert all(t.shape == (0,) for t in z[key][2:]), key
        assert z["starts"][0].shape == (0,) and z["starts"][1].tolist() == [0] and z["starts"][2].shape == (0,)
        lists = z["lists"]
        assert lists["values"].shape == (0,) and lists["offsets"].tolist() == [0] and lists["n_points"] == 1
        assert len(lists["counts"]) == len(lists["row_status"]) == len(lists["page_status"]) == 0


# index_rows_to_bits: "Synchronises (three or four small read-backs)"; index_spans_to_lists: "Synchronises: the pipeline's two totals and ONE
# read-back of statuses, counts and width"
@case("parquet_spans_to_bits_and_lists", "visindex", ["parquet_plain_spans_device", "parquet_dict_spans_device", "index_rows_to_bits",
                                                      "index_spans_to_lists", "index_rows_to_lists", "index_lists_pick", "index_spans_to_bits"])
class _IndexRows:
    """Hand-made v1 PLAIN pages of the index's edge rows (tests/index_lists_util.py) through the span kernel to bitsets and to
    lists, the lists on to index_lists_pick; and tests/test_gpu_visindex_encoded_pages.py's crafted dictionary pages through
    parquet_dict_spans_device, their good rows on to index_spans_to_bits."""
    N_POINTS = 65536

    @staticmethod
    def build():
        import json
        import struct
        from index_lists_util import EDGE_ROWS
        from test_gpu_visindex_encoded_pages import ENTRIES, _crafted, _levels
        rows = {k: v for k, v in EDGE_ROWS.items() if k != "long"}
        rows["thousand"] = json.dumps(list(range(3, 3000, 3)))              # more than one workgroup of text
        names = list(rows)
        split = 6
        pages = [_levels(len(part)) + b"".join(struct.pack("<I", len(rows[k])) + rows[k].encode() for k in part)
                 for part in (names[:split], names[split:])]
        buf, offs = b"", []
        for p in pages:
            offs.append(len(buf))
            buf += p + b"\xee" * 5
        wanted = [k for k in names if k != "spaces"]                         # a row that is skipped: the row table is not every value
        row_index = [names.index(k) if names.index(k) < split else names.index(k) - split for k in wanted]
        n_first = sum(1 for k in wanted if names.index(k) < split)
        plain = (dev(np.frombuffer(buf, dtype=np.uint8)), _i64(offs), _i64([len(p) for p in pages]), _i64([split, len(names) - split]),
                 _i64([0, n_first, len(wanted)]), _i64(row_index))
        cbuf, dictionary, coffs, cpages, crows, flat = _crafted()
        n = len(cpages)
        crafted = {"payload": dev(np.frombuffer(cbuf, dtype=np.uint8)), "dict_table": (_i64([0]), _i64([len(dictionary)]), _i64([len(ENTRIES)]),
                                                                                         _i64([0, len(ENTRIES)]), _i64(range(len(ENTRIES)))),
                   "pages": (_i64(coffs), _i64([len(p[1]) for p in cpages]), _i64([20] * n), _i64(np.arange(n + 1) * len(crows)), _i64(crows * n)),
                   "dict_of_page": (_i64([0] * n), _i64([len(ENTRIES)] * n))}
        samples = [(wanted.index("duplicate"), 3), (wanted.index("descending"), 1), (wanted.index("one"), 0), (wanted.index("one"), 1),
                   (len(wanted), 0), (wanted.index("empty"), 0), (wanted.index("beyond"), 1), (wanted.index("thousand"), 998)] * 40
        return {"rows": rows, "wanted": wanted, "plain": plain, "crafted": crafted, "cpages": cpages, "crows": crows, "flat": flat,
                "samples_np": samples, "samples": _i64(samples).reshape(-1, 2)}

    @staticmethod
    def run(i):
        c, n_points = i["crafted"], _IndexRows.N_POINTS
        lists = engine.index_rows_to_lists(*i["plain"])
        spans = engine.parquet_plain_spans_device(*i["plain"])
        d_start, d_len, d_status = engine.parquet_plain_spans_device(c["payload"], *c["dict_table"], has_levels=False)
        coded = engine.parquet_dict_spans_device(c["payload"], *c["pages"], *c["dict_of_page"], d_start, d_len, has_levels=True)
        good = torch.tensor([k for k, p in enumerate(i["cpages"]) if p[2] == 0], device=DEV)
        n_rows = len(i["crows"])
        return {"bits": engine.index_rows_to_bits(*i["plain"], n_points), "bits_own_width": engine.index_rows_to_bits(*i["plain"]),
                "lists": lists, "lists_from_spans": engine.index_spans_to_lists(i["plain"][0], spans[0], spans[1], spans[2]),
                "picked": engine.index_lists_pick(lists["values"], lists["offsets"], i["samples"], n_points),
                "dict_table": (d_start, d_len, d_status), "coded": coded,
                "coded_bits": engine.index_spans_to_bits(c["payload"], coded[1].view(-1, n_rows)[good].reshape(-1).contiguous(),
                                                         coded[2].view(-1, n_rows)[good].reshape(-1).contiguous(), 400),
                "no_rows": engine.index_spans_to_bits(c["payload"], d_start[:0], d_len[:0], 400)}

    @staticmethod
    def expect(i, z):
        import json
        from mspa.scene import pack_index_lists
        from test_gpu_visindex_encoded_pages import ENTRIES
        z, rows, wanted, n_points = host(z), i["rows"], i["wanted"], _IndexRows.N_POINTS
        texts = [rows[k] for k in wanted]
        declined_bits = {"descending", "negative", "beyond", "float"}        # ascending non-negative integers below n_points
        declined_lists = {"negative", "float"}                               # the parser's: order and duplicates are the text's
        b = z["bits"]
        assert not b["page_status"].any() and [k for k, s in zip(wanted, b["row_status"]) if s] == [k for k in wanted if k in declined_bits]
        taken = [r for r, k in enumerate(wanted) if k not in declined_bits]
        want_bits = pack_index_lists([json.loads(texts[r]) for r in taken], n_points)
        # index_rows_to_bits: "non-zero = declined: that page's rows / that row belong to the host path, their ``bits`` are unspecified"
        # -- the kernel clears every row first, so they are compared between the runs all the same
        assert np.array_equal(b["bits"][taken], want_bits) and b["n_points"] == n_points
        assert z["bits_own_width"]["n_points"] == n_points + 1 and z["bits_own_width"]["bits"].shape[1] == n_points // 64 + 1
        for key in ("lists", "lists_from_spans"):
            lists = z[key]
            assert [k for k, s in zip(wanted, lists["row_status"]) if s] == [k for k in wanted if k in declined_lists], key
            want_lists = [None if k in declined_lists else json.loads(rows[k]) for k in wanted]
            assert lists["n_points"] == n_points + 1, lists["n_points"]
            assert np.array_equal(lists["counts"], np.diff(lists["offsets"])) and lists["offsets"][-1] == len(lists["values"])
            for r, x in enumerate(want_lists):               # a declined row belongs to the host path: only the taken rows are lists
                if x is not None:
                    assert lists["values"][lists["offsets"][r]:lists["offsets"][r + 1]].tolist() == x, (key, wanted[r])
        vertex, status = z["picked"]
        for (row, pos), v, s in zip(i["samples_np"], vertex, status):
            if row < len(want_lists) and want_lists[row] is None:
                continue
            x = want_lists[row] if row < len(want_lists) else None
            want = (-1, _lib.PICK_EROW) if x is None else (-1, _lib.PICK_EPOSITION) if not 0 <= pos < len(x) else \
                (x[pos], 0) if x[pos] < n_points else (-1, _lib.PICK_ERANGE)
            assert (v, s) == want, (row, pos)
        # the crafted dictionary pages: tests/test_gpu_visindex_encoded_pages.py's expectations
        index, start, length, status, code = z["coded"]
        cpages, crows, flat = i["cpages"], i["crows"], i["flat"]
        n = len(cpages)
        index, start, length = (x.reshape(n, len(crows)) for x in (index, start, length))
        assert status.tolist() == [p[2] for p in cpages] and code.tolist() == [p[3] for p in cpages]
        entry_at = z["dict_table"][0].tolist()
        assert z["dict_table"][2].tolist() == [0] and z["dict_table"][1].tolist() == [len(e) for e in ENTRIES]
        picked = []
        for k, (name, _body, st, _c) in enumerate(cpages):
            if st:                                         # "a declined page's rows get index -1 and an empty span": compared
                assert index[k].tolist() == [-1] * len(crows) and not start[k].any() and not length[k].any(), name
                continue
            want = [1] * len(crows) if name == "good_rle_only" else [flat[r] for r in crows]
            assert index[k].tolist() == want and start[k].tolist() == [entry_at[j] for j in want], name
            picked += want
        assert not z["coded_bits"]["row_status"].any()
        assert np.array_equal(z["coded_bits"]["bits"], pack_index_lists([json.loads(ENTRIES[j]) for j in picked], 400))
        assert z["no_rows"]["bits"].shape == (0, 7)


# rle_hybrid_runs_device: "A counting launch, ONE small read-back (the sizes to allocate)"
@case("rle_hybrid", "visindex", ["rle_hybrid_runs_device", "rle_hybrid_expand_device"])
class _RleHybrid:
    @staticmethod
    def build():
        import rle_hybrid_util as RU
        cases = {(bytes(c[1]), c[2], c[3]) for c in RU.valid_cases() + RU.corrupt_cases() + RU.truncation_cases()}
        cases = sorted(cases, key=lambda c: (c[1], c[2], c[0]))
        cases += [(b"", 1, 0), (RU.rle_run(7000, 1, 1), 1, 7000), (RU.rle_run(5, 1, 1) + RU.packed_run([1, 0, 1, 1, 0, 0, 1, 0] * 300, 1)[0], 1, 2405)]
        blob = b"".join(c[0] for c in cases)
        offs = np.concatenate([[0], np.cumsum([len(c[0]) for c in cases])]).astype(np.int64)
        return {"cases": cases, "src": dev(np.frombuffer(blob, dtype=np.uint8)), "off": _i64(offs[:-1]), "nb": _i64(np.diff(offs)),
                "bw": _i64([c[1] for c in cases]), "nv": _i64([c[2] for c in cases])}

    @staticmethod
    def run(i):
        runs = engine.rle_hybrid_runs_device(i["src"], i["off"], i["nb"], i["bw"], i["nv"])
        outside = engine.rle_hybrid_runs_device(i["src"], _i64([i["src"].numel() - 1, -4]), _i64([2, 2]), _i64([1, 1]), _i64([3, 3]))
        return {"runs": runs, "values": engine.rle_hybrid_expand_device(i["src"], runs), "outside": outside,
                "outside_values": engine.rle_hybrid_expand_device(i["src"], outside)}

    @staticmethod
    def expect(i, z):
        z = host(z)                                        # tests/test_gpu_pairtable.py::test_hybrid_streams_expand_as_the_host_reference_takes_them
        runs, values = z["runs"], z["values"]
        begin, status, const = runs["out_begin"], runs["status"], runs["const_value"]
        assert runs["total"] == sum(c[2] for c in i["cases"]) == len(values)
        declined = 0
        for k, (stream, bw, n) in enumerate(i["cases"]):
            rc, want = engine.rle_hybrid_take_host(stream, bw, n, np.arange(n))
            assert status[k] == rc and np.array_equal(values[begin[k]:begin[k + 1]], want), (k, bw, n)      # -1 for what a declined stream did not give
            if const[k] != -1:
                assert rc == 0 and n > 0 and (want == const[k]).all()
            declined += rc != 0
        assert declined > 50 and const[-2] == 1 and const[-1] == -1
        assert z["outside"]["status"].tolist() == [_lib.MSPA_EINVAL] * 2 and z["outside_values"].tolist() == [-1] * 6


# parquet_double_columns_device: "Two small read-backs."
@case("pair_table", "visindex", ["parquet_double_columns_device", "pair_bin_codes", "pair_partition"])
class _PairTable:
    """pairtable.PairTable on small files -- dictionary-coded v1 pages, v2 pages, PLAIN pages of the project's own writer, a file of
    one row -- decodes the four DOUBLE columns (parquet_double_columns_device behind the Snappy block route); then the overlap
    column's classes and per-class row lists at sizes around the 2 048-row tile."""
    SIZES = (1, 65, 2049, 8193)

    @staticmethod
    def build():
        import tempfile
        import pairtable_util as PU
        tmp = tempfile.TemporaryDirectory(prefix="poison_pairtable")
        frames = [PU.frame(2500, 21, scene="scene0000_00"), PU.frame(1, 22, scene="scene0001_00"), PU.frame(3011, 23, scene="scene0002_00")]
        paths = {k: os.path.join(tmp.name, f"{k}.parquet") for k in ("project", "pandas", "v2", "one")}
        PU.write_project(paths["project"], frames)
        PU.write_pandas(paths["pandas"], frames, row_group_size=3000, dictionary_pagesize_limit=4096, data_page_size=8192)
        PU.write_pandas(paths["v2"], frames, row_group_size=3000, data_page_version="2.0", compression="none", data_page_size=8192,
                        dictionary_pagesize_limit=4096)
        PU.write_pandas(paths["one"], [PU.frame(1, 24)])
        overlaps = {n: PU.overlap_column(n, 100 + n) for n in _PairTable.SIZES}
        edges = PU.edges_of(*PU.EDGE_SETS[0]).astype(np.float64)
        return {"tmp": tmp, "paths": paths, "overlaps_np": overlaps, "edges_np": edges, "overlaps": {n: dev(x) for n, x in overlaps.items()},
                "edges": dev(edges)}

    @staticmethod
    def run(i):
        from mspa import pairtable
        out = {"columns": {k: pairtable.PairTable(p, DEV).columns() for k, p in i["paths"].items()}}
        for n, x in i["overlaps"].items():
            codes, tile_counts = engine.pair_bin_codes(x, i["edges"])
            out[f"classes_{n}"] = (codes, tile_counts, engine.pair_partition(codes, tile_counts))
        return out

    @staticmethod
    def expect(i, z):
        import pairtable_util as PU
        import pyarrow.parquet as pq
        from mspa import pairtable
        z = host(z)
        for k, p in i["paths"].items():
            t = pq.read_table(p, columns=list(pairtable.DOUBLE_COLUMNS))
            want = np.stack([t.column(c).to_pandas().to_numpy(dtype=np.float64) for c in pairtable.DOUBLE_COLUMNS])
            assert isinstance(z["columns"][k], np.ndarray), (k, z["columns"][k])
            assert nan_equal_bits(z["columns"][k], want), k
        rows = int(_lib.load().mspa_pair_tile_rows())
        for n, x in i["overlaps_np"].items():
            codes, tile_counts, (order, begin) = z[f"classes_{n}"]
            want = PU.classify_numpy(x, i["edges_np"])
            assert np.array_equal(codes, want)
            assert np.array_equal(tile_counts, np.stack([np.bincount(want[t:t + rows], minlength=256) for t in range(0, n, rows)]))
            assert np.array_equal(begin, np.concatenate([[0], np.cumsum(np.bincount(want, minlength=256))]))
            assert np.array_equal(order, np.argsort(want, kind="stable"))


# parquet_double_columns_device: "Two small read-backs."
@case("pair_table_values_at_the_edges", "visindex", ["parquet_double_columns_device"])
class _PairTableEdges:
    """csrc/pair_table.hip ``load64``: "two aligned words where both lie inside the buffer, bytes otherwise".  Two PLAIN pages of
    three DOUBLE values each, in buffers of their own:

      front  [1 byte][3 values][16 bytes]   the first value starts at byte 1 of ``pages``.  With ``pages`` at 1 (3) mod 8 its address
             is 2 (4) mod 8, ``lo_at`` = that address rounded down to 8 = pages - 1 (- 3) < base: the byte loop, whose result must not
             know the bytes in front of the buffer.  In the plain run (pages at 0 mod 8) lo_at == base: the two-word form.
      back   [16 bytes][1 byte][3 values]   the last value ENDS at the buffer's last byte, bytes 33 .. 40 of 41: its address is
             (pages + 33) mod 8 = 1, 2 or 4, never 0, so lo_at + 16 >= pages + 32 + 16 > pages + 41 in every run: the byte loop.
    The values in between take the two-word form everywhere."""
    VALUES = (0x3FF8000000000000, 0x8000000000000000, 0x7FF8000000ABCDEF, 0x0000000000000001, 0xC08F400000000000, 0x7FF0000000000000)

    @staticmethod
    def build():
        import struct
        v = [struct.pack("<Q", x) for x in _PairTableEdges.VALUES]
        front = b"\x11" + b"".join(v[:3]) + b"\x22" * 16
        back = b"\x33" * 17 + b"".join(v[3:])
        assert len(front) == len(back) == 41
        one = lambda x: _i64([x])                                                # noqa: E731
        return {"front": dev(np.frombuffer(front, dtype=np.uint8)), "back": dev(np.frombuffer(back, dtype=np.uint8)),
                "tables": {"front": (one(1), one(24), one(3)), "back": (one(17), one(24), one(3))},
                "flags": dev(np.zeros(1, dtype=np.int32)), "zero": one(0)}

    @staticmethod
    def run(i):
        out = {}
        for key in ("front", "back"):
            pages, (off, size, values) = i[key], i["tables"][key]
            r = pages.data_ptr() % 8
            if key == "front" and r:
                assert 0 < (r + 1) % 8 and (pages.data_ptr() + 1) // 8 * 8 < pages.data_ptr()        # shift != 0 and lo_at < base
            if key == "back":
                a = pages.data_ptr() + 33
                assert a % 8 and a // 8 * 8 + 16 > pages.data_ptr() + 41                              # shift != 0 and lo_at + 16 > base + bytes
            out[key] = engine.parquet_double_columns_device(pages, off, size, values, i["flags"], i["zero"], 3, i["zero"], i["zero"], i["zero"], i["zero"])
        return out

    @staticmethod
    def expect(i, z):
        z = host(z)
        for key, want in (("front", _PairTableEdges.VALUES[:3]), ("back", _PairTableEdges.VALUES[3:])):
            values, status = z[key]
            assert values.view(np.uint64).tolist() == list(want), (key, values)
            assert not any(np.asarray(status[k]).any() for k in ("layout", "levels", "indices", "values")) and status["null_pages"] == 0


# =====================================================================================================================
# ScanNet prep (K11)
# =====================================================================================================================

# prep_objects: "the slot offsets go up from pageable memory and ``bitset_csr`` reads its total back"
@case("scan_prep", "scanprep", ["prep_labels", "prep_align", "prep_objects"])
class _ScanPrep:
    """One ragged window -- 1, 65, 130 (no objects) and 1001 vertices -- through prep_align, prep_labels and prep_objects (with K9 on
    its membership rows), raw outputs and ``scanprep.prepare_window``'s assembly; then windows of no vertices at all, with and
    without object slots: ``n_words == 0``, the branch of mspa_prep_objects that has no membership rows to clear."""
    SPECS = ((1, 1, "general"), (65, 3, "z"), (130, 0, None), (1001, 7, "general"))

    @staticmethod
    def build():
        import tempfile
        from mspa import scanprep
        tmp = tempfile.TemporaryDirectory(prefix="poison_scanprep")
        scans = []
        for k, (n, objs, align) in enumerate(_ScanPrep.SPECS):
            name = f"scene{k:04d}_00"
            paths = synth.write_raw_scan(tmp.name, name, n, objs, seed=100 + k, axis_align=align)
            files = {f: paths[f] for f in ("mesh_file", "agg_file", "seg_file", "meta_file")}
            scans.append(scanprep.load_raw_scan(name, label_map=scanprep.read_label_mapping(paths["label_map_file"]), **files))
        tabs = [s.tables for s in scans]
        pad = [np.zeros(1, dtype=np.int32)]
        cat = scanprep._cat
        return {"tmp": tmp, "scans": scans, "n_vertices": [s.vertices.shape[0] for s in scans], "n_slots": [t.n_slots for t in tabs],
                "verts": dev(cat([s.vertices for s in scans], np.float32, (6,))),
                "mats": dev(np.stack([np.asarray(s.axis_align_matrix, dtype=np.float64) for s in scans])),
                "seg": dev(cat([s.seg for s in scans], np.int32)),
                "tab_off": dev(engine._ragged_offsets([t.seg2inst.shape[0] for t in tabs])),
                "lab_off": dev(engine._ragged_offsets([t.label_value.shape[0] for t in tabs])),
                "seg2inst": dev(cat([t.seg2inst for t in tabs] + pad, np.int32)), "seg2label": dev(cat([t.seg2label for t in tabs] + pad, np.int32)),
                "label_value": dev(cat([t.label_value for t in tabs], np.uint32).view(np.int32)),
                "nothing": {"verts": torch.zeros((0, 6), dtype=torch.float32, device=DEV), "aligned": torch.zeros((0, 6), dtype=torch.float64, device=DEV),
                            "inst": torch.zeros((0,), dtype=torch.int32, device=DEV)}}

    @staticmethod
    def run(i):
        from mspa import scanprep
        spans = engine.prep_spans(i["n_vertices"], DEV)
        aligned = engine.prep_align(spans, i["verts"], i["mats"])
        inst, label, index = engine.prep_labels(spans, i["seg"], i["tab_off"], i["seg2inst"], i["seg2label"], i["lab_off"], i["label_value"])
        out = {"aligned": aligned, "labels": (inst, label, index), "objects": engine.prep_objects(spans, inst, i["verts"], aligned, i["n_slots"]),
               "window": [r.as_tuple() + (r.num_unique_instances,) for r in scanprep.prepare_window(i["scans"], torch.device(DEV))]}
        e = i["nothing"]
        for name, n_vertices, n_objects in (("no_vertices_no_objects", [0], [0]), ("no_vertices_two_slots", [0, 0], [2, 0])):
            spans = engine.prep_spans(n_vertices, DEV)
            out[name] = engine.prep_objects(spans, e["inst"], e["verts"], e["aligned"], n_objects)
        return out

    @staticmethod
    def expect(i, z):
        import scanprep_util as U
        z = host(z)
        obj, first = z["objects"], 0
        for s, (scan, got) in enumerate(zip(i["scans"], z["window"])):
            want = U.numpy_export(scan)
            U.assert_same_export(got[:-1], want.as_tuple())
            assert got[-1] == want.num_unique_instances == obj["unique"][s], scan.name
            inst = np.asarray(want.instance_ids)
            for k in range(i["n_slots"][s]):                 # the raw rows: a slot without a vertex keeps +inf / -inf and a zero count
                members = np.nonzero(inst == k + 1)[0]
                r = first + k
                assert obj["count"][r] == len(members) and np.array_equal(obj["indices"][obj["offsets"][r]:obj["offsets"][r + 1]], members)
                if len(members) == 0:
                    for name, value in (("lo_unaligned", np.inf), ("hi_unaligned", -np.inf), ("lo_aligned", np.inf), ("hi_aligned", -np.inf)):
                        assert (obj[name][r] == value).all(), (scan.name, k, name)
            assert obj["zero_count"][s] == (inst == 0).sum()
            first += i["n_slots"][s]
        assert i["n_slots"][2] == 0 and first == len(obj["count"])
        a, b = z["no_vertices_no_objects"], z["no_vertices_two_slots"]
        assert a["count"].shape == (0,) and a["unique"].tolist() == [0] and a["zero_count"].tolist() == [0] and a["offsets"].tolist() == [0]
        assert b["count"].tolist() == [0, 0] and b["unique"].tolist() == [0, 0] and b["offsets"].tolist() == [0, 0, 0] and len(b["indices"]) == 0
        assert (b["lo_unaligned"] == np.inf).all() and (b["hi_aligned"] == -np.inf).all()


@case("parse_int_lists_device", "scanprep", ["parse_int_lists_device"])          # "one small read-back: the size to allocate"; offsets and status return on the host
class _ParseIntLists:
    DAMAGED = {1: b"1,,2", 3: b"1 2", 4: b"01,5", 6: b"2147483648", 7: b"12345678901", 9: b"1,2,x", 10: b"-4,5", 12: b",1", 13: b"1,", 15: b"1.5"}

    @staticmethod
    def build():
        rng = np.random.default_rng(2)
        well = [b"", b"  ", b"0", b"7", b"1,2,3", b" 1 ,\t2\n,\r\n3 ", b"2147483647,0", ", ".join(map(str, rng.integers(0, 200000, 1501).tolist())).encode()]
        sound = [b"5, 6, 7", b"", b"9", b"100,200", b"3", b"4,4,4,4", b"1234567890"]
        batch, k = [], 0
        for a in range(17):                                 # damaged arrays between sound ones: a status is set for exactly those
            if a in _ParseIntLists.DAMAGED:
                batch.append(_ParseIntLists.DAMAGED[a])
            else:
                batch.append(sound[k % len(sound)])
                k += 1
        return {"well": well, "batch": batch}

    @staticmethod
    def run(i):
        return {"well": engine.parse_int_lists_device(i["well"], DEV), "batch": engine.parse_int_lists_device(i["batch"], DEV),
                "counted": engine.parse_int_lists_device([b"1,2,3", b"4,5"], DEV, expected_counts=[3, 3]),
                "none": engine.parse_int_lists_device([], DEV), "blank": engine.parse_int_lists_device([b"", b""], DEV)}

    @staticmethod
    def expect(i, z):
        import json
        z = host(z)
        values, off, status = z["well"]
        assert status.tolist() == [0] * len(i["well"])
        for a, text in enumerate(i["well"]):
            assert values[off[a]:off[a + 1]].tolist() == json.loads(b"[" + text + b"]"), a
        values, off, status = z["batch"]
        assert [a for a in range(17) if status[a] != 0] == sorted(_ParseIntLists.DAMAGED)
        for a in range(17):
            if a not in _ParseIntLists.DAMAGED:
                assert values[off[a]:off[a + 1]].tolist() == json.loads(b"[" + i["batch"][a] + b"]"), a
        assert z["counted"][2].tolist() == [0, 16] and z["none"][1].tolist() == [0] and z["blank"][2].tolist() == [0, 0]


# =====================================================================================================================
# Above engine.py: scene upload, heads, the index written and read back
# =====================================================================================================================

@functools.lru_cache(maxsize=None)
def heads_world():
    """tests/test_gpu_heads.py's 96 x 128 world: 7 frames, 3000 points, the oracle's pair table and visibility index."""
    hw = (96, 128)
    sc = synth.make_scene(3001, n_points=3000, n_frames=7, color_hw=hw, depth_hw=hw, invalid_pose_frac=0.15, with_color=False)
    table = O.frames_relations_scene(sc.points[:, :3], sc.K, sc.A, sc.E, sc.depth, sc.color_hw)
    vis = O.visibility_index_scene(sc.points[:, :3], sc.K, sc.A, sc.E, sc.depth, sc.color_hw)
    rows = [{"scene_id": sc.scene_id, "image_id1": a, "image_id2": b, "overlap": max(float(v["overlap"]), 1.0), "distance": float(v["distance"]),
             "yaw": float(v["yaw"]), "pitch": float(v["pitch"])} for (a, b), v in table.items()]
    return sc, rows, vis


def _head_records(scene, sc, rows):
    import random
    from mspa import heads
    out = {}
    random.seed(9)
    out["visual_correspondence"] = heads.visual_correspondence_records(scene, rows, sc.color_hw)
    random.seed(13)
    out["depth_estimation"] = heads.depth_estimation_records(scene, sc.scene_id, sc.color_hw, max_samples=5)
    for qt in ("displacement_vector", "total_distance", "yaw_movement"):
        random.seed(3)
        out["camera_movement_" + qt] = heads.camera_movement_records(scene, rows, qt, sc.color_hw)
    return out


# HOST_STEPS: the heads and the prefetcher work on the host between the launches
@case("heads_end_to_end", "e2e", ["vertex_visibility", "select_common_point", "project_samples", "pair_pose"])
class _HeadsEndToEnd:
    """A scene uploaded directly (SceneOnDevice) and handed out by a ScenePrefetcher whose upload slots are allocated under the
    patch, through the visual-correspondence, depth-estimation and camera-movement heads; then the scene's visibility index
    formatted, paged and compressed on the device (visindex.from_bits)."""
    @staticmethod
    def build():
        sc, rows, vis = heads_world()
        return {"sc": sc, "rows": rows, "vis": vis}

    @staticmethod
    def run(i):
        from mspa import upload, visindex
        from mspa.scene import SceneOnDevice
        sc, rows = i["sc"], i["rows"]
        scene = SceneOnDevice(sc.K, sc.A, sc.E, sc.depth, sc.color_hw, sc.points, DEV)
        out = {"direct": _head_records(scene, sc, rows), "visibility": dict(scene._visibility()), "depth": scene.depth}
        bits, n = scene._visibility()["bits"], int(scene.xyz.shape[0])
        on_host = visindex.from_bits(bits, scene.ids, n)
        on_dev = visindex.from_bits(bits, scene.ids, n, text=True, indices=False)
        paged = visindex.from_bits(bits, scene.ids, n, text=True, indices=False, pages=True, page_bytes=1 << 14)
        out["index"] = {"host": on_host.to_arrow(sc.scene_id).to_pydict(), "device": on_dev.to_arrow(sc.scene_id).to_pydict(),
                        "pages": dict(paged.values_pages)}
        saved = upload._SLOT_POOL                            # slots are pooled per process: this run allocates its own, under the patch
        upload._SLOT_POOL = {}
        try:
            for n_scene, handed in enumerate(upload.ScenePrefetcher([sc, sc], DEV, slots=2, threaded=False)):
                out[f"prefetched_{n_scene}"] = {"records": _head_records(handed, sc, rows), "depth": handed.depth.clone(),
                                                "bits": handed._visibility()["bits"].clone()}
        finally:
            upload._SLOT_POOL = saved
        return out

    @staticmethod
    def expect(i, z):
        import random
        from mspa import heads
        from mspa import templates as T
        from golden_util import close_f64, same_f64
        sc, rows, vis = i["sc"], i["rows"], i["vis"]
        z = host(z)
        ids = O.valid_image_ids(sc.E)
        for key in ("prefetched_0", "prefetched_1"):
            assert z[key]["records"] == z["direct"], key
            assert np.array_equal(z[key]["depth"], z["depth"]) and np.array_equal(z[key]["bits"], z["visibility"]["bits"]), key
        assert np.array_equal(z["depth"].view(np.uint16), np.stack([sc.depth[k] for k in ids]))
        got_bits = unpack_rows(z["visibility"]["bits"], sc.points.shape[0])
        for k, image_id in enumerate(ids):
            assert np.nonzero(got_bits[k])[0].tolist() == list(vis["image_to_points"][image_id]), image_id
        # the records: what tests/test_gpu_heads.py pins them to (the record stage on ORACLE numerics, same seeds)
        got = z["direct"]
        n_common = [len(np.intersect1d(vis["image_to_points"][r["image_id1"]], vis["image_to_points"][r["image_id2"]])) for r in rows]
        random.seed(9)
        draws = heads.visual_correspondence_draws(rows, n_common, T.VISUAL_CORRESPONDENCE)
        want = []
        for n, (row, dr) in enumerate(zip(rows, draws)):
            if dr is None:
                continue
            first, second = (row["image_id2"], row["image_id1"]) if dr["swap"] else (row["image_id1"], row["image_id2"])
            common = np.intersect1d(vis["image_to_points"][first], vis["image_to_points"][second])
            verts = [int(common[j]) for j in dr["positions"]]
            uv1 = np.stack([O.point_2d_in_image(sc.points[v], sc.K, sc.A @ sc.E[first], sc.depth[first], sc.color_hw)[0][0] for v in verts])
            uv2 = np.stack([O.point_2d_in_image(sc.points[v], sc.K, sc.A @ sc.E[second], sc.depth[second], sc.color_hw)[0][0] for v in verts])
            want.append(heads.visual_correspondence_record(row, n, dr, uv1, uv2, sc.color_hw))
        assert len(want) > 3 and sorted(got["visual_correspondence"], key=lambda r: r["id"]) == sorted(want, key=lambda r: r["id"])
        random.seed(13)
        draws = heads.depth_estimation_draws(ids, {k: len(vis["image_to_points"][k]) for k in ids}, 5, T.DEPTH_ESTIMATION)
        want = []
        for dr in draws:
            for j, pick in zip(dr["positions"], dr["picks"]):
                v = vis["image_to_points"][dr["image_id"]][j]
                uv, d = O.point_2d_in_image(sc.points[v], sc.K, sc.A @ sc.E[dr["image_id"]], sc.depth[dr["image_id"]], sc.color_hw)
                want.append(heads.depth_estimation_record(sc.scene_id, dr["image_id"], v, uv[0], float(d[0]), pick, sc.color_hw))
        assert got["depth_estimation"] == want and len(want) == 5
        for qt in ("displacement_vector", "total_distance", "yaw_movement"):
            random.seed(3)
            want = []
            for n, row in enumerate(rows):
                E1, E2 = sc.A @ sc.E[row["image_id1"]], sc.A @ sc.E[row["image_id2"]]
                want.append(heads.camera_movement_record(row, n, qt, (np.linalg.inv(E1) @ E2)[:3, 3], (np.linalg.inv(E2) @ E1)[:3, 3], sc.color_hw))
            records = [dict(r, answer_values=dict(r["answer_values"])) for r in got["camera_movement_" + qt]]
            assert len(records) == len(want) == len(rows)
            for g, w in zip(records, want):
                gv, wv = g["answer_values"].pop("displacement_vector"), w["answer_values"].pop("displacement_vector")
                if qt == "displacement_vector":
                    g.pop("gt_value"), w.pop("gt_value")
                assert g == w
                assert same_f64(gv, wv) or close_f64(gv, wv, rtol=1e-12, scale=1e-9)
        assert z["index"]["device"] == z["index"]["host"] and len(z["index"]["host"]["key"]) == len(ids) + sc.points.shape[0]
        pages = z["index"]["pages"]
        assert int(np.sum(pages["num_values"])) == len(ids) + sc.points.shape[0] and len(pages["chunk"]) == int(np.sum(pages["compressed"]))


# index_rows_to_bits / index_rows_to_lists: "Synchronises"
@case("index_readers", "e2e", ["index_rows_to_bits", "index_rows_to_lists", "index_lists_pick", "snappy_decompress_blocks_device"])
class _IndexReaders:
    """visindex.SceneRowGroups on the edge file of tests/index_lists_util.py (4 KiB pages, one row 190 KB long): the scene's rows
    as bitsets and as lists, picks from the lists -- the staging buffers, payloads and pick tables of visindex.py."""
    NO_BITS = ("beyond", "float")                          # a vertex that is none at this width; a list that is no list of integers

    @staticmethod
    def build():
        import tempfile
        import index_lists_util as LU
        tmp = tempfile.TemporaryDirectory(prefix="poison_index")
        return {"tmp": tmp, "path": LU.edge_file(tmp.name), "request": LU.edge_request()}

    @staticmethod
    def run(i):
        import index_lists_util as LU
        from mspa import visindex
        index = visindex.SceneRowGroups(i["path"])
        index.page_kinds = "any"
        present, bits = index.scene_bits(LU.SCENE, [k for k in i["request"] if k not in _IndexReaders.NO_BITS], LU.N_POINTS)
        lists = index.scene_lists(LU.SCENE, i["request"])
        i.setdefault("lists_of_run", []).append(lists)      # (an object, not an output: expect reads the zero run's, the first)
        picks = [("duplicate", 3), ("descending", 0), ("descending", 1), ("duplicate", 5), ("one", 0), ("long", 0), ("long", 14999),
                 ("long", 29999), ("last", 1), ("bit63", 5), ("spaces", 3), ("beyond", 0), ("float", 1)]
        return {"present": present, "bits": bits, "lists_present": lists.present, "counts": lists.counts, "values": lists.values,
                "picked": lists.pick(picks, LU.N_POINTS), "stats": dict(index.decode_stats)}

    @staticmethod
    def expect(i, z):
        import json
        import index_lists_util as LU
        from mspa.scene import pack_index_lists
        z = host(z)
        present = [k for k in i["request"] if k != "absent"]
        assert z["lists_present"] == present and z["present"] == [k for k in present if k not in _IndexReaders.NO_BITS]
        want = pack_index_lists([json.loads(LU.EDGE_ROWS[k]) for k in z["present"]], LU.N_POINTS)   # tests/test_gpu_visindex_decode.py's statement
        assert np.array_equal(z["bits"], want)
        assert z["counts"].tolist() == [len(json.loads(LU.EDGE_ROWS[k])) for k in present]
        assert z["picked"].tolist() == [5, 5, 3, 700, 7, 1, 29999, 59999, LU.N_POINTS - 1, 65471, 64, 3, 9]
        assert z["stats"]["scenes_declined"] == 0
        LU.check_edge_lists(i["lists_of_run"][0])           # the zero run's lists object against json.loads, in full


# HOST_STEPS: packing, upload and the hand-over of each slot
@case("prefetch_packed_scenes", "e2e", ["inflate_blocks_device", "png_unfilter_device"])
class _PrefetchPacked:
    """Scenes whose depth frames arrive as PNG files, packed (pinned staging) and decoded on the device inside the upload slots: two
    slots, depth shapes that change in a slot (its scanline scratch is reallocated), one frame per scene an 8-bit PNG the packer
    declines and the host reader fills in.  Packing, slots and decode all allocate under the patch."""
    SPECS = (((48, 64), 4), ((60, 80), 5), ((60, 80), 3), ((48, 64), 4))

    @staticmethod
    def build():
        import tempfile
        from PIL import Image
        from mspa import ingest
        from spatial_engine.utils.scannet_utils.handler import _images
        tmp = tempfile.TemporaryDirectory(prefix="poison_packed")
        scenes = []
        for n, (hw, n_frames) in enumerate(_PrefetchPacked.SPECS):
            sc = synth.make_scene(700 + n, n_points=600, n_frames=n_frames, color_hw=hw, depth_hw=hw, invalid_pose_frac=0.0, with_color=False)
            ids = list(sc.valid_image_ids)
            paths = []
            for k, image_id in enumerate(ids):
                paths.append(os.path.join(tmp.name, f"{n}_{image_id}.png"))
                Image.fromarray((sc.depth[image_id] >> 8).astype(np.uint8) if k == 1 else sc.depth[image_id]).save(paths[-1], compress_level=1)
            scenes.append({"sc": sc, "ids": ids, "paths": paths, "hw": hw, "want": ingest.read_depth_frames(paths, 2, general_reader=_images.read_depth)})
        return {"tmp": tmp, "scenes": scenes}

    @staticmethod
    def run(i):
        from mspa import ingest, sweep, upload
        pool = ingest.PinnedBytesPool()
        hosts = []
        for n, s in enumerate(i["scenes"]):
            packed = ingest.pack_scene_depth(s["paths"], 2, pool=pool)
            hosts.append(sweep.HostScene(f"p{n}", s["sc"].K, s["sc"].A, {k: s["sc"].E[k].copy() for k in s["ids"]}, {}, s["hw"], s["sc"].points,
                                         packed=packed, depth_ids=s["ids"]))
        saved = upload._SLOT_POOL
        upload._SLOT_POOL = {}
        try:
            return [{"depth": scene.depth.clone(), "bits": scene._visibility()["bits"].clone()}
                    for scene in upload.ScenePrefetcher(hosts, DEV, slots=2, threaded=False, decode_on_device=True)]
        finally:
            upload._SLOT_POOL = saved

    @staticmethod
    def expect(i, z):
        z = host(z)
        assert len(z) == len(i["scenes"])
        for got, s in zip(z, i["scenes"]):
            assert np.array_equal(got["depth"].view(np.uint16), s["want"])
            assert np.array_equal(s["want"][1], s["sc"].depth[s["ids"][1]] >> 8) and np.array_equal(s["want"][2], s["sc"].depth[s["ids"][2]])
            assert got["bits"].any()
