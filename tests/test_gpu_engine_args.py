"""The argument checks of mspa/engine.py: every tensor is checked before its ``data_ptr()`` reaches libmspa.so.

The table tests launch NO kernel: ``_lib.load`` is replaced by a recorder around the real library.  Host-only entry points
(``*_bytes``, ``*_capacity``, ``*_host``, ``mspa_last_error_string``) pass through; every other ``mspa_*`` function records its
arguments and returns MSPA_OK.  A missing check is therefore a failed assertion here, never a launch with a bad pointer.

  * reject table: per wrapper one valid call and variants with exactly ONE argument wrong (dtype, rank, host tensor,
    non-contiguous, an extent that disagrees with its partner, an output one row short, an ``out`` dict allocated for another
    pair count / image size, an unknown ``want`` name) -> ValueError that names the argument, nothing recorded;
  * accept table: the valid call (slot-style where the wrapper has slots: more rows than n, ``[:F]`` slices) is recorded exactly
    once, pointers = the tensors' ``data_ptr()``, integers = the extents, in the order ``_lib._SIGNATURES`` declares;
  * two real launches: ``select_common_point`` / ``project_samples`` with a non-contiguous index view equal the contiguous call.

``bitset_csr``, ``format_lists_device`` and ``prep_objects`` size a second launch by what the first one wrote -- which a recorder does
not write -- so they are in the reject table only (tests/test_gpu_format_lists.py, test_gpu_scanprep.py run them for real).
"""
import ctypes
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from mspa import engine, synth, _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
HW = (48, 64)
ANY = object()            # an argument the caller cannot see: an internal workspace, a host array
F64, F32, I64, I32, I16, U8 = torch.float64, torch.float32, torch.int64, torch.int32, torch.int16, torch.uint8


class Recorder:
    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if not name.startswith("mspa_") or name.endswith(("_bytes", "_capacity", "_host")) or name == "mspa_last_error_string":
            return fn

        def record(*args):
            self.calls.append((name, args))
            return _lib.MSPA_OK
        return record


@pytest.fixture
def lib(monkeypatch):
    rec = Recorder(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: rec)
    return rec


def z(*shape, dtype=F64):
    return torch.zeros(shape, dtype=dtype, device=DEV)


def strided(t):
    """Same shape, dtype and device, every second element of a buffer twice as wide."""
    return torch.zeros(tuple(t.shape[:-1]) + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)[..., ::2]


def pinhole_mats(n=2):
    return torch.from_numpy(engine.frame_matrices(np.eye(4), None, [np.eye(4)] * n)).to(DEV)


def pair_args(alloc, **kw):
    return dict(depth=z(2, *HW, dtype=I16), mats=pinhole_mats(), pairs=z(2, 2, dtype=I32), image_hw=HW, out=alloc(2, HW), **kw)


def corr_out(n, hw):
    return engine.alloc_pair_correspondences(n, hw, DEV)


def dense_out(n, hw):
    return engine.alloc_pair_outputs(n, hw, engine.PAIR_OUTPUTS, DEV)           # all ten: every output slot of the C ABI is pinned


def cameras(**kw):
    return dict(xyz=z(64, 3), cam_mats=z(2, 3, 16), depth=z(2, *HW, dtype=I16), image_hw=HW, **kw)


def spans():
    return engine.prep_spans([64, 64], DEV)


def edit(d, **kw):
    return {**d, **kw}


def case(fn, make, launch=None, expect=None, strided_ok=(), batched=(), wrong=()):
    """``make()``: the valid keyword arguments.  ``expect(a, r)``: what ``launch`` must have received, from the arguments and the
    wrapper's result.  ``strided_ok``: arguments handed over with their strides (or copied); ``batched``: arguments that may
    carry a leading batch dimension.  ``wrong``: (argument the error names, replacement(a) -> new value of that argument) on top
    of the automatic per-tensor variants."""
    return SimpleNamespace(fn=fn, make=make, launch=launch, expect=expect, strided_ok=strided_ok, batched=batched, wrong=wrong)


S = engine._stream_ptr
CASES = {c.fn: c for c in [
    case("inflate_blocks_device",
         lambda: dict(src=z(64, dtype=U8), offsets=z(8, dtype=I64)[:2], nbytes=z(8, dtype=I64)[:2], block_bytes=300,
                      out=z(3, 512, dtype=U8), status=z(3, dtype=I32)),
         "mspa_inflate_blocks_device",
         lambda a, r: [a["src"], a["offsets"], a["nbytes"], 64, 2, 300, a["out"], 512, a["status"], ANY, S()],
         wrong=[("nbytes", lambda a: z(3, dtype=I64)), ("out", lambda a: z(1, 512, dtype=U8)), ("out", lambda a: z(3, 256, dtype=U8)),
                ("out", lambda a: z(3, 500, dtype=U8)), ("status", lambda a: z(1, dtype=I32))]),
    case("png_unfilter_device",
         lambda: dict(raw=z(4, 12, dtype=U8)[:2], h=2, w=2, status=z(4, dtype=I32), out=z(4, 2, 2, dtype=I16)[:2]),
         "mspa_png_unfilter_device", lambda a, r: [a["raw"], 12, 2, 2, 2, a["out"], a["status"], S()],
         wrong=[("raw", lambda a: z(2, 8, dtype=U8)), ("status", lambda a: z(1, dtype=I32)), ("out", lambda a: z(1, 2, 2, dtype=I16)),
                ("out", lambda a: z(2, 2, 3, dtype=I16))]),
    case("jpeg_decode_device",
         lambda: dict(src=z(64, dtype=U8), offsets=z(2, dtype=I64), nbytes=z(2, dtype=I64),
                      descriptors=z(2, _lib.JPEG_DESC_BYTES, dtype=U8), hw=(8, 8), out=z(3, 8, 8, 3, dtype=U8), status=z(3, dtype=I32)),
         "mspa_jpeg_decode_device",
         lambda a, r: [a["src"], a["offsets"], a["nbytes"], 64, a["descriptors"], 2, 8, 8, a["out"], a["status"], ANY, ANY, S()],
         wrong=[("nbytes", lambda a: z(3, dtype=I64)), ("descriptors", lambda a: z(3, _lib.JPEG_DESC_BYTES, dtype=U8)),
                ("src", lambda a: z(62, dtype=U8)), ("out", lambda a: z(1, 8, 8, 3, dtype=U8)), ("out", lambda a: z(3, 8, 4, 3, dtype=U8)),
                ("status", lambda a: z(1, dtype=I32))]),
    case("jpeg_encode_device",
         lambda: dict(rgb=z(2, 8, 8, 3, dtype=U8), quality=95, out=z(3, 1024, dtype=U8), nbytes=z(3, dtype=I64)),
         "mspa_jpeg_encode_device", lambda a, r: [a["rgb"], 2, 8, 8, 95, 2, a["out"], 1024, a["nbytes"], ANY, ANY, S()],
         wrong=[("rgb", lambda a: z(2, 8, 8, 4, dtype=U8)), ("out", lambda a: z(1, 1024, dtype=U8)), ("nbytes", lambda a: z(1, dtype=I64))]),
    case("png_encode_device",
         lambda: dict(depth=z(2, 4, 4, dtype=I16), out=z(3, 256, dtype=U8), nbytes=z(3, dtype=I64)),
         "mspa_png_encode_device", lambda a, r: [a["depth"], 2, 4, 4, a["out"], 256, a["nbytes"], ANY, ANY, S()],
         wrong=[("out", lambda a: z(1, 256, dtype=U8)), ("nbytes", lambda a: z(1, dtype=I64))]),
    case("draw_spans_device", lambda: dict(images=z(2, 8, 8, 3, dtype=U8), spans=z(2, 5, dtype=I32)),
         "mspa_draw_spans_device", lambda a, r: [a["spans"], 2, a["images"], 2, 8, 8, S()],
         wrong=[("spans", lambda a: z(2, 4, dtype=I32)), ("images", lambda a: z(2, 8, 8, 4, dtype=U8))]),
    case("blend_masks_device", lambda: dict(images=z(2, 8, 8, 3, dtype=U8), labels=z(2, 8, dtype=I64), masks=z(16, dtype=U8)),
         "mspa_blend_masks_device", lambda a, r: [a["labels"], 2, a["masks"], 16, a["images"], 2, 8, 8, S()],
         wrong=[("labels", lambda a: z(2, 7, dtype=I64))]),
    case("resize_rgb_device", lambda: dict(frames=z(2, 8, 8, 3, dtype=U8), hw=(4, 4), out=z(2, 4, 4, 3, dtype=U8)),
         "mspa_resize_rgb_device",
         lambda a, r: [a["frames"], 2, 8, 8, 24, 192, a["out"], 4, 4, _lib.RESIZE_BICUBIC, ANY, ANY, ANY, ANY, ANY, ANY, S()],
         strided_ok=("frames",), wrong=[("out", lambda a: z(3, 4, 4, 3, dtype=U8)), ("frames", lambda a: z(2, 8, 8, 4, dtype=U8))]),
    case("pair_reproject", lambda: pair_args(dense_out, rgb=z(2, *HW, 3, dtype=U8), flags=_lib.PAIR_FAST),
         "mspa_pair_reproject",
         lambda a, r: [a["depth"], a["rgb"], a["mats"], 2, a["pairs"], 2, 48, 64, 48, 64] + [a["out"][k] for k in (
             "vis_bits", "vis_u8", "valid_u8", "pix_i16", "xyz_f32", "rgba", "xyz_f64", "uv_f64", "depth_f64", "counts")] + [_lib.PAIR_FAST, S()],
         wrong=[("mats", lambda a: pinhole_mats(3)), ("mats", lambda a: z(2, 7, 16)), ("pairs", lambda a: z(2, 3, dtype=I32)),
                ("out", lambda a: dense_out(3, HW)), ("out", lambda a: dense_out(1, HW)), ("out", lambda a: dense_out(2, (48, 128))),
                ("out", lambda a: edit(a["out"], counts=strided(a["out"]["counts"]))), ("out", lambda a: edit(a["out"], counts=z(2, 2, dtype=I64))),
                ("out", lambda a: edit(a["out"], vis_bits=a["out"]["vis_bits"].cpu())), ("rgb", lambda a: z(2, 48, 32, 3, dtype=U8)), ("rgb", lambda a: z(3, *HW, 3, dtype=U8))]),
    case("pair_correspondences", lambda: pair_args(corr_out, flags=_lib.PAIR_FAST),
         "mspa_pair_correspondences",
         lambda a, r: [a["depth"], a["mats"], 2, a["pairs"], 2, 48, 64, 48, 64, a["out"]["vis_bits"], a["out"]["cpix"],
                       a["out"]["tile_counts"], a["out"]["counts"], ANY, ANY, _lib.PAIR_FAST, S()],
         wrong=[("mats", lambda a: pinhole_mats(3)), ("out", lambda a: corr_out(3, HW)), ("out", lambda a: corr_out(1, HW)),
                ("out", lambda a: corr_out(2, (48, 128))), ("out", lambda a: {k: v for k, v in a["out"].items() if k != "cpix"}),
                ("out", lambda a: edit(a["out"], counts=z(1, 2, dtype=I32))), ("out", lambda a: edit(a["out"], cpix=a["out"]["cpix"][:, :, :1])),
                ("workspace", lambda a: z(64, dtype=I32).cpu())]),
    case("vertex_visibility", lambda: cameras(want=("bits", "count")),
         "mspa_vertex_visibility_ex",
         lambda a, r: [a["xyz"], 64, 3, 1, 0, a["cam_mats"], 2, a["depth"], 48, 64, 48, 64, 0.001, r["bits"], None, None, None, r["count"], S()],
         strided_ok=("xyz",),
         wrong=[("want", lambda a: ("bits", "bogus")), ("cam_mats", lambda a: z(3, 3, 16)), ("xyz", lambda a: z(64, 2))]),
    case("pair_overlap", lambda: dict(bits=z(2, 1, dtype=I64), pairs=z(2, 2, dtype=I32), want_counts=True),
         "mspa_pair_overlap", lambda a, r: [a["bits"], 2, 1, a["pairs"], 2, r[0], r[1], r[2], S()],
         wrong=[("pairs", lambda a: z(2, 3, dtype=I32))]),
    case("scene_overlap", lambda: dict(bits=z(2, 1, dtype=I64), want_counts=True),
         "mspa_scene_overlap", lambda a, r: [a["bits"], 2, 1, ANY, ANY, r[0], r[1], r[2], S()]),
    case("overlap_matrix", lambda: dict(bits_a=z(3, 1, dtype=I64), bits_b=z(2, 1, dtype=I64)),
         "mspa_overlap_matrix", lambda a, r: [a["bits_a"], 3, a["bits_b"], 2, 1, ANY, ANY, r, S()],
         wrong=[("bits_b", lambda a: z(2, 2, dtype=I64))]),
    case("bitset_csr", lambda: dict(bits=z(2, 1, dtype=I64))),
    case("format_lists_device", lambda: dict(offsets=z(3, dtype=I64), values=z(4, dtype=I32)),
         wrong=[("offsets", lambda a: z(0, dtype=I64))]),
    case("bits_transpose", lambda: dict(bits=z(2, 1, dtype=I64)), "mspa_bits_transpose", lambda a, r: [a["bits"], 2, 1, r, S()]),
    case("extract_yaw_pitch", lambda: dict(E_aligned=z(2, 16)), "mspa_extract_yaw_pitch", lambda a, r: [a["E_aligned"], 2, r[0], r[1], S()],
         wrong=[("E_aligned", lambda a: z(2, 4, 4))]),
    case("pair_pose", lambda: dict(E_aligned=z(2, 16), Einv_aligned=z(2, 16), yaw=z(2), pitch=z(2), pairs=z(2, 2, dtype=I32)),
         "mspa_pair_pose", lambda a, r: [a["E_aligned"], a["Einv_aligned"], a["yaw"], a["pitch"], 2, a["pairs"], 2, r, S()],
         wrong=[("yaw", lambda a: z(3)), ("pitch", lambda a: z(1)), ("Einv_aligned", lambda a: z(3, 16)), ("pairs", lambda a: z(2, 3, dtype=I32)),
                ("pairs", lambda a: z(4, dtype=I32))]),
    case("track_to_world", lambda: dict(tracks_xyz=z(2, 3, 3), c2w=z(2, 16), fx_fy_cx_cy=(1.0, 1.0, 1.0, 1.0), image_hw=HW),
         "mspa_track_to_world", lambda a, r: [a["tracks_xyz"], a["c2w"], 2, 3, ANY, 48, 64, r["world"], r["uvn"], r["ok"], S()],
         wrong=[("c2w", lambda a: z(3, 16)), ("c2w", lambda a: z(2, 4, 4)), ("fx_fy_cx_cy", lambda a: (1.0, 1.0, 1.0)),
                ("want", lambda a: ("world", "bogus")), ("tracks_xyz", lambda a: z(2, 3, 4))]),
    case("track_displacement", lambda: dict(world=z(2, 3, 3), w2c=z(2, 16), c2w=z(2, 16), triples=z(2, 3, dtype=I32)),
         "mspa_track_displacement",
         lambda a, r: [a["world"], a["w2c"], a["c2w"], 2, 3, a["triples"], 2, 0.01, 0.01, r[0], r[1], S()],
         wrong=[("w2c", lambda a: z(3, 16)), ("c2w", lambda a: z(1, 16)), ("world", lambda a: z(2, 3, 2)), ("triples", lambda a: z(2, 2, dtype=I32))]),
    case("check_visibility", lambda: dict(uv=z(4, 2), point_depth=z(4), depth_image=z(*HW, dtype=I16), image_hw=HW, want=("visible",)),
         "mspa_check_visibility_ex",
         lambda a, r: [a["uv"], a["point_depth"], 4, a["depth_image"], 48, 64, 48, 64, 0.001, None, None, r["visible"], S()],
         wrong=[("point_depth", lambda a: z(3)), ("want", lambda a: ("visible", "bogus")), ("uv", lambda a: z(4, 3))]),
    case("select_common_point", lambda: dict(bits=z(2, 1, dtype=I64), selections=z(3, 3, dtype=I32)),
         "mspa_select_common_point", lambda a, r: [a["bits"], 2, 1, a["selections"], 3, r, S()],
         strided_ok=("selections",), wrong=[("selections", lambda a: z(3, 2, dtype=I32))]),
    case("project_samples", lambda: cameras(samples=z(2, 2, dtype=I32)),
         "mspa_project_samples_ex",
         lambda a, r: [a["xyz"], 64, 3, 1, a["cam_mats"], 2, a["depth"], 48, 64, 48, 64, 0.001, a["samples"], 2, r[0], r[1], r[2], S()],
         strided_ok=("xyz", "samples"), wrong=[("samples", lambda a: z(2, 3, dtype=I32)), ("cam_mats", lambda a: z(1, 3, 16))]),
    case("track_rigidity_loss", lambda: dict(tracks_xyz=z(2, 3, 3)),
         "mspa_track_rigidity_loss", lambda a, r: [a["tracks_xyz"], 2, 3, 0.01, r, S()], wrong=[("tracks_xyz", lambda a: z(2, 3, 2))]),
    case("track_rigidity_loss_batch", lambda: dict(tracks_xyz=z(2, 2, 3, 3)),
         "mspa_track_rigidity_loss_batch", lambda a, r: [a["tracks_xyz"], 2, 2, 3, 0.01, r, S()], wrong=[("tracks_xyz", lambda a: z(2, 2, 3, 2))]),
    case("track_linkage", lambda: dict(loss=z(3, 3)),
         "mspa_track_linkage", lambda a, r: [a["loss"], 1, 3, 0.1, r[0], r[1], r[2], ANY, ANY, S()],
         batched=("loss",), wrong=[("loss", lambda a: z(3, 2)), ("loss", lambda a: z(1, 2, 3, 3))]),
    case("object_extents", lambda: dict(vis_bits=z(2, 1, dtype=I64), xyz=z(64, 3), obj_offsets=z(2, dtype=I32), obj_vertices=z(4, dtype=I32)),
         "mspa_object_extents",
         lambda a, r: [a["vis_bits"], 2, 1, a["xyz"], 64, a["obj_offsets"], a["obj_vertices"], 4, 1, r[0], r[1], r[2], S()],
         wrong=[("obj_offsets", lambda a: z(0, dtype=I32)), ("xyz", lambda a: z(64, 4))]),
    case("track_pair_distances", lambda: dict(world=z(2, 3, 3), points=[0, 1], visible_frames=[np.array([0, 1]), np.array([0, 1])]),
         "mspa_track_pair_distances", lambda a, r: [a["world"], 2, 3, ANY, ANY, ANY, 2, 2, ANY, ANY, S()]),
    case("prep_labels",
         lambda: dict(spans=spans(), seg=z(128, dtype=I32), tab_off=z(3, dtype=I64), seg2inst=z(4, dtype=I32), seg2label=z(4, dtype=I32),
                      lab_off=z(3, dtype=I64), label_value=z(4, dtype=I32)),
         "mspa_prep_labels",
         lambda a, r: [a["seg"], a["spans"]["vert_off"], a["spans"]["word_off"], 2, 128, 2, a["tab_off"], a["seg2inst"], a["seg2label"],
                       a["lab_off"], a["label_value"], r[0], r[1], r[2], S()],
         wrong=[("seg2label", lambda a: z(5, dtype=I32)), ("tab_off", lambda a: z(2, dtype=I64)), ("seg", lambda a: z(127, dtype=I32)),
                ("spans", lambda a: edit(a["spans"], vert_off=a["spans"]["vert_off"].cpu()))]),
    case("prep_align", lambda: dict(spans=spans(), vertices=z(128, 6, dtype=F32), axis_align=z(2, 4, 4)),
         "mspa_prep_align",
         lambda a, r: [a["vertices"], a["spans"]["vert_off"], a["spans"]["word_off"], 2, 128, 2, a["axis_align"], r, S()],
         wrong=[("axis_align", lambda a: z(3, 4, 4)), ("vertices", lambda a: z(127, 6, dtype=F32))]),
    case("prep_objects",
         lambda: dict(spans=spans(), instance_ids=z(128, dtype=I32), vertices=z(128, 6, dtype=F32), aligned=z(128, 6), n_objects=[1, 1]),
         wrong=[("aligned", lambda a: z(127, 6)), ("n_objects", lambda a: [1])]),
]}


def variants(c, a):
    """(label, argument the error must name, the keyword arguments with exactly that one changed)."""
    for name, t in a.items():
        if not isinstance(t, torch.Tensor):
            continue
        yield "dtype", name, edit(a, **{name: t.to(I32 if t.dtype == F32 else F32)})
        if name not in c.batched:
            yield "rank", name, edit(a, **{name: t[None]})
        yield "host", name, edit(a, **{name: t.cpu()})
        if name not in c.strided_ok and not strided(t).is_contiguous():
            yield "strided", name, edit(a, **{name: strided(t)})
    for k, (name, replace) in enumerate(c.wrong):
        yield f"wrong[{k}]", name, edit(a, **{name: replace(a)})


@pytest.mark.parametrize("fn", list(CASES))
def test_one_wrong_argument_is_refused_before_the_library(lib, fn):
    c = CASES[fn]
    a = c.make()
    n = 0
    for label, name, bad in variants(c, a):
        with pytest.raises(ValueError, match="mspa.engine") as e:
            getattr(engine, fn)(**bad)
        assert re.match(rf"mspa\.engine: (requirement not met: )?{re.escape(name)}\b", str(e.value)), (fn, label, name, str(e.value))
        assert lib.calls == [], (fn, label, name)
        n += 1
    assert n >= 3


def as_arg(v):
    return v.data_ptr() if isinstance(v, torch.Tensor) else v


@pytest.mark.parametrize("fn", [c.fn for c in CASES.values() if c.launch])
def test_valid_call_reaches_the_library_once_in_declared_order(lib, fn):
    c = CASES[fn]
    a = c.make()
    r = getattr(engine, fn)(**a)
    assert [name for name, _ in lib.calls] == [c.launch]
    got, want, types = lib.calls[0][1], c.expect(a, r), _lib._SIGNATURES[c.launch][1]
    assert len(got) == len(want) == len(types)
    for k, (g, w, ty) in enumerate(zip(got, want, types)):
        if ty is ctypes.c_void_p:
            assert g is None or type(g) is int, (fn, k, g)
        elif ty is ctypes.c_double:
            assert type(g) is float, (fn, k, g)
        elif ty in (ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32):
            assert type(g) is int, (fn, k, g)
        assert w is ANY or g == as_arg(w), (fn, k, g, w)
    # an argument that is handed over with its strides (or copied) is taken as a view as well
    for name in c.strided_ok:
        del lib.calls[:]
        getattr(engine, fn)(**edit(a, **{name: strided(a[name])}))
        assert [name for name, _ in lib.calls] == [c.launch]


def test_default_outputs_are_the_allocators_tables(lib):
    """``out=None`` / no ``out`` at all goes through the same tables the checks read."""
    a = pair_args(corr_out)
    del a["out"]
    out = engine.pair_correspondences(**a)
    assert {k: (tuple(v.shape), v.dtype) for k, v in out.items()} == {k: (tuple(v.shape), v.dtype) for k, v in corr_out(2, HW).items()}
    assert len(lib.calls) == 1
    assert set(engine.alloc_pair_outputs(1, HW, engine.PAIR_OUTPUTS, DEV)) == set(engine.PAIR_OUTPUTS)
    with pytest.raises(ValueError, match="bogus"):
        engine.alloc_pair_outputs(1, HW, ("bogus",), DEV)


def test_select_common_point_takes_a_selection_view():
    bits = torch.tensor([[0b1011], [0b0110]], dtype=I64, device=DEV)
    wide = torch.tensor([[0, 1, 0, 7], [0, 0, 1, 7], [1, 1, 5, 7]], dtype=I32, device=DEV)
    view = wide[:, :3]
    assert not view.is_contiguous()
    got, want = engine.select_common_point(bits, view), engine.select_common_point(bits, view.contiguous())
    assert got.tolist() == want.tolist() == [1, 1, -1]


def test_project_samples_takes_a_sample_view():
    sc = synth.make_scene(1004, n_points=64, n_frames=2, color_hw=HW, depth_hw=HW, invalid_pose_frac=0, with_color=False)
    ids = sc.valid_image_ids
    depth = engine.depth_to_device(np.stack([sc.depth[i] for i in ids]), DEV)
    xyz = torch.from_numpy(np.ascontiguousarray(sc.points[:, :3])).to(DEV)
    cam = torch.from_numpy(engine.camera_matrices(sc.K, [sc.A @ sc.E[i] for i in ids])).to(DEV)
    wide = torch.full((128, 4), 7, dtype=I32, device=DEV)
    wide[:, 0] = torch.arange(128, device=DEV) % 64
    wide[:, 1] = torch.arange(128, device=DEV) // 64
    view = wide[:, :2]
    assert not view.is_contiguous()
    got = engine.project_samples(xyz, cam, depth, HW, view)
    want = engine.project_samples(xyz, cam, depth, HW, view.contiguous())
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), w.cpu().numpy(), equal_nan=True)
    assert want[2].any()                                  # the scene is seen: the comparison is not of two empty answers
