"""PyTorch-ROCm front end of the geometry kernels.

torch is plumbing here: it owns device memory and the stream; every computation is a call into
libmspa.so through ``data_ptr()``.  Host-side matrix preparation (``np.linalg.inv``, ``A @ E``)
uses the very NumPy routines the reference uses (IH:57, IH:113-124, OPS:313) so that what reaches
the kernels is bit-identical to what the reference would multiply with.
"""
from __future__ import annotations

import ctypes
import functools
import types
import os
from typing import Dict, Iterable, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

_AFFINE_ROW = np.array([0.0, 0.0, 0.0, 1.0])
_DEPTH = (torch.int16, torch.uint16)        # uint16 depth values, stored as int16 (torch has few uint16 ops)


def _require(condition: bool, what: str):
    """Argument checks in front of raw device pointers: a real exception, not an ``assert`` that ``python -O`` drops."""
    if not condition:
        raise ValueError(f"mspa.engine: requirement not met: {what}")


def _require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("mspa.engine needs a ROCm GPU (torch.cuda.is_available() is False); "
                           "there is no CPU fallback -- the CPU restatement under oracle/ is test-only")


def _check(name: str, t, dtypes, shape: tuple, contiguous: bool = True) -> torch.Tensor:
    """THE check of a tensor argument before it becomes a raw pointer: a device tensor of dtype ``dtypes`` (one, or a tuple of them)
    whose extents match ``shape`` entry by entry -- k: exactly k, None: any, (k,): at least k (slot buffers are larger than the call's
    n) -- and contiguous, unless the wrapper hands the strides over.  Reads metadata only: no synchronisation.  Returns ``t``."""
    if not isinstance(dtypes, tuple):
        dtypes = (dtypes,)
    if isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in dtypes and t.dim() == len(shape) and (t.is_contiguous() or not contiguous):
        if t.shape == shape:                                                # every entry exact and equal
            return t
        for got, e in zip(t.shape, shape):
            if not (e is None or got == e or (isinstance(e, tuple) and got >= e[0])):
                break
        else:                                                               # no entry objected
            return t
    _require_gpu()                      # on a machine without one, that is the answer whatever the tensor looks like
    extents = ", ".join("any" if e is None else f">= {e[0]}" if isinstance(e, tuple) else str(e) for e in shape)
    got = type(t).__name__
    if isinstance(t, torch.Tensor):
        got = f"{str(t.dtype)[6:]} {list(t.shape)} on {t.device}" + ("" if t.is_contiguous() or not contiguous else f", strides {tuple(t.stride())}")
    raise ValueError(f"mspa.engine: {name}: expected a {'contiguous ' if contiguous else ''}{' / '.join(str(d)[6:] for d in dtypes)} "
                     f"device tensor [{extents}], got {got}")


def _stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    """The raw pointer (None -> NULL) of a tensor that ``_check`` has passed, or that this module allocated itself."""
    return None if t is None else t.data_ptr()


def _workspace(nbytes: int, device) -> torch.Tensor:
    """Scratch of ``nbytes`` rounded up to 16, as uint8, on a 16-byte boundary (allocated as int64 pairs)."""
    return torch.empty(((nbytes + 15) // 16 * 2,), dtype=torch.int64, device=device).view(torch.uint8)


def _check_bits(name: str, bits) -> Tuple[int, int]:
    """A bitset table, int64 [rows, n_words] (K1's output and everything packed like it) -> (rows, n_words)."""
    return tuple(_check(name, bits, torch.int64, (None, None)).shape)


def _check_images(name: str, images) -> Tuple[int, int, int]:
    """An image batch, uint8 [n, H, W, 3] -> (n, H, W)."""
    return tuple(_check(name, images, torch.uint8, (None, None, None, 3)).shape[:3])


def _check_streams(offsets, nbytes) -> int:
    """The ``offsets`` / ``nbytes`` pair that cuts byte streams out of a flat ``src``: int64, one length -> that length."""
    n = _check("offsets", offsets, torch.int64, (None,)).shape[0]
    _check("nbytes", nbytes, torch.int64, (n,))
    return n


def _file_rows(n: int, pitch, out, nbytes, device):
    """The (out [>= n, pitch] uint8, nbytes [>= n] int64) pair the encoders write files into; allocated (``pitch()`` wide) when not given."""
    if out is None:
        out = torch.empty((n, pitch()), dtype=torch.uint8, device=device)
    if nbytes is None:
        nbytes = torch.empty((n,), dtype=torch.int64, device=device)
    return _check("out", out, torch.uint8, ((n,), None)), _check("nbytes", nbytes, torch.int64, ((n,),))


def _check_pair_inputs(depth, mats, pairs) -> Tuple[int, int, int, int]:
    """What both K3 wrappers read: depth [F, DH, DW], mats [F, FRAME_MATS, 16] float64, pairs [B, 2] int32 -> (F, DH, DW, B)."""
    F, DH, DW = _check("depth", depth, _DEPTH, (None, None, None)).shape
    _check("mats", mats, torch.float64, (F, _lib.FRAME_MATS, 16))
    return F, DH, DW, _check("pairs", pairs, torch.int32, (None, 2)).shape[0]


def _check_outputs(out: Dict[str, torch.Tensor], shapes: dict, required: tuple = ()) -> None:
    """A caller's ``out`` dict against the table its allocator allocates from (names the table lacks are not read)."""
    for name in required:
        if out.get(name) is None:
            raise ValueError(f"mspa.engine: out[{name!r}]: this output is not optional")
    for name, t in out.items():                     # once per launch: one comparison per tensor, and _check words a mismatch
        want = shapes.get(name)
        if want is not None and t is not None and ((t.shape, t.dtype) != want or not t.is_cuda or not t.is_contiguous()):
            _check(f"out[{name!r}]", t, want[1], want[0])


def _alloc_wanted(want: Iterable[str], shapes: dict, device) -> Dict[str, torch.Tensor]:
    """The outputs named in ``want``, allocated from ``shapes``; a name the table lacks is an error, not a tensor nothing writes."""
    want = tuple(want)
    unknown = [k for k in want if k not in shapes]
    _require(not unknown, f"want: no output named {unknown}; choose from {tuple(shapes)}")
    return {k: torch.empty(shape, dtype=dtype, device=device) for k, (shape, dtype) in shapes.items() if k in want}


def check_affine(name: str, m: np.ndarray):
    """The kernels take affine matrices with finite entries (include/mspa.h); the reference drops
    frames with non-finite poses before any projection (IH:409-418)."""
    m = np.asarray(m, dtype=np.float64)
    if m.shape != (4, 4) or not np.all(np.isfinite(m)):
        raise ValueError(f"{name}: expected a finite 4x4 matrix")
    if not np.array_equal(m[3], _AFFINE_ROW):
        raise ValueError(f"{name}: last row must be exactly [0, 0, 0, 1], got {m[3]}")
    return m


def _check_affine_stack(name: str, m: np.ndarray) -> np.ndarray:
    m = np.asarray(m, dtype=np.float64)
    if m.ndim != 3 or m.shape[1:] != (4, 4) or not np.all(np.isfinite(m)):
        raise ValueError(f"{name}: expected finite 4x4 matrices")
    if not np.array_equal(m[:, 3, :], np.broadcast_to(_AFFINE_ROW, (m.shape[0], 4))):
        bad = int(np.nonzero(~(m[:, 3, :] == _AFFINE_ROW).all(axis=1))[0][0])
        raise ValueError(f"{name}[{bad}]: last row must be exactly [0, 0, 0, 1], got {m[bad, 3]}")
    return m


def frame_matrices(K: np.ndarray, A: Optional[np.ndarray], E_list: Sequence[np.ndarray]) -> np.ndarray:
    """[F, 8, 16] float64 frame records for mspa_pair_reproject (slot order of include/mspa.h).  All frames in one batched
    ``A @ E`` / ``np.linalg.inv`` call: NumPy runs the same per-matrix dgemm / dgesv as for a single 4x4, so every entry is
    bit-identical to the reference's one-frame-at-a-time expressions (tests/test_host_cpu.py pins that)."""
    K = check_affine("K", K)
    A = np.eye(4) if A is None else check_affine("A", A)
    Kinv = check_affine("inv(K)", np.linalg.inv(K))                       # OPS:313
    F = len(E_list)
    out = np.empty((F, _lib.FRAME_MATS, 16), dtype=np.float64)
    if F == 0:
        return out
    E = _check_affine_stack("E", np.stack([np.asarray(e, dtype=np.float64) for e in E_list]))
    AE = A @ E                                                             # IH:113-124
    Einv_al = _check_affine_stack("inv(A@E)", np.linalg.inv(AE))          # IH:57
    out[:, _lib.MAT_KINV] = Kinv.reshape(16)
    out[:, _lib.MAT_E] = E.reshape(F, 16)
    out[:, _lib.MAT_A] = A.reshape(16)
    out[:, _lib.MAT_EINV_ALIGNED] = Einv_al.reshape(F, 16)
    out[:, _lib.MAT_K] = K.reshape(16)
    # composed products for MSPA_PAIR_FAST (any float64 evaluation order will do: lanes near a
    # decision boundary are re-evaluated with the exact chain inside the kernel)
    out[:, _lib.MAT_UNPROJ] = (AE @ Kinv).reshape(F, 16)
    out[:, _lib.MAT_REPROJ] = (K @ Einv_al).reshape(F, 16)
    out[:, _lib.MAT_BOUNDS] = frame_bounds(Kinv, E, A, Einv_al, K)
    return out


def frame_bounds(Kinv: np.ndarray, E: np.ndarray, A: np.ndarray, Einv_al: np.ndarray, K: np.ndarray) -> np.ndarray:
    """[F, 16] float64: slot MSPA_MAT_BOUNDS of the frame records -- the coefficients from which the fast kernels derive
    their guard band as a BOUND (include/mspa.h; DESIGN.md section 4, "guard").  With |.| entrywise:
      Uabs = |A| |E| |inv(K)|        (frame as frame 1: pixel * depth -> aligned world)
      Nabs = |K| |inv(A E)|          (frame as frame 2: aligned world -> homogeneous image coordinates)
    Every float64 evaluation order of K2 inv(A E2) A E1 inv(K1) p -- the reference's five products, the composed 3x4 of the
    fast kernels -- stays within GUARD_C * 2^-53 * (Nabs Uabs |p|) of the exact value; the kernels evaluate an upper
    estimate of that product of magnitudes per tile from these ten numbers.  Same values as mspa_frame_bounds_host up to
    the summation order of the magnitudes (tests/test_host_cpu.py)."""
    F = E.shape[0]
    Ua = (np.abs(A) @ np.abs(E)) @ np.abs(Kinv)                           # [F, 4, 4]
    Na = np.abs(K) @ np.abs(Einv_al)
    c = _lib.GUARD_C * 2.0 ** -53
    b = np.zeros((F, 16), dtype=np.float64)
    b[:, 0:4] = Ua[:, :3, :].max(axis=1)
    b[:, 3] *= 1000.0
    b[:, 4:7] = c * ((Na[:, :3, 0] + Na[:, :3, 1]) + Na[:, :3, 2])
    b[:, 8:11] = c * 1000.0 * Na[:, :3, 3]
    return b


def fast_path_ok(K: np.ndarray) -> bool:
    """MSPA_PAIR_FAST reads the camera-2 depth off the third image row: K[2] must be 0 0 1 0."""
    return bool(np.array_equal(np.asarray(K, dtype=np.float64)[2], np.array([0.0, 0.0, 1.0, 0.0])))


def camera_matrices(K: np.ndarray, E_aligned_list: Sequence[np.ndarray]) -> np.ndarray:
    """[n, 3, 16] float64 records for mspa_vertex_visibility: inv(E_aligned), K (one batched inverse, see frame_matrices) and
    the guard-bound coefficients of the composed kernels (slot MSPA_CAM_BOUNDS of include/mspa.h: magnitudes of
    |K| |inv(E_aligned)|; the same numbers mspa_camera_bounds_host computes)."""
    K = check_affine("K", K)
    n = len(E_aligned_list)
    out = np.zeros((n, _lib.CAM_MATS, 16), dtype=np.float64)
    if n == 0:
        return out
    E = _check_affine_stack("E_aligned", np.stack([np.asarray(e, dtype=np.float64) for e in E_aligned_list]))
    Einv = _check_affine_stack("inv(E_aligned)", np.linalg.inv(E))                         # IH:57
    out[:, _lib.CAM_EINV] = Einv.reshape(n, 16)
    out[:, _lib.CAM_K] = K.reshape(16)
    Na = np.abs(K) @ np.abs(Einv)
    c = _lib.GUARD_C * 2.0 ** -53 * 1000.0
    nr = (Na[:, :3, 0] + Na[:, :3, 1]) + Na[:, :3, 2]
    out[:, _lib.CAM_BOUNDS, 0] = c * (nr[:, 0] + nr[:, 1])
    out[:, _lib.CAM_BOUNDS, 1] = c * nr[:, 2]
    out[:, _lib.CAM_BOUNDS, 2] = c * (Na[:, 0, 3] + Na[:, 1, 3])
    out[:, _lib.CAM_BOUNDS, 3] = c * Na[:, 2, 3]
    return out


def depth_to_device(depth: np.ndarray, device="cuda") -> torch.Tensor:
    """uint16 depth frames -> device int16 tensor holding the same bits (torch has few uint16 ops)."""
    d = np.ascontiguousarray(depth, dtype=np.uint16)
    return torch.from_numpy(d.view(np.int16)).to(device)


def gather_blocks_host(blocks, dst: np.ndarray, n_threads: int = 4) -> None:
    """``dst[k] = blocks[k]`` for equally shaped, C-contiguous host arrays of ``dst``'s dtype, copied by ``n_threads``
    native threads (mspa_gather_blocks_host): the staging of a scene's depth frames into pinned memory."""
    n = len(blocks)
    if n == 0:
        return
    if dst.shape[0] < n or not dst.flags.c_contiguous:
        raise ValueError("gather_blocks_host: destination too small or not contiguous")
    block_bytes = int(dst[0].nbytes)
    ptrs = (ctypes.c_void_p * n)()
    for k, b in enumerate(blocks):
        if b.nbytes != block_bytes or b.dtype.itemsize != dst.dtype.itemsize or not b.flags.c_contiguous:
            raise ValueError("gather_blocks_host: block %d is not a contiguous array of the destination's frame size" % k)
        ptrs[k] = b.ctypes.data
    _lib.check(_lib.load().mspa_gather_blocks_host(ptrs, n, block_bytes, dst.ctypes.data, int(n_threads)))


def inflate_blocks_device(src: torch.Tensor, offsets: torch.Tensor, nbytes: torch.Tensor, block_bytes: int,
                          out: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None):
    """``len(offsets)`` zlib streams resident on the device -- stream k = ``src[offsets[k] : offsets[k] + nbytes[k]]`` (uint8;
    offsets multiples of 8) -- inflated by one wave each into ``out[k, :block_bytes]`` (mspa_inflate_blocks_device; replaces
    the per-frame zlib.decompress / cv2.imread of the reference, extract_posed_images.py:49-57, info_handler.py:149-155).
    Returns (out [n, pitch] uint8, status [n] int32): status 0 = inflated to exactly ``block_bytes`` with a matching
    Adler-32; anything else = decode that block on the host.  An ``out`` allocated here has the pitch ``block_bytes`` rounded up
    to 256 and zeros behind ``block_bytes``; a caller's ``out`` keeps what it held there.  Only enqueues; read ``status`` after a
    synchronisation."""
    _check("src", src, torch.uint8, (None,))
    n = _check_streams(offsets, nbytes)
    if out is None:
        out = torch.empty((n, (int(block_bytes) + 255) // 256 * 256), dtype=torch.uint8, device=src.device)
        if n and 0 < int(block_bytes) < out.shape[1]:
            out[:, int(block_bytes):].zero_()             # the kernels write a row's first block_bytes: at most 255 bytes of padding a row
    _check("out", out, torch.uint8, ((n,), (block_bytes,)))
    _require(out.shape[1] % 256 == 0, f"out: a pitch that is a multiple of 256, got {out.shape[1]}")
    status = torch.empty((n,), dtype=torch.int32, device=src.device) if status is None else _check("status", status, torch.int32, ((n,),))
    work = torch.empty((max(n, 1),), dtype=torch.int32, device=src.device)
    _lib.check(_lib.load().mspa_inflate_blocks_device(_ptr(src), _ptr(offsets), _ptr(nbytes), int(src.numel()), n, int(block_bytes),
                                                      _ptr(out), int(out.shape[1]), _ptr(status), _ptr(work), _stream_ptr()))
    return out, status


def png_unfilter_device(raw: torch.Tensor, h: int, w: int, status: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``raw[k, : h * (2 w + 1)]`` -- the inflated scanlines of n 16-bit greyscale PNG images -- to ``out[k, h, w]`` (int16
    storage of the uint16 depth values, like every depth tensor here): the five PNG row filters undone on the device
    (mspa_png_unfilter_device).  Images with ``status[k] != 0`` are skipped; a filter byte > 4 sets status 3.  ``raw`` starts
    4-byte aligned and its pitch is a multiple of 4 (MspaError otherwise, as from the C ABI)."""
    n = _check("raw", raw, torch.uint8, (None, (h * (2 * w + 1),))).shape[0]
    if _ptr(raw) % 4 or int(raw.shape[1]) % 4:
        raise _lib.MspaError(_lib.MSPA_EINVAL, "png_unfilter_device: raw must start 4-byte aligned, with a pitch that is a multiple of 4")
    _check("status", status, torch.int32, ((n,),))
    out = torch.empty((n, h, w), dtype=torch.int16, device=raw.device) if out is None else _check("out", out, torch.int16, ((n,), h, w))
    _lib.check(_lib.load().mspa_png_unfilter_device(_ptr(raw), int(raw.shape[1]), n, int(h), int(w), _ptr(out), _ptr(status),
                                                    _stream_ptr()))
    return out


def png_unfilter8_device(raw: torch.Tensor, h: int, w: int, status: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``raw[k, : h * (w + 1)]`` -- the inflated scanlines of n 8-bit greyscale PNG images (instance masks) -- to ``out[k, h, w]``
    uint8: the five PNG row filters undone on the device with bytes-per-pixel 1 (mspa_png_unfilter8_device).  Images with
    ``status[k] != 0`` are skipped; a filter byte > 4 sets status 3.  ``raw`` starts 4-byte aligned and its pitch is a multiple of
    4 (MspaError otherwise, as from the C ABI)."""
    n = _check("raw", raw, torch.uint8, (None, (h * (w + 1),))).shape[0]
    if _ptr(raw) % 4 or int(raw.shape[1]) % 4:
        raise _lib.MspaError(_lib.MSPA_EINVAL, "png_unfilter8_device: raw must start 4-byte aligned, with a pitch that is a multiple of 4")
    _check("status", status, torch.int32, ((n,),))
    out = torch.empty((n, h, w), dtype=torch.uint8, device=raw.device) if out is None else _check("out", out, torch.uint8, ((n,), h, w))
    _lib.check(_lib.load().mspa_png_unfilter8_device(_ptr(raw), int(raw.shape[1]), n, int(h), int(w), _ptr(out), _ptr(status),
                                                     _stream_ptr()))
    return out


SPLIT_LABELS = 256


def instance_split(labels: torch.Tensor, valid: torch.Tensor, xyz: torch.Tensor, rgb: Optional[torch.Tensor] = None):
    """The stable split of F frames' valid pixels by instance label (mspa_instance_split_count / _scatter): ``labels`` [F, H, W]
    uint8 (0 = nothing), ``valid`` [F, P] uint8 and ``xyz`` [F, P, 3] float64 as K3 exact wrote them (P = H * W), ``rgb`` optionally
    [F, H, W, 3] uint8.  Returns (counts [F, 256] int32, offsets [F * 256 + 1] int64, xyz [total, 3] float64, rgb [total, 3] uint8 or
    None, pixel [total] int32, lo [F, 256, 3], hi [F, 256, 3] float64): segment (f, v) is rows ``offsets[f * 256 + v] :
    offsets[f * 256 + v + 1]``, the selected pixels of frame f with label v in ascending pixel index; lo / hi are its extents
    (+inf / -inf where it is empty).  ``counts`` and ``offsets`` come back on the HOST (NumPy): reading the counts is the call's
    one synchronisation, and every accessor indexes with them."""
    F, H, W = _check("labels", labels, torch.uint8, (None, None, None)).shape
    P = H * W
    _check("valid", valid, torch.uint8, (F, P))
    _check("xyz", xyz, torch.float64, (F, P, 3))
    if rgb is not None:
        _check("rgb", rgb, torch.uint8, (F, H, W, 3))
    _require(F <= 65535 and P < 2 ** 31, f"at most 65535 frames of fewer than 2^31 pixels per launch, got {F} x {P}")
    lib, dev = _lib.load(), labels.device
    counts_d = torch.empty((F, SPLIT_LABELS), dtype=torch.int32, device=dev)
    nbytes = int(lib.mspa_instance_split_workspace_bytes(F, P))
    work = _workspace(nbytes, dev)
    _lib.check(lib.mspa_instance_split_count(_ptr(labels), _ptr(valid), F, P, _ptr(counts_d), _ptr(work), nbytes, _stream_ptr()))
    counts = counts_d.cpu().numpy()                                         # the one synchronisation
    offsets = np.zeros(F * SPLIT_LABELS + 1, dtype=np.int64)
    np.cumsum(counts.reshape(-1), out=offsets[1:])
    total = int(offsets[-1])
    out_xyz = torch.empty((max(total, 1), 3), dtype=torch.float64, device=dev)   # (never a null pointer: an empty tensor has none)
    out_rgb = torch.empty((max(total, 1), 3), dtype=torch.uint8, device=dev) if rgb is not None else None
    out_pixel = torch.empty((max(total, 1),), dtype=torch.int32, device=dev)
    lo = torch.empty((F, SPLIT_LABELS, 3), dtype=torch.float64, device=dev)
    hi = torch.empty((F, SPLIT_LABELS, 3), dtype=torch.float64, device=dev)
    offsets_d = torch.from_numpy(offsets).to(dev)
    if F:
        _lib.check(lib.mspa_instance_split_scatter(_ptr(labels), _ptr(valid), _ptr(xyz), _ptr(rgb), F, P, H, W, _ptr(offsets_d), _ptr(work),
                                                   _ptr(out_xyz), _ptr(out_rgb), _ptr(out_pixel), _ptr(lo), _ptr(hi), _stream_ptr()))
    return counts, offsets, out_xyz[:total], None if out_rgb is None else out_rgb[:total], out_pixel[:total], lo, hi


def instance_split_host(labels: np.ndarray, valid: np.ndarray, xyz: np.ndarray, rgb: Optional[np.ndarray] = None, reversed_order: bool = False):
    """``instance_split`` on the CPU through the same header (mspa_instance_split_host): NumPy in, NumPy out, no GPU.  For the
    tests: ``reversed_order`` walks tiles and waves in the opposite order, which must not change a byte."""
    labels = np.ascontiguousarray(labels, dtype=np.uint8)
    F = labels.shape[0]
    P = int(np.prod(labels.shape[1:]))
    valid = np.ascontiguousarray(valid, dtype=np.uint8).reshape(F, P)
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(F, P, 3)
    rgb = None if rgb is None else np.ascontiguousarray(rgb, dtype=np.uint8).reshape(F, P, 3)
    lib = _lib.load()
    counts = np.zeros((F, SPLIT_LABELS), dtype=np.int32)
    offsets = np.zeros(F * SPLIT_LABELS + 1, dtype=np.int64)
    work = np.zeros(max(int(lib.mspa_instance_split_workspace_bytes(F, P)) // 4, 4), dtype=np.int32)
    head = (labels.ctypes.data, valid.ctypes.data, xyz.ctypes.data, None if rgb is None else rgb.ctypes.data, F, P, counts.ctypes.data,
            offsets.ctypes.data, work.ctypes.data)
    _lib.check(lib.mspa_instance_split_host(*head, None, None, None, None, None, 0))
    total = int(offsets[-1])
    out_xyz = np.zeros((max(total, 1), 3), dtype=np.float64)
    out_rgb = None if rgb is None else np.zeros((max(total, 1), 3), dtype=np.uint8)
    out_pixel = np.zeros(max(total, 1), dtype=np.int32)
    lo, hi = np.zeros((F, SPLIT_LABELS, 3)), np.zeros((F, SPLIT_LABELS, 3))
    _lib.check(lib.mspa_instance_split_host(*head, out_xyz.ctypes.data, None if out_rgb is None else out_rgb.ctypes.data,
                                            out_pixel.ctypes.data, lo.ctypes.data, hi.ctypes.data, int(bool(reversed_order))))
    return counts, offsets, out_xyz[:total], None if out_rgb is None else out_rgb[:total], out_pixel[:total], lo, hi


JPEG_STATUS ={0: "decoded", 1: "not a JPEG / malformed header", 2: "outside the accepted subset", 3: "another size",
               4: "bad entropy-coded data", 5: "restart marker missing or out of sequence", 6: "no EOI after the last MCU",
               7: "block out of range"}


def jpeg_parse_host(payloads: Sequence) -> Tuple[np.ndarray, np.ndarray]:
    """Headers of n JPEG payloads (bytes-like or uint8 arrays) -> (descriptors [n, MSPA_JPEG_DESC_BYTES] uint8, status [n]
    int32) through mspa_jpeg_parse_host: status 0 = the device decodes this image, anything else = decode it on the host."""
    n = len(payloads)
    keep = [np.frombuffer(p, dtype=np.uint8) if not isinstance(p, np.ndarray) else np.ascontiguousarray(p, dtype=np.uint8)
            for p in payloads]
    desc = np.zeros((n, _lib.JPEG_DESC_BYTES), dtype=np.uint8)
    status = np.zeros((n,), dtype=np.int32)
    if n:
        ptrs = (ctypes.c_void_p * n)(*[a.ctypes.data if a.size else None for a in keep])
        lens = np.array([a.size for a in keep], dtype=np.int64)
        _lib.check(_lib.load().mspa_jpeg_parse_host(ptrs, lens.ctypes.data, n, desc.ctypes.data, status.ctypes.data))
    return desc, status


def jpeg_desc_fields(desc: np.ndarray) -> Dict[str, np.ndarray]:
    """The documented fields of parsed descriptors (include/mspa.h): per image h, w, components, restart interval, sampling
    factors, quantisation tables (natural order) and the entropy-coded segment's offset / length in the payload."""
    d = np.ascontiguousarray(np.asarray(desc, dtype=np.uint8).reshape(-1, _lib.JPEG_DESC_BYTES))
    i32 = d[:, :192].view(np.int32)
    i64 = d[:, 48:64].view(np.int64)
    return {"status": i32[:, 0].copy(), "h": i32[:, 1].copy(), "w": i32[:, 2].copy(), "ncomp": i32[:, 3].copy(),
            "restart_interval": i32[:, 4].copy(), "mcus_x": i32[:, 7].copy(), "mcus_y": i32[:, 8].copy(),
            "samp_h": i32[:, 16:19].copy(), "samp_v": i32[:, 19:22].copy(), "tq": i32[:, 22:25].copy(),
            "scan_offset": i64[:, 0].copy(), "scan_bytes": i64[:, 1].copy(),
            "qt": d[:, 192:576].view(np.uint16).reshape(-1, 3, 64).copy()}


def _jpeg_decode(entry: str, tail: tuple, src, offsets, nbytes, descriptors, hw, out, status):
    """The two device decodes' shared front: checks, allocation of ``out`` ([n, H, W, *tail]) and ``status``, workspace, the call."""
    H, W = int(hw[0]), int(hw[1])
    _require(H > 0 and W > 0, f"hw: a positive (H, W), got {(H, W)}")
    _check("src", src, torch.uint8, (None,))
    _require(src.numel() % 4 == 0, f"src: a multiple of 4 bytes long, got {src.numel()}")
    n = _check_streams(offsets, nbytes)
    _check("descriptors", descriptors, torch.uint8, (n, _lib.JPEG_DESC_BYTES))
    out = torch.empty((n, H, W) + tail, dtype=torch.uint8, device=src.device) if out is None else _check("out", out, torch.uint8, ((n,), H, W) + tail)
    status = torch.empty((n,), dtype=torch.int32, device=src.device) if status is None else _check("status", status, torch.int32, ((n,),))
    if n == 0:
        return out, status
    lib = _lib.load()
    work = _workspace(int(lib.mspa_jpeg_workspace_bytes(n, H, W)), src.device)
    _lib.check(getattr(lib, entry)(_ptr(src), _ptr(offsets), _ptr(nbytes), int(src.numel()), _ptr(descriptors), n, H, W,
                                   _ptr(out), _ptr(status), _ptr(work), int(work.numel()), _stream_ptr()))
    return out, status


def jpeg_decode_device(src: torch.Tensor, offsets: torch.Tensor, nbytes: torch.Tensor, descriptors: torch.Tensor, hw: Tuple[int, int],
                       out: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None):
    """``len(offsets)`` JPEG payloads resident on the device -- payload k = ``src[offsets[k] : offsets[k] + nbytes[k]]`` (uint8,
    ``src`` a multiple of 4 bytes long) -- with their descriptors (``jpeg_parse_host``, uploaded: [n, MSPA_JPEG_DESC_BYTES]
    uint8) decoded into ``out[k]`` = [H, W, 3] uint8 RGB (mspa_jpeg_decode_device; replaces the per-frame cv2.imread /
    Pillow decode of the colour frames).  Returns (out, status): status 0 = bit-identical to libjpeg-turbo's decode;
    anything else = decode that frame on the host.  Only enqueues; read ``status`` after a synchronisation."""
    return _jpeg_decode("mspa_jpeg_decode_device", (3,), src, offsets, nbytes, descriptors, hw, out, status)


def jpeg_decode_luma_device(src: torch.Tensor, offsets: torch.Tensor, nbytes: torch.Tensor, descriptors: torch.Tensor, hw: Tuple[int, int],
                            out: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None):
    """``jpeg_decode_device`` for the grey image alone: ``out[k]`` = [H, W] uint8, component 0 after the IDCT
    (mspa_jpeg_decode_luma_device) -- what ``cv2.imread(path, IMREAD_GRAYSCALE)`` and Pillow's ``draft("L")`` return for a
    baseline JPEG.  Same arguments, same (out, status) contract; only enqueues."""
    return _jpeg_decode("mspa_jpeg_decode_luma_device", (), src, offsets, nbytes, descriptors, hw, out, status)


def laplacian_moments(luma: torch.Tensor) -> torch.Tensor:
    """[n, H, W] uint8 grey images -> [n, B, 2] int64: per image and block of rows (B = mspa_laplacian_blocks) the sum and the
    sum of squares of the 4-neighbour Laplacian with reflect-101 borders (mspa_laplacian_moments_device): exact integers,
    deterministic.  ``laplacian_variance`` turns them into ``cv2.Laplacian(img, cv2.CV_64F).var()``.  Only enqueues."""
    n, H, W = _check("luma", luma, torch.uint8, (None, None, None)).shape
    _require(H > 0 and W > 0 and n <= 65535, f"luma: at most 65 535 non-empty images, got {list(luma.shape)}")
    lib = _lib.load()
    partials = torch.empty((n, int(lib.mspa_laplacian_blocks(H, W)), 2), dtype=torch.int64, device=luma.device)
    if n:
        _lib.check(lib.mspa_laplacian_moments_device(_ptr(luma), n, H, W, _ptr(partials), _stream_ptr()))
    return partials


def laplacian_variance(partials, n_pixels: int) -> np.ndarray:
    """``laplacian_moments``' output (device tensor or array) for images of ``n_pixels`` pixels -> [n] float64: the exact
    population variance (N S2 - S1^2) / N^2 from Python integers, rounded once."""
    p = partials.cpu().numpy() if isinstance(partials, torch.Tensor) else np.asarray(partials)
    N = int(n_pixels)
    out = np.empty((p.shape[0],), dtype=np.float64)
    for i, blocks in enumerate(p.tolist()):
        s1, s2 = sum(b[0] for b in blocks), sum(b[1] for b in blocks)
        out[i] = (N * s2 - s1 * s1) / (N * N)
    return out


def _knn_check(xyz_shape, k: int) -> int:
    k = int(k)
    _require(1 <= k <= _lib.KNN_MAX_K, f"k: between 1 and {_lib.KNN_MAX_K}, got {k}")
    _require(xyz_shape[0] <= 1 << 30, f"xyz: at most 2^30 points, got {xyz_shape[0]}")
    return k


def knn_mean_distance(xyz: torch.Tensor, k: int, want_evals: bool = False):
    """[N, 3] float64 finite points -> [N] float64: the mean Euclidean distance from each point to its min(k, N) nearest points,
    itself included at distance 0, summed in ascending order (what Open3D's ``SearchKNN`` on the cloud's own tree returns);
    exact search over a uniform grid (csrc/knn_grid_core.h, mspa_knn_mean_distance_device).  With ``want_evals`` also [N]
    int32, the distances each point evaluated.  The grid's box is the per-axis order statistics of rank N // 100 and
    N - 1 - N // 100, read back from a device sort: synchronises once."""
    N = _check("xyz", xyz, torch.float64, (None, 3)).shape[0]
    k = _knn_check(xyz.shape, k)
    mean = torch.empty((N,), dtype=torch.float64, device=xyz.device)
    evals = torch.empty((N,), dtype=torch.int32, device=xyz.device) if want_evals else None
    if N:
        lib = _lib.load()
        r = N // 100
        box = torch.sort(xyz, dim=0).values[[r, N - 1 - r]].cpu().numpy()
        _require(bool(np.isfinite(box).all()), "xyz: finite coordinates")
        box = np.ascontiguousarray(box, dtype=np.float64)
        grid = np.zeros((_lib.KNN_GRID_BYTES,), dtype=np.uint8)
        _lib.check(lib.mspa_knn_grid_host(box[0].ctypes.data, box[1].ctypes.data, N, k, grid.ctypes.data))
        cells = torch.empty((N,), dtype=torch.int32, device=xyz.device)
        _lib.check(lib.mspa_knn_cells_device(_ptr(xyz), N, grid.ctypes.data, _ptr(cells), _stream_ptr()))
        order = torch.sort(cells, stable=True).indices
        work = _workspace(int(lib.mspa_knn_workspace_bytes(N, k)), xyz.device)
        _lib.check(lib.mspa_knn_mean_distance_device(_ptr(xyz), N, k, grid.ctypes.data, _ptr(order), _ptr(mean), _ptr(evals),
                                                     _ptr(work), int(work.numel()), _stream_ptr()))
    return (mean, evals) if want_evals else mean


def knn_mean_distance_host(xyz, k: int, want_evals: bool = False):
    """``knn_mean_distance`` on the CPU for a NumPy [N, 3] cloud: the same grid walk through the same header
    (mspa_knn_mean_distance_host).  The device's twin for tests on a machine without a GPU, not a fallback."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float64)
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError(f"mspa.engine: xyz: expected [N, 3], got {list(xyz.shape)}")
    k = _knn_check(xyz.shape, k)
    mean = np.empty((xyz.shape[0],), dtype=np.float64)
    evals = np.empty((xyz.shape[0],), dtype=np.int32) if want_evals else None
    _lib.check(_lib.load().mspa_knn_mean_distance_host(xyz.ctypes.data, xyz.shape[0], k, mean.ctypes.data,
                                                       evals.ctypes.data if want_evals else None))
    return (mean, evals) if want_evals else mean


JPEG_SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}


def _subsampling(subsampling) -> int:
    if isinstance(subsampling, str):
        _require(subsampling in JPEG_SUBSAMPLING, f"subsampling: one of {sorted(JPEG_SUBSAMPLING)}")
        return JPEG_SUBSAMPLING[subsampling]
    _require(int(subsampling) in (0, 1, 2), "subsampling: 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0)")
    return int(subsampling)


def jpeg_encode_capacity(hw: Tuple[int, int], subsampling="4:2:0") -> int:
    """Worst-case bytes of one baseline JPEG file of ``hw`` (mspa_jpeg_encode_capacity)."""
    n = int(_lib.load().mspa_jpeg_encode_capacity(int(hw[0]), int(hw[1]), _subsampling(subsampling)))
    _require(n > 0, "hw: 1 <= H, W <= 65535")
    return n


def jpeg_encode_header_host(hw: Tuple[int, int], quality: int = 95, subsampling="4:2:0") -> bytes:
    """The bytes up to the end of SOS of the file ``jpeg_encode_device`` (and Pillow) writes for this shape, quality and
    subsampling (mspa_jpeg_encode_header_host)."""
    buf = np.zeros((1024,), dtype=np.uint8)
    n = ctypes.c_int64(0)
    _lib.check(_lib.load().mspa_jpeg_encode_header_host(int(hw[0]), int(hw[1]), int(quality), _subsampling(subsampling),
                                                         buf.ctypes.data, buf.size, ctypes.byref(n)))
    return buf[:n.value].tobytes()


def jpeg_encode_device(rgb: torch.Tensor, quality: int = 95, subsampling="4:2:0", out: Optional[torch.Tensor] = None,
                       nbytes: Optional[torch.Tensor] = None):
    """[n, H, W, 3] uint8 RGB on the device -> (out [n, pitch] uint8, nbytes [n] int64): row k holds image k's whole baseline
    JPEG file, byte for byte what Pillow's ``Image.fromarray(rgb[k]).save(f, "JPEG", quality=quality,
    subsampling=subsampling)`` writes (mspa_jpeg_encode_device).  The default ``out`` has the worst-case pitch
    (``jpeg_encode_capacity``); with a narrower one, a file longer than the pitch is cut off there and its ``nbytes`` says how
    long it is.  Only enqueues; read ``nbytes`` after a synchronisation."""
    n, H, W = _check_images("rgb", rgb)
    _require(1 <= H <= 65535 and 1 <= W <= 65535, f"rgb: 1 <= H, W <= 65535, got {(H, W)}")
    _require(isinstance(quality, (int, np.integer)) and 1 <= int(quality) <= 100, f"quality: an integer in 1..100, got {quality!r}")
    _require(n <= 65535, f"rgb: at most 65 535 images in one call, got {n}")
    ss = _subsampling(subsampling)
    out, nbytes = _file_rows(n, lambda: jpeg_encode_capacity((H, W), ss), out, nbytes, rgb.device)
    if n == 0:
        return out, nbytes
    lib = _lib.load()
    work = _workspace(int(lib.mspa_jpeg_encode_workspace_bytes(n, H, W, ss)), rgb.device)
    _lib.check(lib.mspa_jpeg_encode_device(_ptr(rgb), n, H, W, int(quality), ss, _ptr(out), int(out.shape[1]),
                                           _ptr(nbytes), _ptr(work), int(work.numel()), _stream_ptr()))
    return out, nbytes


def png_encode_capacity(hw: Tuple[int, int]) -> int:
    """Worst-case bytes of one 16-bit greyscale PNG file of ``hw`` (mspa_png_encode_capacity)."""
    n = int(_lib.load().mspa_png_encode_capacity(int(hw[0]), int(hw[1])))
    _require(n > 0, "hw: 1 <= H, W <= 8192")
    return n


def png_encode_device(depth: torch.Tensor, out: Optional[torch.Tensor] = None, nbytes: Optional[torch.Tensor] = None):
    """[n, H, W] depth on the device (uint16 values stored as int16, as ``depth_device``; uint16 is accepted too) ->
    (files [n, pitch] uint8, nbytes [n] int64): row k holds frame k's whole 16-bit greyscale PNG file, whose pixels equal
    the input and whose filtered scanlines are Pillow's (mspa_png_encode_device).  The default ``out`` has the pitch
    ``png_encode_capacity`` rounded up to 4.  Runs on the current torch stream and only enqueues; read ``nbytes`` after a
    synchronisation."""
    n, H, W = _check("depth", depth, _DEPTH, (None, None, None)).shape
    _require(1 <= H <= 8192 and 1 <= W <= 8192, f"depth: 1 <= H, W <= 8192, got {(H, W)}")
    _require(n <= 65535, f"depth: at most 65 535 frames in one call, got {n}")
    out, nbytes = _file_rows(n, lambda: (png_encode_capacity((H, W)) + 3) // 4 * 4, out, nbytes, depth.device)
    if n == 0:
        return out, nbytes
    lib = _lib.load()
    work = _workspace(int(lib.mspa_png_encode_workspace_bytes(n, H, W)), depth.device)
    _lib.check(lib.mspa_png_encode_device(_ptr(depth), n, H, W, _ptr(out), int(out.shape[1]), _ptr(nbytes), _ptr(work),
                                          int(work.numel()), _stream_ptr()))
    return out, nbytes


def draw_spans_device(images: torch.Tensor, spans: torch.Tensor) -> None:
    """Paint int32 span records [S, 5] = (image, y, x0, x1, 0xRRGGBB) into ``images`` ([n, H, W, 3] uint8, in place;
    mspa_draw_spans_device).  Records grouped by (image, y), call order kept inside a group (``annotate.pack_spans``)."""
    n, H, W = _check_images("images", images)
    _check("spans", spans, torch.int32, (None, 5))
    _lib.check(_lib.load().mspa_draw_spans_device(_ptr(spans), int(spans.shape[0]), _ptr(images), n, H, W, _stream_ptr()))


def blend_masks_device(images: torch.Tensor, labels: torch.Tensor, masks: torch.Tensor) -> None:
    """Blend 8-bit label masks into ``images`` ([n, H, W, 3] uint8, in place) with Pillow's arithmetic
    (mspa_blend_masks_device): int64 records [L, 8] = (image, x, y, mask w, mask h, 0xRRGGBB, offset into ``masks``, 0), grouped
    by image with call order kept inside a group (``annotate.DeviceAnnotator`` packs them)."""
    n, H, W = _check_images("images", images)
    _check("labels", labels, torch.int64, (None, 8))
    _check("masks", masks, torch.uint8, (None,))
    _lib.check(_lib.load().mspa_blend_masks_device(_ptr(labels), int(labels.shape[0]), _ptr(masks), int(masks.numel()), _ptr(images),
                                                   n, H, W, _stream_ptr()))


RESIZE_FILTERS = {"bilinear": _lib.RESIZE_BILINEAR, "bicubic": _lib.RESIZE_BICUBIC}
_RESIZE_TABLES: Dict[tuple, tuple] = {}


def _resize_filter(resample) -> int:
    if isinstance(resample, str):
        _require(resample.lower() in RESIZE_FILTERS, f"resample: one of {sorted(RESIZE_FILTERS)}")
        return RESIZE_FILTERS[resample.lower()]
    _require(int(resample) in RESIZE_FILTERS.values(), "resample: 2 (bilinear) or 3 (bicubic), Pillow's numbers")
    return int(resample)


def resize_coeffs_host(n_in: int, n_out: int, resample="bicubic") -> Tuple[np.ndarray, np.ndarray]:
    """(bounds [n_out, 2] int32, coeffs [n_out, ksize] int32): Pillow's fixed-point resampling table of one axis
    (mspa_resize_coeffs_host)."""
    lib = _lib.load()
    f = _resize_filter(resample)
    ksize = ctypes.c_int32(0)
    _lib.check(lib.mspa_resize_coeffs_host(int(n_in), int(n_out), f, None, None, ctypes.byref(ksize)))
    bounds = np.zeros((int(n_out), 2), dtype=np.int32)
    coeffs = np.zeros((int(n_out), ksize.value), dtype=np.int32)
    _lib.check(lib.mspa_resize_coeffs_host(int(n_in), int(n_out), f, bounds.ctypes.data, coeffs.ctypes.data, ctypes.byref(ksize)))
    return bounds, coeffs


def _resize_tables(n_in: int, n_out: int, f: int, device) -> tuple:
    """The device copy of one axis's tables, built once per (in, out, filter, device)."""
    device = torch.device(device)
    key = (n_in, n_out, f, device.type, device.index if device.index is not None else torch.cuda.current_device())
    hit = _RESIZE_TABLES.get(key)
    if hit is None:
        bounds, coeffs = resize_coeffs_host(n_in, n_out, f)
        if len(_RESIZE_TABLES) >= 64:                   # a tree of many shapes: forget the oldest
            _RESIZE_TABLES.pop(next(iter(_RESIZE_TABLES)))
        hit = _RESIZE_TABLES[key] = (torch.from_numpy(bounds).to(device), torch.from_numpy(coeffs).to(device))
    return hit


def resize_rgb_pillow(frames: np.ndarray, hw: Tuple[int, int], resample="bicubic") -> np.ndarray:
    """The definition: Pillow's ``Image.resize`` of each [h, w, 3] uint8 frame of ``frames`` to ``hw`` = (H, W), on the host."""
    from PIL import Image
    f = _resize_filter(resample)
    H, W = int(hw[0]), int(hw[1])
    out = np.empty((len(frames), H, W, 3), dtype=np.uint8)
    for k, img in enumerate(frames):
        out[k] = np.asarray(Image.fromarray(np.ascontiguousarray(img)).resize((W, H), f))
    return out


def resize_rgb_device(frames: torch.Tensor, hw: Tuple[int, int], resample="bicubic", out: Optional[torch.Tensor] = None,
                      fallback: bool = True) -> torch.Tensor:
    """[n, h, w, 3] uint8 RGB on the device -> [n, H, W, 3] uint8 with ``hw`` = (H, W): bit for bit Pillow's
    ``Image.fromarray(frames[k]).resize((W, H), resample)`` for ``resample`` "bicubic" (Pillow's default) or "bilinear"
    (mspa_resize_rgb_device).  ``frames`` may be a strided view as long as a pixel's three bytes and a row's pixels are adjacent
    (rows and images may be padded).  A per-axis factor outside 1/8 .. 8 is declined by the kernels: with ``fallback`` Pillow
    resizes those frames on the host (download, resize, upload), without it ``MspaError`` (code MSPA_EUNSUPPORTED) is raised.
    Only enqueues on the current stream otherwise."""
    n, h, w = _check("frames", frames, torch.uint8, (None, None, None, 3), contiguous=False).shape[:3]
    H, W = int(hw[0]), int(hw[1])
    _require(1 <= h <= 65535 and 1 <= w <= 65535 and 1 <= H <= 65535 and 1 <= W <= 65535, f"1 <= h, w, H, W <= 65535, got {(h, w, H, W)}")
    _require(n <= 65535, f"frames: at most 65 535 images in one call, got {n}")
    f = _resize_filter(resample)
    st = frames.stride()
    if n and not (st[3] == 1 and st[2] == 3 and st[1] >= 3 * w and (n == 1 or st[0] >= (h - 1) * st[1] + 3 * w)):
        frames = frames.contiguous()
        st = frames.stride()
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=frames.device) if out is None else _check("out", out, torch.uint8, (n, H, W, 3))
    if n == 0:
        return out
    lib = _lib.load()
    bx = kx = by = ky = None
    try:
        if w != W:
            bx, kx = _resize_tables(w, W, f, frames.device)
        if h != H:
            by, ky = _resize_tables(h, H, f, frames.device)
        ws_bytes = int(lib.mspa_resize_workspace_bytes(n, h, w, H, W))
        work = _workspace(ws_bytes, frames.device) if ws_bytes else None
        image_pitch = int(st[0]) if n > 1 else h * int(st[1])      # a single image's stride(0) means nothing
        _lib.check(lib.mspa_resize_rgb_device(frames.data_ptr(), n, h, w, int(st[1]), image_pitch,
                                              _ptr(out), H, W, f, _ptr(bx), _ptr(kx), _ptr(by), _ptr(ky),
                                              _ptr(work), int(work.numel()) if work is not None else 0, _stream_ptr()))
    except _lib.MspaError as e:
        if e.code != _lib.MSPA_EUNSUPPORTED or not fallback:
            raise
        out.copy_(torch.from_numpy(resize_rgb_pillow(frames.cpu().numpy(), (H, W), f)).to(out.device))
    return out


def _require_pinhole(mats: torch.Tensor):
    """MSPA_PAIR_FAST reads the camera-2 depth off the third image row: K's third row must be 0 0 1 0 in EVERY frame record
    (include/mspa.h).  The records live on the device, so the check is one read-back of all frames' rows the first time a
    table OBJECT is seen; the verdict rides on that tensor object (with its in-place version counter), so later launches on
    the same table enqueue without touching the host -- a per-call read-back would synchronise the stream in the hot enqueue
    path -- and a new table can never inherit another one's verdict (round 3 keyed a global cache by storage address, which
    the caching allocator hands to the next scene's table: ADVICE round 3).  ``SceneOnDevice`` and the bench keep one table
    object per scene / run; a caller that re-wraps the storage in a fresh tensor per call pays the read-back each time."""
    cached = getattr(mats, "_mspa_pinhole", None)
    if cached is None or cached[0] != mats._version:
        rows = mats[:, _lib.MAT_K, 8:12]
        want = torch.tensor([0.0, 0.0, 1.0, 0.0], dtype=torch.float64, device=mats.device)
        ok = bool((rows == want).all().item()) if mats.shape[0] else True
        cached = (mats._version, ok)
        try:
            mats._mspa_pinhole = cached
        except AttributeError:                            # a tensor subclass without a __dict__: check every time
            pass
    _require(cached[1], "MSPA_PAIR_FAST needs a pinhole K (third row 0 0 1 0) in every frame record; use flags=0 for this camera")


PAIR_OUTPUTS = ("vis_bits", "vis_u8", "valid_u8", "pix_i16", "xyz_f32", "rgba", "xyz_f64", "uv_f64",
                "depth_f64", "counts")


@functools.lru_cache(maxsize=16)
def _pair_output_shapes(n_pairs: int, H: int, W: int) -> dict:
    """name -> (shape, dtype) of mspa_pair_reproject's outputs: allocated by ``alloc_pair_outputs``, checked by ``pair_reproject``
    (which asks per launch: the last few tables are kept; read-only)."""
    P = H * W
    return types.MappingProxyType({
        "vis_bits": ((n_pairs, (P + 63) // 64), torch.int64),
        "vis_u8": ((n_pairs, P), torch.uint8),
        "valid_u8": ((n_pairs, P), torch.uint8),
        "pix_i16": ((n_pairs, P, 2), torch.int16),
        "xyz_f32": ((n_pairs, P, 3), torch.float32),
        "rgba": ((n_pairs, P), torch.int32),
        "xyz_f64": ((n_pairs, P, 3), torch.float64),
        "uv_f64": ((n_pairs, P, 2), torch.float64),
        "depth_f64": ((n_pairs, P), torch.float64),
        "counts": ((n_pairs, 2), torch.int32),
    })


def alloc_pair_outputs(n_pairs: int, image_hw: Tuple[int, int], outputs: Iterable[str], device="cuda"):
    shapes = _pair_output_shapes(n_pairs, *image_hw)
    out = {}
    for name in outputs:
        if name not in shapes:
            raise ValueError(f"unknown pair output {name!r}; choose from {PAIR_OUTPUTS}")
        shape, dtype = shapes[name]
        out[name] = torch.empty(shape, dtype=dtype, device=device)
    return out


def pair_reproject(depth: torch.Tensor, mats: torch.Tensor, pairs: torch.Tensor, image_hw: Tuple[int, int],
                   out: Dict[str, torch.Tensor], rgb: Optional[torch.Tensor] = None, flags: int = 0):
    """Enqueue K3 on the current stream.  depth [F,DH,DW] int16(bits of uint16), mats [F,8,16] f64,
    pairs [B,2] int32, rgb [F,H,W,3] uint8 (only for out['rgba']).  ``out`` comes from
    alloc_pair_outputs and is filled in place; a caller's own ``out['pix_i16']`` starts 4-byte aligned (MspaError otherwise, as
    from the C ABI: a view one int16 into a buffer is refused).
    Only enqueues, with one exception: under MSPA_PAIR_FAST the first launch
    on a ``mats`` tensor object (and the first after an in-place write to it) reads the pinhole verdict back
    (``_require_pinhole``), which waits for the current stream."""
    F, DH, DW, n = _check_pair_inputs(depth, mats, pairs)
    if flags & _lib.PAIR_FAST:
        _require_pinhole(mats)
    H, W = image_hw
    if rgb is not None:
        _check("rgb", rgb, torch.uint8, (F, H, W, 3))
    _check_outputs(out, _pair_output_shapes(n, H, W))
    _lib.check(_lib.load().mspa_pair_reproject(
        _ptr(depth), _ptr(rgb), _ptr(mats), F, _ptr(pairs), n, DH, DW, H, W,
        *map(_ptr, map(out.get, PAIR_OUTPUTS)), flags, _stream_ptr()))          # PAIR_OUTPUTS is in the C ABI's order
    return out


def corr_tiles(image_hw: Tuple[int, int]) -> Tuple[int, int]:
    """(stripes across, bands down) of the 64 x 48-pixel tiles the compacted correspondence output is segmented by."""
    H, W = image_hw
    return (W + _lib.CORR_TILE_W - 1) // _lib.CORR_TILE_W, (H + _lib.CORR_TILE_H - 1) // _lib.CORR_TILE_H


@functools.lru_cache(maxsize=16)
def _pair_correspondence_shapes(n_pairs: int, H: int, W: int) -> dict:
    """name -> (shape, dtype) of mspa_pair_correspondences' outputs (include/mspa.h), as ``_pair_output_shapes``."""
    ns, nb = corr_tiles((H, W))
    return types.MappingProxyType({"vis_bits": ((n_pairs, (H * W + 63) // 64), torch.int64),
            "cpix": ((n_pairs, ns * nb, _lib.CORR_TILE_CAP, 2), torch.int16),
            "tile_counts": ((n_pairs, ns * nb), torch.int32),
            "counts": ((n_pairs, 2), torch.int32)})


def alloc_pair_correspondences(n_pairs: int, image_hw: Tuple[int, int], device="cuda", counts: bool = True):
    """Caller-owned outputs of ``pair_correspondences`` (include/mspa.h, mspa_pair_correspondences)."""
    return {name: torch.empty(shape, dtype=dtype, device=device)
            for name, (shape, dtype) in _pair_correspondence_shapes(n_pairs, *image_hw).items() if counts or name != "counts"}


def pair_correspondences(depth: torch.Tensor, mats: torch.Tensor, pairs: torch.Tensor, image_hw: Tuple[int, int],
                         out: Optional[Dict[str, torch.Tensor]] = None, flags: int = _lib.PAIR_FAST,
                         workspace: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """Enqueue K3 with the compacted correspondence output: the visibility bitset plus, per 64 x 48 tile of frame 1, the
    frame-2 pixel (xi, yi) of its VISIBLE pixels in (row, column) order.  One fused kernel on whole-tile shapes with
    MSPA_PAIR_FAST (640x480); other shapes / the reference-order mode go through a dense table in ``workspace`` (int32 or
    uint8, allocated here when not given or too small).  ``out`` from ``alloc_pair_correspondences``.  Only enqueues, with
    ``pair_reproject``'s exception: the pinhole verdict of a ``mats`` object that MSPA_PAIR_FAST sees for the first time."""
    lib = _lib.load()
    F, DH, DW, n = _check_pair_inputs(depth, mats, pairs)
    if flags & _lib.PAIR_FAST:
        _require_pinhole(mats)
    H, W = image_hw
    if out is None:
        out = alloc_pair_correspondences(n, image_hw, depth.device)
    else:
        _check_outputs(out, _pair_correspondence_shapes(n, H, W), required=("vis_bits", "cpix", "tile_counts"))
    if workspace is not None:
        _check("workspace", workspace, (torch.int32, torch.uint8), (None,))
    need = int(lib.mspa_pair_correspondences_workspace_bytes(n, DH, DW, H, W, flags))
    _require(need >= 0, "image_hw and the depth frames' size: within [2, 32767]")
    if need == 0 and _ptr(depth) & 3:      # the pointer rule of csrc/pair_route.h route(), which the size query cannot apply
        # a depth VIEW at an odd 2-byte offset: the fused kernel's 4-byte LDS-DMA cannot take it and the C entry point goes
        # through the dense table, which needs a workspace although the size query (it cannot see the pointer) said 0
        need = n * H * W * 4
    if need and (workspace is None or workspace.numel() * workspace.element_size() < need):
        workspace = torch.empty((need + 3) // 4, dtype=torch.int32, device=depth.device)
    _lib.check(lib.mspa_pair_correspondences(
        _ptr(depth), _ptr(mats), F, _ptr(pairs), n, DH, DW, H, W, _ptr(out["vis_bits"]), _ptr(out["cpix"]),
        _ptr(out["tile_counts"]), _ptr(out.get("counts")), _ptr(workspace) if need else None,
        workspace.numel() * workspace.element_size() if need else 0, flags, _stream_ptr()))
    return out


def correspondences_rowmajor(out: Dict[str, torch.Tensor], image_hw: Tuple[int, int], pair: int):
    """One pair's compacted correspondences re-ordered to ``np.nonzero(visible)`` order (torch indexing as plumbing, for
    consumers and tests that want the flat view): returns (pixel index i = y * W + x in frame 1 [n_vis] int64, xi [n_vis],
    yi [n_vis] int16 in frame 2), all on the device."""
    H, W = image_hw
    ns, nb = corr_tiles(image_hw)
    bits = out["vis_bits"][pair]
    P = H * W
    shifts = torch.arange(64, device=bits.device, dtype=torch.int64)
    vis = ((bits.unsqueeze(1) >> shifts) & 1).reshape(-1)[:P].reshape(H, W).bool()
    # rank of every visible pixel inside its tile, in (row, column) order of the tile
    pad = torch.zeros((nb * _lib.CORR_TILE_H, ns * _lib.CORR_TILE_W), dtype=torch.bool, device=bits.device)
    pad[:H, :W] = vis
    tiles = pad.reshape(nb, _lib.CORR_TILE_H, ns, _lib.CORR_TILE_W).permute(0, 2, 1, 3).reshape(nb * ns, -1)
    rank = torch.cumsum(tiles.to(torch.int32), dim=1) - 1
    rank_img = rank.reshape(nb, ns, _lib.CORR_TILE_H, _lib.CORR_TILE_W).permute(0, 2, 1, 3).reshape(nb * _lib.CORR_TILE_H, -1)[:H, :W]
    yy, xx = torch.nonzero(vis, as_tuple=True)
    t = (yy // _lib.CORR_TILE_H) * ns + (xx // _lib.CORR_TILE_W)
    e = out["cpix"][pair][t, rank_img[yy, xx].long()]
    return yy * W + xx, e[:, 0], e[:, 1]


def _check_cameras(xyz, cam_mats, depth, min_components: int = 3) -> Tuple[int, int, int]:
    """What K1 and K6b project: xyz float64 [N, >= 3] handed over WITH its strides (any positive ones: rows, or a [3, N] SoA tensor's
    ``.t()``), depth [I, DH, DW] and cam_mats [I, CAM_MATS, 16] float64 (``camera_matrices``) -> (I, DH, DW)."""
    _check("xyz", xyz, torch.float64, (None, (min_components,)), contiguous=False)
    _require(xyz.stride(0) > 0 and xyz.stride(1) > 0, f"xyz: positive strides, got {tuple(xyz.stride())}")
    I, DH, DW = _check("depth", depth, _DEPTH, (None, None, None)).shape
    _check("cam_mats", cam_mats, torch.float64, (I, _lib.CAM_MATS, 16))
    return I, DH, DW


def vertex_visibility(xyz: torch.Tensor, cam_mats: torch.Tensor, depth: torch.Tensor, image_hw: Tuple[int, int],
                      want: Iterable[str] = ("bits", "count"), homogeneous: bool = False,
                      depth_scale: float = 0.001) -> Dict[str, torch.Tensor]:
    """Enqueue K1.  xyz [N,3] or [N,C>=3] float64 rows (or a [3,N] SoA tensor with soa=True layout
    given as xyz.t()); cam_mats [I,3,16]; depth [I,DH,DW].  Returns the requested outputs.
    ``homogeneous``: the rows are general homogeneous points (x, y, z, w) (``project_points`` takes any [N, 4], IH:46-72);
    ``depth_scale``: the handler's ``depth_value_scale`` (IH:76, IH:368)."""
    I, DH, DW = _check_cameras(xyz, cam_mats, depth, 4 if homogeneous else 3)
    n = xyz.shape[0]
    H, W = image_hw
    out = _alloc_wanted(want, {"bits": ((I, (n + 63) // 64), torch.int64), "mask": ((I, n), torch.uint8),
                               "uv": ((I, n, 2), torch.float64), "depth": ((I, n), torch.float64),
                               "count": ((I,), torch.int32)}, xyz.device)
    _lib.check(_lib.load().mspa_vertex_visibility_ex(
        xyz.data_ptr(), n, xyz.stride(0), xyz.stride(1), 1 if homogeneous else 0, _ptr(cam_mats), I, _ptr(depth), DH, DW, H, W,
        float(depth_scale), _ptr(out.get("bits")), _ptr(out.get("mask")), _ptr(out.get("uv")), _ptr(out.get("depth")),
        _ptr(out.get("count")), _stream_ptr()))
    return out


def all_pairs(n: int, device="cuda") -> torch.Tensor:
    """(i, j), i < j, in the row-major order of the reference's nested loops (CFR:176-178)."""
    return torch.triu_indices(n, n, offset=1, device=device).t().contiguous().to(torch.int32)


def pair_overlap(bits: torch.Tensor, pairs: torch.Tensor, want_counts: bool = False):
    """Enqueue K2 on K1's bitsets.  Returns overlap [n_pairs] f64 (+ inter, union int32)."""
    F, n_words = _check_bits("bits", bits)
    n_pairs = _check("pairs", pairs, torch.int32, (None, 2)).shape[0]
    overlap = torch.empty((n_pairs,), dtype=torch.float64, device=bits.device)
    inter = torch.empty((n_pairs,), dtype=torch.int32, device=bits.device) if want_counts else None
    uni = torch.empty((n_pairs,), dtype=torch.int32, device=bits.device) if want_counts else None
    _lib.check(_lib.load().mspa_pair_overlap(_ptr(bits), F, n_words, _ptr(pairs), n_pairs,
                                             _ptr(overlap), _ptr(inter), _ptr(uni), _stream_ptr()))
    return (overlap, inter, uni) if want_counts else overlap


def _overlap_workspace(n_a: int, n_b: int, n_words: int, device) -> torch.Tensor:
    nbytes = int(_lib.load().mspa_overlap_workspace_bytes(n_a, n_b, n_words))
    return torch.empty((max(nbytes, 4) + 3) // 4, dtype=torch.int32, device=device)


def scene_overlap(bits: torch.Tensor, want_counts: bool = False):
    """Enqueue the tiled K2 over ALL pairs i < j of a scene's bitsets, in ``all_pairs`` order (CFR:176-178).
    Returns overlap [F(F-1)/2] f64 (+ inter, union int32) -- identical to ``pair_overlap(bits, all_pairs(F))``."""
    F, n_words = _check_bits("bits", bits)
    n_pairs = F * (F - 1) // 2
    dev = bits.device
    overlap = torch.empty((n_pairs,), dtype=torch.float64, device=dev)
    inter = torch.empty((n_pairs,), dtype=torch.int32, device=dev) if want_counts else None
    uni = torch.empty((n_pairs,), dtype=torch.int32, device=dev) if want_counts else None
    if n_pairs and n_words:
        ws = _overlap_workspace(F, F, n_words, dev)
        _lib.check(_lib.load().mspa_scene_overlap(_ptr(bits), F, n_words, _ptr(ws), ws.numel() * 4, _ptr(overlap),
                                                  _ptr(inter), _ptr(uni), _stream_ptr()))
    elif n_pairs:                           # bitsets of no points: no launch has a word to read; every union is empty (CFR:136)
        overlap.fill_(float("nan"))
        if want_counts:
            inter.zero_()
            uni.zero_()
    return (overlap, inter, uni) if want_counts else overlap


def overlap_matrix(bits_a: torch.Tensor, bits_b: torch.Tensor) -> torch.Tensor:
    """Enqueue the tiled K2 on a rectangle: |a_i & b_j| for every row pair, [n_a, n_b] int32 (object visibility:
    objects x images, compute_object_visibility.py:72-152)."""
    n_a, n_words = _check_bits("bits_a", bits_a)
    n_b = _check("bits_b", bits_b, torch.int64, (None, n_words)).shape[0]         # both tables: one word count
    out = torch.empty((n_a, n_b), dtype=torch.int32, device=bits_a.device)
    if n_a and n_b and n_words:
        ws = _overlap_workspace(n_a, n_b, n_words, bits_a.device)
        _lib.check(_lib.load().mspa_overlap_matrix(_ptr(bits_a), n_a, _ptr(bits_b), n_b, n_words, _ptr(ws),
                                                   ws.numel() * 4, _ptr(out), _stream_ptr()))
    else:
        out.zero_()                         # (no rows, or bitsets of no points: nothing is launched and nothing intersects)
    return out


def bitset_csr(bits: torch.Tensor):
    """K9: rows of a bit matrix -> CSR of their set bits.  bits [R, n_words] int64 (device) -> (offsets [R+1] int64,
    indices [nnz] int32), both on the device; row r's set-bit positions, ascending, are indices[offsets[r]:offsets[r+1]].
    One small read-back (the number of set bits: the size to allocate)."""
    lib = _lib.load()
    R, n_words = _check_bits("bits", bits)
    dev = bits.device
    if R == 0 or n_words == 0:
        return torch.zeros((R + 1,), dtype=torch.int64, device=dev), torch.zeros((0,), dtype=torch.int32, device=dev)
    counts = torch.empty((R * n_words,), dtype=torch.int32, device=dev)
    _lib.check(lib.mspa_bits_popcount(_ptr(bits), R * n_words, _ptr(counts), _stream_ptr()))
    incl = torch.cumsum(counts, dim=0, dtype=torch.int64)              # torch as plumbing: one prefix sum
    word_offsets = (incl - counts).contiguous()
    total = int(incl[-1].item())
    indices = torch.empty((total,), dtype=torch.int32, device=dev)
    if total:
        _lib.check(lib.mspa_bits_expand(_ptr(bits), R, n_words, _ptr(word_offsets), _ptr(indices), _stream_ptr()))
    offsets = torch.cat([word_offsets[::n_words], incl[-1:]])
    return offsets, indices


def format_lists_device(offsets: torch.Tensor, values: torch.Tensor, tokens: Optional[Sequence[bytes]] = None):
    """K10: the JSON text of every list of a CSR table, written on the device (``json.dumps`` form: "[1, 2, 3]", "[]";
    make_visibility_info.py:38-73).  ``offsets`` [n + 1] int64, ``values`` [nnz] int32 (device).  ``tokens`` None: the items are
    integers; else item e is the text ``tokens[values[e]]`` (bytes, e.g. an already quoted image id).  Returns (text [bytes] uint8,
    text_offsets [n + 1] int32) on the device: arrow's string layout."""
    lib = _lib.load()
    n = _check("offsets", offsets, torch.int64, ((1,),)).numel() - 1
    nnz = _check("values", values, torch.int32, (None,)).numel()
    dev = offsets.device
    tok = tok_off = None
    n_tokens = 0
    if tokens is not None:
        n_tokens = len(tokens)
        lens = np.array([len(t) for t in tokens], dtype=np.int64)
        tok_off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)).to(dev)
        tok = torch.from_numpy(np.frombuffer(b"".join(tokens) or b"\0", dtype=np.uint8).copy()).to(dev)
    cost = torch.empty((max(nnz, 1),), dtype=torch.int32, device=dev)
    bad = torch.zeros((1,), dtype=torch.int32, device=dev)
    _lib.check(lib.mspa_format_list_costs_device(_ptr(values) if nnz else None, nnz, _ptr(tok_off), n_tokens, _ptr(cost), _ptr(bad), _stream_ptr()))
    T = torch.zeros((nnz + 1,), dtype=torch.int64, device=dev)                   # torch as plumbing: two prefix sums
    if nnz:
        torch.cumsum(cost[:nnz], dim=0, dtype=torch.int64, out=T[1:])
    NE = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
    if n:
        torch.cumsum((offsets[1:] > offsets[:-1]).to(torch.int64), dim=0, out=NE[1:])
    head = torch.stack([2 * n + T[-1] - 2 * NE[-1], bad[0].to(torch.int64)]).cpu()     # one small read-back: the size to allocate
    total = int(head[0])
    _require(int(head[1]) == 0, "format_lists_device: token id out of range")
    _require(total <= 0x7fffffff, "format_lists_device: more than 2 GiB of text")
    text = torch.empty((max(total, 1),), dtype=torch.uint8, device=dev)
    text_offsets = torch.empty((n + 1,), dtype=torch.int32, device=dev)
    _lib.check(lib.mspa_format_lists_device(_ptr(offsets), _ptr(values) if nnz else None, n, nnz, _ptr(T), _ptr(NE), _ptr(tok), _ptr(tok_off),
                                            _ptr(text), total, _ptr(text_offsets), _stream_ptr()))
    return text[:total], text_offsets


def snappy_capacity(n: int) -> int:
    """Worst-case bytes of the Snappy stream of ``n`` input bytes (mspa_snappy_capacity)."""
    cap = int(_lib.load().mspa_snappy_capacity(int(n)))
    _require(cap > 0, "n: 0 <= n < 2^31")
    return cap


def snappy_compress_device(src: torch.Tensor, offsets: torch.Tensor, nbytes: torch.Tensor):
    """K12: a batch of byte streams -- stream s is ``src[offsets[s] : offsets[s] + nbytes[s]]`` (``src`` uint8, ``offsets`` /
    ``nbytes`` int64, all on the device; streams may be empty) -- each compressed into one Snappy stream by the library's own
    deterministic compressor (csrc/snappy_core.h; byte for byte mspa_snappy_compress_host).  Returns (out uint8 [total], starts
    int64 [n + 1]) on the device: stream s is ``out[starts[s] : starts[s + 1]]``.  Three small read-backs (block count, total,
    the kernels' flag): the call returns with the streams written."""
    out, starts, bad = _snappy_compress(src, offsets, nbytes)
    _require(int(bad.item()) == 0, "snappy_compress_device: a destination fell outside the output")
    return out, starts


def _streams_inside(src, offsets, nbytes):
    """Per stream of a table: it lies inside ``src`` and is shorter than 2 GiB (bool, on the device)."""
    return (offsets >= 0) & (nbytes >= 0) & (nbytes <= 0x7fffffff) & (offsets <= src.numel() - nbytes)


def _snappy_compress(src, offsets, nbytes):
    """``snappy_compress_device`` without its last read-back: (out, starts, the compact kernels' flag, still on the device)."""
    lib = _lib.load()
    n = _check_streams(offsets, nbytes)
    _check("src", src, torch.uint8, (None,))
    dev = src.device
    if n == 0:
        return (torch.empty((0,), dtype=torch.uint8, device=dev), torch.zeros((1,), dtype=torch.int64, device=dev),
                torch.zeros((1,), dtype=torch.int32, device=dev))
    # torch as plumbing: the prefix sums of blocks and of preamble lengths, and the argument check no kernel should have to make
    block_prefix = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
    torch.cumsum((nbytes + (_lib.SNAPPY_BLOCK - 1)) // _lib.SNAPPY_BLOCK, dim=0, out=block_prefix[1:])
    vlen = 1 + (nbytes >= 1 << 7).to(torch.int64) + (nbytes >= 1 << 14) + (nbytes >= 1 << 21) + (nbytes >= 1 << 28)
    vprefix = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
    torch.cumsum(vlen, dim=0, out=vprefix[1:])
    head = torch.stack([block_prefix[-1], _streams_inside(src, offsets, nbytes).all().to(torch.int64)]).cpu()
    _require(int(head[1]) == 1, "offsets / nbytes: every stream lies inside src and is shorter than 2 GiB")
    n_blocks = int(head[0])
    _require(n_blocks <= 0x7fffffff, "nbytes: fewer than 2^31 blocks of 64 KiB in one call")
    slots = _workspace(int(lib.mspa_snappy_workspace_bytes(n_blocks)), dev)
    sizes = torch.empty((max(n_blocks, 1),), dtype=torch.int64, device=dev)
    _lib.check(lib.mspa_snappy_compress_device(_ptr(src), src.numel(), _ptr(offsets), _ptr(nbytes), n, _ptr(block_prefix), n_blocks,
                                               _ptr(slots), slots.numel(), _ptr(sizes), _stream_ptr()))
    size_prefix = torch.zeros((n_blocks + 1,), dtype=torch.int64, device=dev)
    if n_blocks:
        torch.cumsum(sizes[:n_blocks], dim=0, out=size_prefix[1:])
    head = torch.stack([size_prefix[-1] + vprefix[-1], sizes[:n_blocks].min() if n_blocks else size_prefix[0]]).cpu()
    _require(int(head[1]) >= 0, "snappy_compress_device: a block was refused by the kernel (stream table out of range)")
    total = int(head[0])
    out = torch.empty((total,), dtype=torch.uint8, device=dev)
    bad = torch.zeros((1,), dtype=torch.int32, device=dev)
    _lib.check(lib.mspa_snappy_compact_device(_ptr(nbytes), n, _ptr(block_prefix), n_blocks, _ptr(slots), slots.numel(), _ptr(size_prefix),
                                              _ptr(vprefix), _ptr(out), total, _ptr(bad), _stream_ptr()))
    starts = size_prefix[block_prefix] + vprefix
    return out, starts, bad


def parquet_string_pages_device(text_offsets: torch.Tensor, data: torch.Tensor, page_bytes: int = 1 << 20, return_payload: bool = False):
    """K12: a string column in arrow's layout on the device (``text_offsets`` int32 [rows + 1], ``data`` uint8: what
    ``format_lists_device`` returns) -> its parquet v1 data pages, PLAIN BYTE_ARRAY with RLE definition levels (no nulls),
    Snappy-compressed.  A page ends after the first value at which its PLAIN bytes reach ``page_bytes``.  Returns a dict:
    ``chunk`` (uint8, device: the pages' compressed bytes back to back), ``compressed`` / ``uncompressed`` / ``num_values``
    (int64 numpy, per page) and, with ``return_payload``, ``payload`` (uint8, device: the uncompressed payloads back to back).
    The offsets come to the host (the page cuts are a serial rule over them); the text does not.  Synchronises the current
    stream."""
    lib = _lib.load()
    rows = _check("text_offsets", text_offsets, torch.int32, ((1,),)).numel() - 1
    _check("data", data, torch.uint8, (None,))
    _require(int(page_bytes) >= 1, "page_bytes >= 1")
    _require(data.numel() <= 0x7fffffff, "data: less than 2 GiB of text")
    dev = data.device
    offs = text_offsets.cpu().numpy()
    empty = {"chunk": torch.empty((0,), dtype=torch.uint8, device=dev), "compressed": np.zeros(0, np.int64),
             "uncompressed": np.zeros(0, np.int64), "num_values": np.zeros(0, np.int64)}
    if return_payload:
        empty["payload"] = torch.empty((0,), dtype=torch.uint8, device=dev)
    if rows == 0:
        return empty
    _require(int(offs[0]) >= 0 and int(offs[-1]) <= data.numel() and bool((np.diff(offs) >= 0).all()),
             "text_offsets: non-decreasing and inside data")
    cuts = np.empty(rows + 1, dtype=np.int64)
    n_pages = int(lib.mspa_parquet_page_cuts_host(offs.ctypes.data, rows, int(page_bytes), cuts.ctypes.data, rows + 1))
    if n_pages < 0:
        _lib.check(n_pages)
    cuts = cuts[:n_pages + 1]
    nv = np.diff(cuts)
    levels = 1 + 1 + (nv >= 1 << 6) + (nv >= 1 << 13) + (nv >= 1 << 20) + (nv >= 1 << 27)       # varint(nv << 1), then 0x01
    plain = 4 * nv + (offs[cuts[1:]].astype(np.int64) - offs[cuts[:-1]].astype(np.int64))
    pay = 4 + levels + plain
    _require(int(pay.max()) <= 0x7fffffff, "a page of 2 GiB or more: raise page_bytes' granularity")
    table = np.zeros((3, n_pages + 1), dtype=np.int64)                                          # cuts, payload offsets, payload sizes
    table[0] = cuts
    np.cumsum(pay, out=table[1, 1:])
    table[2, :n_pages] = pay
    total = int(table[1, -1])
    table_dev = torch.from_numpy(table).to(dev)
    payload = torch.empty((total,), dtype=torch.uint8, device=dev)
    bad = torch.zeros((1,), dtype=torch.int32, device=dev)
    _lib.check(lib.mspa_parquet_string_pages_device(_ptr(text_offsets), rows, _ptr(data) if data.numel() else None, data.numel(),
                                                    _ptr(table_dev[0]), _ptr(table_dev[1]), n_pages, total, _ptr(payload), _ptr(bad),
                                                    _stream_ptr()))
    chunk, starts, bad2 = _snappy_compress(payload, table_dev[1, :n_pages].contiguous(), table_dev[2, :n_pages].contiguous())
    head = torch.cat([starts, bad.to(torch.int64), bad2.to(torch.int64)]).cpu().numpy()
    _require(int(head[-2]) == 0 and int(head[-1]) == 0, "parquet_string_pages_device: the page tables do not describe the text")
    out = {"chunk": chunk, "compressed": np.diff(head[:n_pages + 1]), "uncompressed": pay.astype(np.int64), "num_values": nv.astype(np.int64)}
    if return_payload:
        out["payload"] = payload
    return out


def snappy_decompress_device(src: torch.Tensor, offsets: torch.Tensor, nbytes: torch.Tensor, out_sizes: torch.Tensor):
    """A batch of raw Snappy streams decoded on the device, one wave per stream: stream s is ``src[offsets[s] : offsets[s] +
    nbytes[s]]`` (``src`` uint8, the tables int64, all on the device; streams may be empty, overlap or leave gaps) and decodes to
    ``out_sizes[s]`` bytes (what its preamble must say).  Returns (out uint8 [sum of out_sizes], out_offsets int64 [n + 1],
    status int32 [n]) on the device: stream s is ``out[out_offsets[s] : out_offsets[s + 1]]`` where ``status[s] == 0`` -- byte for
    byte mspa_snappy_decompress_host -- and was declined with the host's code (``_lib.SNAPPY_E*``; MSPA_EINVAL for a table entry
    outside ``src``) otherwise.  One small read-back (the size to allocate)."""
    lib = _lib.load()
    n = _check_streams(offsets, nbytes)
    _check("src", src, torch.uint8, (None,))
    _check("out_sizes", out_sizes, torch.int64, (n,))
    dev = src.device
    out_offsets = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
    status = torch.zeros((n,), dtype=torch.int32, device=dev)
    if n == 0:
        return torch.empty((0,), dtype=torch.uint8, device=dev), out_offsets, status
    torch.cumsum(out_sizes.clamp(min=0), dim=0, out=out_offsets[1:])      # a negative size is the kernel's to refuse (MSPA_EINVAL)
    total = int(out_offsets[-1].item())
    out = torch.empty((max(total, 1),), dtype=torch.uint8, device=dev)
    _lib.check(lib.mspa_snappy_decompress_device(_ptr(src) if src.numel() else None, src.numel(), _ptr(offsets), _ptr(nbytes), n, _ptr(out),
                                                 total, _ptr(out_offsets), _ptr(out_sizes), _ptr(status), _stream_ptr()))
    return out[:total], out_offsets, status


def _block_tables(src, offsets, nbytes, out_sizes):
    """What the block route's two calls share: the checks, the prefix sums (torch as plumbing) and ONE small read-back -- the
    bytes to allocate, the block count and the sum of the compressed sizes (streams may overlap: that sum sizes the workspace)."""
    n = _check_streams(offsets, nbytes)
    _check("src", src, torch.uint8, (None,))
    _check("out_sizes", out_sizes, torch.int64, (n,))
    dev = src.device
    out_offsets = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
    block_prefix = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
    if n == 0:
        return 0, out_offsets, block_prefix, 0, 0, 0
    sizes = out_sizes.clamp(min=0, max=0x7fffffff)            # a size outside is the kernel's to refuse (MSPA_EINVAL)
    torch.cumsum(sizes, dim=0, out=out_offsets[1:])
    torch.cumsum((sizes + (_lib.SNAPPY_BLOCK - 1)) // _lib.SNAPPY_BLOCK, dim=0, out=block_prefix[1:])
    head = torch.stack([out_offsets[-1], block_prefix[-1], (nbytes * _streams_inside(src, offsets, nbytes)).sum()]).cpu()
    total, n_blocks, stream_bytes = int(head[0]), int(head[1]), int(head[2])
    _require(n_blocks <= 0x7fffffff, "out_sizes: fewer than 2^31 blocks of 64 KiB in one call")
    return n, out_offsets, block_prefix, total, n_blocks, stream_bytes


def _blocks_workspace(who, stream_bytes, n, n_blocks, dev):
    """The block route's workspace for a batch; ``who``: the caller, for the message."""
    ws_bytes = int(_lib.load().mspa_snappy_blocks_workspace_bytes(stream_bytes, n, n_blocks))
    _require(ws_bytes >= 0, who + ": sizes beyond the workspace's range")
    return _workspace(ws_bytes, dev)


def snappy_block_starts_device(src: torch.Tensor, offsets: torch.Tensor, nbytes: torch.Tensor, out_sizes: torch.Tensor):
    """The block-start scan alone, for a batch of raw Snappy streams as ``snappy_decompress_device`` takes them: where each
    64 KiB block's elements begin in the compressed bytes.  Returns (starts int64 [n_blocks + n], block_prefix int64 [n + 1],
    route int32 [n]) on the device: stream s's starts are ``starts[block_prefix[s] + s : block_prefix[s + 1] + s + 1]`` (one more
    than its blocks; the last is ``nbytes[s]``) where ``route[s]`` is its block count -- then they are
    mspa_snappy_block_starts_host's; ``route[s] == 0``: the stream is empty, not blockwise or not decodable, its starts are
    unspecified.  One small read-back (the sizes to allocate)."""
    lib = _lib.load()
    n, _out_offsets, block_prefix, _total, n_blocks, stream_bytes = _block_tables(src, offsets, nbytes, out_sizes)
    dev = src.device
    starts = torch.full((n_blocks + n,), -1, dtype=torch.int64, device=dev)
    route = torch.zeros((n,), dtype=torch.int32, device=dev)
    if n == 0:
        return starts, block_prefix, route
    ws = _blocks_workspace("snappy_block_starts_device", stream_bytes, n, n_blocks, dev)
    _lib.check(lib.mspa_snappy_block_starts_device(_ptr(src) if src.numel() else None, src.numel(), _ptr(offsets), _ptr(nbytes), n,
                                                   _ptr(out_sizes), _ptr(block_prefix), n_blocks, stream_bytes, _ptr(ws), ws.numel(),
                                                   _ptr(starts), _ptr(route), _stream_ptr()))
    return starts, block_prefix, route


def snappy_decompress_blocks_device(src: torch.Tensor, offsets: torch.Tensor, nbytes: torch.Tensor, out_sizes: torch.Tensor):
    """``snappy_decompress_device`` by blocks: the same arguments, the same (out, out_offsets, status) for every input, and
    ``route`` int32 [n] behind them.  A stream whose elements respect the 64 KiB block boundaries both writers keep (pyarrow's
    and this library's) is decoded by one wave per block -- ``route[s]`` = its block count; every other stream, every stream of
    one block and every stream with anything the matter with it is decoded (or declined, with the host's code) by the one-wave
    kernel -- ``route[s] == 0``.  The workspace is about 8 bytes per compressed byte.  One small read-back (the sizes to
    allocate)."""
    lib = _lib.load()
    n, out_offsets, block_prefix, total, n_blocks, stream_bytes = _block_tables(src, offsets, nbytes, out_sizes)
    dev = src.device
    status = torch.zeros((n,), dtype=torch.int32, device=dev)
    route = torch.zeros((n,), dtype=torch.int32, device=dev)
    if n == 0:
        return torch.empty((0,), dtype=torch.uint8, device=dev), out_offsets, status, route
    out = torch.empty((max(total, 1),), dtype=torch.uint8, device=dev)
    ws = _blocks_workspace("snappy_decompress_blocks_device", stream_bytes, n, n_blocks, dev)
    _lib.check(lib.mspa_snappy_decompress_blocks_device(_ptr(src) if src.numel() else None, src.numel(), _ptr(offsets), _ptr(nbytes), n,
                                                        _ptr(out), total, _ptr(out_offsets), _ptr(out_sizes), _ptr(block_prefix), n_blocks,
                                                        stream_bytes, _ptr(ws), ws.numel(), _ptr(status), _ptr(route), _stream_ptr()))
    return out[:total], out_offsets, status, route


def _check_page_tables(page_offsets, page_sizes, page_values, row_begin, row_index):
    """The page and row tables the span kernels read -> (n_pages, n_rows)."""
    n_pages = _check_streams(page_offsets, page_sizes)
    _check("page_values", page_values, torch.int64, (n_pages,))
    _check("row_begin", row_begin, torch.int64, (n_pages + 1,))
    n_rows = _check("row_index", row_index, torch.int64, (None,)).shape[0]
    _require(n_pages > 0 or n_rows == 0, "rows need pages")
    return n_pages, n_rows


def parquet_plain_spans_device(pages: torch.Tensor, page_offsets: torch.Tensor, page_sizes: torch.Tensor, page_values: torch.Tensor,
                               row_begin: torch.Tensor, row_index: torch.Tensor, has_levels: bool = True):
    """Where the needed rows' texts lie in PLAIN BYTE_ARRAY pages (mspa_parquet_plain_spans_device; the tables as
    ``index_rows_to_bits`` describes them) -> (start int64 [rows], length int64 [rows], page_status int32 [pages]), on the
    device.  With ``has_levels=False`` and every entry as a row, a decompressed dictionary page gives the span table
    ``parquet_dict_spans_device`` looks its indices up in.  Only enqueues."""
    n_pages, n_rows = _check_page_tables(page_offsets, page_sizes, page_values, row_begin, row_index)
    _check("pages", pages, torch.uint8, (None,))
    dev = pages.device
    start = torch.zeros((n_rows,), dtype=torch.int64, device=dev)
    length = torch.zeros((n_rows,), dtype=torch.int64, device=dev)
    page_status = torch.zeros((n_pages,), dtype=torch.int32, device=dev)
    if n_pages:
        _lib.check(_lib.load().mspa_parquet_plain_spans_device(_ptr(pages) if pages.numel() else None, pages.numel(), _ptr(page_offsets),
                                                               _ptr(page_sizes), _ptr(page_values), n_pages, 1 if has_levels else 0,
                                                               _ptr(row_begin), _ptr(row_index), n_rows, _ptr(start), _ptr(length),
                                                               _ptr(page_status), _stream_ptr()))
    return start, length, page_status


def parquet_dict_spans_device(pages: torch.Tensor, page_offsets: torch.Tensor, page_sizes: torch.Tensor, page_values: torch.Tensor,
                              row_begin: torch.Tensor, row_index: torch.Tensor, dict_begin: torch.Tensor, dict_count: torch.Tensor,
                              dict_start: torch.Tensor, dict_length: torch.Tensor, has_levels: bool = True):
    """``parquet_plain_spans_device`` for dictionary-coded data pages (RLE_DICTIONARY / PLAIN_DICTIONARY: a byte of bit width,
    then the indices as RLE / bit-packed runs), the same page and row tables.  Page p's dictionary is entries ``dict_begin[p] :
    dict_begin[p] + dict_count[p]`` of the span table ``dict_start`` / ``dict_length`` (all int64, on the device) -- the spans of
    the dictionary pages' entries in ``pages``.  Returns (index int32 [rows], start int64 [rows], length int64 [rows],
    page_status int32 [pages], page_code int32 [pages]) on the device.  Status: 0 taken, 1 a table entry outside the page, 2
    levels, 3 malformed runs -- the code is then mspa_rle_hybrid_take_host's (``_lib.RLE_E*``) --, 4 an index beyond the
    dictionary; a declined page's rows get index -1 and an empty span.  Only enqueues."""
    n_pages, n_rows = _check_page_tables(page_offsets, page_sizes, page_values, row_begin, row_index)
    _check("pages", pages, torch.uint8, (None,))
    _check("dict_begin", dict_begin, torch.int64, (n_pages,))
    _check("dict_count", dict_count, torch.int64, (n_pages,))
    n_dict = _check("dict_start", dict_start, torch.int64, (None,)).shape[0]
    _check("dict_length", dict_length, torch.int64, (n_dict,))
    dev = pages.device
    index = torch.full((n_rows,), -1, dtype=torch.int32, device=dev)
    start = torch.zeros((n_rows,), dtype=torch.int64, device=dev)
    length = torch.zeros((n_rows,), dtype=torch.int64, device=dev)
    page_status = torch.zeros((n_pages,), dtype=torch.int32, device=dev)
    page_code = torch.zeros((n_pages,), dtype=torch.int32, device=dev)
    if n_pages:
        _lib.check(_lib.load().mspa_parquet_dict_spans_device(
            _ptr(pages) if pages.numel() else None, pages.numel(), _ptr(page_offsets), _ptr(page_sizes), _ptr(page_values), n_pages,
            1 if has_levels else 0, _ptr(row_begin), _ptr(row_index), n_rows, _ptr(dict_begin), _ptr(dict_count),
            _ptr(dict_start) if n_dict else None, _ptr(dict_length) if n_dict else None, n_dict, _ptr(index), _ptr(start), _ptr(length),
            _ptr(page_status), _ptr(page_code), _stream_ptr()))
    return index, start, length, page_status, page_code


def rle_hybrid_take_host(stream, bit_width: int, n_values: int, rows) -> Tuple[int, np.ndarray]:
    """mspa_rle_hybrid_take_host on the host: values ``rows`` (ascending, < ``n_values``) of the RLE / bit-packed hybrid
    ``stream`` (bytes) -> (0 or the code it is declined with (``_lib.RLE_E*``), int32 [len(rows)]).  Rows that do not ascend or
    are >= ``n_values`` raise (MSPA_EINVAL)."""
    stream = bytes(stream)
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    _require(rows.ndim == 1, "rows: one dimension")
    _require(-(1 << 31) <= int(bit_width) < (1 << 31) and 0 <= int(n_values), "bit_width: an int32; n_values >= 0")
    _require(len(stream) <= 0x7fffffff, "stream: less than 2 GiB")
    src = np.frombuffer(stream, dtype=np.uint8)
    out = np.full(len(rows), -1, dtype=np.int32)
    rc = int(_lib.load().mspa_rle_hybrid_take_host(src.ctypes.data if len(stream) else None, len(stream), int(bit_width), int(n_values),
                                                   rows.ctypes.data if len(rows) else None, len(rows), out.ctypes.data if len(rows) else None))
    if rc == _lib.MSPA_EINVAL:
        _lib.check(rc)
    return rc, out


def rle_hybrid_runs_device(src: torch.Tensor, offsets: torch.Tensor, nbytes: torch.Tensor, bit_widths: torch.Tensor, n_values: torch.Tensor):
    """The run tables of a batch of RLE / bit-packed hybrid streams whose values are ALL wanted (mspa_rle_hybrid_runs_device):
    stream s is ``src[offsets[s] : + nbytes[s]]`` with ``bit_widths[s]`` bits a value and ``n_values[s]`` values (int64 device
    tensors, one length).  Returns a dict, everything on the device: ``out_begin`` int64 [n + 1] (where each stream's values go
    in the expansion), ``total`` (its last entry, an int), ``status`` int32 [n] (0, ``_lib.RLE_E*``, MSPA_EINVAL for a stream
    outside ``src``), ``const_value`` int32 [n] (the value of a stream that is one RLE run, else -1), ``n_runs`` (an int) and the
    run table ``run_first`` / ``run_pos`` int64, ``run_info`` int32.  A counting launch, ONE small read-back (the sizes to
    allocate), a writing launch."""
    lib = _lib.load()
    n = _check_streams(offsets, nbytes)
    _check("src", src, torch.uint8, (None,))
    _check("bit_widths", bit_widths, torch.int64, (n,))
    _check("n_values", n_values, torch.int64, (n,))
    dev = src.device
    out_begin = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
    run_begin = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
    run_count = torch.zeros((n,), dtype=torch.int64, device=dev)
    status = torch.zeros((n,), dtype=torch.int32, device=dev)
    const_value = torch.full((n,), -1, dtype=torch.int32, device=dev)
    got = {"out_begin": out_begin, "total": 0, "status": status, "const_value": const_value, "n_runs": 0}
    for name, dtype in (("run_first", torch.int64), ("run_pos", torch.int64), ("run_info", torch.int32)):
        got[name] = torch.zeros((0,), dtype=dtype, device=dev)
    if n == 0:
        return got
    torch.cumsum(n_values.clamp(min=0), dim=0, out=out_begin[1:])     # a negative count is the kernel's to refuse (MSPA_EINVAL)

    def launch(begin, n_runs, count, st, const):
        _lib.check(lib.mspa_rle_hybrid_runs_device(_ptr(src) if src.numel() else None, src.numel(), _ptr(offsets), _ptr(nbytes), _ptr(bit_widths),
                                                   _ptr(n_values), _ptr(out_begin), _ptr(begin), n, n_runs, _ptr(count), _ptr(st), _ptr(const),
                                                   _ptr(got["run_first"]) if n_runs else None, _ptr(got["run_pos"]) if n_runs else None,
                                                   _ptr(got["run_info"]) if n_runs else None, _stream_ptr()))

    launch(None, 0, run_count, status, const_value)
    torch.cumsum(run_count, dim=0, out=run_begin[1:])
    head = torch.stack([out_begin[-1], run_begin[-1]]).cpu()
    got["total"], got["n_runs"] = int(head[0]), int(head[1])
    if got["n_runs"]:
        got["run_first"], got["run_pos"] = (torch.zeros((got["n_runs"],), dtype=torch.int64, device=dev) for _ in range(2))
        got["run_info"] = torch.full((got["n_runs"],), 2, dtype=torch.int32, device=dev)          # a slot nothing writes is a hole
        launch(run_begin, got["n_runs"], torch.empty_like(run_count), torch.empty_like(status), torch.empty_like(const_value))
    return got


def rle_hybrid_expand_device(src: torch.Tensor, runs: dict) -> torch.Tensor:
    """``rle_hybrid_runs_device``'s run tables -> every stream's values back to back, int32 [``runs["total"]``] on the device:
    what ``rle_hybrid_take_host`` gives for rows 0 .. n - 1 of each stream, -1 for the values a declined stream did not give.
    One lane per value; only enqueues."""
    _check("src", src, torch.uint8, (None,))
    n_runs, total = int(runs["n_runs"]), int(runs["total"])
    _check("run_first", runs["run_first"], torch.int64, (n_runs,))
    _check("run_pos", runs["run_pos"], torch.int64, (n_runs,))
    _check("run_info", runs["run_info"], torch.int32, (n_runs,))
    _require(total >= 0 and (n_runs > 0 or total == 0), "values need runs")
    out = torch.empty((total,), dtype=torch.int32, device=src.device)
    if total:
        _lib.check(_lib.load().mspa_rle_hybrid_expand_device(_ptr(src) if src.numel() else None, src.numel(), _ptr(runs["run_first"]),
                                                             _ptr(runs["run_pos"]), _ptr(runs["run_info"]), n_runs, _ptr(out), total,
                                                             _stream_ptr()))
    return out


def parquet_double_columns_device(pages: torch.Tensor, page_offsets: torch.Tensor, page_sizes: torch.Tensor, page_values: torch.Tensor,
                                  page_flags: torch.Tensor, page_first: torch.Tensor, n_out: int, level_offsets: torch.Tensor,
                                  level_sizes: torch.Tensor, dict_offsets: torch.Tensor, dict_count: torch.Tensor):
    """Decompressed data pages of DOUBLE column chunks -> float64 [``n_out``] on the device, nulls as NaN.  Page p is
    ``pages[page_offsets[p] : + page_sizes[p]]`` with ``page_values[p]`` rows that go to ``out[page_first[p] ..]`` (``page_first``
    ascends from 0 and the pages cover ``n_out``: several chunks are laid out one behind the other by the caller).
    ``page_flags[p]`` (int32): ``_lib.PAGE_LEVELS_INLINE`` (a v1 page: u32 length + RLE definition levels in front),
    ``_lib.PAGE_LEVELS_GIVEN`` (a v2 page: its level bytes are ``pages[level_offsets[p] : + level_sizes[p]]``),
    ``_lib.PAGE_DICT_CODED`` (a byte of bit width and hybrid indices into the PLAIN dictionary ``pages[dict_offsets[p] : + 8 *
    dict_count[p]]``); without the last the values are PLAIN.  All tables int64 but the flags.  Returns (out, status): status a
    dict of int32 device tensors [pages] -- ``layout`` (1: a length runs past the page), ``levels`` / ``indices`` (the hybrid
    streams' codes, ``_lib.RLE_E*``), ``values`` (5: a level, index or value the page does not hold) -- all zero for a column
    that was taken, plus ``null_pages`` (an int: pages whose levels are not one run of ones).  Two small read-backs."""
    lib = _lib.load()
    n_pages = _check_streams(page_offsets, page_sizes)
    _check("pages", pages, torch.uint8, (None,))
    for name, t in (("page_values", page_values), ("page_first", page_first), ("level_offsets", level_offsets), ("level_sizes", level_sizes),
                    ("dict_offsets", dict_offsets), ("dict_count", dict_count)):
        _check(name, t, torch.int64, (n_pages,))
    _check("page_flags", page_flags, torch.int32, (n_pages,))
    n_out = int(n_out)
    _require(n_out >= 0 and (n_pages > 0 or n_out == 0), "rows need pages")
    dev = pages.device
    out = torch.empty((n_out,), dtype=torch.float64, device=dev)
    zeros = torch.zeros((n_pages,), dtype=torch.int32, device=dev)
    status = {"layout": zeros, "levels": zeros, "indices": zeros, "values": zeros, "null_pages": 0}
    if n_out == 0:
        return out, status
    src = _ptr(pages) if pages.numel() else None
    layout = torch.zeros((_lib.LAYOUT_ROWS, n_pages), dtype=torch.int64, device=dev)
    layout[_lib.LAYOUT_LEVEL_OFFSET], layout[_lib.LAYOUT_LEVEL_BYTES] = level_offsets, level_sizes
    status["layout"] = torch.zeros((n_pages,), dtype=torch.int32, device=dev)
    _lib.check(lib.mspa_parquet_double_layout_device(src, pages.numel(), _ptr(page_offsets), _ptr(page_sizes), _ptr(page_flags), n_pages,
                                                     _ptr(layout), _ptr(status["layout"]), _stream_ptr()))
    # the level streams (bit width 1) and the index streams of every page, as one batch of hybrid streams
    has_levels = (page_flags & (_lib.PAGE_LEVELS_INLINE | _lib.PAGE_LEVELS_GIVEN)) != 0
    coded = (page_flags & _lib.PAGE_DICT_CODED) != 0
    ok = status["layout"] == 0
    level_values, index_values = page_values * (has_levels & ok), page_values * (coded & ok)
    head = torch.stack([level_values.sum(), index_values.sum()]).cpu()
    levels = rank = indices = None
    level_begin = index_begin = torch.zeros((n_pages,), dtype=torch.int64, device=dev)
    n_levels = n_indices = 0
    if int(head[0]):
        runs = rle_hybrid_runs_device(pages, layout[_lib.LAYOUT_LEVEL_OFFSET].contiguous(), layout[_lib.LAYOUT_LEVEL_BYTES].contiguous(),
                                      torch.ones((n_pages,), dtype=torch.int64, device=dev), level_values)
        status["levels"] = runs["status"]
        nulls = has_levels & ok & (runs["const_value"] != 1)
        status["null_pages"] = int(nulls.sum().item())
        if status["null_pages"]:                                 # otherwise every level is 1 and row r takes value r
            levels = rle_hybrid_expand_device(pages, runs)
            rank = torch.cumsum(levels, dim=0, dtype=torch.int64) - levels
            level_begin, n_levels = runs["out_begin"][:-1].contiguous(), runs["total"]
    if int(head[1]):
        runs = rle_hybrid_runs_device(pages, layout[_lib.LAYOUT_VALUE_OFFSET].contiguous(), layout[_lib.LAYOUT_VALUE_BYTES].contiguous(),
                                      layout[_lib.LAYOUT_BIT_WIDTH].contiguous(), index_values)
        # the indices of a page with nulls are fewer than its rows: its stream may end early, and the rows that need one say so
        status["indices"] = torch.where(runs["status"] == _lib.RLE_ESHORT, torch.zeros_like(runs["status"]), runs["status"])
        indices = rle_hybrid_expand_device(pages, runs)
        index_begin, n_indices = runs["out_begin"][:-1].contiguous(), runs["total"]
    status["values"] = torch.zeros((n_pages,), dtype=torch.int32, device=dev)
    _lib.check(lib.mspa_parquet_double_column_device(src, pages.numel(), _ptr(layout), _ptr(page_values), _ptr(page_flags), _ptr(page_first),
                                                     n_pages, _ptr(levels), _ptr(rank), _ptr(level_begin), n_levels, _ptr(indices),
                                                     _ptr(index_begin), n_indices, _ptr(dict_offsets), _ptr(dict_count), _ptr(out), n_out,
                                                     _ptr(status["values"]), _stream_ptr()))
    return out, status


def pair_tiles(n: int) -> int:
    """Tiles (one wave's share of rows) of an ``n``-row pair table in ``pair_bin_codes`` / ``pair_partition``."""
    rows = int(_lib.load().mspa_pair_tile_rows())
    return (int(n) + rows - 1) // rows


def pair_bin_codes_host(overlap, edges) -> Tuple[np.ndarray, np.ndarray]:
    """mspa_pair_bin_codes_host: the sampler's bin rule on the host -> (codes uint8 [n], counts int64 [256])."""
    x = np.ascontiguousarray(overlap, dtype=np.float64)
    e = np.ascontiguousarray(edges, dtype=np.float64)
    _require(x.ndim == 1 and e.ndim == 1, "overlap, edges: one dimension")
    codes, counts = np.empty(len(x), dtype=np.uint8), np.zeros(_lib.PAIR_CLASSES, dtype=np.int64)
    _lib.check(_lib.load().mspa_pair_bin_codes_host(x.ctypes.data if len(x) else None, len(x), e.ctypes.data, len(e),
                                                    codes.ctypes.data if len(x) else None, counts.ctypes.data))
    return codes, counts


def pair_bin_codes(overlap: torch.Tensor, edges: torch.Tensor):
    """The sampler's class of every row of ``overlap`` (float64 [n], n < 2^31) for the bin ``edges`` (float64 [2 .. 251], strictly
    ascending: the caller's to see to) -> (codes uint8 [n]: the bin, ``_lib.PAIR_CLASS_ZERO`` or ``_lib.PAIR_CLASS_DROPPED``;
    tile_counts int32 [tiles, 256]: rows per class in each tile of ``pair_tiles``), on the device.  Only enqueues."""
    n = _check("overlap", overlap, torch.float64, (None,)).shape[0]
    n_edges = _check("edges", edges, torch.float64, (None,)).shape[0]
    _require(2 <= n_edges <= _lib.PAIR_MAX_BINS + 1 and n <= 0x7fffffff, "2 <= edges <= 251, fewer than 2^31 rows")
    n_tiles = pair_tiles(n)
    codes = torch.empty((n,), dtype=torch.uint8, device=overlap.device)
    tile_counts = torch.zeros((n_tiles, _lib.PAIR_CLASSES), dtype=torch.int32, device=overlap.device)
    if n:
        _lib.check(_lib.load().mspa_pair_bin_codes_device(_ptr(overlap), n, _ptr(edges), n_edges, _ptr(codes), _ptr(tile_counts), n_tiles,
                                                          _stream_ptr()))
    return codes, tile_counts


def pair_partition(codes: torch.Tensor, tile_counts: torch.Tensor):
    """``pair_bin_codes``' results -> (order int32 [n], begin int64 [257]) on the device: ``order[begin[c] : begin[c + 1]]`` are
    the file rows of class c, ascending.  The scan over (class, tile) is torch's (plumbing); the scatter is the kernel's.  Only
    enqueues."""
    n = _check("codes", codes, torch.uint8, (None,)).shape[0]
    n_tiles = pair_tiles(n)
    _check("tile_counts", tile_counts, torch.int32, (n_tiles, _lib.PAIR_CLASSES))
    dev = codes.device
    begin = torch.zeros((_lib.PAIR_CLASSES + 1,), dtype=torch.int64, device=dev)
    order = torch.empty((n,), dtype=torch.int32, device=dev)
    if n == 0:
        return order, begin
    torch.cumsum(tile_counts.sum(dim=0, dtype=torch.int64), dim=0, out=begin[1:])
    in_class = torch.cumsum(tile_counts, dim=0, dtype=torch.int64) - tile_counts          # rows of the class in the tiles in front
    tile_offsets = (in_class + begin[:-1]).to(torch.int32).contiguous()
    _lib.check(_lib.load().mspa_pair_partition_device(_ptr(codes), n, _ptr(tile_offsets), n_tiles, _ptr(order), _stream_ptr()))
    return order, begin


def index_rows_to_bits(pages: torch.Tensor, page_offsets: torch.Tensor, page_sizes: torch.Tensor, page_values: torch.Tensor,
                       row_begin: torch.Tensor, row_index: torch.Tensor, n_points: Optional[int] = None, has_levels: bool = True):
    """Rows of the visibility index straight from their pages to bitset rows, on the device.  ``pages`` (uint8) holds the
    uncompressed payloads of v1 PLAIN BYTE_ARRAY data pages: page p is ``pages[page_offsets[p] : + page_sizes[p]]`` with
    ``page_values[p]`` values (``has_levels``: behind RLE definition levels that must be one run of ones).  Rows ``row_begin[p] ..
    row_begin[p + 1]`` of the row table belong to page p and ``row_index[r]`` is row r's value number inside its page, ascending
    within a page (all int64, on the device).  Each row's text must be a JSON list of ascending non-negative integers.

    mspa_parquet_plain_spans_device -> mspa_index_rows_brackets_device -> (prefix sum) -> mspa_index_rows_gather_device ->
    mspa_parse_int_list_flags_device -> (prefix sum) -> mspa_parse_int_list_device -> mspa_index_lists_to_bits_device.

    Returns a dict: ``bits`` int64 [rows, ceil(n_points / 64)] on the device (scene.pack_index_lists' layout), ``n_points``
    (given, or 1 + the largest parsed value), ``page_status`` / ``row_status`` (int32 numpy; non-zero = declined: that page's
    rows / that row belong to the host path, their ``bits`` are unspecified), ``start`` / ``length`` (int64, device: where each
    row's text lies in ``pages``).  Less than 2 GiB of list text a call.  Synchronises (three or four small read-backs)."""
    _require(n_points is None or 0 <= int(n_points) <= 0x7fffffff, "n_points: 0 <= n_points < 2^31")
    start, length, page_status = parquet_plain_spans_device(pages, page_offsets, page_sizes, page_values, row_begin, row_index, has_levels)
    return index_spans_to_bits(pages, start, length, n_points, page_status)


def _spans_to_lists(pages: torch.Tensor, start: torch.Tensor, length: torch.Tensor, page_status: Optional[torch.Tensor]):
    """THE pipeline from row spans to parsed lists, enqueued once for ``index_spans_to_lists`` and ``index_spans_to_bits``:
    brackets -> (prefix sum) -> gather -> flags -> (prefix sum) -> parse.  Returns (values int32 [max(count, 1)], count,
    offsets int64 [rows + 1], status int32 [2, max(rows, 1)] -- brackets, parser --, page_status, n_pages), all tensors on the
    device; for no rows ``values`` and ``offsets`` are None.  Two read-backs (the text's and the values' totals)."""
    lib = _lib.load()
    _check("pages", pages, torch.uint8, (None,))
    n_rows = _check("start", start, torch.int64, (None,)).shape[0]
    _check("length", length, torch.int64, (n_rows,))
    if page_status is None:
        page_status = torch.zeros((0,), dtype=torch.int32, device=pages.device)
    n_pages = _check("page_status", page_status, torch.int32, (None,)).shape[0]
    dev, st = pages.device, _stream_ptr()
    i64 = dict(dtype=torch.int64, device=dev)
    status = torch.zeros((2, max(n_rows, 1)), dtype=torch.int32, device=dev)                 # brackets, parser
    if n_rows == 0:
        return None, 0, None, status, page_status, n_pages
    inner_start, inner_len = torch.empty((n_rows,), **i64), torch.empty((n_rows,), **i64)
    pages_ptr = _ptr(pages) if pages.numel() else None
    _lib.check(lib.mspa_index_rows_brackets_device(pages_ptr, pages.numel(), _ptr(start), _ptr(length), n_rows, _ptr(inner_start),
                                                   _ptr(inner_len), _ptr(status[0]), st))
    prefix = torch.zeros((n_rows + 1,), **i64)                                                # torch as plumbing: the prefix sums
    torch.cumsum(inner_len, dim=0, out=prefix[1:])
    n_bytes = int(prefix[-1].item())
    _require(n_bytes <= 0x7fffffff, "index_rows_to_bits: 2 GiB of list text or more in one call")
    text = torch.empty((max(n_bytes, 1),), dtype=torch.uint8, device=dev)
    _lib.check(lib.mspa_index_rows_gather_device(pages_ptr, pages.numel(), _ptr(inner_start), _ptr(prefix), n_rows, _ptr(text), n_bytes, st))
    flags = torch.empty((max(n_bytes, 1),), **i64)
    _lib.check(lib.mspa_parse_int_list_flags_device(_ptr(text), _ptr(prefix), n_rows, n_bytes, _ptr(flags), _ptr(status[1]), st))
    T = torch.zeros((n_bytes + 1,), **i64)
    if n_bytes:
        torch.cumsum(flags[:n_bytes], dim=0, out=T[1:])
    del flags
    count = int(T[-1].item()) & 0xffffffff
    values = torch.empty((max(count, 1),), dtype=torch.int32, device=dev)
    offsets = torch.empty((n_rows + 1,), **i64)
    _lib.check(lib.mspa_parse_int_list_device(_ptr(text), _ptr(prefix), n_rows, n_bytes, _ptr(T), None, _ptr(values), count, _ptr(offsets),
                                              _ptr(status[1]), st))
    return values, count, offsets, status, page_status, n_pages


def index_spans_to_lists(pages: torch.Tensor, start: torch.Tensor, length: torch.Tensor, page_status: Optional[torch.Tensor] = None):
    """``index_spans_to_bits`` one step short: the rows as LISTS, for the readers that take ``len(row)`` and ``row[j]`` (a
    duplicate counts, the order is the text's -- neither survives a bitset).  Row r's text is ``pages[start[r] : start[r] +
    length[r]]``.  Returns a dict: ``values`` int32 [n] and ``offsets`` int64 [rows + 1] on the device (CSR: row r is
    ``values[offsets[r] : offsets[r + 1]]`` -- what ``index_lists_pick`` takes), ``counts`` (int64 numpy, ``diff(offsets)``),
    ``row_status`` (int32 numpy: brackets | parser; a declined row has count 0 and belongs to the host path), ``page_status``
    (int32 numpy), ``n_points`` (1 + the largest parsed value: the width ``index_spans_to_bits`` takes for ``n_points=None``),
    ``start`` / ``length``.  Synchronises: the pipeline's two totals and ONE read-back of statuses, counts and width."""
    values, count, offsets, status, page_status, n_pages = _spans_to_lists(pages, start, length, page_status)
    n_rows = start.shape[0]
    if n_rows == 0:
        dev = pages.device
        return {"values": torch.zeros((0,), dtype=torch.int32, device=dev), "offsets": torch.zeros((1,), dtype=torch.int64, device=dev),
                "counts": np.zeros(0, np.int64), "row_status": np.zeros(0, np.int32), "page_status": np.zeros(n_pages, np.int32), "n_points": 1,
                "start": start, "length": length}
    values = values[:count]
    top = values.max().to(torch.int64).reshape(1) if count else torch.zeros((1,), dtype=torch.int64, device=pages.device)
    back = torch.cat([page_status.to(torch.int64), (status[0] | status[1])[:n_rows].to(torch.int64), offsets[1:] - offsets[:-1], top]).cpu().numpy()
    return {"values": values, "offsets": offsets, "counts": back[n_pages + n_rows:-1].copy(),
            "row_status": back[n_pages:n_pages + n_rows].astype(np.int32), "page_status": back[:n_pages].astype(np.int32),
            "n_points": int(back[-1]) + 1, "start": start, "length": length}


def index_rows_to_lists(pages: torch.Tensor, page_offsets: torch.Tensor, page_sizes: torch.Tensor, page_values: torch.Tensor,
                        row_begin: torch.Tensor, row_index: torch.Tensor, has_levels: bool = True):
    """``index_rows_to_bits`` for the readers of lists: the same pages and tables -> ``index_spans_to_lists``' dict."""
    start, length, page_status = parquet_plain_spans_device(pages, page_offsets, page_sizes, page_values, row_begin, row_index, has_levels)
    return index_spans_to_lists(pages, start, length, page_status)


def index_lists_pick(values: torch.Tensor, offsets: torch.Tensor, samples: torch.Tensor, n_points: int):
    """Element ``position`` of row ``row`` for every sample (mspa_index_lists_pick_device): ``values`` int32 [n] / ``offsets``
    int64 [rows + 1] as ``index_spans_to_lists`` leaves them, ``samples`` int64 [n_samples, 2] (row, position), all on the device
    -> (vertex int32 [n_samples], status int32 [n_samples]) on the device.  Status 0: ``vertex = values[offsets[row] +
    position]``; otherwise vertex -1 and ``_lib.PICK_EROW`` (1, no such row), ``PICK_EPOSITION`` (2, outside the list),
    ``PICK_ERANGE`` (4, the value is outside [0, n_points)) or ``PICK_EOFFSETS`` (8, the row's offsets leave ``values``).  Only
    enqueues: the caller reads ``status`` before a vertex goes anywhere that indexes with it (``project_samples``)."""
    n_values = _check("values", values, torch.int32, (None,)).shape[0]
    n_rows = _check("offsets", offsets, torch.int64, ((1,),)).shape[0] - 1
    n = _check("samples", samples, torch.int64, (None, 2)).shape[0]
    _require(0 <= int(n_points) <= 0x7fffffff, "n_points: 0 <= n_points < 2^31")
    vertex = torch.empty((n,), dtype=torch.int32, device=values.device)
    status = torch.empty((n,), dtype=torch.int32, device=values.device)
    if n:
        _lib.check(_lib.load().mspa_index_lists_pick_device(_ptr(values) if n_values else None, n_values, _ptr(offsets), n_rows, _ptr(samples), n,
                                                            int(n_points), _ptr(vertex), _ptr(status), _stream_ptr()))
    return vertex, status


def index_spans_to_bits(pages: torch.Tensor, start: torch.Tensor, length: torch.Tensor, n_points: Optional[int] = None,
                        page_status: Optional[torch.Tensor] = None):
    """``index_rows_to_bits`` behind the span kernels: row r's text is ``pages[start[r] : start[r] + length[r]]`` (int64, on the
    device -- from ``parquet_plain_spans_device``, ``parquet_dict_spans_device`` or both merged) -> the same dict;
    ``page_status`` (int32, device) rides along in the read-back of the rows' status.  The lists come from the pipeline
    ``index_spans_to_lists`` runs; mspa_index_lists_to_bits_device follows."""
    _require(n_points is None or 0 <= int(n_points) <= 0x7fffffff, "n_points: 0 <= n_points < 2^31")
    values, count, offsets, status, page_status, n_pages = _spans_to_lists(pages, start, length, page_status)
    n_rows = start.shape[0]
    i64 = dict(dtype=torch.int64, device=pages.device)
    if n_rows == 0:
        n_points = int(n_points or 1)
        return {"bits": torch.zeros((0, (n_points + 63) // 64), **i64), "n_points": n_points, "page_status": np.zeros(n_pages, np.int32),
                "row_status": np.zeros(0, np.int32), "start": start, "length": length}
    if n_points is None:
        n_points = (int(values[:count].max().item()) if count else 0) + 1
    n_points = int(n_points)
    n_words = (n_points + 63) // 64
    bits = torch.empty((n_rows, n_words), **i64)
    bits_status = torch.zeros((n_rows,), dtype=torch.int32, device=pages.device)
    _lib.check(_lib.load().mspa_index_lists_to_bits_device(_ptr(values), count, _ptr(offsets), n_rows, n_points, _ptr(bits) if n_words else None,
                                                           n_words, _ptr(bits_status), _stream_ptr()))
    row_status = (status[0] | status[1])[:n_rows] | bits_status
    back = torch.cat([page_status, row_status]).cpu().numpy()
    return {"bits": bits, "n_points": n_points, "page_status": back[:n_pages], "row_status": back[n_pages:], "start": start, "length": length}


def bits_transpose(bits: torch.Tensor) -> torch.Tensor:
    """K9: [R, n_words] int64 bit matrix -> its transpose [n_words * 64, ceil(R / 64)] (padding bits zero)."""
    R, n_words = _check_bits("bits", bits)
    out = torch.empty((n_words * 64, (R + 63) // 64), dtype=torch.int64, device=bits.device)
    if R and n_words:
        _lib.check(_lib.load().mspa_bits_transpose(_ptr(bits), R, n_words, _ptr(out), _stream_ptr()))
    else:
        out.zero_()
    return out


def extract_yaw_pitch_host(E_aligned_list: Sequence[np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
    """Per-frame angles as CFR:86-100 computes them, with NumPy on the host (the reference's own libm / BLAS calls are the
    only way to be bit-identical with it).  The arctan2 / arcsin / degrees ufuncs run once over all frames (the same
    element loops a scalar call goes through); the norm stays one ``dot`` per frame, because that is what
    ``np.linalg.norm`` of a 3-vector is and a vectorised sum of squares rounds differently.  tests/test_host_cpu.py holds
    this against the oracle's literal per-frame form bit for bit."""
    n = len(E_aligned_list)
    if n == 0:
        return np.zeros(0, dtype=np.float64), np.zeros(0, dtype=np.float64)
    Z = np.ascontiguousarray(np.stack([np.asarray(E) for E in E_aligned_list])[:, :3, 2], dtype=np.float64)
    yaw = np.degrees(np.arctan2(Z[:, 1], Z[:, 0]))
    norm = np.sqrt(np.array([z.dot(z) for z in Z], dtype=np.float64))       # np.linalg.norm(z) == sqrt(z.dot(z)) for real 1-D z
    pitch = np.degrees(np.arcsin(Z[:, 2] / norm))
    return yaw, pitch


def extract_yaw_pitch(E_aligned: torch.Tensor):
    """Device form of CFR:86-100 for frames that are already resident: E_aligned [F,16] f64 -> (yaw [F], pitch [F]) in
    degrees.  Within a few ulp of ``extract_yaw_pitch_host`` (device libm is not glibc); the pair-table writers keep the
    host path so that the parquet columns are the reference's bits."""
    F = _check("E_aligned", E_aligned, torch.float64, (None, 16)).shape[0]
    yaw = torch.empty((F,), dtype=torch.float64, device=E_aligned.device)
    pitch = torch.empty((F,), dtype=torch.float64, device=E_aligned.device)
    _lib.check(_lib.load().mspa_extract_yaw_pitch(_ptr(E_aligned), F, _ptr(yaw), _ptr(pitch), _stream_ptr()))
    return yaw, pitch


def pair_pose(E_aligned: torch.Tensor, Einv_aligned: torch.Tensor, yaw: torch.Tensor, pitch: torch.Tensor,
              pairs: torch.Tensor) -> torch.Tensor:
    """Enqueue K4.  E_aligned / Einv_aligned [F,16] f64, yaw / pitch [F] f64, pairs [n,2] i32 ->
    [n,6] f64: distance, dyaw, dpitch, translation of inv(E_i) @ E_j."""
    F = _check("E_aligned", E_aligned, torch.float64, (None, 16)).shape[0]
    _check("Einv_aligned", Einv_aligned, torch.float64, (F, 16))
    _check("yaw", yaw, torch.float64, (F,))
    _check("pitch", pitch, torch.float64, (F,))
    n = _check("pairs", pairs, torch.int32, (None, 2)).shape[0]
    out = torch.empty((n, 6), dtype=torch.float64, device=E_aligned.device)
    _lib.check(_lib.load().mspa_pair_pose(_ptr(E_aligned), _ptr(Einv_aligned), _ptr(yaw), _ptr(pitch), F, _ptr(pairs),
                                          n, _ptr(out), _stream_ptr()))
    return out


def _check_tracks(name: str, tracks) -> Tuple[int, int]:
    """Track points, float64 [T, P, 3] (camera space, or K5a's world positions) -> (T, P)."""
    return tuple(_check(name, tracks, torch.float64, (None, None, 3)).shape[:2])


def track_to_world(tracks_xyz: torch.Tensor, c2w: Optional[torch.Tensor], fx_fy_cx_cy: Sequence[float],
                   image_hw: Tuple[int, int], want=("world", "uvn", "ok")) -> Dict[str, torch.Tensor]:
    """Enqueue K5a.  tracks_xyz [T,P,3] f64, c2w [T,16] f64 (np.linalg.inv(extrinsics_w2c) on the host)."""
    T, P = _check_tracks("tracks_xyz", tracks_xyz)
    if c2w is not None:
        _check("c2w", c2w, torch.float64, (T, 16))
    _require(len(fx_fy_cx_cy) == 4, f"fx_fy_cx_cy: four numbers, got {len(fx_fy_cx_cy)}")
    out = _alloc_wanted(want, {"world": ((T, P, 3), torch.float64), "uvn": ((T, P, 2), torch.float64),
                               "ok": ((T, P), torch.uint8)}, tracks_xyz.device)
    intr = (ctypes.c_double * 4)(*[float(v) for v in fx_fy_cx_cy])
    H, W = image_hw
    _lib.check(_lib.load().mspa_track_to_world(_ptr(tracks_xyz), _ptr(c2w), T, P, intr, H, W, _ptr(out.get("world")),
                                               _ptr(out.get("uvn")), _ptr(out.get("ok")), _stream_ptr()))
    return out


def track_displacement(world: torch.Tensor, w2c: torch.Tensor, c2w: torch.Tensor, triples: torch.Tensor,
                       obj_threshold: float = 0.01, cam_threshold: float = 0.01):
    """Enqueue K5b.  Returns ([n,5] f64: distance, dx, dy, dz (camera-1 axes), binning distance;
    [n,2] u8: point_moving, cam_moving)."""
    T, P = _check_tracks("world", world)
    _check("w2c", w2c, torch.float64, (T, 16))
    _check("c2w", c2w, torch.float64, (T, 16))
    n = _check("triples", triples, torch.int32, (None, 3)).shape[0]
    out = torch.empty((n, 5), dtype=torch.float64, device=world.device)
    flags = torch.empty((n, 2), dtype=torch.uint8, device=world.device)
    _lib.check(_lib.load().mspa_track_displacement(_ptr(world), _ptr(w2c), _ptr(c2w), T, P, _ptr(triples), n,
                                                   obj_threshold, cam_threshold, _ptr(out), _ptr(flags), _stream_ptr()))
    return out, flags


def check_visibility(uv: torch.Tensor, point_depth: Optional[torch.Tensor], depth_image: Optional[torch.Tensor],
                     image_hw: Tuple[int, int], want=("visible",), depth_scale: float = 0.001) -> Dict[str, torch.Tensor]:
    """The reference's three predicates on already-projected points (IH:337-386)."""
    n = _check("uv", uv, torch.float64, (None, 2)).shape[0]
    if point_depth is not None:
        _check("point_depth", point_depth, torch.float64, (n,))
    dh, dw = _check("depth_image", depth_image, _DEPTH, (None, None)).shape if depth_image is not None else (0, 0)
    flags = ((n,), torch.uint8)
    out = _alloc_wanted(want, {"in_bounds": flags, "by_depth": flags, "visible": flags}, uv.device)
    H, W = image_hw
    _lib.check(_lib.load().mspa_check_visibility_ex(_ptr(uv), _ptr(point_depth), n, _ptr(depth_image), dh, dw, H, W, float(depth_scale),
                                                    _ptr(out.get("in_bounds")), _ptr(out.get("by_depth")),
                                                    _ptr(out.get("visible")), _stream_ptr()))
    return out


def select_common_point(bits: torch.Tensor, selections: torch.Tensor) -> torch.Tensor:
    """Enqueue K6a.  bits [F, n_words] int64 (K1), selections [n, 3] int32 (image1, image2, j) ->
    [n] int32 vertex index: element j of np.intersect1d of the two visible lists (-1 if out of range)."""
    F, n_words = _check_bits("bits", bits)
    n = _check("selections", selections, torch.int32, (None, 3), contiguous=False).shape[0]
    selections = selections.contiguous()        # a copy, if one is made, has to outlive the launch: a named tensor, not a temporary
    out = torch.empty((n,), dtype=torch.int32, device=bits.device)
    _lib.check(_lib.load().mspa_select_common_point(_ptr(bits), F, n_words, _ptr(selections), n, _ptr(out), _stream_ptr()))
    return out


def project_samples(xyz: torch.Tensor, cam_mats: torch.Tensor, depth: torch.Tensor, image_hw: Tuple[int, int],
                    samples: torch.Tensor, depth_scale: float = 0.001):
    """Enqueue K6b.  samples [n, 2] int32 (vertex, image) -> (uv [n,2] f64, depth [n] f64, visible [n] u8)."""
    I, DH, DW = _check_cameras(xyz, cam_mats, depth)
    n = _check("samples", samples, torch.int32, (None, 2), contiguous=False).shape[0]
    samples = samples.contiguous()              # named, as in select_common_point
    dev = xyz.device
    uv = torch.empty((n, 2), dtype=torch.float64, device=dev)
    d = torch.empty((n,), dtype=torch.float64, device=dev)
    vis = torch.empty((n,), dtype=torch.uint8, device=dev)
    H, W = image_hw
    _lib.check(_lib.load().mspa_project_samples_ex(xyz.data_ptr(), xyz.shape[0], xyz.stride(0), xyz.stride(1), _ptr(cam_mats), I,
                                                   _ptr(depth), DH, DW, H, W, float(depth_scale), _ptr(samples), n,
                                                   _ptr(uv), _ptr(d), _ptr(vis), _stream_ptr()))
    return uv, d, vis


def track_rigidity_loss(tracks_xyz: torch.Tensor, smoothing_factor: float = 0.01) -> torch.Tensor:
    """Enqueue K7: [T,P,3] f64 tracks -> [P,P] f64 accumulated thresholded distance change (OM_C:66-78)."""
    T, P = _check_tracks("tracks_xyz", tracks_xyz)
    out = torch.empty((P, P), dtype=torch.float64, device=tracks_xyz.device)
    _lib.check(_lib.load().mspa_track_rigidity_loss(_ptr(tracks_xyz), T, P, float(smoothing_factor), _ptr(out), _stream_ptr()))
    return out


def track_rigidity_loss_batch(tracks_xyz: torch.Tensor, smoothing_factor: float = 0.01) -> torch.Tensor:
    """Enqueue K7 for equal-shape track blocks in one launch: [B,T,P,3] f64 -> [B,P,P] f64, each the single form's matrix."""
    B, T, P, _ = _check("tracks_xyz", tracks_xyz, torch.float64, (None, None, None, 3)).shape
    out = torch.empty((B, P, P), dtype=torch.float64, device=tracks_xyz.device)
    _lib.check(_lib.load().mspa_track_rigidity_loss_batch(_ptr(tracks_xyz), B, T, P, float(smoothing_factor), _ptr(out), _stream_ptr()))
    return out


def linkage_backend() -> str:
    """Where the object-movement callers run linkage + fcluster: "scipy" (default: on the host, on the downloaded K7 matrix) or
    "device" (``MSPA_LINKAGE=device``: K7b, identical to SciPy).  Read at every call."""
    value = os.environ.get("MSPA_LINKAGE", "scipy").strip().lower() or "scipy"
    if value not in ("scipy", "device"):
        raise ValueError(f"MSPA_LINKAGE={value!r}: expected 'scipy' or 'device'")
    return value


LINKAGE_NONFINITE_TEXT = "The condensed distance matrix must contain only finite values."      # SciPy's, for status 1


def track_linkage(loss: torch.Tensor, threshold: float = 0.1):
    """Enqueue K7b: SciPy's ``linkage(squareform(loss, checks=False), 'average')`` and ``fcluster(Z, threshold, 'distance')`` of
    K7 matrices, one workgroup per matrix.  loss [P,P] or [B,P,P] f64 (left untouched) -> (Z [.., P-1, 4] f64 bit for bit SciPy's,
    labels [.., P] i32, status [..] i32: 0 ok, 1 a non-finite entry (SciPy raises there), 2 iteration cap).  Enqueue only: the
    status is a device tensor like the rest.  P < 2 has no merge: Z is empty, a single point gets label 1."""
    lib = _lib.load()
    single = isinstance(loss, torch.Tensor) and loss.dim() == 2
    _check("loss", loss, torch.float64, (None, None) if single else (None, None, None))
    _require(loss.shape[-1] == loss.shape[-2], f"loss: square matrices [P, P] or [B, P, P], got {list(loss.shape)}")
    B, P = (1 if single else loss.shape[0]), loss.shape[-1]
    dev = loss.device
    status = torch.zeros((B,), dtype=torch.int32, device=dev)
    if P < 2:
        Z = torch.zeros((B, 0, 4), dtype=torch.float64, device=dev)
        labels = torch.ones((B, P), dtype=torch.int32, device=dev)
    else:
        Z = torch.empty((B, P - 1, 4), dtype=torch.float64, device=dev)
        labels = torch.empty((B, P), dtype=torch.int32, device=dev)
        need = lib.mspa_track_linkage_workspace_bytes(B, P)
        if need < 0:
            raise _lib.MspaError(_lib.MSPA_EINVAL, f"track_linkage: {P} points, at most {_lib.LINKAGE_MAX_POINTS} are supported")
        ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
        _lib.check(lib.mspa_track_linkage(_ptr(loss), B, P, float(threshold), _ptr(Z), _ptr(labels), _ptr(status), _ptr(ws), need,
                                          _stream_ptr()))
    return (Z[0], labels[0], status[0]) if single else (Z, labels, status)


def track_rigid_groups(tracks_xyz: torch.Tensor, threshold: float = 0.1, smoothing_factor: float = 0.01):
    """rigid_body_segmentation (OM_C:49-92) with both halves on the device: K7, then K7b, and only the labels (4 P bytes) and
    the status come back.  [T,P,3] f64 tracks -> the reference's list of index lists (``np.where(labels == i)`` for i = 1..max).
    Raises what SciPy raises: ValueError for a non-finite distance and for fewer than two points."""
    _check_tracks("tracks_xyz", tracks_xyz)
    if tracks_xyz.shape[1] < 2:
        raise ValueError("The number of observations cannot be determined on an empty distance matrix.")
    _, labels, status = track_linkage(track_rigidity_loss(tracks_xyz, smoothing_factor), threshold)
    host = torch.cat([labels, status.reshape(1)]).cpu().numpy()
    labels, status = host[:-1], int(host[-1])
    if status == _lib.LINKAGE_NONFINITE:
        raise ValueError(LINKAGE_NONFINITE_TEXT)
    if status != _lib.LINKAGE_OK:
        raise RuntimeError(f"track_linkage: status {status} (iteration cap reached: a bug in the kernel's tie rules)")
    return [np.where(labels == i)[0].tolist() for i in range(1, int(labels.max()) + 1)]


def object_extents(vis_bits: torch.Tensor, xyz: torch.Tensor, obj_offsets: torch.Tensor, obj_vertices: torch.Tensor):
    """Enqueue K8: per (object, image) min / max xyz of the object's visible vertices and their count.
    vis_bits [F, n_words] int64, xyz [V,3] f64, objects as CSR (int32).  Returns (lo [O,F,3], hi [O,F,3], count [O,F])."""
    F, n_words = _check_bits("vis_bits", vis_bits)
    _check("xyz", xyz, torch.float64, (None, 3))
    O = _check("obj_offsets", obj_offsets, torch.int32, ((1,),)).numel() - 1
    _check("obj_vertices", obj_vertices, torch.int32, (None,))
    dev = vis_bits.device
    lo = torch.empty((O, F, 3), dtype=torch.float64, device=dev)
    hi = torch.empty((O, F, 3), dtype=torch.float64, device=dev)
    count = torch.empty((O, F), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().mspa_object_extents(_ptr(vis_bits), F, n_words, _ptr(xyz), xyz.shape[0], _ptr(obj_offsets),
                                               _ptr(obj_vertices), obj_vertices.numel(), O, _ptr(lo), _ptr(hi), _ptr(count),
                                               _stream_ptr()))
    return lo, hi, count


def track_pair_distances(world: torch.Tensor, points: Sequence[int], visible_frames: Sequence[np.ndarray]):
    """K5c: for each selected point, the distances between its world positions in every two of its visible
    frames (i < j, row-major).  Returns a list of float64 NumPy arrays, one per point (n(n-1)/2 entries).  Synchronises the
    current stream: four small tables go up from pageable memory and the distances come back to the host."""
    T, P = _check_tracks("world", world)
    S = len(points)
    if S == 0:
        return []
    lens = np.array([len(v) for v in visible_frames], dtype=np.int64)
    f_off = np.zeros(S + 1, dtype=np.int64)
    f_off[1:] = np.cumsum(lens)
    o_off = np.zeros(S + 1, dtype=np.int64)
    o_off[1:] = np.cumsum(lens * (lens - 1) // 2)
    dev = world.device
    frames = np.concatenate([np.asarray(v, dtype=np.int32) for v in visible_frames]) if f_off[-1] else np.zeros(0, np.int32)
    if frames.size and (frames.min() < 0 or frames.max() >= T):
        raise ValueError("frame index outside the track")
    pts = np.asarray(points, dtype=np.int32)
    if pts.min() < 0 or pts.max() >= P:
        raise ValueError("point index outside the track")
    out = torch.empty((int(o_off[-1]),), dtype=torch.float64, device=dev)
    if o_off[-1]:
        # named tensors: a temporary would be freed (and its block reused by the next upload) before the launch
        pts_t = torch.from_numpy(pts).to(dev)
        f_off_t = torch.from_numpy(f_off.astype(np.int32)).to(dev)
        frames_t = torch.from_numpy(frames).to(dev)
        o_off_t = torch.from_numpy(o_off).to(dev)
        _lib.check(_lib.load().mspa_track_pair_distances(_ptr(world), T, P, _ptr(pts_t), _ptr(f_off_t), _ptr(frames_t), S,
                                                         int(lens.max()), _ptr(o_off_t), _ptr(out), _stream_ptr()))
    host = out.cpu().numpy()
    return [host[o_off[s]:o_off[s + 1]] for s in range(S)]


# ---- K5d: the pair mining of the object-movement head (csrc/track_mining.hip) -----------------------------------------------------------

TRACK_MINING_BUDGET_BYTES = 1 << 30      # (key, payload) ping-pong of the selected points ordered in one launch: 24 B per moving pair
TRACK_MINING_PAIR_BYTES = 24


def track_mining_backend() -> str:
    """Where ``heads.object_movement_mine_pairs`` classifies, orders and picks a scene's frame pairs: "host" (default: K5c's
    distances downloaded, NumPy on them) or "device" (``MSPA_TRACK_MINING=device``: K5d, the same pairs and draws).  Read at
    every call."""
    value = os.environ.get("MSPA_TRACK_MINING", "host").strip().lower() or "host"
    if value not in ("host", "device"):
        raise ValueError(f"MSPA_TRACK_MINING={value!r}: expected 'host' or 'device'")
    return value


def track_pair_stats(world: torch.Tensor, visibility: torch.Tensor, points: torch.Tensor, object_not_moving_threshold: float = 0.01,
                     future_frame_windows: float = 1e8) -> Dict[str, torch.Tensor]:
    """Enqueue K5d's statistics.  world [T,P,3] f64 (K5a), visibility [T,P] u8, points [n] i32 -> the state the other three calls
    read: ``frames`` [n,T] i32 and ``positions`` [n,T,3] f64 (a point's visible frames and its positions there: the first V of a
    row) and ``stats`` [n,6] i64 (``_lib.TRACK_STAT_*``: V, static and moving pairs, the bits of the smallest and the largest
    moving distance, flags)."""
    T, P = _check_tracks("world", world)
    _require(T <= _lib.TRACK_MAX_FRAMES, f"world: at most {_lib.TRACK_MAX_FRAMES} frames, got {T}")
    _check("visibility", visibility, torch.uint8, (T, P))
    n = _check("points", points, torch.int32, (None,)).shape[0]
    dev = world.device
    state = {"frames": torch.empty((n, T), dtype=torch.int32, device=dev), "positions": torch.empty((n, T, 3), dtype=torch.float64, device=dev),
             "stats": torch.empty((n, _lib.TRACK_STAT_WORDS), dtype=torch.int64, device=dev)}
    _lib.check(_lib.load().mspa_track_pair_stats(_ptr(world), _ptr(visibility), T, P, _ptr(points), n, float(object_not_moving_threshold),
                                                 float(future_frame_windows), _ptr(state["frames"]), _ptr(state["positions"]),
                                                 _ptr(state["stats"]), _stream_ptr()))
    return state


def _check_track_state(state) -> Tuple[int, int]:
    """What ``track_pair_stats`` returned -> (n, T)."""
    _require(isinstance(state, dict) and {"frames", "positions", "stats"} <= set(state), "state: the dict track_pair_stats returned")
    n, T = _check("state[frames]", state["frames"], torch.int32, (None, None)).shape
    _check("state[positions]", state["positions"], torch.float64, (n, T, 3))
    _check("state[stats]", state["stats"], torch.int64, (n, _lib.TRACK_STAT_WORDS))
    return n, T


def track_pair_bin_counts(state: Dict[str, torch.Tensor], edges: torch.Tensor, object_not_moving_threshold: float = 0.01,
                          future_frame_windows: float = 1e8) -> torch.Tensor:
    """Enqueue K5d's second pass: edges [n,11] f64 (``np.histogram_bin_edges`` of each point's smallest and largest moving distance)
    -> [n,10] i32, the moving pairs per bin (``np.digitize``, then ``min(.., 9)``)."""
    n, T = _check_track_state(state)
    _check("edges", edges, torch.float64, (n, _lib.TRACK_BINS + 1))
    out = torch.empty((n, _lib.TRACK_BINS), dtype=torch.int32, device=edges.device)
    _lib.check(_lib.load().mspa_track_pair_bin_counts(_ptr(state["frames"]), _ptr(state["positions"]), _ptr(state["stats"]), T, n, _ptr(edges),
                                                      float(object_not_moving_threshold), float(future_frame_windows), _ptr(out), _stream_ptr()))
    return out


def track_pair_sort(keys: torch.Tensor, payload: torch.Tensor, seg_offsets: torch.Tensor, payload_ordered: bool = False) -> None:
    """Enqueue K5d's segmented sort on its own, in place: keys [2,N] i64 (bit patterns, compared UNSIGNED) and payload [2,N] i32
    (likewise); row 0 holds the data and the result, row 1 is scratch.  Segment s is [seg_offsets[s], seg_offsets[s+1]) (i64, on
    the device), ordered by (key, payload).  ``payload_ordered``: every segment ascends in its payload already."""
    N = _check("keys", keys, torch.int64, (2, None)).shape[1]
    _check("payload", payload, torch.int32, (2, N))
    n_seg = _check("seg_offsets", seg_offsets, torch.int64, ((1,),)).shape[0] - 1
    _lib.check(_lib.load().mspa_track_pair_sort(_ptr(keys), _ptr(payload), _ptr(seg_offsets), n_seg, N, int(bool(payload_ordered)), _stream_ptr()))


def track_pair_order(state: Dict[str, torch.Tensor], rows: torch.Tensor, seg_offsets: torch.Tensor, n_total: int,
                     object_not_moving_threshold: float = 0.01, future_frame_windows: float = 1e8) -> Tuple[torch.Tensor, torch.Tensor]:
    """Enqueue K5d's order: rows [s] i32 (rows of the state: the selected points), seg_offsets [s+1] i64 (running sum of their
    moving counts, ``n_total`` its last entry) -> (keys [2,n_total] i64, payload [2,n_total] i32); row 0 holds every selected point's
    moving pairs as (bits of d, (i << 16) | j) in ascending order, row 1 is the sort's scratch."""
    n, T = _check_track_state(state)
    s = _check("rows", rows, torch.int32, (None,)).shape[0]
    _check("seg_offsets", seg_offsets, torch.int64, (s + 1,))
    n_total = int(n_total)
    _require(n_total >= 0, f"n_total: not negative, got {n_total}")
    keys = torch.empty((2, n_total), dtype=torch.int64, device=rows.device)
    payload = torch.empty((2, n_total), dtype=torch.int32, device=rows.device)
    _lib.check(_lib.load().mspa_track_pair_order(_ptr(state["frames"]), _ptr(state["positions"]), _ptr(state["stats"]), T, n, _ptr(rows),
                                                 _ptr(seg_offsets), s, n_total, float(object_not_moving_threshold), float(future_frame_windows),
                                                 _ptr(keys), _ptr(payload), _stream_ptr()))
    return keys, payload


def track_pair_resolve(state: Dict[str, torch.Tensor], bin_counts: torch.Tensor, rows: torch.Tensor, seg_offsets: torch.Tensor,
                       payload: torch.Tensor, picks: np.ndarray, class_counts: np.ndarray, object_not_moving_threshold: float = 0.01,
                       future_frame_windows: float = 1e8) -> torch.Tensor:
    """Enqueue K5d's resolve: picks [k,3] i32 ON THE HOST (selected point, class 0..9 a bin / 10 static, rank) and class_counts
    [s,11] i32 on the host (the classes' sizes: a rank outside them is refused before any launch) -> [k,2] i32 (frame1, frame2) on
    the device.  ``payload`` is ``track_pair_order``'s.  The picks go up from pageable memory, which waits for the current stream:
    of the K5d calls this one does not return before the work in front of it has run."""
    n, T = _check_track_state(state)
    _check("bin_counts", bin_counts, torch.int32, (n, _lib.TRACK_BINS))
    s = _check("rows", rows, torch.int32, (None,)).shape[0]
    _check("seg_offsets", seg_offsets, torch.int64, (s + 1,))
    n_total = _check("payload", payload, torch.int32, (2, None)).shape[1]
    picks = np.ascontiguousarray(picks, dtype=np.int32)
    class_counts = np.ascontiguousarray(class_counts, dtype=np.int32)
    _require(picks.ndim == 2 and picks.shape[1] == 3, f"picks: a host array [k, 3], got {list(picks.shape)}")
    _require(class_counts.shape == (s, _lib.TRACK_CLASSES), f"class_counts: a host array [{s}, {_lib.TRACK_CLASSES}], got {list(class_counts.shape)}")
    k = picks.shape[0]
    out = torch.empty((k, 2), dtype=torch.int32, device=rows.device)
    picks_dev = torch.from_numpy(picks).to(rows.device)                    # named: alive until the launch is enqueued
    _lib.check(_lib.load().mspa_track_pair_resolve(_ptr(state["frames"]), _ptr(state["positions"]), _ptr(state["stats"]), _ptr(bin_counts), T, n,
                                                   _ptr(rows), _ptr(seg_offsets), s, _ptr(payload), n_total, picks.ctypes.data,
                                                   class_counts.ctypes.data, _ptr(picks_dev), k, float(object_not_moving_threshold),
                                                   float(future_frame_windows), _ptr(out), _stream_ptr()))
    return out


# ---- K11: ScanNet instance data from raw scans (csrc/scene_prep.hip) -----------------------------------------------------------------

def _ragged_offsets(counts: Sequence[int]) -> np.ndarray:
    off = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(np.asarray(counts, dtype=np.int64), out=off[1:])
    return off


def prep_spans(n_vertices: Sequence[int], device) -> dict:
    """The two offset tables every K11 launch shares: ``vert_off`` (prefix sum of the scenes' vertex counts) and ``word_off`` (prefix
    sum of ceil(N / 64): a wave works on 64 consecutive vertices of one scene)."""
    n = np.asarray(n_vertices, dtype=np.int64)
    _require(n.ndim == 1 and (n >= 0).all(), "vertex counts: non-negative, one per scene")
    vert_off, word_off = _ragged_offsets(n), _ragged_offsets((n + 63) // 64)
    return {"n_scenes": int(n.size), "n_vertices": int(vert_off[-1]), "n_waves": int(word_off[-1]), "max_words": int(((n + 63) // 64).max()) if n.size else 0,
            "vert_off_host": vert_off, "vert_off": torch.from_numpy(vert_off).to(device), "word_off": torch.from_numpy(word_off).to(device)}


def _check_spans(spans: dict) -> Tuple[int, int]:
    """The ``prep_spans`` tables as the K11 launches read them -> (n_scenes, n_vertices)."""
    for k in ("vert_off", "word_off"):
        _check(f"spans[{k!r}]", spans[k], torch.int64, (spans["n_scenes"] + 1,))
    return spans["n_scenes"], spans["n_vertices"]


def prep_labels(spans: dict, seg: torch.Tensor, tab_off: torch.Tensor, seg2inst: torch.Tensor, seg2label: torch.Tensor,
                lab_off: torch.Tensor, label_value: torch.Tensor):
    """Enqueue ``mspa_prep_labels``: (instance_ids, label_ids) as int32 tensors holding uint32 bits, and the label index (int32)."""
    S, N = _check_spans(spans)
    _check("seg", seg, torch.int32, (N,))
    _check("tab_off", tab_off, torch.int64, (S + 1,))
    _check("lab_off", lab_off, torch.int64, (S + 1,))
    _check("seg2inst", seg2inst, torch.int32, (None,))
    _check("seg2label", seg2label, torch.int32, (seg2inst.shape[0],))          # the two tables: one length
    _check("label_value", label_value, torch.int32, (None,))                   # uint32 bits
    dev = seg.device
    inst = torch.empty((N,), dtype=torch.int32, device=dev)
    label = torch.empty((N,), dtype=torch.int32, device=dev)
    index = torch.empty((N,), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().mspa_prep_labels(_ptr(seg), _ptr(spans["vert_off"]), _ptr(spans["word_off"]), S, N, spans["n_waves"], _ptr(tab_off),
                                            _ptr(seg2inst), _ptr(seg2label), _ptr(lab_off), _ptr(label_value), _ptr(inst), _ptr(label), _ptr(index),
                                            _stream_ptr()))
    return inst, label, index


def prep_align(spans: dict, vertices: torch.Tensor, axis_align: torch.Tensor) -> torch.Tensor:
    """Enqueue ``mspa_prep_align``: [N, 6] float32 -> [N, 6] float64, xyz through each scene's 4x4 (``np.dot(pts, A.T)`` bits)."""
    S, N = _check_spans(spans)
    _check("vertices", vertices, torch.float32, (N, 6))
    _check("axis_align", axis_align, torch.float64, (S, 4, 4))
    out = torch.empty((N, 6), dtype=torch.float64, device=vertices.device)
    _lib.check(_lib.load().mspa_prep_align(_ptr(vertices), _ptr(spans["vert_off"]), _ptr(spans["word_off"]), S, N, spans["n_waves"], _ptr(axis_align),
                                           _ptr(out), _stream_ptr()))
    return out


def prep_objects(spans: dict, instance_ids: torch.Tensor, vertices: torch.Tensor, aligned: torch.Tensor, n_objects: Sequence[int]) -> dict:
    """Enqueue ``mspa_prep_objects`` and K9 on its membership rows.  ``n_objects[s]``: object slots of scene s (slot k - 1 <-> id k).
    Returns device tensors: count [M], lo / hi_unaligned and lo / hi_aligned [M, 3] float64, unique [S], and the stable split as CSR
    (``offsets`` [M + 1] int64, ``indices`` int32: scene-local vertex numbers, ascending within an object).  Synchronises the
    current stream: the slot offsets go up from pageable memory and ``bitset_csr`` reads its total back."""
    S, N = _check_spans(spans)
    _require(len(n_objects) == S, f"n_objects: one per scene ({S}), got {len(n_objects)}")
    _check("instance_ids", instance_ids, torch.int32, (N,))
    _check("vertices", vertices, torch.float32, (N, 6))
    _check("aligned", aligned, torch.float64, (N, 6))
    dev = instance_ids.device
    obj_off_host = _ragged_offsets(n_objects)
    M, n_words = int(obj_off_host[-1]), spans["max_words"]
    obj_off = torch.from_numpy(obj_off_host).to(dev)
    bits = torch.empty((M, n_words), dtype=torch.int64, device=dev)
    count = torch.empty((M,), dtype=torch.int32, device=dev)
    ext = [torch.empty((M, 3), dtype=torch.float64, device=dev) for _ in range(4)]
    zero_count = torch.empty((S,), dtype=torch.int32, device=dev)
    unique = torch.empty((S,), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().mspa_prep_objects(_ptr(instance_ids), _ptr(vertices), _ptr(aligned), _ptr(spans["vert_off"]), _ptr(spans["word_off"]), S, N,
                                             spans["n_waves"], _ptr(obj_off), M, _ptr(bits), n_words, _ptr(count), _ptr(ext[0]), _ptr(ext[1]),
                                             _ptr(ext[2]), _ptr(ext[3]), _ptr(zero_count), _ptr(unique), _stream_ptr()))
    offsets, indices = bitset_csr(bits)
    return {"count": count, "lo_unaligned": ext[0], "hi_unaligned": ext[1], "lo_aligned": ext[2], "hi_aligned": ext[3], "unique": unique,
            "zero_count": zero_count, "offsets": offsets, "indices": indices, "obj_off_host": obj_off_host}


def _int_list_buffers(texts: Sequence[bytes]):
    off = _ragged_offsets([len(t) for t in texts])
    return np.frombuffer(bytearray(b"".join(texts) or b"\0"), dtype=np.uint8), off


def parse_int_lists_host(texts: Sequence[bytes], capacities: Optional[Sequence[int]] = None, n_threads: Optional[int] = None):
    """``mspa_parse_int_list_host`` over the pool threads: the text between the brackets of JSON integer lists -> (list of int32
    arrays, status [n]).  A declined array (status != 0) comes back as None: ``json.loads`` is the caller's fallback."""
    from . import hostinfo
    n = len(texts)
    if n == 0:
        return [], np.zeros(0, dtype=np.int32)
    buf, off = _int_list_buffers(texts)
    cap = _ragged_offsets([(len(t) + 1) // 2 for t in texts] if capacities is None else capacities)
    out = np.empty(max(int(cap[-1]), 1), dtype=np.int32)
    counts, status = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)
    _lib.check(_lib.load().mspa_parse_int_list_host(buf.ctypes.data, off.ctypes.data, n, out.ctypes.data, cap.ctypes.data, counts.ctypes.data,
                                                    status.ctypes.data, int(n_threads or hostinfo.effective_cpus())))
    return [out[cap[a]:cap[a] + counts[a]] if status[a] == 0 else None for a in range(n)], status


def parse_int_lists_device(texts: Sequence[bytes], device, expected_counts: Optional[Sequence[int]] = None):
    """The same lists parsed on the device (one lane per byte; ``mspa_parse_int_list_flags_device`` -> prefix sum ->
    ``mspa_parse_int_list_device``).  Returns (values int32 [total] on the device, offsets int64 [n + 1] and status int32 [n] on the
    host).  Arrays with status != 0 were declined -- non-negative plain lists only -- and belong to the host parser."""
    _require_gpu()
    lib = _lib.load()
    n = len(texts)
    if n == 0:
        return torch.zeros((0,), dtype=torch.int32, device=device), np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32)
    buf, off = _int_list_buffers(texts)
    n_bytes = int(off[-1])
    _require(n_bytes <= 0x7fffffff, "parse_int_lists_device: more than 2 GiB of text")
    text = torch.from_numpy(buf).to(device)
    text_off = torch.from_numpy(off).to(device)
    status = torch.empty((max(n, 1),), dtype=torch.int32, device=device)
    flags = torch.empty((max(n_bytes, 1),), dtype=torch.int64, device=device)
    _lib.check(lib.mspa_parse_int_list_flags_device(_ptr(text), _ptr(text_off), n, n_bytes, _ptr(flags), _ptr(status), _stream_ptr()))
    T = torch.zeros((n_bytes + 1,), dtype=torch.int64, device=device)                # torch as plumbing: one prefix sum
    if n_bytes:
        torch.cumsum(flags[:n_bytes], dim=0, out=T[1:])
    total = int(T[-1].item()) & 0xffffffff                                             # one small read-back: the size to allocate
    values = torch.empty((max(total, 1),), dtype=torch.int32, device=device)
    expected = None if expected_counts is None else torch.from_numpy(np.asarray(expected_counts, dtype=np.int64)).to(device)
    out_off = torch.empty((n + 1,), dtype=torch.int64, device=device)
    _lib.check(lib.mspa_parse_int_list_device(_ptr(text), _ptr(text_off), n, n_bytes, _ptr(T), _ptr(expected), _ptr(values), total, _ptr(out_off),
                                              _ptr(status), _stream_ptr()))
    return values[:total], out_off.cpu().numpy(), status[:n].cpu().numpy()


def parse_int_lists(texts: Sequence[bytes], device=None, expected_counts: Optional[Sequence[int]] = None, n_threads: Optional[int] = None):
    """JSON integer lists -> list of int32 arrays (None where neither parser takes the text: not a plain list of int32).  ``device``
    None: the native host threads.  Else the device parses and the host threads take what it declines, so the result is the
    host parser's for every input."""
    if device is None:
        return parse_int_lists_host(texts, expected_counts, n_threads)[0]
    values, off, status = parse_int_lists_device(texts, device, expected_counts)
    host = values.cpu().numpy()
    out = [host[off[a]:off[a + 1]] if status[a] == 0 else None for a in range(len(texts))]
    declined = [a for a in range(len(texts)) if status[a] != 0]
    if declined:
        redo = parse_int_lists_host([texts[a] for a in declined], None, n_threads)[0]
        for a, r in zip(declined, redo):
            out[a] = r
    return out
