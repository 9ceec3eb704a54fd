"""Cleaning and boxing a ragged batch of clouds on the device: the k-nearest mean distance, the statistical-outlier rule and the
kept rows' extents for every segment at once (csrc/cloud_segments.hip, rule in csrc/cloud_segments_core.h).

A batch is ``rows`` [N, C >= 3] on the device plus ``offsets`` [S + 1], a HOST int64 array: ascending, ``offsets[0] = 0``,
``offsets[S] = N``; segment s is ``rows[offsets[s]:offsets[s + 1]]``, and empty segments are allowed anywhere.  The number of
launches and of read-backs of each function does not depend on S.  Per segment the search is the single-cloud op's
(``engine.knn_mean_distance``) bit for bit; the two sums of the rule follow the order csrc/cloud_segments_core.h states, which
is not ``torch.sum``'s, so a threshold may differ from ``ops.remove_statistical_outliers``' in the last bits.

torch is plumbing, as in ``mspa.engine``: the segmented order statistics (two sorts), the one sort of the keys, ``nonzero`` and
``index_select``.  Host tables go up through pinned memory without a host wait.

Two further ops take the same batch: ``voxel_down_sample_segments`` (csrc/voxel_segments.hip) thins every segment on a voxel grid,
and ``dbscan_segments`` / ``largest_cluster_segments`` (csrc/dbscan_segments.hip, rule in csrc/dbscan_core.h) label every segment
as scikit-learn's DBSCAN does and keep its largest cluster.  ``footprint_hull_segments`` / ``upright_boxes_segments``
(csrc/upright_segments.hip, rule in csrc/upright_box_core.h) give every segment the exact convex hull of its (x, y) footprint and
its upright minimal box: the z extent times the minimum-area rectangle around that hull.  ``upright_iou`` / ``upright_iou_matrix``
(csrc/upright_iou.hip, rule in csrc/upright_iou_core.h) score such boxes against each other, pair by pair or set against set.
``target_index`` / ``TargetIndex.nearest`` / ``fit_segments`` / ``cloud_fit_segments`` (csrc/cloud_distance.hip, rule in
csrc/cloud_distance_core.h) compare the clouds of one batch with those of another: per row the distance to, and the row of, the nearest
point of the segment its pair names, and a per-pair summary of those distances.  ``rigid_fit_segments`` / ``transform_segments`` /
``TargetIndex.register`` / ``register_segments`` (csrc/cloud_align.hip, rule in csrc/cloud_align_core.h) say by which rotation and
translation one cloud lies off another: the rigid fit of matched rows (Kabsch / Horn) per pair, and point-to-point ICP on top of
``nearest``.  ``knn_segments`` / ``normals_segments`` (csrc/cloud_normals.hip, rule in csrc/cloud_normals_core.h) name the k nearest
rows of every row inside its own segment and fit a plane to them: a unit normal, towards the segment's viewpoint where one is given,
the surface variation and a status per row.  ``plane_fit_segments`` and ``TargetIndex.register(estimation="point_to_plane")``
(csrc/cloud_align_plane.hip, rule in csrc/cloud_align_plane_core.h) are point-to-plane ICP on top of the search and those normals.
"""
from __future__ import annotations


import numpy as np
import torch

from . import _lib
from .engine import _check, _ptr, _require, _stream_ptr, _workspace


def _offsets(offsets, n_rows: int) -> np.ndarray:
    """The host offsets of a batch of ``n_rows`` rows, checked: int64 [S + 1], ascending from 0 to ``n_rows``."""
    if isinstance(offsets, torch.Tensor):
        _require(not offsets.is_cuda, "offsets: a host array (the launch shapes come from it)")
        offsets = offsets.numpy()
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    _require(off.ndim == 1 and off.size >= 1, f"offsets: [S + 1], got {list(off.shape)}")
    _require(off.size - 1 <= _lib.SEGMENTS_MAX, f"offsets: at most 2^24 segments, got {off.size - 1}")
    _require(int(off[0]) == 0 and int(off[-1]) == n_rows and bool((np.diff(off) >= 0).all()),
             f"offsets: ascending from 0 to the {n_rows} rows")
    return off


def _upload(*arrays, device) -> list:
    """Host arrays -> device tensors of the same dtypes and shapes through ONE pinned staging buffer and one non-blocking copy,
    each part on a 16-byte boundary.  Enqueues only."""
    arrays = [np.ascontiguousarray(a) for a in arrays]
    starts, total = [], 0
    for a in arrays:
        starts.append(total)
        total += (a.nbytes + 15) // 16 * 16
    staged = torch.empty((max(total, 16),), dtype=torch.uint8, pin_memory=True)
    view = staged.numpy()
    for a, at in zip(arrays, starts):
        view[at:at + a.nbytes] = a.reshape(-1).view(np.uint8)
    on_device = staged.to(device, non_blocking=True)
    return [on_device[at:at + a.nbytes].view(torch.from_numpy(np.empty((0,), dtype=a.dtype)).dtype).reshape(a.shape)
            for a, at in zip(arrays, starts)]


def _offsets_of(counts) -> np.ndarray:
    """Per-segment counts [S] -> the offsets [S + 1] of the rows they count, back to back: a host int64 array from 0."""
    offsets = np.zeros((len(counts) + 1,), dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    return offsets


def _knn_check(k: int) -> int:
    k = int(k)
    _require(1 <= k <= _lib.KNN_MAX_K, f"k: between 1 and {_lib.KNN_MAX_K}, got {k}")
    return k


def _search_tables(xyz: torch.Tensor, off: np.ndarray, k: int):
    """The tables of a non-empty batch's search: (grids [S, 112] uint8 on the host, and on the device the offsets, the grids and
    cell_base).  Holds THE read-back of ``knn_mean_distance_segments``; raises its ValueError."""
    lib = _lib.load()
    N, S = int(xyz.shape[0]), off.size - 1
    counts = np.diff(off)
    live = np.nonzero(counts)[0]
    rank = counts[live] // 100
    where = np.concatenate([off[live] + rank, off[live] + counts[live] - 1 - rank])
    off_dev, where_dev = _upload(off, where, device=xyz.device)
    # the segmented order statistics: every column ascending, then stably by segment -- each segment's range holds its own values ascending
    segment = torch.searchsorted(off_dev[1:], torch.arange(N, dtype=torch.int64, device=xyz.device), right=True).to(torch.int32)
    values, by_value = torch.sort(xyz.t().contiguous(), dim=1)
    by_segment = torch.sort(segment[by_value], dim=1, stable=True).indices
    ranked = values.gather(1, by_segment).index_select(1, where_dev)                      # [3, 2 * live]
    finite = torch.isfinite(xyz).all().to(torch.float64).reshape(1)
    back = torch.cat([ranked.reshape(-1), finite]).cpu().numpy()                            # THE read-back
    if back[-1] != 1.0:
        raise ValueError("mspa.cloud_segments: requirement not met: xyz: finite coordinates")
    box = back[:-1].reshape(3, 2, live.size)
    lo, hi = np.zeros((S, 3)), np.zeros((S, 3))
    lo[live], hi[live] = box[:, 0].T, box[:, 1].T
    grids = np.zeros((S, _lib.KNN_GRID_BYTES), dtype=np.uint8)
    cell_base = np.zeros((S + 1,), dtype=np.int64)
    _lib.check(lib.mspa_knn_segments_grids_host(lo.ctypes.data, hi.ctypes.data, off.ctypes.data, S, k, grids.ctypes.data))
    _lib.check(lib.mspa_knn_segments_tables_host(off.ctypes.data, S, k, cell_base.ctypes.data))
    grids_dev, base_dev = _upload(grids, cell_base, device=xyz.device)
    return grids, off_dev, grids_dev, base_dev


def knn_mean_distance_segments(xyz: torch.Tensor, offsets, k: int, want_evals: bool = False):
    """[N, 3] float64 finite points and host ``offsets`` [S + 1] -> ``avg`` [N] float64: per segment what
    ``engine.knn_mean_distance(xyz[a:b], k)`` returns, bit for bit (the mean distance from each point to its min(k, n_s) nearest
    points of its own segment, itself included).  With ``want_evals`` also [N] int32, the distances each point evaluated.  One
    read-back per call, whatever S is: the boxes of all segments (the per-axis order statistics of rank n_s // 100 and
    n_s - 1 - n_s // 100, from two device sorts) together with the flag that every coordinate is finite; non-finite
    coordinates raise ValueError."""
    N = _check("xyz", xyz, torch.float64, (None, 3)).shape[0]
    off = _offsets(offsets, N)
    k = _knn_check(k)
    _require(N <= 1 << 30, f"xyz: at most 2^30 points, got {N}")
    S = off.size - 1
    mean = torch.empty((N,), dtype=torch.float64, device=xyz.device)
    evals = torch.empty((N,), dtype=torch.int32, device=xyz.device) if want_evals else None
    if N == 0:
        return (mean, evals) if want_evals else mean
    lib = _lib.load()
    grids, off_dev, grids_dev, base_dev = _search_tables(xyz, off, k)
    keys = torch.empty((N,), dtype=torch.int64, device=xyz.device)
    _lib.check(lib.mspa_knn_segments_cells_device(_ptr(xyz), off.ctypes.data, S, grids.ctypes.data, _ptr(off_dev), _ptr(grids_dev),
                                                  _ptr(base_dev), _ptr(keys), _stream_ptr()))
    order = torch.sort(keys, stable=True).indices
    work = _workspace(int(lib.mspa_knn_segments_workspace_bytes(off.ctypes.data, S, k)), xyz.device)
    _lib.check(lib.mspa_knn_segments_mean_distance_device(_ptr(xyz), off.ctypes.data, S, k, grids.ctypes.data, _ptr(off_dev), _ptr(grids_dev),
                                                          _ptr(base_dev), _ptr(order), _ptr(mean), _ptr(evals), _ptr(work),
                                                          int(work.numel()), _stream_ptr()))
    return (mean, evals) if want_evals else mean


def outlier_stats_segments(avg: torch.Tensor, offsets, std_ratio: float, xyz: torch.Tensor) -> dict:
    """``avg`` [N] float64 (``knn_mean_distance_segments``' output), host ``offsets`` [S + 1] and the rows' ``xyz`` [N, 3] float64 ->
    a dict of device tensors: ``keep`` [N] bool, the rows that stay, and per segment ``kept`` [S] int64, ``mean``, ``sd``, ``thr`` [S]
    float64 and ``lo`` / ``hi`` [S, 3] float64, the extents of the kept rows (+inf / -inf where none stays).  The rule is
    ``ops.remove_statistical_outliers``' per segment, with the two sums in the order csrc/cloud_segments_core.h states; a segment
    of fewer than two rows has NaN statistics and keeps nothing.  Enqueue only: the offsets go up through pinned memory and
    nothing is read back."""
    N = _check("avg", avg, torch.float64, (None,)).shape[0]
    _check("xyz", xyz, torch.float64, (N, 3))
    off = _offsets(offsets, N)
    S = off.size - 1
    std_ratio = float(std_ratio)
    _require(np.isfinite(std_ratio), f"std_ratio: finite, got {std_ratio}")
    dev = avg.device
    keep = torch.empty((N,), dtype=torch.uint8, device=dev)
    out = {"keep": keep.view(torch.bool), "kept": torch.empty((S,), dtype=torch.int64, device=dev)}
    for name in ("mean", "sd", "thr"):
        out[name] = torch.empty((S,), dtype=torch.float64, device=dev)
    for name in ("lo", "hi"):
        out[name] = torch.empty((S, 3), dtype=torch.float64, device=dev)
    if S:
        off_dev, = _upload(off, device=dev)
        _lib.check(_lib.load().mspa_outlier_segments_device(_ptr(avg), _ptr(xyz), off.ctypes.data, S, std_ratio, _ptr(off_dev), _ptr(keep),
                                                            _ptr(out["kept"]), _ptr(out["mean"]), _ptr(out["sd"]), _ptr(out["thr"]),
                                                            _ptr(out["lo"]), _ptr(out["hi"]), _stream_ptr()))
    return out


def _check_rule(nb_neighbors, std_ratio) -> None:
    """``ops.remove_statistical_outliers``' argument errors, word for word."""
    if nb_neighbors < 1 or std_ratio <= 0:
        raise RuntimeError("remove_statistical_outliers: nb_neighbors must be at least 1 and std_ratio positive "
                           f"(got {nb_neighbors}, {std_ratio})")
    if nb_neighbors > _lib.KNN_MAX_K:
        raise NotImplementedError(f"remove_statistical_outliers: nb_neighbors is limited to {_lib.KNN_MAX_K} (got {nb_neighbors})")


def clean_segments(rows: torch.Tensor, offsets, nb_neighbors=20, std_ratio=1.0):
    """``remove_statistical_outliers_segments`` plus the kept rows' indices into ``rows`` [M] int64 (device), ascending: ``(rows_kept,
    offsets_kept, lo, hi, index)``.  For a caller that filters further per-row arrays the same way."""
    _check_rule(nb_neighbors, std_ratio)
    _require(isinstance(rows, torch.Tensor) and rows.is_cuda and rows.dim() == 2 and rows.shape[1] >= 3,
             "rows: a device tensor [N, C >= 3]")
    off = _offsets(offsets, int(rows.shape[0]))
    xyz = rows[:, :3].to(torch.float64).contiguous()
    try:
        avg = knn_mean_distance_segments(xyz, off, int(nb_neighbors))
    except ValueError as e:
        if "finite coordinates" in str(e):
            raise ValueError("remove_statistical_outliers: the cloud has non-finite coordinates") from None
        raise
    stats = outlier_stats_segments(avg, off, std_ratio, xyz)
    kept = stats["kept"].cpu().numpy()                                                      # THE second read-back
    kept_offsets = _offsets_of(kept)
    index = torch.nonzero_static(stats["keep"], size=int(kept_offsets[-1])).flatten()       # its size is known: no read-back of its own
    return rows.index_select(0, index), kept_offsets, stats["lo"], stats["hi"], index


def remove_statistical_outliers_segments(rows: torch.Tensor, offsets, nb_neighbors=20, std_ratio=1.0):
    """A batch ``rows`` [N, C >= 3] (device; all columns and the dtype are kept, float32 coordinates are widened exactly for the
    search, as the single-cloud op does) and host ``offsets`` [S + 1] -> ``(rows_kept, offsets_kept, lo, hi)``: per segment the rows
    ``ops.remove_statistical_outliers(rows[a:b], nb_neighbors, std_ratio)`` keeps, in ascending order and back to back;
    ``offsets_kept`` [S + 1] a host int64 array again; ``lo`` / ``hi`` [S, 3] float64 (device) the kept rows' extents, +inf / -inf
    where none stays.  The same exceptions as the single-cloud op: RuntimeError for ``nb_neighbors < 1`` or ``std_ratio <= 0``,
    NotImplementedError above 64, ValueError for non-finite coordinates.  Two read-backs per call, whatever S is: the boxes of all
    segments (``knn_mean_distance_segments``) and the kept counts."""
    return clean_segments(rows, offsets, nb_neighbors, std_ratio)[:4]


def knn_mean_distance_segments_host(xyz, offsets, k: int, want_evals: bool = False):
    """``knn_mean_distance_segments`` on the CPU for NumPy input, through the same headers (mspa_knn_segments_mean_distance_host).
    The device's twin for tests on a machine without a GPU, not a fallback."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float64)
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError(f"mspa.cloud_segments: xyz: expected [N, 3], got {list(xyz.shape)}")
    off = _offsets(offsets, xyz.shape[0])
    k = _knn_check(k)
    mean = np.empty((xyz.shape[0],), dtype=np.float64)
    evals = np.empty((xyz.shape[0],), dtype=np.int32) if want_evals else None
    _lib.check(_lib.load().mspa_knn_segments_mean_distance_host(xyz.ctypes.data, off.ctypes.data, off.size - 1, k, mean.ctypes.data,
                                                                evals.ctypes.data if want_evals else None))
    return (mean, evals) if want_evals else mean


def outlier_stats_segments_host(avg, offsets, std_ratio: float, xyz) -> dict:
    """``outlier_stats_segments`` on the CPU for NumPy input (mspa_outlier_segments_host): the same keys, NumPy arrays."""
    avg = np.ascontiguousarray(avg, dtype=np.float64)
    xyz = np.ascontiguousarray(xyz, dtype=np.float64)
    N = avg.shape[0]
    if avg.ndim != 1 or xyz.shape != (N, 3):
        raise ValueError(f"mspa.cloud_segments: avg [N] and xyz [N, 3], got {list(avg.shape)} and {list(xyz.shape)}")
    off = _offsets(offsets, N)
    S = off.size - 1
    keep = np.zeros((N,), dtype=np.uint8)
    out = {"kept": np.zeros((S,), dtype=np.int64), "mean": np.zeros((S,)), "sd": np.zeros((S,)), "thr": np.zeros((S,)),
           "lo": np.zeros((S, 3)), "hi": np.zeros((S, 3))}
    _lib.check(_lib.load().mspa_outlier_segments_host(avg.ctypes.data, xyz.ctypes.data, off.ctypes.data, S, float(std_ratio), keep.ctypes.data,
                                                      *(out[n].ctypes.data for n in ("kept", "mean", "sd", "thr", "lo", "hi"))))
    out["keep"] = keep.astype(bool)
    return out


def remove_statistical_outliers_segments_host(rows, offsets, nb_neighbors=20, std_ratio=1.0):
    """``remove_statistical_outliers_segments`` over the two host twins, NumPy in and out: for tests on a machine without a GPU."""
    _check_rule(nb_neighbors, std_ratio)
    rows = np.asarray(rows)
    off = _offsets(offsets, rows.shape[0])
    xyz = np.ascontiguousarray(rows[:, :3], dtype=np.float64)
    if not np.isfinite(xyz).all():
        raise ValueError("remove_statistical_outliers: the cloud has non-finite coordinates")
    stats = outlier_stats_segments_host(knn_mean_distance_segments_host(xyz, off, int(nb_neighbors)), off, std_ratio, xyz)
    kept_offsets = _offsets_of(stats["kept"])
    return rows[stats["keep"]], kept_offsets, stats["lo"], stats["hi"]


VOXEL_NON_FINITE, VOXEL_OUT_OF_RANGE = 1, 2       # csrc/voxel_grid_core.h: the bits of the flag word


def _check_voxel_size(voxel_size) -> float:
    """Open3D's error kind for a bad size, and ``remove_statistical_outliers``' for its arguments."""
    try:
        size = float(voxel_size)
    except (TypeError, ValueError):
        size = float("nan")
    if not (0.0 < size < float("inf")):
        raise RuntimeError(f"voxel_down_sample: voxel_size must be positive and finite (got {voxel_size})")
    return size


def _raise_voxel_flags(flags: int, voxel_size: float) -> None:
    if flags & VOXEL_NON_FINITE:
        raise ValueError("voxel_down_sample: the cloud has non-finite coordinates")
    if flags & VOXEL_OUT_OF_RANGE:
        raise ValueError(f"voxel_down_sample: voxel_size {voxel_size} is too small for a segment's extent "
                         f"(a voxel index reaches 2^{_lib.VOXEL_AXIS_BITS} on an axis)")


def _cell_keys(rows: torch.Tensor, C: int, off: np.ndarray, side: float, seg_out: torch.Tensor):
    """The cell keys of a non-empty batch ``rows`` [N, C] float64 on a grid of ``side``, sorted: ``seg_out`` [S + 1] int32 (device) has
    its first S entries zeroed and takes the flag word in its last.  -> ``(off_dev, base_dev, keys, order, work)``: the offsets and
    the extents pass's tile table on the device, the keys [N] int64 in row order, the rows' order [N] int64 by (segment, key) with
    ties in row order, and the workspace of ``mspa_voxel_segments_workspace_bytes`` the keys pass used.  Enqueues only."""
    lib = _lib.load()
    N, S, dev = int(rows.shape[0]), off.size - 1, rows.device
    tile_base = np.zeros((S + 1,), dtype=np.int64)
    _lib.check(lib.mspa_voxel_segments_tables_host(off.ctypes.data, S, tile_base.ctypes.data))
    off_dev, base_dev = _upload(off, tile_base, device=dev)
    keys = torch.empty((N,), dtype=torch.int64, device=dev)
    segment = torch.empty((N,), dtype=torch.int32, device=dev)
    work = _workspace(int(lib.mspa_voxel_segments_workspace_bytes(off.ctypes.data, S)), dev)
    _lib.check(lib.mspa_voxel_segments_keys_device(_ptr(rows), C, off.ctypes.data, S, side, _ptr(off_dev), _ptr(base_dev), _ptr(keys),
                                                   _ptr(segment), _ptr(seg_out), _ptr(work), int(work.numel()), _stream_ptr()))
    order = torch.sort(keys, stable=True).indices
    if S > 1:                                              # stably by segment behind stably by key: (segment, key), ties in row order
        order = order.gather(0, torch.sort(segment.gather(0, order), stable=True).indices)
    return off_dev, base_dev, keys, order, work


def voxel_down_sample_segments(rows: torch.Tensor, offsets, voxel_size):
    """A batch ``rows`` [N, C >= 3] (device; float64, or a dtype that widens to it exactly) with finite xyz in front and host
    ``offsets`` [S + 1] -> ``(out_rows [M, C] float64, out_offsets [S + 1] host int64, counts [M] int32)``: per segment one row per
    occupied voxel of a grid of ``voxel_size``, every column (colour and other extra columns included) the mean over the voxel's
    rows, ``counts`` the rows each voxel took.  The rule is csrc/voxel_grid_core.h's: per axis ``min_bound = lo - voxel_size * 0.5``
    with ``lo`` the segment's own minimum, ``idx = floor((p - min_bound) / voxel_size)``; segments stay in order and a segment's
    voxels come in ascending (ix, iy, iz); a voxel's rows are summed in ascending row index, sequentially up to 64 rows and as 64
    strided lane sums folded by halving strides above.  It restates Open3D's ``voxel_down_sample`` as the maintainers recall it
    and is not checked against Open3D (whose output order is its hash map's).  The same bits on every run.  One read-back per call,
    whatever S is: the per-segment voxel counts together with the flag word.  ``voxel_size <= 0`` or non-finite raises RuntimeError;
    a non-finite xyz anywhere, or a voxel index of 2^21 or more on an axis (``voxel_size`` too small), raises ValueError.  torch is
    plumbing: two stable sorts (by key, then by segment; one when S = 1)."""
    size = _check_voxel_size(voxel_size)
    _require(isinstance(rows, torch.Tensor) and rows.is_cuda and rows.dim() == 2 and rows.shape[1] >= 3, "rows: a device tensor [N, C >= 3]")
    rows = _check("rows", rows.to(torch.float64).contiguous(), torch.float64, (None, (3,)))
    N, C = int(rows.shape[0]), int(rows.shape[1])
    _require(C <= _lib.VOXEL_MAX_COLUMNS, f"rows: at most {_lib.VOXEL_MAX_COLUMNS} columns, got {C}")
    off = _offsets(offsets, N)
    _require(N <= 1 << 30, f"rows: at most 2^30 rows, got {N}")
    S = off.size - 1
    dev = rows.device
    if N == 0:
        return (torch.empty((0, C), dtype=torch.float64, device=dev), np.zeros((S + 1,), dtype=np.int64),
                torch.empty((0,), dtype=torch.int32, device=dev))
    lib = _lib.load()
    seg_voxels = torch.empty((S + 1,), dtype=torch.int32, device=dev)
    off_dev, _base_dev, keys, order, work = _cell_keys(rows, C, off, size, seg_voxels)
    _lib.check(lib.mspa_voxel_segments_heads_device(off.ctypes.data, S, _ptr(off_dev), _ptr(keys), _ptr(order), _ptr(seg_voxels), _ptr(work),
                                                    int(work.numel()), _stream_ptr()))
    back = seg_voxels.cpu().numpy()                        # THE read-back
    _raise_voxel_flags(int(back[S]), size)
    out_offsets = _offsets_of(back[:S])
    M = int(out_offsets[-1])
    out_rows = torch.empty((M, C), dtype=torch.float64, device=dev)
    counts = torch.empty((M,), dtype=torch.int32, device=dev)
    _lib.check(lib.mspa_voxel_segments_means_device(_ptr(rows), C, off.ctypes.data, S, _ptr(off_dev), _ptr(order), M, _ptr(out_rows), _ptr(counts),
                                                    _ptr(work), int(work.numel()), _stream_ptr()))
    return out_rows, out_offsets, counts


def voxel_down_sample_segments_host(rows, offsets, voxel_size):
    """``voxel_down_sample_segments`` on the CPU for NumPy input, through the same header (mspa_voxel_segments_host): NumPy arrays
    out, the same exceptions.  The device's twin for tests and for input that has no device, not a fallback."""
    size = _check_voxel_size(voxel_size)
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    if rows.ndim != 2 or rows.shape[1] < 3 or rows.shape[1] > _lib.VOXEL_MAX_COLUMNS:
        raise ValueError(f"mspa.cloud_segments: rows: expected [N, C >= 3], got {list(rows.shape)}")
    N, C = rows.shape
    off = _offsets(offsets, N)
    S = off.size - 1
    out_rows = np.empty((N, C), dtype=np.float64)
    out_counts = np.empty((N,), dtype=np.int32)
    out_offsets = np.zeros((S + 1,), dtype=np.int64)
    flags = np.zeros((1,), dtype=np.int32)
    _lib.check(_lib.load().mspa_voxel_segments_host(rows.ctypes.data, C, off.ctypes.data, S, size, out_rows.ctypes.data, out_offsets.ctypes.data,
                                                    out_counts.ctypes.data, flags.ctypes.data))
    _raise_voxel_flags(int(flags[0]), size)
    M = int(out_offsets[-1])
    return out_rows[:M].copy(), out_offsets, out_counts[:M].copy()


DBSCAN_CAP_REACHED = 4                            # csrc/dbscan_core.h: the third bit of the flag word


def _check_dbscan(eps, min_points):
    """``remove_statistical_outliers``' error kind for bad arguments -> (eps, min_points, the cell side)."""
    try:
        e, m = float(eps), int(min_points)
        if m != min_points:
            m = 0
    except (TypeError, ValueError):
        e, m = float("nan"), 0
    side = _lib.load().mspa_dbscan_cell_side(e) if e == e else -1.0
    if not side > 0.0 or m < 1:
        raise RuntimeError(f"cluster_dbscan: eps must be positive and finite and min_points at least 1 (got {eps}, {min_points})")
    return e, m, side


def _raise_dbscan_flags(flags: int, eps: float) -> None:
    if flags & VOXEL_NON_FINITE:
        raise ValueError("cluster_dbscan: the cloud has non-finite coordinates")
    if flags & VOXEL_OUT_OF_RANGE:
        raise ValueError(f"cluster_dbscan: eps {eps} is too small for a segment's extent "
                         f"(a cell index reaches 2^{_lib.VOXEL_AXIS_BITS} on an axis)")
    if flags & DBSCAN_CAP_REACHED:
        raise RuntimeError("cluster_dbscan: a union-find loop reached its iteration cap (csrc/dbscan_core.h)")


def _dbscan_device(rows: torch.Tensor, offsets, eps, min_points, want_keep: bool):
    """The device op: (labels [N] int32, keep [N] uint8 or None, back [2 S + 1] host int32: kept, clusters, flag word, and the kept
    rows' extents lo / hi [S, 3] or None).  Holds THE read-back of ``dbscan_segments`` and ``largest_cluster_segments``."""
    e, m, side = _check_dbscan(eps, min_points)
    _require(isinstance(rows, torch.Tensor) and rows.is_cuda and rows.dim() == 2 and rows.shape[1] >= 3, "rows: a device tensor [N, C >= 3]")
    xyz = _check("rows", rows[:, :3].to(torch.float64).contiguous(), torch.float64, (None, 3))
    N = int(xyz.shape[0])
    off = _offsets(offsets, N)
    _require(N <= 1 << 30, f"rows: at most 2^30 rows, got {N}")
    S = off.size - 1
    dev = rows.device
    labels = torch.empty((N,), dtype=torch.int32, device=dev)
    keep = torch.empty((N,), dtype=torch.uint8, device=dev) if want_keep else None
    lo = torch.full((S, 3), float("inf"), dtype=torch.float64, device=dev) if want_keep else None
    hi = torch.full((S, 3), float("-inf"), dtype=torch.float64, device=dev) if want_keep else None
    if N == 0:
        return labels, keep, np.zeros((2 * S + 1,), dtype=np.int32), lo, hi
    lib = _lib.load()
    seg = torch.empty((2 * S + 1,), dtype=torch.int32, device=dev)
    off_dev, base_dev, keys, order, _cells_work = _cell_keys(xyz, 3, off, side, seg[S:])     # as the down-sample sorts
    work = _workspace(int(lib.mspa_dbscan_segments_workspace_bytes(off.ctypes.data, S)), dev)
    _lib.check(lib.mspa_dbscan_segments_device(_ptr(xyz), 3, off.ctypes.data, S, e, m, _ptr(off_dev), _ptr(keys), _ptr(order), _ptr(base_dev),
                                               _ptr(labels), _ptr(keep), _ptr(lo), _ptr(hi), _ptr(seg), _ptr(work), int(work.numel()),
                                               _stream_ptr()))
    back = seg.cpu().numpy()                               # THE read-back
    _raise_dbscan_flags(int(back[2 * S]), e)
    return labels, keep, back, lo, hi


def dbscan_segments(rows: torch.Tensor, offsets, eps, min_points):
    """A batch ``rows`` [N, C >= 3] (device; xyz in front, float64 or a dtype that widens to it exactly) and host ``offsets`` [S + 1]
    -> ``(labels [N] int32 device, clusters [S] host int64)``: per segment the labels of
    ``sklearn.cluster.DBSCAN(eps, min_samples=min_points, algorithm="kd_tree").fit(rows[a:b, :3]).labels_``, value for value, and the
    number of clusters.  The rule is csrc/dbscan_core.h's: ``near(i, j)`` iff ``(dx*dx + dy*dy) + dz*dz <= eps*eps`` in float64, a
    point near itself; a point is core with ``min_points`` near points, itself and duplicates included; clusters are the connected
    components of the core points, numbered in ascending order of their lowest core row; any other point takes the lowest cluster
    number among the core points near it, or -1.  The same values on every run.  One read-back per call, whatever S is: the
    per-segment cluster counts together with the flag word.  ``eps <= 0``, non-finite ``eps`` or ``min_points < 1`` raises
    RuntimeError; a non-finite xyz anywhere, or a cell index of 2^21 or more on an axis (``eps`` too small for a segment's extent),
    raises ValueError.  torch is plumbing: the two stable sorts of the cell keys (one when S = 1).  The work of a point grows with
    the rows of the 27 cells around it: thin fused clouds (``voxel_down_sample_segments``) first."""
    labels, _keep, back, _lo, _hi = _dbscan_device(rows, offsets, eps, min_points, False)
    S = (back.size - 1) // 2
    return labels, back[S:2 * S].astype(np.int64)


def largest_cluster_segments(rows: torch.Tensor, offsets, eps, min_points):
    """``dbscan_segments`` and then, per segment, the rows of its largest cluster (the most rows, core and border together; a tie
    goes to the lowest cluster number; a segment that is all noise keeps nothing): ``(rows_kept, offsets_kept, lo, hi, index)``,
    shaped like ``clean_segments``' -- all columns and the dtype kept, ``offsets_kept`` [S + 1] a host int64 array, ``lo`` / ``hi``
    [S, 3] float64 (device) the kept rows' extents (+inf / -inf where none stays), ``index`` [M] int64 (device) the kept rows'
    indices into ``rows``, ascending.  One read-back per call, whatever S is: the kept counts with the flag word.  The exceptions are
    ``dbscan_segments``'."""
    _labels, keep, back, lo, hi = _dbscan_device(rows, offsets, eps, min_points, True)
    S = (back.size - 1) // 2
    kept_offsets = _offsets_of(back[:S])
    index = torch.nonzero_static(keep.view(torch.bool), size=int(kept_offsets[-1])).flatten()    # its size is known: no read-back of its own
    return rows.index_select(0, index), kept_offsets, lo, hi, index


def _dbscan_host(rows, offsets, eps, min_points, want_keep: bool):
    e, m, _side = _check_dbscan(eps, min_points)
    rows = np.asarray(rows)
    if rows.ndim != 2 or rows.shape[1] < 3:
        raise ValueError(f"mspa.cloud_segments: rows: expected [N, C >= 3], got {list(rows.shape)}")
    xyz = np.ascontiguousarray(rows[:, :3], dtype=np.float64)
    N = xyz.shape[0]
    off = _offsets(offsets, N)
    S = off.size - 1
    labels = np.full((N,), -1, dtype=np.int32)
    clusters, kept = np.zeros((S,), dtype=np.int32), np.zeros((S,), dtype=np.int32)
    keep = np.zeros((N,), dtype=np.uint8)
    flags = np.zeros((1,), dtype=np.int32)
    _lib.check(_lib.load().mspa_dbscan_segments_host(xyz.ctypes.data, 3, off.ctypes.data, S, e, m, labels.ctypes.data, clusters.ctypes.data,
                                                     keep.ctypes.data if want_keep else None, kept.ctypes.data if want_keep else None,
                                                     flags.ctypes.data))
    _raise_dbscan_flags(int(flags[0]), e)
    return rows, off, labels, clusters.astype(np.int64), keep.astype(bool), kept.astype(np.int64)


def dbscan_segments_host(rows, offsets, eps, min_points):
    """``dbscan_segments`` on the CPU for NumPy input, through the same header (mspa_dbscan_segments_host): NumPy arrays out, the
    same exceptions.  The device's twin for tests and for input that has no device, not a fallback."""
    _rows, _off, labels, clusters, _keep, _kept = _dbscan_host(rows, offsets, eps, min_points, False)
    return labels, clusters


def largest_cluster_segments_host(rows, offsets, eps, min_points):
    """``largest_cluster_segments`` on the CPU for NumPy input, through the same header: NumPy arrays out, the same exceptions."""
    rows, off, _labels, _clusters, keep, kept = _dbscan_host(rows, offsets, eps, min_points, True)
    S = off.size - 1
    kept_offsets = _offsets_of(kept)
    index = np.nonzero(keep)[0].astype(np.int64)
    out = rows[index]
    lo, hi = np.full((S, 3), np.inf), np.full((S, 3), -np.inf)
    for s in range(S):
        part = np.asarray(out[kept_offsets[s]:kept_offsets[s + 1], :3], dtype=np.float64)
        if len(part):
            lo[s], hi[s] = part.min(axis=0), part.max(axis=0)
    return out, kept_offsets, lo, hi, index


UPRIGHT_NON_FINITE, UPRIGHT_OUT_OF_WINDOW, UPRIGHT_CAP_REACHED = 1, 2, 4      # csrc/upright_box_core.h: the bits of the flag word
UPRIGHT_EDGE_TILE = 256                                                      # csrc/upright_segments.hip: edges one workgroup takes


def _raise_upright_flags(flags: int) -> None:
    if flags & UPRIGHT_NON_FINITE:
        raise ValueError("upright_boxes: the cloud has non-finite coordinates")
    if flags & UPRIGHT_OUT_OF_WINDOW:
        raise ValueError("upright_boxes: a non-zero |x| or |y| lies outside [2^-200, 2^200] (csrc/upright_box_core.h)")
    if flags & UPRIGHT_CAP_REACHED:
        raise RuntimeError("upright_boxes: a hull chain reached its iteration cap (csrc/upright_box_core.h)")


def _upright_device(rows: torch.Tensor, offsets):
    """The device op: (boxes [S, 8] float64, hull index [H] int64, hull_offsets [S + 1] host, chosen edges [S] int32, survivors [S]
    host int64).  Holds THE two read-backs of ``upright_boxes_segments`` and ``footprint_hull_segments``."""
    _require(isinstance(rows, torch.Tensor) and rows.is_cuda and rows.dim() == 2 and rows.shape[1] >= 3, "rows: a device tensor [N, C >= 3]")
    xyz = _check("rows", rows[:, :3].to(torch.float64).contiguous(), torch.float64, (None, 3))
    N = int(xyz.shape[0])
    off = _offsets(offsets, N)
    _require(N <= 1 << 30, f"rows: at most 2^30 rows, got {N}")
    S = off.size - 1
    dev = rows.device
    boxes = torch.full((S, 8), float("nan"), dtype=torch.float64, device=dev)
    edges = torch.full((S,), -1, dtype=torch.int32, device=dev)
    if N == 0:
        return boxes, torch.empty((0,), dtype=torch.int64, device=dev), np.zeros((S + 1,), dtype=np.int64), edges, np.zeros((S,), dtype=np.int64)
    lib = _lib.load()
    tile_base = np.zeros((S + 1,), dtype=np.int64)
    _lib.check(lib.mspa_voxel_segments_tables_host(off.ctypes.data, S, tile_base.ctypes.data))
    off_dev, base_dev = _upload(off, tile_base, device=dev)
    rows_list = torch.empty((N,), dtype=torch.int64, device=dev)
    ext = torch.empty((S, 10), dtype=torch.float64, device=dev)
    seg = torch.empty((S + 1,), dtype=torch.int32, device=dev)
    work = _workspace(int(lib.mspa_upright_filter_workspace_bytes(off.ctypes.data, S)), dev)
    _lib.check(lib.mspa_upright_filter_device(_ptr(xyz), 3, off.ctypes.data, S, _ptr(off_dev), _ptr(base_dev), _ptr(rows_list), _ptr(ext), _ptr(seg),
                                              _ptr(work), int(work.numel()), _stream_ptr()))
    back = seg.cpu().numpy()                               # THE first read-back
    _raise_upright_flags(int(back[S]))
    survivors = back[:S].astype(np.int64)
    kept_off = _offsets_of(survivors)
    M = int(kept_off[-1])
    kept_dev, = _upload(kept_off, device=dev)
    index = rows_list[:M]
    xy = xyz.index_select(0, index)[:, :2]
    order = torch.sort(xy[:, 1], stable=True).indices      # stably by y, by x, by segment: (segment, x, y), ties in row order
    order = order.gather(0, torch.sort(xy[:, 0].gather(0, order), stable=True).indices)
    if S > 1:
        segment = torch.searchsorted(kept_dev[1:], torch.arange(M, dtype=torch.int64, device=dev), right=True)
        order = order.gather(0, torch.sort(segment.gather(0, order), stable=True).indices)
    pts = xy.index_select(0, order).contiguous()
    row = index.gather(0, order)
    stack = torch.empty((2, M), dtype=torch.int32, device=dev)
    counts = torch.empty((2 * S + 1,), dtype=torch.int32, device=dev)
    _lib.check(lib.mspa_upright_hull_device(_ptr(pts), kept_off.ctypes.data, S, _ptr(kept_dev), _ptr(stack), _ptr(counts), _stream_ptr()))
    back = counts.cpu().numpy()                            # THE second read-back
    _raise_upright_flags(int(back[2 * S]))
    lower, upper = back[0:2 * S:2].astype(np.int64), back[1:2 * S:2].astype(np.int64)
    hull_off = _offsets_of(np.where(lower <= 0, 0, np.where((lower == 1) | (upper <= 1), 1, lower + upper - 2)))
    H = int(hull_off[-1])
    edge_base = _offsets_of((np.diff(hull_off) + UPRIGHT_EDGE_TILE - 1) // UPRIGHT_EDGE_TILE)
    hull_dev, edge_base_dev = _upload(hull_off, edge_base, device=dev)
    hull_index = torch.empty((H,), dtype=torch.int64, device=dev)
    work = _workspace(int(lib.mspa_upright_boxes_workspace_bytes(hull_off.ctypes.data, S)), dev)
    _lib.check(lib.mspa_upright_boxes_device(_ptr(pts), _ptr(row), kept_off.ctypes.data, hull_off.ctypes.data, S, _ptr(kept_dev), _ptr(hull_dev),
                                             _ptr(edge_base_dev), _ptr(stack), _ptr(counts), _ptr(ext), _ptr(hull_index), _ptr(edges), _ptr(boxes),
                                             _ptr(work), int(work.numel()), _stream_ptr()))
    return boxes, hull_index, hull_off, edges, survivors


def upright_boxes_segments(rows: torch.Tensor, offsets, want_hull: bool = False, want_edges: bool = False, want_survivors: bool = False):
    """A batch ``rows`` [N, C >= 3] (device; xyz in front, float64 or a dtype that widens to it exactly; extra columns are not read)
    and host ``offsets`` [S + 1] -> ``boxes`` [S, 8] float64 (device): per segment the upright minimal box
    ``[cx, cy, cz, length, width, height, ux, uy]`` -- the z extent of the segment (``cz`` and ``height`` are ``calculate_aabb``'s) times
    the minimum-area rectangle around the convex hull of its (x, y) footprint; ``length >= width``, ``(ux, uy)`` the unit direction of
    the length with ``ux > 0``, or ``ux == 0`` and ``uy > 0``.  An empty segment gives eight NaN; one distinct (x, y) gives sizes 0 and the
    axis (1, 0).  The rule is csrc/upright_box_core.h's: the hull is the exact one (``footprint_hull_segments``), the rectangle is
    the all-edges one -- for every hull edge the spans of the hull along and across it, ``m = (along * across) / (d . d)``, the lowest
    edge with the smallest ``m`` -- and every step is one float64 operation in the header's order, so the boxes are the host twin's
    bit for bit and the same bits on every run.  ``want_hull`` adds ``(index, hull_offsets)``, ``want_edges`` the chosen edges [S]
    int32 (device; -1 for an empty segment), ``want_survivors`` the rows per segment [S] (host int64) that the device's filter left
    for the hull.  At most two read-backs per call, whatever S is: the survivor counts with the flag word, and the hull counts with
    the flag word.  A non-finite x, y or z, or a non-zero ``|x|`` or ``|y|`` outside [2^-200, 2^200], raises ValueError.  torch is
    plumbing: the three stable sorts of the survivors (two when S = 1)."""
    boxes, index, hull_offsets, edges, survivors = _upright_device(rows, offsets)
    out = (boxes,) + ((index, hull_offsets) if want_hull else ()) + ((edges,) if want_edges else ()) + ((survivors,) if want_survivors else ())
    return out[0] if len(out) == 1 else out


def footprint_hull_segments(rows: torch.Tensor, offsets):
    """A batch ``rows`` [N, C >= 3] (device) and host ``offsets`` [S + 1] -> ``(index [H] int64 device, hull_offsets [S + 1] host
    int64)``: per segment the strict convex hull of its distinct (x, y) pairs as indices into ``rows``, counter-clockwise from the
    lexicographically smallest vertex (x, then y); collinear boundary points are not vertices; a vertex is the lowest row that holds
    its coordinates; 0 vertices for an empty segment, 1 for one distinct point, 2 for collinear points.  The orientation test is
    exact (csrc/upright_box_core.h), so the hull is the mathematical one and does not depend on the order of the rows.  At most two
    read-backs per call, whatever S is: the survivor counts with the flag word, and the hull counts with the flag word.  The
    exceptions are ``upright_boxes_segments``'."""
    _boxes, index, hull_offsets, _edges, _survivors = _upright_device(rows, offsets)
    return index, hull_offsets


def _upright_host(rows, offsets):
    rows = np.asarray(rows)
    if rows.ndim != 2 or rows.shape[1] < 3:
        raise ValueError(f"mspa.cloud_segments: rows: expected [N, C >= 3], got {list(rows.shape)}")
    xyz = np.ascontiguousarray(rows[:, :3], dtype=np.float64)
    N = xyz.shape[0]
    off = _offsets(offsets, N)
    S = off.size - 1
    index = np.zeros((max(N, 1),), dtype=np.int64)
    hull_off = np.zeros((S + 1,), dtype=np.int64)
    edges = np.full((max(S, 1),), -1, dtype=np.int32)
    boxes = np.full((max(S, 1), 8), np.nan)
    flags = np.zeros((1,), dtype=np.int32)
    _lib.check(_lib.load().mspa_upright_segments_host(xyz.ctypes.data, 3, off.ctypes.data, S, index.ctypes.data, hull_off.ctypes.data,
                                                      edges.ctypes.data, boxes.ctypes.data, flags.ctypes.data))
    _raise_upright_flags(int(flags[0]))
    return boxes[:S], index[:int(hull_off[-1])].copy(), hull_off, edges[:S]


def upright_boxes_segments_host(rows, offsets, want_hull: bool = False, want_edges: bool = False):
    """``upright_boxes_segments`` on the CPU for NumPy input, through the same header (mspa_upright_segments_host): NumPy arrays out,
    the same exceptions.  It runs no filter in front of the hull (none can change it).  The device's twin for tests and for input
    that has no device, not a fallback."""
    boxes, index, hull_offsets, edges = _upright_host(rows, offsets)
    out = (boxes,) + ((index, hull_offsets) if want_hull else ()) + ((edges,) if want_edges else ())
    return out[0] if len(out) == 1 else out


def footprint_hull_segments_host(rows, offsets):
    """``footprint_hull_segments`` on the CPU for NumPy input, through the same header: NumPy arrays out, the same exceptions.  The
    device's twin, not a fallback."""
    _boxes, index, hull_offsets, _edges = _upright_host(rows, offsets)
    return index, hull_offsets


def upright_corners(boxes: torch.Tensor) -> torch.Tensor:
    """Upright boxes [..., 8] -> their corners [..., 8, 3]: the four footprint corners counter-clockwise from
    ``centre - length / 2 * u - width / 2 * n`` (``n = (-uy, ux)``) at the lower z, then the same four at the upper z.  Enqueue only."""
    zero = torch.zeros_like(boxes[..., 0])
    centre = boxes[..., :3]
    u = torch.stack([boxes[..., 6], boxes[..., 7], zero], dim=-1) * (boxes[..., 3:4] / 2)          # half the length along the axis
    n = torch.stack([-boxes[..., 7], boxes[..., 6], zero], dim=-1) * (boxes[..., 4:5] / 2)         # half the width across it
    up = torch.stack([zero, zero, boxes[..., 5] / 2], dim=-1)
    foot = [centre - u - n, centre + u - n, centre + u + n, centre - u + n]
    return torch.stack([c - up for c in foot] + [c + up for c in foot], dim=-2)


def upright_yaw(boxes: torch.Tensor) -> torch.Tensor:
    """Upright boxes [..., 8] -> the angle of the length's direction against +x, ``atan2(uy, ux)``, in (-pi / 2, pi / 2].  Enqueue
    only.  Its last bits are torch's ``atan2``, not pinned by the rule: the rule itself carries the axis, not an angle."""
    return torch.atan2(boxes[..., 7], boxes[..., 6])


def boxes_of(lo: torch.Tensor, hi: torch.Tensor) -> torch.Tensor:
    """Extents lo / hi [..., 3] -> [..., 6]: ``[(hi + lo) / 2, hi - lo]``, what ``ops.calculate_aabb`` returns for the rows they
    span; NaN where lo > hi (the +inf / -inf of a segment without rows).  Enqueue only."""
    box = torch.cat([(hi + lo) / 2, hi - lo], dim=-1)
    return torch.where((lo > hi).any(dim=-1, keepdim=True), torch.full_like(box, float("nan")), box)


def iou_3d(boxes: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """``ops.calculate_iou_3d``'s device branch along a trailing axis: boxes [..., 6] against gt [..., 6] -> [...]; the same torch
    operations in the same order, so each entry equals the single call's.  NaN boxes give NaN."""
    dim = torch.minimum(boxes[..., :3] + boxes[..., 3:] / 2, gt[..., :3] + gt[..., 3:] / 2) - \
        torch.maximum(boxes[..., :3] - boxes[..., 3:] / 2, gt[..., :3] - gt[..., 3:] / 2)
    inter = torch.where((dim > 0).all(dim=-1), dim.prod(dim=-1), torch.zeros((), dtype=dim.dtype, device=dim.device))
    return inter / (boxes[..., 3:].prod(dim=-1) + gt[..., 3:].prod(dim=-1) - inter)


def _iou_boxes(name: str, boxes, trailing: int) -> torch.Tensor:
    """A box argument of the upright IoU, checked: a float64 device tensor [..., 8] with at least ``trailing`` axes -> itself."""
    ok = isinstance(boxes, torch.Tensor) and boxes.dim() >= trailing and boxes.shape[-1] == 8 and boxes.dtype == torch.float64
    if not ok or not boxes.is_cuda:                        # _check words the refusal (and says so where there is no device at all)
        _check(name, boxes, torch.float64, (None,) * (trailing - 1) + (8,))
        _require(False, f"{name}: a float64 device tensor [..., 8]")
    return boxes


def _iou_launch(a2: torch.Tensor, b2: torch.Tensor, G: int, A: int, B: int, mode: int, shape, want_parts: bool):
    a2 = _check("a", a2.contiguous(), torch.float64, (None, 8))
    b2 = _check("b", b2.contiguous(), torch.float64, (None, 8))
    out = torch.empty(tuple(shape), dtype=torch.float64, device=a2.device)
    parts = torch.empty(tuple(shape) + (2,), dtype=torch.float64, device=a2.device) if want_parts else None
    _lib.check(_lib.load().mspa_upright_iou_device(_ptr(a2), int(a2.shape[0]), _ptr(b2), int(b2.shape[0]), G, A, B, mode, _ptr(out), _ptr(parts),
                                                   _stream_ptr()))
    return (out, parts) if want_parts else out


def _pair_shapes(a_shape, b_shape):
    """The leading shapes of two pair arguments -> the output's shape; equal, or one of them a single box."""
    a_lead, b_lead = tuple(a_shape[:-1]), tuple(b_shape[:-1])
    a_single, b_single = int(np.prod(a_lead)) == 1 and len(a_lead) <= 1, int(np.prod(b_lead)) == 1 and len(b_lead) <= 1
    _require(a_lead == b_lead or a_single or b_single, f"a and b: equal leading shapes, or one of them a single box; got {list(a_shape)} and {list(b_shape)}")
    return a_lead if a_lead == b_lead or b_single else b_lead


def upright_iou(a: torch.Tensor, b: torch.Tensor, want_parts: bool = False):
    """Upright boxes ``a`` [..., 8] against ``b`` [..., 8] (float64 device tensors ``[cx, cy, cz, length, width, height, ux, uy]`` with
    equal leading shapes, or one of them a single box [8] / [1, 8] against all of the other) -> [...] float64 (device): per pair the
    volume of the intersection over that of the union.  The rule is csrc/upright_iou_core.h's: the footprints are the rectangles
    ``upright_corners`` draws, the one of the smaller ``length * width`` is clipped against the other by Sutherland-Hodgman in that
    one's frame, the area is a shoelace sum, ``inter = area * dz`` with ``iou_3d``'s z overlap, and ``iou = inter / (va + vb - inter)``
    with ``v = (length * width) * height``.  Every step is one float64 operation in the header's order, so the values are the host
    twin's bit for bit, the same bits on every run, and ``upright_iou(a, b)`` and ``upright_iou(b, a)`` are the same bits.  A box
    with a non-finite value (the eight NaN of an empty segment), a negative size, an axis with ``|ux^2 + uy^2 - 1| > 2^-20`` or a
    non-zero centre or size outside [2^-200, 2^200] gives NaN, not an exception; two boxes equal in all eight values give exactly
    1.0 (NaN with zero volume); otherwise ``0 <= iou <= 1``, or NaN where both volumes are zero.  ``want_parts`` adds [..., 2]: the
    footprint intersection area and the z overlap.  Enqueue only: one launch on the current stream and nothing is read back.  A dtype
    other than float64 or a last axis other than 8 raises ValueError."""
    a, b = _iou_boxes("a", a, 1), _iou_boxes("b", b, 1)
    shape = _pair_shapes(a.shape, b.shape)
    return _iou_launch(a.reshape(-1, 8), b.reshape(-1, 8), 0, 0, 0, _lib.UPRIGHT_IOU_PAIRS, shape, want_parts)


def upright_iou_matrix(a: torch.Tensor, b: torch.Tensor, want_parts: bool = False):
    """Upright boxes ``a`` [..., A, 8] against ``b`` [..., B, 8] (float64 device tensors with equal leading shapes) -> [..., A, B]
    float64 (device): entry (i, j) is ``upright_iou(a[..., i, :], b[..., j, :])``, bit for bit; the matrix of a set against itself
    equals its transpose byte for byte and has 1.0 on its diagonal (NaN for a refused or zero-volume box).  ``want_parts`` adds
    [..., A, B, 2].  Enqueue only: one launch on the current stream and nothing is read back.  The exceptions are ``upright_iou``'s."""
    a, b = _iou_boxes("a", a, 2), _iou_boxes("b", b, 2)
    _require(a.shape[:-2] == b.shape[:-2], f"a and b: equal leading shapes in front of [A, 8] and [B, 8]; got {list(a.shape)} and {list(b.shape)}")
    G, A, B = int(np.prod(a.shape[:-2])), int(a.shape[-2]), int(b.shape[-2])
    return _iou_launch(a.reshape(-1, 8), b.reshape(-1, 8), G, A, B, _lib.UPRIGHT_IOU_MATRIX, tuple(a.shape[:-2]) + (A, B), want_parts)


def _iou_boxes_host(name: str, boxes, trailing: int) -> np.ndarray:
    boxes = np.asarray(boxes)
    if boxes.dtype != np.float64 or boxes.ndim < trailing or boxes.shape[-1] != 8:
        raise ValueError(f"mspa.cloud_segments: {name}: expected float64 [..., 8], got {boxes.dtype} {list(boxes.shape)}")
    return boxes


def _iou_host(a2, b2, G, A, B, mode, shape, want_parts):
    a2, b2 = np.ascontiguousarray(a2), np.ascontiguousarray(b2)
    out = np.empty(tuple(shape), dtype=np.float64)
    parts = np.empty(tuple(shape) + (2,), dtype=np.float64) if want_parts else None
    _lib.check(_lib.load().mspa_upright_iou_host(a2.ctypes.data, a2.shape[0], b2.ctypes.data, b2.shape[0], G, A, B, mode, out.ctypes.data,
                                                 parts.ctypes.data if want_parts else None))
    return (out, parts) if want_parts else out


def upright_iou_host(a, b, want_parts: bool = False):
    """``upright_iou`` on the CPU for NumPy input, through the same header (mspa_upright_iou_host): NumPy arrays out, the same
    ValueErrors.  The device's twin for tests and for input that has no device, not a fallback."""
    a, b = _iou_boxes_host("a", a, 1), _iou_boxes_host("b", b, 1)
    try:
        shape = _pair_shapes(a.shape, b.shape)
    except ValueError as e:
        raise ValueError(str(e).replace("mspa.engine", "mspa.cloud_segments")) from None
    return _iou_host(a.reshape(-1, 8), b.reshape(-1, 8), 0, 0, 0, _lib.UPRIGHT_IOU_PAIRS, shape, want_parts)


def upright_iou_matrix_host(a, b, want_parts: bool = False):
    """``upright_iou_matrix`` on the CPU for NumPy input, through the same header: NumPy arrays out, the same ValueErrors.  The
    device's twin, not a fallback."""
    a, b = _iou_boxes_host("a", a, 2), _iou_boxes_host("b", b, 2)
    if a.shape[:-2] != b.shape[:-2]:
        raise ValueError(f"mspa.cloud_segments: a and b: equal leading shapes in front of [A, 8] and [B, 8]; got {list(a.shape)} and {list(b.shape)}")
    G, A, B = int(np.prod(a.shape[:-2])), int(a.shape[-2]), int(b.shape[-2])
    return _iou_host(a.reshape(-1, 8), b.reshape(-1, 8), G, A, B, _lib.UPRIGHT_IOU_MATRIX, tuple(a.shape[:-2]) + (A, B), want_parts)


def upright_iou_bound_host(a, b):
    """Pairs ``a`` [P, 8] and ``b`` [P, 8] (NumPy float64) -> ``(area_bound [P], iou_bound [P])``: csrc/upright_iou_core.h's
    forward-error bounds of ``upright_iou``'s footprint area and IoU against the exact rational values for the same doubles; NaN for
    a refused pair, and an IoU bound of NaN where the IoU is."""
    a, b = _iou_boxes_host("a", a, 2), _iou_boxes_host("b", b, 2)
    if a.ndim != 2 or a.shape != b.shape:
        raise ValueError(f"mspa.cloud_segments: a and b: [P, 8] each, got {list(a.shape)} and {list(b.shape)}")
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    area, iou = np.empty((a.shape[0],)), np.empty((a.shape[0],))
    _lib.check(_lib.load().mspa_upright_iou_bound_host(a.ctypes.data, b.ctypes.data, a.shape[0], area.ctypes.data, iou.ctypes.data))
    return area, iou


def upright_of_aabb(boxes6: torch.Tensor) -> torch.Tensor:
    """``calculate_aabb`` boxes [..., 6] ``[cx, cy, cz, dx, dy, dz]`` -> the same boxes as upright ones [..., 8]: length = max(dx, dy),
    width = min(dx, dy), height = dz, the axis (1, 0) where dx >= dy and (0, 1) where dy > dx.  A box with a NaN is eight NaN.
    torch operations only.  Enqueue only."""
    dx, dy = boxes6[..., 3], boxes6[..., 4]
    turned = dy > dx
    one, zero = torch.ones_like(dx), torch.zeros_like(dx)
    out = torch.stack([boxes6[..., 0], boxes6[..., 1], boxes6[..., 2], torch.maximum(dx, dy), torch.minimum(dx, dy), boxes6[..., 5],
                       torch.where(turned, zero, one), torch.where(turned, one, zero)], dim=-1)
    return torch.where(torch.isnan(boxes6).any(dim=-1, keepdim=True), torch.full_like(out, float("nan")), out)


# ---- nearest-point distances between the clouds of two batches (csrc/cloud_distance.hip, rule in csrc/cloud_distance_core.h) ------------

FIT_KEYS = ("rows", "finite", "within", "sum", "sum_sq", "max")
ORDER_QUERIES = True                              # TargetIndex.nearest: lanes take the output rows in the order of their cells (measured)


def _grid_k_of(_grid_k) -> int:
    return _lib.CLOUD_DISTANCE_GRID_K if _grid_k is None else _knn_check(_grid_k)


def _cap_of(max_distance) -> float:
    """``max_distance`` (None: no cap) -> what the entry points take: finite and > 0, or +inf for none."""
    if max_distance is None:
        return float("inf")
    cap = float(max_distance)
    _require(0.0 < cap < float("inf"), f"max_distance: finite and > 0, got {max_distance}")
    return cap


def _tau_of(tau) -> float:
    tau = float(tau)
    _require(0.0 <= tau < float("inf"), f"tau: finite and >= 0, got {tau}")
    return tau


def _pair_tables(q_off: np.ndarray, St: int, pairs):
    """``(pairs [P, 2] host int64, out_offsets [P + 1] host int64)`` of a query batch's offsets, the number of target segments and a
    caller's pair table (None: pair s is (s, s), which needs as many segments on either side)."""
    Sq = q_off.size - 1
    if pairs is None:
        _require(Sq == St, f"pairs: none needs as many query segments as target segments, got {Sq} and {St}")
        pairs = np.repeat(np.arange(Sq, dtype=np.int64), 2).reshape(Sq, 2)
    else:
        if isinstance(pairs, torch.Tensor):
            _require(not pairs.is_cuda, "pairs: a host array (the launch shapes come from it)")
            pairs = pairs.numpy()
        pairs = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2) if np.size(pairs) == 0 else np.ascontiguousarray(pairs, dtype=np.int64)
        _require(pairs.ndim == 2 and pairs.shape[1] == 2, f"pairs: [P, 2], got {list(pairs.shape)}")
        _require(pairs.shape[0] <= _lib.CLOUD_DISTANCE_MAX_PAIRS, f"pairs: at most 2^24 pairs, got {pairs.shape[0]}")
        _require(bool(((pairs >= 0) & (pairs < np.array([Sq, St]))).all()),
                 f"pairs: (query segment, target segment) inside [0, {Sq}) x [0, {St})")
    out_offsets = _offsets_of(np.diff(q_off)[pairs[:, 0]])
    _require(int(out_offsets[-1]) <= _lib.CLOUD_DISTANCE_MAX_ROWS, f"pairs: at most 2^30 output rows, got {int(out_offsets[-1])}")
    return pairs, out_offsets


def _xyz_of(name: str, rows) -> torch.Tensor:
    _require(isinstance(rows, torch.Tensor) and rows.is_cuda and rows.dim() == 2 and rows.shape[1] >= 3, f"{name}: a device tensor [N, C >= 3]")
    return _check(name, rows[:, :3].to(torch.float64).contiguous(), torch.float64, (None, 3))


class TargetIndex:
    """The search structure of a batch of target clouds on the device (``target_index``): the rows sorted by grid cell per segment
    (``pts`` [N, 3] float64), their original rows (``order`` [N] int64), the first sorted row of every cell (``starts`` int32), the
    grid records and the offsets -- on the device, with the host copies the entry points check.  Build it once, query it any number
    of times."""

    def __init__(self, offsets, grid_k, grids, off_dev, grids_dev, base_dev, pts, order, starts, device):
        self.offsets, self.grid_k, self.grids, self.device = offsets, grid_k, grids, device
        self.off_dev, self.grids_dev, self.base_dev, self.pts, self.order, self.starts = off_dev, grids_dev, base_dev, pts, order, starts
        self.xyz = None                                                        # the targets in their own order, once ``targets()`` was asked

    def nearest(self, queries: torch.Tensor, q_offsets, pairs=None, max_distance=None, want_index: bool = True, want_evals: bool = False,
                _ordered=None) -> dict:
        """A batch ``queries`` [Nq, C >= 3] (device; xyz in front, float64 or a dtype that widens to it exactly) with host ``q_offsets``
        [Sq + 1] and a host pair table ``pairs`` [P, 2] int64 -- pair p searches the rows of query segment ``pairs[p, 0]`` in target
        segment ``pairs[p, 1]``; None: pair s is (s, s) -- -> a dict: ``distance`` [M] float64 (device), per output row the distance to
        the nearest row of the pair's target segment; ``index`` [M] int64 (device; with ``want_index``), that row's index into the
        targets the index was built from, the lowest among equally near ones; ``offsets`` [P + 1] host int64, the output rows of pair
        p are ``offsets[p]:offsets[p + 1]``, as many as the query segment has; ``evals`` [M] int32 (with ``want_evals``), the distances
        each row evaluated.  The rule is csrc/cloud_distance_core.h's: ``d2 = (dx*dx + dy*dy) + dz*dz`` in float64 and
        ``distance = sqrt(min d2)``, the bits of a brute force over all rows; an empty target segment gives +inf and -1, a query row
        with a non-finite coordinate NaN and -1 (no exception); with ``max_distance`` (finite, > 0) a row farther than that gives +inf
        and -1 and every other row is unchanged -- without it a query far from its target walks the target's whole grid.  The lanes
        take the output rows in the order of their cell in the target's grid (a keys pass and one ``torch.sort`` in front of the
        search; ``_ordered=False``: in input order); the outputs are the same bytes either way.  Enqueue only: the keys pass, the sort
        and the search on the current stream, the host tables go up through pinned memory and nothing is read back."""
        xyz = _xyz_of("queries", queries)
        q_off = _offsets(q_offsets, int(xyz.shape[0]))
        St = self.offsets.size - 1
        pairs, out_offsets = _pair_tables(q_off, St, pairs)
        cap = _cap_of(max_distance)
        P, M, dev = pairs.shape[0], int(out_offsets[-1]), self.device
        _require(xyz.device == dev, f"queries: on the index's device {dev}, got {xyz.device}")
        out = {"distance": torch.empty((M,), dtype=torch.float64, device=dev), "offsets": out_offsets}
        if want_index:
            out["index"] = torch.empty((M,), dtype=torch.int64, device=dev)
        if want_evals:
            out["evals"] = torch.empty((M,), dtype=torch.int32, device=dev)
        if M:
            lib = _lib.load()
            q_dev, pairs_dev, out_dev = _upload(q_off, pairs, out_offsets, device=dev)
            perm = None
            if ORDER_QUERIES if _ordered is None else _ordered:             # lanes of a wave then walk neighbouring cells: the same bytes out
                keys = torch.empty((M,), dtype=torch.int64, device=dev)
                _lib.check(lib.mspa_cloud_distance_keys_device(self.offsets.ctypes.data, St, self.grid_k, self.grids.ctypes.data, _ptr(self.grids_dev),
                                                               _ptr(xyz), q_off.ctypes.data, q_off.size - 1, _ptr(q_dev), pairs.ctypes.data,
                                                               _ptr(pairs_dev), P, out_offsets.ctypes.data, _ptr(out_dev), _ptr(keys), _stream_ptr()))
                perm = torch.sort(keys).indices
            _lib.check(lib.mspa_cloud_distance_device(
                _ptr(self.pts), _ptr(self.starts), int(self.starts.numel()), _ptr(self.order), self.offsets.ctypes.data, St, self.grid_k, self.grids.ctypes.data,
                _ptr(self.off_dev), _ptr(self.grids_dev), _ptr(self.base_dev), _ptr(xyz), q_off.ctypes.data, q_off.size - 1, _ptr(q_dev),
                pairs.ctypes.data, _ptr(pairs_dev), P, out_offsets.ctypes.data, _ptr(out_dev), _ptr(perm), cap, _ptr(out["distance"]), _ptr(out.get("index")),
                _ptr(out.get("evals")), _stream_ptr()))
        return out

    def register(self, queries, q_offsets, pairs=None, *, max_distance, iterations: int = 30, init=None, sync_every=None,
                  want_history: bool = False, estimation: str = "point_to_point", normals=None) -> dict:
        """Point-to-point ICP of every pair: a batch ``queries`` [Nq, C >= 3] (device) with host ``q_offsets`` and the host pair table of
        ``nearest`` -> a dict of device tensors: ``R`` [P, 3, 3] and ``t`` [P, 3] float64, the transform that carries pair p's query
        segment onto its target segment; ``status`` [P] int32 and ``used`` [P] int64 of the last fit (``rigid_fit_segments``');
        ``converged_at`` [P] int64, the first iteration whose fit returned the transform it started from bit for bit, -1 if none did;
        ``fitness`` [P] = finite / rows and ``inlier_rmse`` [P] = sqrt(sum_sq / finite) of ``fit_segments`` under the final transform
        (Open3D's two result fields); ``offsets`` [P + 1] host int64.  With T_0 = ``init`` ([P, 4, 4] or [P, 3, 4], host or device; None:
        the identity), iteration k transforms the ORIGINAL query rows by T_k, searches them with the cap ``max_distance`` (required,
        finite, > 0: Open3D's max_correspondence_distance) and fits the original rows to their matches: the fit IS T_(k+1), no
        transforms are composed, equal correspondences give equal bits, and a pair that has converged reproduces its 12 numbers from
        then on.  A pair whose fit is not ok keeps its transform.  With ``want_history`` also ``history_used`` [K, P] int64 and
        ``history_rmse`` [K, P] float64, the rows and the rmse of the correspondences each fit used.  ``iterations + 1`` searches.
        Enqueue only: every launch on the current stream, the host tables go up once through pinned memory and nothing is read back --
        zero host synchronisations.  With ``sync_every=n`` instead: ONE read-back of ``converged_at`` (8 P bytes) after every n
        iterations and after the last, ceil(iterations / n) read-backs at most, and the loop ends at the first that shows no -1; the
        result is byte for byte the full loop's, because every pair then sits at its fixed point (``all_converged``: what the last
        read-back showed).
        ``estimation="point_to_plane"`` with ``normals`` ([Nt, 3] float64 on the device: the normals of the index's targets in their
        own order, ``normals_segments``') puts ``plane_fit_segments``' step in the fit's place: T_(k+1) is T_k moved by one linearised
        point-to-plane step (rule in csrc/cloud_align_plane_core.h), its rotation rebuilt from a normalised quaternion every step;
        ``status`` is then few below 6 used rows and degenerate where the matched normals leave a motion unconstrained (a flat
        target), and ``history_rmse`` stays the point distances'.  ``converged_at`` is the same rule, but a linearised step need not
        ever reproduce its transform bit for bit: ``iterations`` is then the stop.  The same searches, launches in the fit's place
        and read-backs.  The default is the point-to-point loop above, byte for byte, with its launches."""
        xyz = _xyz_of("queries", queries)
        q_off = _offsets(q_offsets, int(xyz.shape[0]))
        St = self.offsets.size - 1
        pairs, out_offsets = _pair_tables(q_off, St, pairs)
        cap = _required_cap(max_distance)
        K, every = _iterations_of(iterations, sync_every)
        P, M, dev = pairs.shape[0], int(out_offsets[-1]), self.device
        _require(xyz.device == dev, f"queries: on the index's device {dev}, got {xyz.device}")
        plane = _estimation_of(estimation, normals)
        if plane:
            normals = _normals_of(normals, int(self.pts.shape[0]), dev)
        T = _transforms_of(init, P, dev)
        f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)     # noqa: E731
        i64 = lambda *shape: torch.empty(shape, dtype=torch.int64, device=dev)       # noqa: E731
        out = {"status": torch.empty((P,), dtype=torch.int32, device=dev), "used": i64(P), "converged_at": torch.full((P,), -1, dtype=torch.int64, device=dev),
               "offsets": out_offsets}
        if want_history:
            out["history_used"], out["history_rmse"] = i64(K, P), f64(K, P)
        if P == 0:
            out["R"], out["t"] = _split(T)
            out["fitness"], out["inlier_rmse"] = f64(0), f64(0)
            return out
        lib = _lib.load()
        tabs = _AlignTables(q_off, pairs, out_offsets, St, dev)
        targets = self.targets()
        moved, distance, index, moments, T_next = f64(M, 3), f64(M), i64(M), f64(P, 32 if plane else 16), f64(P, 12)
        summary = {name: (i64(P) if name in FIT_KEYS[:3] else f64(P)) for name in FIT_KEYS}

        def search(T_now):
            tabs.transform(xyz, T_now, moved)
            if not M:
                return
            perm = None
            if ORDER_QUERIES:
                keys = i64(M)
                _lib.check(lib.mspa_cloud_distance_keys_device(self.offsets.ctypes.data, St, self.grid_k, self.grids.ctypes.data, _ptr(self.grids_dev),
                                                               _ptr(moved), out_offsets.ctypes.data, P, _ptr(tabs.out_dev), tabs.search_pairs.ctypes.data,
                                                               _ptr(tabs.search_dev), P, out_offsets.ctypes.data, _ptr(tabs.out_dev), _ptr(keys), _stream_ptr()))
                perm = torch.sort(keys).indices
            _lib.check(lib.mspa_cloud_distance_device(
                _ptr(self.pts), _ptr(self.starts), int(self.starts.numel()), _ptr(self.order), self.offsets.ctypes.data, St, self.grid_k, self.grids.ctypes.data,
                _ptr(self.off_dev), _ptr(self.grids_dev), _ptr(self.base_dev), _ptr(moved), out_offsets.ctypes.data, P, _ptr(tabs.out_dev),
                tabs.search_pairs.ctypes.data, _ptr(tabs.search_dev), P, out_offsets.ctypes.data, _ptr(tabs.out_dev), _ptr(perm), cap, _ptr(distance),
                _ptr(index), None, _stream_ptr()))

        def summarise():
            _lib.check(lib.mspa_cloud_distance_fit_device(_ptr(distance), out_offsets.ctypes.data, P, 0.0, _ptr(tabs.out_dev),
                                                          *(_ptr(summary[name]) for name in FIT_KEYS), _stream_ptr()))
            return summary["finite"].to(torch.float64), torch.sqrt(summary["sum_sq"] / summary["finite"].to(torch.float64))

        done = K
        for k in range(K):
            search(T)
            if plane:
                tabs.plane_fit(xyz, targets, normals, index, T, k, moments, T_next, out["used"], out["status"], None, out["converged_at"])
            else:
                tabs.fit(xyz, targets, index, T, k, moments, T_next, out["used"], out["status"], None, out["converged_at"])
            T, T_next = T_next, T
            if want_history:
                out["history_used"][k].copy_(out["used"])
                out["history_rmse"][k].copy_(summarise()[1])
            if sync_every is not None and ((k + 1) % every == 0 or k + 1 == K):
                out["all_converged"] = bool((out["converged_at"].cpu() != -1).all())          # THE read-back of sync_every
                if out["all_converged"]:
                    done = k + 1
                    break
        if want_history and done < K:                                # every pair sits at its fixed point: the full loop repeats this row
            out["history_used"][done:] = out["history_used"][done - 1]
            out["history_rmse"][done:] = out["history_rmse"][done - 1]
        search(T)
        finite, rmse = summarise()
        out["fitness"], out["inlier_rmse"] = finite / summary["rows"].to(torch.float64), rmse
        out["R"], out["t"] = _split(T)
        return out

    def targets(self) -> torch.Tensor:
        """The targets the index was built from, [N, 3] float64 in their own order: ``pts`` scattered back through ``order``, once per
        index (enqueue only)."""
        if self.xyz is None:
            self.xyz = torch.empty_like(self.pts)
            self.xyz[self.order] = self.pts
        return self.xyz


def target_index(targets: torch.Tensor, offsets, _grid_k=None) -> TargetIndex:
    """A batch ``targets`` [N, C >= 3] (device; xyz in front, float64 or a dtype that widens to it exactly) with host ``offsets``
    [S + 1] -> its ``TargetIndex``: per segment the grid ``knn_mean_distance_segments`` builds (the box of the per-axis order
    statistics of rank n_s // 100 and n_s - 1 - n_s // 100), the rows sorted by cell with ONE sort of the whole batch, and the first
    sorted row of every cell.  One read-back per call, whatever S is: the boxes of all segments with the flag that every coordinate
    is finite (``knn_mean_distance_segments``'); non-finite coordinates raise its ValueError.  ``_grid_k`` sizes the cells; results
    do not depend on it."""
    xyz = _xyz_of("targets", targets)
    N, dev = int(xyz.shape[0]), xyz.device
    off = _offsets(offsets, N)
    _require(N <= 1 << 30, f"targets: at most 2^30 rows, got {N}")
    k, S = _grid_k_of(_grid_k), off.size - 1
    lib = _lib.load()
    cell_base = np.zeros((S + 1,), dtype=np.int64)
    _lib.check(lib.mspa_knn_segments_tables_host(off.ctypes.data, S, k, cell_base.ctypes.data))
    slots = int(cell_base[S]) + S
    starts = torch.zeros((max(slots, 1),), dtype=torch.int32, device=dev)      # the slots behind a segment's cells are never written
    pts = torch.empty((N, 3), dtype=torch.float64, device=dev)
    if N == 0:
        grids = np.zeros((S, _lib.KNN_GRID_BYTES), dtype=np.uint8)
        off_dev, grids_dev, base_dev = _upload(off, grids, cell_base, device=dev)
        return TargetIndex(off, k, grids, off_dev, grids_dev, base_dev, pts, torch.empty((0,), dtype=torch.int64, device=dev), starts, dev)
    grids, off_dev, grids_dev, base_dev = _search_tables(xyz, off, k)
    keys = torch.empty((N,), dtype=torch.int64, device=dev)
    _lib.check(lib.mspa_knn_segments_cells_device(_ptr(xyz), off.ctypes.data, S, grids.ctypes.data, _ptr(off_dev), _ptr(grids_dev),
                                                  _ptr(base_dev), _ptr(keys), _stream_ptr()))
    order = torch.sort(keys, stable=True).indices
    _lib.check(lib.mspa_knn_segments_index_device(_ptr(xyz), off.ctypes.data, S, k, grids.ctypes.data, _ptr(off_dev), _ptr(grids_dev), _ptr(base_dev),
                                                  _ptr(order), _ptr(pts), _ptr(keys), _ptr(starts), int(starts.numel()), _stream_ptr()))
    return TargetIndex(off, k, grids, off_dev, grids_dev, base_dev, pts, order, starts, dev)


def nearest_segments(queries: torch.Tensor, q_offsets, targets: torch.Tensor, t_offsets, pairs=None, max_distance=None, want_index: bool = True,
                     want_evals: bool = False, _grid_k=None) -> dict:
    """``target_index(targets, t_offsets).nearest(queries, q_offsets, ...)``: per row of a query segment the distance to, and the row
    of, the nearest point of the target segment its pair names.  ``target_index``' one read-back and its ValueError."""
    return target_index(targets, t_offsets, _grid_k).nearest(queries, q_offsets, pairs, max_distance, want_index, want_evals)


def fit_segments(distance: torch.Tensor, offsets, tau) -> dict:
    """``distance`` [M] float64 (device; ``TargetIndex.nearest``'s) with its host ``offsets`` [P + 1] and a threshold ``tau`` (finite,
    >= 0) -> a dict of six device tensors [P]: ``rows`` int64, the rows of the pair; ``finite`` int64, those with d < inf; ``within``
    int64, those with d <= tau (NaN counts nowhere); ``sum`` and ``sum_sq`` float64, the sums of d and of d * d over the finite rows
    in the order csrc/cloud_segments_core.h states (256 lane sums folded by halving strides; not ``torch.sum``'s); ``max`` float64,
    the largest finite d, -inf where there is none.  Means and shares are one division each and left to the caller.  Enqueue only:
    one launch on the current stream, the offsets go up through pinned memory and nothing is read back."""
    M = _check("distance", distance, torch.float64, (None,)).shape[0]
    off = _offsets(offsets, M)
    tau = _tau_of(tau)
    P, dev = off.size - 1, distance.device
    out = {name: torch.empty((P,), dtype=torch.int64 if name in FIT_KEYS[:3] else torch.float64, device=dev) for name in FIT_KEYS}
    if P:
        off_dev, = _upload(off, device=dev)
        _lib.check(_lib.load().mspa_cloud_distance_fit_device(_ptr(distance), off.ctypes.data, P, tau, _ptr(off_dev),
                                                              *(_ptr(out[name]) for name in FIT_KEYS), _stream_ptr()))
    return out


def cloud_fit_segments(a: torch.Tensor, a_offsets, b: torch.Tensor, b_offsets, tau, max_distance=None) -> dict:
    """Two batches of as many segments, segment s of ``a`` against segment s of ``b``, in both directions -> a dict: ``a_to_b`` and
    ``b_to_a``, the ``fit_segments`` summaries of ``a``'s rows searched in ``b`` and of ``b``'s rows searched in ``a``, and four
    float64 device tensors [S] as torch expressions of the two: ``precision`` = within / rows of a_to_b, ``recall`` = within / rows of
    b_to_a, ``fscore`` = 2 precision recall / (precision + recall) (0 where both are 0), ``chamfer`` = sum / finite of a_to_b plus
    sum / finite of b_to_a, the two mean nearest distances.  NaN where a side is empty.  Two read-backs: one ``target_index`` per
    side."""
    tau = _tau_of(tau)
    ab = nearest_segments(a, a_offsets, b, b_offsets, None, max_distance, want_index=False)
    ba = nearest_segments(b, b_offsets, a, a_offsets, None, max_distance, want_index=False)
    out = {"a_to_b": fit_segments(ab["distance"], ab["offsets"], tau), "b_to_a": fit_segments(ba["distance"], ba["offsets"], tau)}
    out.update(_fit_scores(out["a_to_b"], out["b_to_a"], torch))
    return out


def _fit_scores(ab: dict, ba: dict, xp) -> dict:
    """precision, recall, fscore and chamfer of two summaries, with ``xp`` torch or NumPy (the same float64 operations)."""
    as_f64 = (lambda t: t.to(torch.float64)) if xp is torch else (lambda t: t.astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        precision, recall = as_f64(ab["within"]) / as_f64(ab["rows"]), as_f64(ba["within"]) / as_f64(ba["rows"])
        both = precision + recall
        fscore = xp.where(both == 0, both, (2 * precision * recall) / both)
        chamfer = ab["sum"] / as_f64(ab["finite"]) + ba["sum"] / as_f64(ba["finite"])
    return {"precision": precision, "recall": recall, "fscore": fscore, "chamfer": chamfer}


def nearest_segments_host(queries, q_offsets, targets, t_offsets, pairs=None, max_distance=None, want_evals: bool = False, _grid_k=None) -> dict:
    """``nearest_segments`` on the CPU for NumPy input, through the same headers (mspa_cloud_distance_host): NumPy arrays out
    (``distance``, ``index``, ``offsets`` and, when wanted, ``evals``).  Non-finite targets raise ValueError.  The device's twin for
    tests and for input that has no device, not a fallback."""
    sides = []
    for name, rows in (("queries", queries), ("targets", targets)):
        rows = np.asarray(rows)
        if rows.ndim != 2 or rows.shape[1] < 3:
            raise ValueError(f"mspa.cloud_segments: {name}: expected [N, C >= 3], got {list(rows.shape)}")
        sides.append(np.ascontiguousarray(rows[:, :3], dtype=np.float64))
    q, t = sides
    q_off, t_off = _offsets(q_offsets, q.shape[0]), _offsets(t_offsets, t.shape[0])
    if not np.isfinite(t).all():
        raise ValueError("mspa.cloud_segments: requirement not met: xyz: finite coordinates")
    pairs, out_offsets = _pair_tables(q_off, t_off.size - 1, pairs)
    cap, k = _cap_of(max_distance), _grid_k_of(_grid_k)
    M = int(out_offsets[-1])
    out = {"distance": np.empty((M,), dtype=np.float64), "index": np.empty((M,), dtype=np.int64), "offsets": out_offsets}
    if want_evals:
        out["evals"] = np.empty((M,), dtype=np.int32)
    _lib.check(_lib.load().mspa_cloud_distance_host(t.ctypes.data, t_off.ctypes.data, t_off.size - 1, k, q.ctypes.data, q_off.ctypes.data,
                                                    q_off.size - 1, pairs.ctypes.data, pairs.shape[0], out_offsets.ctypes.data, cap,
                                                    out["distance"].ctypes.data, out["index"].ctypes.data,
                                                    out["evals"].ctypes.data if want_evals else None))
    return out


def fit_segments_host(distance, offsets, tau) -> dict:
    """``fit_segments`` on the CPU for NumPy input, through the same headers (mspa_cloud_distance_fit_host): the same six keys, NumPy
    arrays.  The device's twin, not a fallback."""
    distance = np.ascontiguousarray(distance, dtype=np.float64)
    if distance.ndim != 1:
        raise ValueError(f"mspa.cloud_segments: distance: expected [M], got {list(distance.shape)}")
    off = _offsets(offsets, distance.shape[0])
    tau = _tau_of(tau)
    P = off.size - 1
    out = {name: np.zeros((P,), dtype=np.int64 if name in FIT_KEYS[:3] else np.float64) for name in FIT_KEYS}
    _lib.check(_lib.load().mspa_cloud_distance_fit_host(distance.ctypes.data, off.ctypes.data, P, tau, *(out[name].ctypes.data for name in FIT_KEYS)))
    return out


def cloud_fit_segments_host(a, a_offsets, b, b_offsets, tau, max_distance=None) -> dict:
    """``cloud_fit_segments`` over the host twins, NumPy in and out: for tests on a machine without a GPU."""
    ab = nearest_segments_host(a, a_offsets, b, b_offsets, None, max_distance)
    ba = nearest_segments_host(b, b_offsets, a, a_offsets, None, max_distance)
    out = {"a_to_b": fit_segments_host(ab["distance"], ab["offsets"], tau), "b_to_a": fit_segments_host(ba["distance"], ba["offsets"], tau)}
    out.update(_fit_scores(out["a_to_b"], out["b_to_a"], np))
    return out


# ---- rigid alignment of the clouds of two batches (csrc/cloud_align.hip, rule in csrc/cloud_align_core.h) -------------------------------

ALIGN_STATUS = {"ok": _lib.CLOUD_ALIGN_OK, "few": _lib.CLOUD_ALIGN_FEW, "degenerate": _lib.CLOUD_ALIGN_DEGENERATE}


def _transforms_of(init, P: int, device=None):
    """``init`` (None: the identity; [P, 4, 4] or [P, 3, 4], host or device) -> [P, 12] float64, R row-major then t: a fresh device
    tensor on ``device``, or a NumPy array where ``device`` is None.  A host ``init`` must be finite; a device one is not read back
    (a non-finite transform makes non-finite rows, which the search answers with -1: the pair is FEW and keeps it)."""
    if init is None:
        init = np.tile(np.eye(3, 4), (P, 1, 1))
    on_device = isinstance(init, torch.Tensor) and init.is_cuda
    if not on_device:
        init = np.asarray(init.numpy() if isinstance(init, torch.Tensor) else init, dtype=np.float64)
    _require(init.ndim == 3 and tuple(init.shape) in ((P, 4, 4), (P, 3, 4)), f"init: [P, 4, 4] or [P, 3, 4] with P = {P}, got {list(init.shape)}")
    if on_device:
        _require(device is not None and init.device == device, "init: on the queries' device")
        init = init.to(torch.float64)
        return torch.cat([init[:, :3, :3].reshape(P, 9), init[:, :3, 3]], dim=1).contiguous()
    _require(bool(np.isfinite(init).all()), "init: finite")
    flat = np.ascontiguousarray(np.concatenate([init[:, :3, :3].reshape(P, 9), init[:, :3, 3]], axis=1))
    return flat if device is None else _upload(flat, device=device)[0].clone()


def _fit_pairs(q_off: np.ndarray, pairs):
    """``(pairs, out_offsets, St)`` of a fit or a transform, which name no target batch: the second column only has to be a segment
    number, and St is one more than its largest."""
    if pairs is None:
        return _pair_tables(q_off, q_off.size - 1, None) + (q_off.size - 1,)
    _require(not (isinstance(pairs, torch.Tensor) and pairs.is_cuda), "pairs: a host array (the launch shapes come from it)")
    host = np.asarray(pairs, dtype=np.int64)
    St = int(host[:, 1].max()) + 1 if host.ndim == 2 and host.shape[1:] == (2,) and host.shape[0] else 0
    return _pair_tables(q_off, St, pairs) + (St,)


def _split(T):
    """[P, 12] -> (R [P, 3, 3], t [P, 3]), views."""
    return T[:, :9].reshape(-1, 3, 3), T[:, 9:]


def _join(R, t, P: int, xp):
    _require(tuple(R.shape) == (P, 3, 3) and tuple(t.shape) == (P, 3), f"R and t: [P, 3, 3] and [P, 3] with P = {P}, got {list(R.shape)} and {list(t.shape)}")
    return xp.cat([R.reshape(P, 9), t], dim=1).contiguous() if xp is torch else np.ascontiguousarray(np.concatenate([R.reshape(P, 9), t], axis=1))


class _AlignTables:
    """The host tables of a batch of pairs and their device copies, uploaded once (enqueue only)."""

    def __init__(self, q_off, pairs, out_offsets, St, device):
        self.q_off, self.pairs, self.out, self.St, self.P, self.M = q_off, pairs, out_offsets, St, pairs.shape[0], int(out_offsets[-1])
        # the search's pair table: the transformed rows lie in output-row order, so query segment p is pair p itself
        self.search_pairs = np.ascontiguousarray(np.stack([np.arange(self.P, dtype=np.int64), pairs[:, 1]], axis=1))
        if device is not None and self.P:
            self.q_dev, self.pairs_dev, self.out_dev, self.search_dev = _upload(q_off, pairs, out_offsets, self.search_pairs, device=device)

    def transform(self, xyz, T, out):
        _lib.check(_lib.load().mspa_cloud_align_transform_device(
            _ptr(xyz), self.q_off.ctypes.data, self.q_off.size - 1, _ptr(self.q_dev), self.St, self.pairs.ctypes.data, _ptr(self.pairs_dev), self.P,
            self.out.ctypes.data, _ptr(self.out_dev), _ptr(T), _ptr(out), _stream_ptr()))

    def fit(self, xyz, targets, index, init, iteration, moments, T, used, status, eigen=None, converged=None):
        _lib.check(_lib.load().mspa_cloud_align_fit_device(
            _ptr(xyz), self.q_off.ctypes.data, self.q_off.size - 1, _ptr(self.q_dev), _ptr(targets), int(targets.shape[0]), self.St,
            self.pairs.ctypes.data, _ptr(self.pairs_dev), self.P, self.out.ctypes.data, _ptr(self.out_dev), _ptr(index), _ptr(init), iteration,
            _ptr(moments), _ptr(T), _ptr(used), _ptr(status), _ptr(eigen), _ptr(converged), _stream_ptr()))

    def plane_fit(self, xyz, targets, normals, index, init, iteration, moments, T, used, status, rmse=None, converged=None):
        _lib.check(_lib.load().mspa_cloud_align_plane_fit_device(
            _ptr(xyz), self.q_off.ctypes.data, self.q_off.size - 1, _ptr(self.q_dev), _ptr(targets), _ptr(normals), int(targets.shape[0]), self.St,
            self.pairs.ctypes.data, _ptr(self.pairs_dev), self.P, self.out.ctypes.data, _ptr(self.out_dev), _ptr(index), _ptr(init), iteration,
            _ptr(moments), _ptr(T), _ptr(used), _ptr(status), _ptr(rmse), _ptr(converged), _stream_ptr()))


def _index_of(index, M: int, device) -> torch.Tensor:
    _require(isinstance(index, torch.Tensor) and index.device == device and index.dtype == torch.int64 and tuple(index.shape) == (M,),
             f"index: a device int64 tensor [M] with M = {M}")
    return index.contiguous()


def rigid_fit_segments(queries: torch.Tensor, q_offsets, targets: torch.Tensor, index: torch.Tensor, pairs=None, init=None,
                       want_parts: bool = False) -> dict:
    """The rigid fit (Kabsch / Horn) of matched rows, pair by pair: a batch ``queries`` [Nq, C >= 3] (device) with host ``q_offsets``
    [Sq + 1], ``targets`` [Nt, C >= 3] (device), ``index`` [M] int64 (device; per output row a row of ``targets`` or -1 -- what
    ``TargetIndex.nearest`` returns, or ``arange`` for rows that correspond one to one) and the host pair table of ``nearest`` (only
    its first column is read; None: pair s is query segment s) -> a dict of device tensors ``R`` [P, 3, 3] and ``t`` [P, 3] float64,
    the proper rotation and the translation with the least sum of squares of ``R q + t - targets[index]`` over the used rows (index
    >= 0 and a finite query row); ``used`` [P] int64; ``status`` [P] int32 (``ALIGN_STATUS``: ok, few = fewer than 3 used rows,
    degenerate = collinear or coincident rows); ``offsets`` [P + 1] host int64; with ``want_parts`` ``eigen`` [P, 4], the eigenvalues
    of Horn's matrix in descending order.  A pair that is not ok gets the transform of ``init`` ([P, 4, 4] or [P, 3, 4]; None: the
    identity).  The rule is csrc/cloud_align_core.h's: centred sums in the order csrc/cloud_segments_core.h states, Horn's quaternion
    by a fixed number of Jacobi sweeps -- the same bits on every run, and equal correspondences give equal bits.  Enqueue only: two
    launches on the current stream, the host tables go up through pinned memory and nothing is read back."""
    xyz, tgt = _xyz_of("queries", queries), _xyz_of("targets", targets)
    q_off = _offsets(q_offsets, int(xyz.shape[0]))
    pairs, out_offsets, St = _fit_pairs(q_off, pairs)
    P, M, dev = pairs.shape[0], int(out_offsets[-1]), xyz.device
    _require(tgt.device == dev, "targets: on the queries' device")
    index = _index_of(index, M, dev)
    T0 = _transforms_of(init, P, dev)
    T = torch.empty((P, 12), dtype=torch.float64, device=dev)
    out = {"used": torch.empty((P,), dtype=torch.int64, device=dev), "status": torch.empty((P,), dtype=torch.int32, device=dev), "offsets": out_offsets}
    if want_parts:
        out["eigen"] = torch.empty((P, 4), dtype=torch.float64, device=dev)
    if P:
        moments = torch.empty((P, 16), dtype=torch.float64, device=dev)
        _AlignTables(q_off, pairs, out_offsets, St, dev).fit(xyz, tgt, index, T0, 0, moments, T, out["used"], out["status"], out.get("eigen"))
    out["R"], out["t"] = _split(T)
    return out


def transform_segments(queries: torch.Tensor, q_offsets, R: torch.Tensor, t: torch.Tensor, pairs=None) -> dict:
    """A batch ``queries`` [Nq, C >= 3] (device) with host ``q_offsets`` [Sq + 1], per pair ``R`` [P, 3, 3] and ``t`` [P, 3] (device
    float64) and the host pair table of ``nearest`` (None: pair s is query segment s) -> a dict: ``xyz`` [M, 3] float64 (device), the
    rows of pair p's query segment as ``y_a = ((R_a0 x + R_a1 y) + R_a2 z) + t_a`` at ``offsets[p]:offsets[p + 1]`` -- in output-row
    order, a batch of P segments -- and ``offsets`` [P + 1] host int64.  Enqueue only: one launch on the current stream, the host
    tables go up through pinned memory and nothing is read back."""
    xyz = _xyz_of("queries", queries)
    q_off = _offsets(q_offsets, int(xyz.shape[0]))
    pairs, out_offsets, St = _fit_pairs(q_off, pairs)
    P, M, dev = pairs.shape[0], int(out_offsets[-1]), xyz.device
    _require(isinstance(R, torch.Tensor) and isinstance(t, torch.Tensor) and R.device == dev and t.device == dev and R.dtype == t.dtype == torch.float64,
             "R and t: float64 tensors on the queries' device")
    T = _join(R, t, P, torch)
    out = {"xyz": torch.empty((M, 3), dtype=torch.float64, device=dev), "offsets": out_offsets}
    if M:
        _AlignTables(q_off, pairs, out_offsets, St, dev).transform(xyz, T, out["xyz"])
    return out


def _iterations_of(iterations, sync_every):
    K = int(iterations)
    _require(K >= 1, f"iterations: at least 1, got {iterations}")
    if sync_every is not None:
        _require(int(sync_every) >= 1, f"sync_every: at least 1, got {sync_every}")
    return K, K if sync_every is None else int(sync_every)


def _required_cap(max_distance) -> float:
    _require(max_distance is not None, "max_distance: required (finite and > 0): without it a far query walks its target's whole grid on every iteration")
    return _cap_of(max_distance)


def register_segments(queries: torch.Tensor, q_offsets, targets: torch.Tensor, t_offsets, pairs=None, *, max_distance, iterations: int = 30, init=None,
                      sync_every=None, want_history: bool = False, _grid_k=None, estimation: str = "point_to_point", normals=None) -> dict:
    """``target_index(targets, t_offsets).register(queries, q_offsets, ...)``: point-to-point ICP of every pair's query segment onto
    its target segment (``estimation="point_to_plane"`` with the targets' ``normals``: point-to-plane).  ``target_index``' one
    read-back and its ValueError."""
    return target_index(targets, t_offsets, _grid_k).register(queries, q_offsets, pairs, max_distance=max_distance, iterations=iterations, init=init,
                                                              sync_every=sync_every, want_history=want_history, estimation=estimation, normals=normals)


def _host_rows(name: str, rows) -> np.ndarray:
    rows = np.asarray(rows)
    if rows.ndim != 2 or rows.shape[1] < 3:
        raise ValueError(f"mspa.cloud_segments: {name}: expected [N, C >= 3], got {list(rows.shape)}")
    return np.ascontiguousarray(rows[:, :3], dtype=np.float64)


def _transform_host(q, q_off, St, pairs, out_offsets, T):
    out = np.empty((int(out_offsets[-1]), 3), dtype=np.float64)
    _lib.check(_lib.load().mspa_cloud_align_transform_host(q.ctypes.data, q_off.ctypes.data, q_off.size - 1, St, pairs.ctypes.data, pairs.shape[0],
                                                           out_offsets.ctypes.data, T.ctypes.data, out.ctypes.data))
    return out


def _fit_host(q, q_off, t, St, pairs, out_offsets, index, T0, iteration, want_parts=False, converged=None):
    P = pairs.shape[0]
    T, used, status = np.zeros((P, 12), dtype=np.float64), np.zeros((P,), dtype=np.int64), np.zeros((P,), dtype=np.int32)
    eigen = np.zeros((P, 4), dtype=np.float64) if want_parts else None
    _lib.check(_lib.load().mspa_cloud_align_fit_host(q.ctypes.data, q_off.ctypes.data, q_off.size - 1, t.ctypes.data, t.shape[0], St, pairs.ctypes.data, P,
                                                     out_offsets.ctypes.data, index.ctypes.data, T0.ctypes.data, iteration, T.ctypes.data,
                                                     used.ctypes.data, status.ctypes.data, eigen.ctypes.data if want_parts else None,
                                                     converged.ctypes.data if converged is not None else None))
    return T, used, status, eigen


def rigid_fit_segments_host(queries, q_offsets, targets, index, pairs=None, init=None, want_parts: bool = False) -> dict:
    """``rigid_fit_segments`` on the CPU for NumPy input, through the same header (mspa_cloud_align_fit_host): NumPy arrays out.  The
    device's twin for tests and for input that has no device, not a fallback."""
    q, t = _host_rows("queries", queries), _host_rows("targets", targets)
    q_off = _offsets(q_offsets, q.shape[0])
    pairs, out_offsets, St = _fit_pairs(q_off, pairs)
    index = np.ascontiguousarray(index, dtype=np.int64)
    _require(index.shape == (int(out_offsets[-1]),), f"index: int64 [M] with M = {int(out_offsets[-1])}")
    T, used, status, eigen = _fit_host(q, q_off, t, St, pairs, out_offsets, index, _transforms_of(init, pairs.shape[0]), 0, want_parts)
    out = {"R": _split(T)[0], "t": _split(T)[1], "used": used, "status": status, "offsets": out_offsets}
    if want_parts:
        out["eigen"] = eigen
    return out


def transform_segments_host(queries, q_offsets, R, t, pairs=None) -> dict:
    """``transform_segments`` on the CPU for NumPy input (mspa_cloud_align_transform_host).  The device's twin, not a fallback."""
    q = _host_rows("queries", queries)
    q_off = _offsets(q_offsets, q.shape[0])
    pairs, out_offsets, St = _fit_pairs(q_off, pairs)
    T = _join(np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64), pairs.shape[0], np)
    return {"xyz": _transform_host(q, q_off, St, pairs, out_offsets, T), "offsets": out_offsets}


def register_segments_host(queries, q_offsets, targets, t_offsets, pairs=None, *, max_distance, iterations: int = 30, init=None, sync_every=None,
                           want_history: bool = False, want_index: bool = False, _grid_k=None, estimation: str = "point_to_point", normals=None) -> dict:
    """``register_segments`` on the CPU for NumPy input: the same loop over the host twins, ``nearest_segments_host`` for its searches.
    NumPy arrays out; with ``want_index`` also ``history_index`` [K, M], the correspondences of every iteration.  The device's twin,
    not a fallback."""
    q, t = _host_rows("queries", queries), _host_rows("targets", targets)
    q_off, t_off = _offsets(q_offsets, q.shape[0]), _offsets(t_offsets, t.shape[0])
    St = t_off.size - 1
    plane = _estimation_of(estimation, normals)
    if plane:
        normals = _normals_of(normals, t.shape[0])
    pairs, out_offsets = _pair_tables(q_off, St, pairs)
    cap = _required_cap(max_distance)
    K, every = _iterations_of(iterations, sync_every)
    P, M = pairs.shape[0], int(out_offsets[-1])
    T = _transforms_of(init, P)
    tabs = _AlignTables(q_off, pairs, out_offsets, St, None)
    converged = np.full((P,), -1, dtype=np.int64)
    out = {"offsets": out_offsets, "converged_at": converged, "used": np.zeros((P,), dtype=np.int64), "status": np.zeros((P,), dtype=np.int32)}
    hist_used, hist_rmse, hist_index = np.zeros((K, P), dtype=np.int64), np.zeros((K, P)), np.zeros((K, M), dtype=np.int64)

    def search(T_now):
        moved = _transform_host(q, q_off, St, pairs, out_offsets, T_now)
        found = nearest_segments_host(moved, out_offsets, t, t_off, tabs.search_pairs, cap, _grid_k=_grid_k)
        fit = fit_segments_host(found["distance"], out_offsets, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            return found["index"], fit, np.sqrt(fit["sum_sq"] / fit["finite"].astype(np.float64))

    done = K
    for k in range(K):
        index, _fit, rmse = search(T)
        if plane:
            T, out["used"], out["status"], _ = _plane_fit_host(q, q_off, t, normals, St, pairs, out_offsets, index, T, k, converged)
        else:
            T, out["used"], out["status"], _ = _fit_host(q, q_off, t, St, pairs, out_offsets, index, T, k, False, converged)
        hist_used[k], hist_rmse[k], hist_index[k] = out["used"], rmse, index
        if sync_every is not None and ((k + 1) % every == 0 or k + 1 == K):
            out["all_converged"] = bool((converged != -1).all())
            if out["all_converged"]:
                done = k + 1
                break
    hist_used[done:], hist_rmse[done:], hist_index[done:] = hist_used[done - 1], hist_rmse[done - 1], hist_index[done - 1]
    _index, fit, rmse = search(T)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["fitness"], out["inlier_rmse"] = fit["finite"].astype(np.float64) / fit["rows"].astype(np.float64), rmse
    out["R"], out["t"] = _split(T)
    if want_history:
        out["history_used"], out["history_rmse"] = hist_used, hist_rmse
    if want_index:
        out["history_index"] = hist_index
    return out


# ---- the k nearest rows and the normals of a batch (csrc/cloud_normals.hip, rule in csrc/cloud_normals_core.h) ----------------------------

NORMALS_STATUS = {"ok": _lib.CLOUD_NORMALS_OK, "few": _lib.CLOUD_NORMALS_FEW, "degenerate": _lib.CLOUD_NORMALS_DEGENERATE}


def _viewpoints_of(viewpoints, S: int, device=None):
    """``viewpoints`` (None: none anywhere; [S, 3], host or device; a NaN row: none for that segment) -> [S, 3] float64: a device
    tensor on ``device``, or a NumPy array where ``device`` is None.  Enqueue only: a host array goes up through pinned memory."""
    if viewpoints is None:
        return None
    on_device = isinstance(viewpoints, torch.Tensor) and viewpoints.is_cuda
    if not on_device:
        viewpoints = np.asarray(viewpoints.numpy() if isinstance(viewpoints, torch.Tensor) else viewpoints, dtype=np.float64)
    _require(tuple(viewpoints.shape) == (S, 3), f"viewpoints: [S, 3] with S = {S}, got {list(viewpoints.shape)}")
    if on_device:
        _require(device is not None and viewpoints.device == device, "viewpoints: on the rows' device")
        return viewpoints.to(torch.float64).contiguous()
    flat = np.ascontiguousarray(viewpoints)
    return flat if device is None else (_upload(flat, device=device)[0] if S else torch.empty((0, 3), dtype=torch.float64, device=device))


def _normals_device(rows, offsets, k, max_distance, viewpoints, want_fit: bool, want_table: bool) -> dict:
    xyz = _xyz_of("rows", rows)
    N, dev = int(xyz.shape[0]), xyz.device
    off = _offsets(offsets, N)
    k, cap, S = _knn_check(k), _cap_of(max_distance), off.size - 1
    _require(N <= 1 << 30, f"rows: at most 2^30 rows, got {N}")
    views = _viewpoints_of(viewpoints, S, dev)
    out = {"used": torch.empty((N,), dtype=torch.int32, device=dev)}
    if want_fit:
        out["normal"] = torch.empty((N, 3), dtype=torch.float64, device=dev)
        out["curvature"] = torch.empty((N,), dtype=torch.float64, device=dev)
        out["status"] = torch.empty((N,), dtype=torch.uint8, device=dev)
    if want_table:
        out["index"] = torch.empty((N, k), dtype=torch.int64, device=dev)
        out["distance"] = torch.empty((N, k), dtype=torch.float64, device=dev)
    if N == 0:
        return out
    lib = _lib.load()
    grids, off_dev, grids_dev, base_dev = _search_tables(xyz, off, k)
    cell_base = np.zeros((S + 1,), dtype=np.int64)
    _lib.check(lib.mspa_knn_segments_tables_host(off.ctypes.data, S, k, cell_base.ctypes.data))
    starts = torch.zeros((int(cell_base[S]) + S,), dtype=torch.int32, device=dev)             # the slots behind a segment's cells are never written
    pts = torch.empty((N, 3), dtype=torch.float64, device=dev)
    keys = torch.empty((N,), dtype=torch.int64, device=dev)
    _lib.check(lib.mspa_knn_segments_cells_device(_ptr(xyz), off.ctypes.data, S, grids.ctypes.data, _ptr(off_dev), _ptr(grids_dev),
                                                  _ptr(base_dev), _ptr(keys), _stream_ptr()))
    order = torch.sort(keys, stable=True).indices
    _lib.check(lib.mspa_knn_segments_index_device(_ptr(xyz), off.ctypes.data, S, k, grids.ctypes.data, _ptr(off_dev), _ptr(grids_dev), _ptr(base_dev),
                                                  _ptr(order), _ptr(pts), _ptr(keys), _ptr(starts), int(starts.numel()), _stream_ptr()))
    _lib.check(lib.mspa_cloud_normals_device(_ptr(pts), _ptr(starts), int(starts.numel()), _ptr(order), off.ctypes.data, S, k, grids.ctypes.data,
                                             _ptr(off_dev), _ptr(grids_dev), _ptr(base_dev), cap, _ptr(views), _ptr(out.get("normal")),
                                             _ptr(out.get("curvature")), _ptr(out["used"]), _ptr(out.get("status")), _ptr(out.get("index")),
                                             _ptr(out.get("distance")), _stream_ptr()))
    return out


def knn_segments(rows: torch.Tensor, offsets, k: int, max_distance=None):
    """A batch ``rows`` [N, C >= 3] (device; xyz in front, float64 or a dtype that widens to it exactly) with host ``offsets`` [S + 1]
    -> ``(index, distance)``: ``index`` [N, k] int64 (device), per row the min(k, n_s) rows of its OWN segment with the smallest
    ``(d2, row)`` as rows of the batch, in that order, the row itself first among them at distance 0 (Open3D's KNN search), -1 behind
    them; ``distance`` [N, k] float64, ``sqrt(d2)`` with ``d2 = (dx*dx + dy*dy) + dz*dz``, +inf behind them.  With ``max_distance``
    (finite, > 0) only rows with ``d2 <= max_distance * max_distance`` count (Open3D's hybrid search).  The rule is
    csrc/cloud_normals_core.h's; the bits are those of a brute force with ``np.lexsort((row, d2))``.  ``1 <= k <= 64``.  One read-back
    per call, whatever S is: ``knn_mean_distance_segments``' boxes with the flag that every coordinate is finite; non-finite
    coordinates raise its ValueError."""
    out = _normals_device(rows, offsets, k, max_distance, None, False, True)
    return out["index"], out["distance"]


def normals_segments(rows: torch.Tensor, offsets, k: int = 30, max_distance=None, viewpoints=None, want_neighbours: bool = False) -> dict:
    """A batch ``rows`` [N, C >= 3] (device) with host ``offsets`` [S + 1] -> a dict of device tensors, per row: ``normal`` [N, 3]
    float64, the unit eigenvector of the smallest eigenvalue of the centred second moments of the row's ``knn_segments`` neighbours
    (the row itself among them; ``max_distance`` as there); ``curvature`` [N] float64 = l0 / ((l0 + l1) + l2), the surface variation;
    ``used`` [N] int32, the neighbours found; ``status`` [N] uint8 (``NORMALS_STATUS``: ok, few = fewer than 3 neighbours, degenerate =
    collinear, coincident or isotropic neighbours: l1 - l0 <= 2^-26 (l2 - l0)).  A row that is not ok has a NaN normal and a NaN
    curvature.  Sign: the first non-zero component is positive; with ``viewpoints`` ([S, 3], host or device; a NaN row: none for that
    segment) a normal is negated where ``(v - p) . n < 0``, so it points towards its segment's viewpoint.  With ``want_neighbours``
    also ``index`` and ``distance`` [N, k], ``knn_segments``' table from the same walk.  The rule is csrc/cloud_normals_core.h's:
    sequential sums in ascending ``(d2, row)`` order, a fixed number of Jacobi sweeps -- the same bits on every run and in any order
    of the rows inside a grid cell; rows in a plane ``z = const`` with integer z get (0, 0, 1) and 0.0 exactly.  One read-back per
    call, whatever S is: ``knn_mean_distance_segments``' boxes with the flag that every coordinate is finite; non-finite coordinates
    raise its ValueError.  One launch behind the index's."""
    return _normals_device(rows, offsets, k, max_distance, viewpoints, True, bool(want_neighbours))


def _normals_host(rows, offsets, k, max_distance, viewpoints, want_fit: bool, want_table: bool) -> dict:
    xyz = _host_rows("rows", rows)
    N = xyz.shape[0]
    off = _offsets(offsets, N)
    k, cap, S = _knn_check(k), _cap_of(max_distance), off.size - 1
    views = _viewpoints_of(viewpoints, S)
    if not np.isfinite(xyz).all():
        raise ValueError("mspa.cloud_segments: requirement not met: xyz: finite coordinates")
    out = {"used": np.zeros((N,), dtype=np.int32)}
    if want_fit:
        out.update(normal=np.zeros((N, 3)), curvature=np.zeros((N,)), status=np.zeros((N,), dtype=np.uint8))
    if want_table:
        out.update(index=np.zeros((N, k), dtype=np.int64), distance=np.zeros((N, k)))
    at = lambda name: out[name].ctypes.data if name in out else None               # noqa: E731
    _lib.check(_lib.load().mspa_cloud_normals_host(xyz.ctypes.data, off.ctypes.data, S, k, cap, views.ctypes.data if views is not None else None,
                                                   at("normal"), at("curvature"), at("used"), at("status"), at("index"), at("distance")))
    return out


def knn_segments_host(rows, offsets, k: int, max_distance=None):
    """``knn_segments`` on the CPU for NumPy input, through the same headers (mspa_cloud_normals_host): NumPy arrays out.  The device's
    twin for tests and for input that has no device, not a fallback."""
    out = _normals_host(rows, offsets, k, max_distance, None, False, True)
    return out["index"], out["distance"]


def normals_segments_host(rows, offsets, k: int = 30, max_distance=None, viewpoints=None, want_neighbours: bool = False) -> dict:
    """``normals_segments`` on the CPU for NumPy input, through the same headers (mspa_cloud_normals_host): the same keys, NumPy arrays.
    The device's twin, not a fallback."""
    return _normals_host(rows, offsets, k, max_distance, viewpoints, True, bool(want_neighbours))


# ---- point-to-plane on top of the two (csrc/cloud_align_plane.hip, rule in csrc/cloud_align_plane_core.h) ------------------------------

def _estimation_of(estimation, normals) -> bool:
    """True for point-to-plane.  ``normals`` belong to it and to nothing else."""
    _require(estimation in ("point_to_point", "point_to_plane"), f"estimation: 'point_to_point' or 'point_to_plane', got {estimation!r}")
    plane = estimation == "point_to_plane"
    _require(plane == (normals is not None), "normals: the targets' normals [Nt, 3], with estimation='point_to_plane' and only with it")
    return plane


def _normals_of(normals, Nt: int, device=None):
    """The targets' normals, checked: [Nt, 3] float64, a device tensor on ``device`` or, where ``device`` is None, a NumPy array.  NaN
    rows are allowed: they constrain nothing."""
    if device is None:
        normals = np.ascontiguousarray(normals.cpu().numpy() if isinstance(normals, torch.Tensor) else normals, dtype=np.float64)
        _require(normals.shape == (Nt, 3), f"normals: [Nt, 3] with Nt = {Nt}, got {list(normals.shape)}")
        return normals
    _require(isinstance(normals, torch.Tensor) and normals.device == device and tuple(normals.shape) == (Nt, 3),
             f"normals: a tensor [Nt, 3] with Nt = {Nt} on the targets' device")
    return normals.to(torch.float64).contiguous()


def plane_fit_segments(queries: torch.Tensor, q_offsets, targets: torch.Tensor, normals: torch.Tensor, index: torch.Tensor, pairs=None,
                       init=None) -> dict:
    """One linearised point-to-plane step, pair by pair: a batch ``queries`` [Nq, C >= 3] (device) with host ``q_offsets`` [Sq + 1],
    ``targets`` [Nt, C >= 3] with their ``normals`` [Nt, 3] (device), ``index`` [M] int64 (device; per output row a row of ``targets``
    or -1: what ``TargetIndex.nearest`` returns for the rows under ``init``) and the host pair table of ``nearest`` (only its first
    column is read; None: pair s is query segment s) -> a dict of device tensors ``R`` [P, 3, 3] and ``t`` [P, 3] float64: ``init``
    ([P, 4, 4] or [P, 3, 4]; None: the identity) moved by the step that minimises, to first order, the sum of squares of
    ``(y - targets[index]) . normals[index]`` over the used rows, ``y = init q`` (index >= 0, a finite query row, a finite normal);
    ``used`` [P] int64; ``status`` [P] int32 (``ALIGN_STATUS``: few = fewer than 6 used rows, degenerate = the matched normals leave a
    motion unconstrained, as a flat target does); ``rmse`` [P], sqrt of the mean squared plane distance under ``init``; ``offsets``
    [P + 1] host int64.  A pair that is not ok, and a step that is exactly zero, keep ``init`` bit for bit.  The rule is
    csrc/cloud_align_plane_core.h's: sums in the order csrc/cloud_segments_core.h states, a written-out L D L^T, the rotation rebuilt
    from a normalised quaternion, so max |R^T R - I| stays within 32 * 2^-53 after any number of steps.  Enqueue only: two launches on
    the current stream, the host tables go up through pinned memory and nothing is read back."""
    xyz, tgt = _xyz_of("queries", queries), _xyz_of("targets", targets)
    q_off = _offsets(q_offsets, int(xyz.shape[0]))
    pairs, out_offsets, St = _fit_pairs(q_off, pairs)
    P, M, dev = pairs.shape[0], int(out_offsets[-1]), xyz.device
    _require(tgt.device == dev, "targets: on the queries' device")
    normals = _normals_of(normals, int(tgt.shape[0]), dev)
    index = _index_of(index, M, dev)
    T0 = _transforms_of(init, P, dev)
    T = torch.empty((P, 12), dtype=torch.float64, device=dev)
    out = {"used": torch.empty((P,), dtype=torch.int64, device=dev), "status": torch.empty((P,), dtype=torch.int32, device=dev),
           "rmse": torch.empty((P,), dtype=torch.float64, device=dev), "offsets": out_offsets}
    if P:
        moments = torch.empty((P, 32), dtype=torch.float64, device=dev)
        _AlignTables(q_off, pairs, out_offsets, St, dev).plane_fit(xyz, tgt, normals, index, T0, 0, moments, T, out["used"], out["status"], out["rmse"])
    out["R"], out["t"] = _split(T)
    return out


def _plane_fit_host(q, q_off, t, normals, St, pairs, out_offsets, index, T0, iteration, converged=None):
    P = pairs.shape[0]
    T, used, status, rmse = np.zeros((P, 12)), np.zeros((P,), dtype=np.int64), np.zeros((P,), dtype=np.int32), np.zeros((P,))
    _lib.check(_lib.load().mspa_cloud_align_plane_fit_host(q.ctypes.data, q_off.ctypes.data, q_off.size - 1, t.ctypes.data, normals.ctypes.data, t.shape[0],
                                                           St, pairs.ctypes.data, P, out_offsets.ctypes.data, index.ctypes.data, T0.ctypes.data, iteration,
                                                           T.ctypes.data, used.ctypes.data, status.ctypes.data, rmse.ctypes.data,
                                                           converged.ctypes.data if converged is not None else None))
    return T, used, status, rmse


def plane_fit_segments_host(queries, q_offsets, targets, normals, index, pairs=None, init=None) -> dict:
    """``plane_fit_segments`` on the CPU for NumPy input, through the same header (mspa_cloud_align_plane_fit_host): NumPy arrays out.
    The device's twin for tests and for input that has no device, not a fallback."""
    q, t = _host_rows("queries", queries), _host_rows("targets", targets)
    q_off = _offsets(q_offsets, q.shape[0])
    pairs, out_offsets, St = _fit_pairs(q_off, pairs)
    normals = _normals_of(normals, t.shape[0])
    index = np.ascontiguousarray(index, dtype=np.int64)
    _require(index.shape == (int(out_offsets[-1]),), f"index: int64 [M] with M = {int(out_offsets[-1])}")
    T, used, status, rmse = _plane_fit_host(q, q_off, t, normals, St, pairs, out_offsets, index, _transforms_of(init, pairs.shape[0]), 0)
    return {"R": _split(T)[0], "t": _split(T)[1], "used": used, "status": status, "rmse": rmse, "offsets": out_offsets}
