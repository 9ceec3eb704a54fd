"""Mirror of the reference's handler/ops.py: the object-cloud tool chain mask -> cloud (``project_mask_to_3d``, kernel K3) ->
cleaned cloud (``remove_statistical_outliers``: exact k-nearest search on the device; ``remove_truncated_outliers``) -> box
(``calculate_aabb``, ``convert_to_corners``) -> IoU (``calculate_iou_3d``, ``calculate_iou_2d``), and the frame filter
(``filter_images_laplacian``, ``calculate_image_sharpness``: grey decode and Laplacian moments on the device).  NumPy in gives
NumPy out; a device tensor in gives a device tensor out."""
from __future__ import annotations

from typing import List

import numpy as np
import torch

from mspa import engine, ingest

from ._images import read_color_rgb, read_depth

__all__ = ["filter_images_laplacian", "calculate_image_sharpness", "convert_to_corners", "calculate_iou_2d", "calculate_iou_3d",
           "remove_statistical_outliers", "remove_truncated_outliers", "calculate_aabb", "project_mask_to_3d"]
# (upstream's nine names, which tests/test_handler_ops_cpu.py pins; ``voxel_down_sample``, ``cluster_dbscan`` and
# ``calculate_upright_box``, ``calculate_iou_upright`` and ``compute_point_cloud_distance`` below are this project's own and are reached
# as ``ops.voxel_down_sample`` and so on)


def _same_device(a, b):
    """Two arguments of which at least one is a tensor, both as tensors where the device tensor lives."""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    dev = a.device if a.is_cuda else b.device
    return a.to(dev), b.to(dev)


def filter_images_laplacian(image_paths, threshold=100):
    """The paths whose sharpness score is at least ``threshold``, in their order (OPS:14-19); one batched call scores them all."""
    image_paths = list(image_paths)
    scores = ingest.image_sharpness(image_paths)
    return [p for p, s in zip(image_paths, scores) if s >= threshold]


def calculate_image_sharpness(image_path):
    """Variance of the Laplacian of the file's grey image (OPS:22-34): ``mspa.ingest.image_sharpness`` of one file.  The value
    is the exact population variance rounded once; upstream's ``laplacian.var()`` is within a few ulps of it.  An unreadable
    file raises ``ValueError("Unable to read image from: ...")``."""
    return np.float64(ingest.image_sharpness([image_path])[0])


def convert_to_corners(bounding_boxes) -> List[np.ndarray]:
    """Per box [cx, cy, cz, dx, dy, dz, ...] its eight corners, [8, 3] float32 (OPS:37-94): corner j takes +d/2 on x where bit 0 of
    j is set, on y where bit 1 is, on z where bit 2 is, and -d/2 elsewhere.  Each coordinate is formed in the box's own
    precision and then narrowed, as upstream's array literal does.  Device boxes give device corners."""
    corners = []
    for bbox in bounding_boxes:
        if isinstance(bbox, torch.Tensor):
            sign = torch.tensor([[1 if j >> a & 1 else -1 for a in range(3)] for j in range(8)], dtype=bbox.dtype, device=bbox.device)
            half = bbox[3:6] / 2
            plus, minus = bbox[:3] + half, bbox[:3] - half
            corners.append(torch.where(sign > 0, plus[None, :], minus[None, :]).to(torch.float32))
        else:
            rows = [[bbox[a] + bbox[3 + a] / 2 if j >> a & 1 else bbox[a] - bbox[3 + a] / 2 for a in range(3)] for j in range(8)]
            corners.append(np.array(rows, dtype=np.float32))
    return corners


def calculate_iou_2d(mask1, mask2):
    """Intersection over union of two binary masks (OPS:97-111); 0.0 when the union is empty."""
    if isinstance(mask1, torch.Tensor) or isinstance(mask2, torch.Tensor):
        a, b = _same_device(mask1, mask2)
        union = (a.bool() | b.bool()).sum()
        return torch.where(union != 0, (a.bool() & b.bool()).sum() / union.clamp(min=1), torch.zeros_like(union, dtype=torch.float32))
    union = np.sum(np.logical_or(mask1, mask2))
    if union == 0:
        return 0.0
    return np.sum(np.logical_and(mask1, mask2)) / union


def calculate_iou_3d(box1, box2):
    """Intersection over union of two axis-aligned boxes [x, y, z, dx, dy, dz] (OPS:114-135); the intersection counts only
    when it is positive along every axis."""
    if isinstance(box1, torch.Tensor) or isinstance(box2, torch.Tensor):
        box1, box2 = _same_device(box1, box2)
        dim = torch.minimum(box1[:3] + box1[3:] / 2, box2[:3] + box2[3:] / 2) - torch.maximum(box1[:3] - box1[3:] / 2, box2[:3] - box2[3:] / 2)
        inter = torch.where((dim > 0).all(), dim.prod(), torch.zeros((), dtype=dim.dtype, device=dim.device))
        return inter / (box1[3:].prod() + box2[3:].prod() - inter)
    dim = np.minimum(box1[:3] + box1[3:] / 2, box2[:3] + box2[3:] / 2) - np.maximum(box1[:3] - box1[3:] / 2, box2[:3] - box2[3:] / 2)
    inter = np.prod(dim) if np.all(dim > 0) else 0
    return inter / (np.prod(box1[3:]) + np.prod(box2[3:]) - inter)


def calculate_iou_upright(box1, box2):
    """Intersection over union of two upright boxes ``[cx, cy, cz, length, width, height, ux, uy]`` (``calculate_upright_box``'s):
    where ``calculate_iou_3d`` of the axis-aligned boxes ignores the couch's own length and width, this one scores the boxes as they
    stand.  It is the one-pair case of ``mspa.cloud_segments.upright_iou`` (rule in csrc/upright_iou_core.h: the footprints clipped by
    Sutherland-Hodgman, every step one float64 operation), symmetric in its arguments bit for bit, the same bits on the device as on
    the host.  NumPy in gives a Python float (the host twin of the kernel); device tensors in give a device scalar, and nothing is
    read back.  A box the rule refuses (a non-finite value, a negative size, an axis that is no unit vector) gives NaN.  No
    reference counterpart."""
    from mspa import cloud_segments
    if isinstance(box1, torch.Tensor) or isinstance(box2, torch.Tensor):
        box1, box2 = _same_device(box1, box2)
        if box1.is_cuda:
            return cloud_segments.upright_iou(box1.to(torch.float64).reshape(8), box2.to(torch.float64).reshape(8))
        box1, box2 = box1.numpy(), box2.numpy()
    one = cloud_segments.upright_iou_host(np.asarray(box1, dtype=np.float64).reshape(8), np.asarray(box2, dtype=np.float64).reshape(8))
    return float(one)


def remove_statistical_outliers(point_cloud_data, nb_neighbors=20, std_ratio=1.0):
    """[N, C >= 3] cloud -> the rows Open3D's ``remove_statistical_outlier(nb_neighbors, std_ratio)`` keeps, all columns, the
    input's dtype, ascending row order (OPS:138-160).  The rule, as restated here (Open3D is not a dependency):
      avg[i] = mean distance from point i to its min(nb_neighbors, N) nearest points, itself included (exact search on the
               device, ``mspa.engine.knn_mean_distance``);
      mean = (sum of the positive avg) / N;  sd = sqrt(sum over the positive avg of (avg - mean)^2 / (N - 1));
      row i stays iff 0 < avg[i] < mean + std_ratio * sd.
    N = 0 and N = 1 (a 0 / 0 threshold) give an empty result.  ``nb_neighbors < 1`` or ``std_ratio <= 0`` raises RuntimeError,
    as Open3D does.  Deviations: non-finite coordinates raise ValueError, and ``nb_neighbors > 64`` raises
    NotImplementedError (the kernel keeps at most 64 candidates per point)."""
    if nb_neighbors < 1 or std_ratio <= 0:
        raise RuntimeError("remove_statistical_outliers: nb_neighbors must be at least 1 and std_ratio positive "
                           f"(got {nb_neighbors}, {std_ratio})")
    if nb_neighbors > engine._lib.KNN_MAX_K:
        raise NotImplementedError(f"remove_statistical_outliers: nb_neighbors is limited to {engine._lib.KNN_MAX_K} "
                                  f"(got {nb_neighbors})")
    is_tensor = isinstance(point_cloud_data, torch.Tensor)
    data = point_cloud_data if is_tensor else np.asarray(point_cloud_data)
    n = int(data.shape[0])
    if n == 0:
        return data[:0, :]
    xyz = (data[:, :3] if is_tensor else torch.from_numpy(np.ascontiguousarray(data[:, :3]))).to("cuda", torch.float64).contiguous()
    if not bool(torch.isfinite(xyz).all()):
        raise ValueError("remove_statistical_outliers: the cloud has non-finite coordinates")
    avg = engine.knn_mean_distance(xyz, int(nb_neighbors))
    pos = avg > 0
    zero = torch.zeros((), dtype=torch.float64, device=avg.device)
    mean = torch.where(pos, avg, zero).sum() / n
    dev = avg - mean
    sd = torch.sqrt(torch.where(pos, dev * dev, zero).sum() / (n - 1))             # n = 1: 0 / 0, nothing passes
    ind = torch.nonzero(pos & (avg < mean + std_ratio * sd)).flatten()
    from .info_handler import _like                 # (info_handler imports this module: not at the top)
    ind = _like(ind, point_cloud_data)
    return data[ind.to(data.device) if is_tensor else ind, :]


def voxel_down_sample(point_cloud_data, voxel_size):
    """[N, C >= 3] cloud -> [M, C] float64: one row per occupied voxel of a grid of ``voxel_size`` whose origin is the cloud's
    per-axis minimum minus half a voxel; every column (colour and other extra columns included) is the mean over the voxel's rows.
    The step in front of ``remove_statistical_outliers`` for a cloud fused from overlapping views.  It is the S = 1 case of
    ``mspa.cloud_segments.voxel_down_sample_segments`` (rule in csrc/voxel_grid_core.h): voxels in ascending (ix, iy, iz), a
    voxel's rows summed in ascending row order, the same bits on every run.  The rule restates Open3D's ``voxel_down_sample`` as
    the maintainers recall it and is not checked against Open3D (whose row order is its hash map's); Open3D is not a dependency.
    NumPy in gives NumPy out (the host twin of the kernels), a device tensor in gives a device tensor out; N = 0 returns the empty
    [0, C].  ``voxel_size <= 0`` or non-finite raises RuntimeError, as Open3D does; non-finite coordinates, or a size so small
    that a voxel index reaches 2^21 on an axis, raise ValueError.  No reference counterpart."""
    from mspa import cloud_segments
    is_tensor = isinstance(point_cloud_data, torch.Tensor)
    data = point_cloud_data if is_tensor else np.asarray(point_cloud_data)
    offsets = np.array([0, int(data.shape[0])], dtype=np.int64)
    if is_tensor and data.is_cuda:
        return cloud_segments.voxel_down_sample_segments(data, offsets, voxel_size)[0]
    out = cloud_segments.voxel_down_sample_segments_host(data.numpy() if is_tensor else data, offsets, voxel_size)[0]
    return torch.from_numpy(out) if is_tensor else out


def cluster_dbscan(point_cloud_data, eps, min_points):
    """[N, C >= 3] cloud -> labels [N] int32: density clustering of the xyz columns, -1 for noise.  The name and the arguments are
    Open3D's ``cluster_dbscan(eps, min_points)``; the labels are scikit-learn's, value for value:
    ``sklearn.cluster.DBSCAN(eps, min_samples=min_points, algorithm="kd_tree").fit(xyz).labels_`` (a point counts itself; clusters
    are numbered in ascending order of their lowest core row; a point that is not core takes the lowest cluster number among the
    core points within ``eps``).  It is the S = 1 case of ``mspa.cloud_segments.dbscan_segments`` (rule in csrc/dbscan_core.h), the
    same values on every run.  The step between ``remove_statistical_outliers`` and ``calculate_aabb`` for a cloud whose mask
    bleeds onto what lies behind the object: keep ``cloud[labels == np.bincount(labels[labels >= 0]).argmax()]``.  NumPy in gives
    NumPy out (the host twin of the kernels), a device tensor in gives a device tensor out; N = 0 returns the empty [0].
    ``eps <= 0``, non-finite ``eps`` or ``min_points < 1`` raises RuntimeError; non-finite coordinates, or an ``eps`` so small that a
    cell index reaches 2^21 on an axis, raise ValueError.  Neither Open3D nor scikit-learn is a dependency.  No reference
    counterpart."""
    from mspa import cloud_segments
    is_tensor = isinstance(point_cloud_data, torch.Tensor)
    data = point_cloud_data if is_tensor else np.asarray(point_cloud_data)
    offsets = np.array([0, int(data.shape[0])], dtype=np.int64)
    if is_tensor and data.is_cuda:
        return cloud_segments.dbscan_segments(data, offsets, eps, min_points)[0]
    out = cloud_segments.dbscan_segments_host(data.numpy() if is_tensor else data, offsets, eps, min_points)[0]
    return torch.from_numpy(out) if is_tensor else out


def calculate_upright_box(point_cloud_data):
    """[N, C >= 3] cloud -> its upright minimal box [8] float64: ``[cx, cy, cz, length, width, height, ux, uy]``, the z extent of
    the cloud (``cz`` and ``height`` are ``calculate_aabb``'s) times the minimum-area rectangle around the convex hull of its (x, y)
    footprint; ``length >= width``, and ``(ux, uy)`` is the unit direction of the length with ``ux > 0``, or ``ux == 0`` and ``uy > 0``.
    Where ``calculate_aabb`` gives a couch standing at 30 degrees in its room a box that is far longer and wider than the couch,
    this box has the couch's own length and width.  It is the S = 1 case of ``mspa.cloud_segments.upright_boxes_segments`` (rule in
    csrc/upright_box_core.h: an exact hull, the all-edges rectangle, every step one float64 operation), the same bits on every run
    and the same bits on the device as on the host.  NumPy in gives NumPy out (the host twin of the kernels), a device tensor in
    gives a device tensor out; N = 0 returns eight NaN.  Non-finite coordinates, or a non-zero ``|x|`` or ``|y|`` outside
    [2^-200, 2^200], raise ValueError.  No reference counterpart: upstream's lengths and widths are those of the axis-aligned box."""
    from mspa import cloud_segments
    is_tensor = isinstance(point_cloud_data, torch.Tensor)
    data = point_cloud_data if is_tensor else np.asarray(point_cloud_data)
    offsets = np.array([0, int(data.shape[0])], dtype=np.int64)
    if is_tensor and data.is_cuda:
        return cloud_segments.upright_boxes_segments(data, offsets)[0]
    out = cloud_segments.upright_boxes_segments_host(data.numpy() if is_tensor else data, offsets)[0]
    return torch.from_numpy(out.copy()) if is_tensor else out.copy()


def compute_point_cloud_distance(source, target):
    """[n, C >= 3] cloud ``source`` and [m, C >= 3] cloud ``target`` -> [n] float64: for every row of ``source`` the distance to the
    nearest row of ``target`` -- the primitive behind the Chamfer distance, the one-sided Hausdorff distance and precision / recall at
    a threshold.  The name is Open3D's ``PointCloud.compute_point_cloud_distance``; the rule restates it (Euclidean distance to the
    nearest target point) and is not checked against Open3D, which is not a dependency.  It is the one-pair case of
    ``mspa.cloud_segments.nearest_segments`` (rule in csrc/cloud_distance_core.h): ``sqrt(min((dx*dx + dy*dy) + dz*dz))`` in float64, the
    bits of a brute force over all rows, the same bits on the device as on the host.  NumPy in gives NumPy out (the host twin of the
    kernel); a device tensor in gives a device tensor out.  An empty ``target`` gives +inf, a ``source`` row with a non-finite
    coordinate NaN; a non-finite ``target`` coordinate raises ValueError.  No reference counterpart."""
    from mspa import cloud_segments
    if isinstance(source, torch.Tensor) or isinstance(target, torch.Tensor):
        source, target = _same_device(source, target)
        if source.is_cuda:
            return cloud_segments.nearest_segments(source, np.array([0, source.shape[0]], dtype=np.int64), target,
                                                   np.array([0, target.shape[0]], dtype=np.int64), want_index=False)["distance"]
        return torch.from_numpy(compute_point_cloud_distance(source.numpy(), target.numpy()))
    source, target = np.asarray(source), np.asarray(target)
    return cloud_segments.nearest_segments_host(source, np.array([0, source.shape[0]], dtype=np.int64), target,
                                                np.array([0, target.shape[0]], dtype=np.int64))["distance"]


def registration_icp(source, target, max_correspondence_distance, init=None, max_iteration: int = 30, estimation: str = "point_to_point",
                     target_normals=None):
    """[n, C >= 3] cloud ``source`` and [m, C >= 3] cloud ``target`` -> a dict: ``transformation`` [4, 4] float64, the rigid transform
    that carries ``source`` onto ``target`` by point-to-point ICP from ``init`` ([4, 4]; None: the identity), and Open3D's two result
    fields under it, ``fitness`` (the share of source rows with a target row within ``max_correspondence_distance``) and
    ``inlier_rmse`` (the root mean square distance of those rows).  The name and the arguments are Open3D's
    ``pipelines.registration.registration_icp`` with ``TransformationEstimationPointToPoint``; the rule restates it WITHOUT Open3D's
    relative-change stop -- it runs ``max_iteration`` iterations, from its fixed point on each reproduces the same transform -- and is
    not checked against Open3D, which is not a dependency.  Every iteration fits the ORIGINAL source rows to their nearest target
    rows (csrc/cloud_align_core.h: Horn's quaternion by a fixed number of Jacobi sweeps, float64), so no transforms are composed.  It
    is the one-pair case of ``mspa.cloud_segments.register_segments``: NumPy in gives NumPy out (the host twin of the kernels), a
    device tensor in gives device tensors out, the same bits either way.  ``estimation="point_to_plane"`` is Open3D's
    ``TransformationEstimationPointToPlane``: every iteration moves the transform by one linearised point-to-plane step against the
    target's normals (csrc/cloud_align_plane_core.h), ``target_normals`` [m, 3] or, where None, ``estimate_normals(target, 30)``; a
    target that leaves a motion unconstrained (a single plane) keeps ``init``.  No reference counterpart."""
    from mspa import cloud_segments
    one = lambda rows: np.array([0, rows.shape[0]], dtype=np.int64)           # noqa: E731
    if estimation not in ("point_to_point", "point_to_plane"):
        raise ValueError(f"registration_icp: estimation must be 'point_to_point' or 'point_to_plane', got {estimation!r}")
    if estimation == "point_to_point" and target_normals is not None:
        raise ValueError("registration_icp: target_normals belong to estimation='point_to_plane'")
    plane = estimation == "point_to_plane"
    if isinstance(source, torch.Tensor) or isinstance(target, torch.Tensor):
        source, target = _same_device(source, target)
        if source.is_cuda:
            extra = {}
            if plane:
                normals = estimate_normals(target, 30) if target_normals is None else torch.as_tensor(target_normals, dtype=torch.float64).to(target.device)
                extra = {"estimation": estimation, "normals": normals}
            out = cloud_segments.register_segments(source, one(source), target, one(target), max_distance=max_correspondence_distance,
                                                   iterations=max_iteration, init=None if init is None else torch.as_tensor(init)[None], **extra)
            T = torch.eye(4, dtype=torch.float64, device=source.device)
            T[:3, :3], T[:3, 3] = out["R"][0], out["t"][0]
            return {"transformation": T, "fitness": out["fitness"][0], "inlier_rmse": out["inlier_rmse"][0]}
        host = registration_icp(source.numpy(), target.numpy(), max_correspondence_distance, None if init is None else torch.as_tensor(init).cpu().numpy(),
                                max_iteration, estimation, None if target_normals is None else torch.as_tensor(target_normals).cpu().numpy())
        return {k: torch.as_tensor(v) for k, v in host.items()}
    source, target = np.asarray(source), np.asarray(target)
    if isinstance(init, torch.Tensor):
        init = init.cpu().numpy()
    extra = {}
    if plane:
        if isinstance(target_normals, torch.Tensor):
            target_normals = target_normals.cpu().numpy()
        extra = {"estimation": estimation, "normals": estimate_normals(target, 30) if target_normals is None else np.asarray(target_normals, dtype=np.float64)}
    out = cloud_segments.register_segments_host(source, one(source), target, one(target), max_distance=max_correspondence_distance,
                                                iterations=max_iteration, init=None if init is None else np.asarray(init, dtype=np.float64)[None], **extra)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = out["R"][0], out["t"][0]
    return {"transformation": T, "fitness": out["fitness"][0], "inlier_rmse": out["inlier_rmse"][0]}


def estimate_normals(point_cloud_data, k: int = 30, radius=None, camera_location=None):
    """[n, C >= 3] cloud -> [n, 3] float64: per row the unit normal of the plane through its ``k`` nearest rows (itself among them;
    with a ``radius`` only those within it: Open3D's ``KDTreeSearchParamHybrid(radius, max_nn=k)``, without one
    ``KDTreeSearchParamKNN(k)``), the eigenvector of the smallest eigenvalue of their covariance.  With a ``camera_location`` [3] the
    normals point towards it (Open3D's ``orient_normals_towards_camera_location``); without one the first non-zero component is
    positive.  A row with fewer than 3 neighbours, or with collinear, coincident or isotropic ones, has a NaN normal where Open3D
    leaves an arbitrary one.  The name is Open3D's ``PointCloud.estimate_normals``; the rule restates it and is not checked against
    Open3D, which is not a dependency.  It is the one-segment case of ``mspa.cloud_segments.normals_segments`` (rule in
    csrc/cloud_normals_core.h): NumPy in gives NumPy out (the host twin of the kernel), a device tensor in gives a device tensor
    out, the same bits either way.  No reference counterpart."""
    from mspa import cloud_segments
    is_tensor = isinstance(point_cloud_data, torch.Tensor)
    data = point_cloud_data if is_tensor else np.asarray(point_cloud_data)
    offsets = np.array([0, int(data.shape[0])], dtype=np.int64)
    view = None
    if camera_location is not None:
        view = camera_location.reshape(1, 3) if isinstance(camera_location, torch.Tensor) else np.asarray(camera_location, dtype=np.float64).reshape(1, 3)
    if is_tensor and data.is_cuda:
        return cloud_segments.normals_segments(data, offsets, k, radius, view)["normal"]
    if isinstance(view, torch.Tensor):
        view = view.cpu().numpy()
    out = cloud_segments.normals_segments_host(data.numpy() if is_tensor else data, offsets, k, radius, view)["normal"]
    return torch.from_numpy(out) if is_tensor else out


def remove_truncated_outliers(point_cloud_data, tx: float, ty: float, tz: float):
    """Drop, per axis, the ``int(t * N)`` rows with the smallest and the largest coordinate, and keep the rows that survive on
    all three axes, in ascending row order (OPS:163-208).  Which of several equal coordinates goes is ``np.argsort``'s
    choice, so NumPy input is ranked by NumPy itself and the result is upstream's by construction; a device tensor is ranked
    by ``torch.argsort(stable=True)``.  Upstream's quirks stay: all-zero ratios return the input itself, and a zero count on
    one axis next to a non-zero ratio elsewhere selects ``[0:-0]``, nothing."""
    assert tx < 0.5 and ty < 0.5 and tz < 0.5, "tx, ty, tz must be less than 0.5."
    n = len(point_cloud_data)
    if tx == 0 and ty == 0 and tz == 0:
        return point_cloud_data
    if isinstance(point_cloud_data, torch.Tensor):
        keep = torch.ones((n,), dtype=torch.bool, device=point_cloud_data.device)
        for axis, t in enumerate((tx, ty, tz)):
            cut = int(t * n)
            ranked = torch.argsort(point_cloud_data[:, axis], stable=True)
            inside = torch.zeros_like(keep)
            if 2 * cut < n:
                inside[ranked[cut:-cut]] = True
            keep &= inside
        return point_cloud_data[keep]
    valid = None
    for axis, t in enumerate((tx, ty, tz)):
        cut = int(t * n)
        ranked = np.argsort(point_cloud_data[:, axis])
        inside = ranked[cut:-cut] if 2 * cut < n else np.array([])
        valid = inside if valid is None else np.intersect1d(valid, inside)
    return point_cloud_data[valid]


def calculate_aabb(point_cloud_data):
    """[N, C >= 3] cloud -> [cx, cy, cz, dx, dy, dz]: centre and size of its axis-aligned bounding box (OPS:211-232)."""
    if isinstance(point_cloud_data, torch.Tensor):
        lo, hi = point_cloud_data[:, :3].min(dim=0).values, point_cloud_data[:, :3].max(dim=0).values
        return torch.cat([(hi + lo) / 2, hi - lo])
    lo, hi = np.min(point_cloud_data[:, :3], axis=0), np.max(point_cloud_data[:, :3], axis=0)
    return np.concatenate([(hi + lo) / 2, hi - lo])


def project_mask_to_3d(depth_image, intrinsic_matrix, extrinsic_matrix, mask=None,
                       world_to_axis_align_matrix=None, color_image=None):
    """Same contract as the reference's ``project_mask_to_3d`` (ops.py:235-329): back-project the
    mask's pixels (mask spans the colour grid; ``None`` = every pixel, needs ``color_image``) through
    inv(K), E and optionally A; returns ``[M, 3]`` or ``[M, 6]`` float64 in row-major mask order with
    zero-depth pixels dropped.  Runs kernel K3 in exact mode (float64 outputs)."""
    if isinstance(depth_image, str):
        depth_image = read_depth(depth_image)
    if isinstance(color_image, str):
        color_image = read_color_rgb(color_image)
    if mask is None:
        mask = np.ones(color_image.shape[:2], dtype=bool)          # AttributeError when both are None, as upstream
    mask = np.asarray(mask)
    H, W = mask.shape[:2]
    A = np.eye(4) if world_to_axis_align_matrix is None else np.asarray(world_to_axis_align_matrix, np.float64)
    K = np.asarray(intrinsic_matrix, np.float64)
    E = np.asarray(extrinsic_matrix, np.float64)
    mats = torch.from_numpy(engine.frame_matrices(K, A, [E])).cuda()
    depth = engine.depth_to_device(np.asarray(depth_image)[None], "cuda")
    pairs = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
    out = engine.alloc_pair_outputs(1, (H, W), ("xyz_f64", "valid_u8"), "cuda")
    engine.pair_reproject(depth, mats, pairs, (H, W), out)
    # only the mask's rows cross PCIe: the selection happens on the device (a 5 % mask downloads 0.4 MB instead of 7.4 MB)
    full = bool(mask.all())
    keep_t = out["valid_u8"][0].bool() if full else \
        (out["valid_u8"][0].bool() & torch.from_numpy(np.ascontiguousarray(mask.reshape(-1) != 0)).cuda())
    idx = torch.nonzero(keep_t).flatten()                         # row-major mask order, as np.where gives it (OPS:276-278)
    xyz = out["xyz_f64"][0].index_select(0, idx).cpu().numpy()
    keep = idx.cpu().numpy()
    # (world_to_axis_align_matrix is None -> A = identity in the frame record: x*1 + 0*y + 0*z + 0 is exact, the result
    # equals E @ cam as upstream computes it without the third product)
    if color_image is not None:
        rgb = np.asarray(color_image).reshape(-1, color_image.shape[-1])[keep]
        return np.hstack((xyz, rgb))
    return xyz
