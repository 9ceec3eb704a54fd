"""Per-object point clouds of a scene's frames from their instance masks, batched on the device.

The reference builds an object's cloud per (image, object): ``get_instance_mask`` reads ``instance-filt/<image>.png`` and compares
it with ``target_id + 1``, ``project_image_to_3d_with_mask`` reads the depth frame (and the colour frame) again and back-projects
the mask's pixels.  A frame with 30 objects decodes the same files 30 times and runs K3 30 times over the same pixels.  ``build``
does: one decode of the depth frames, the label images and (when asked) the colour frames on the device, then per chunk of frames
ONE ``engine.pair_reproject`` exact launch with pairs (f, f) and one ``engine.instance_split``.  What comes back, ``InstanceClouds``, holds
the rows of every (image, label) segment back to back on the device -- value for value what the composition returns per object, in
its order -- and hands out views.  ``LAST_INSTANCE_CLOUDS`` says which path the last call took, and why.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import engine, ingest

LAST_INSTANCE_CLOUDS: Dict[str, str] = {}        # {"path": "device" | "host", "reason": why the per-object host composition ran}


class InstanceClouds:
    """The clouds of every (image, object) of one call.  ``rows`` [total, 3 or 6] float64 (device): xyz, then -- with colour --
    the RGB columns converted to float64, as ``np.hstack((xyz, rgb))`` does; segment (frame k, label v) is
    ``rows[offsets[k * L + v] : offsets[k * L + v + 1]]`` in ascending pixel index; ``counts`` [F, L] and ``offsets`` are host
    arrays (L = 256 on the device path); ``pixel`` [total] int32 the rows' pixel indices my * W + mx; ``lo`` / ``hi`` [F, L, 3]
    the segments' extents (+inf / -inf where empty).  Object ``target_id`` is label ``target_id + 1``, as upstream."""

    def __init__(self, image_ids: Sequence, counts: np.ndarray, rows: torch.Tensor, pixel: Optional[torch.Tensor], lo: torch.Tensor,
                 hi: torch.Tensor, rgb: Optional[torch.Tensor] = None, *, centres=None):
        self.image_ids = list(image_ids)
        # ``centres``: [F, 3] host float64, None, or a function without arguments that returns one of the two -- ``build`` passes a
        # function, so the poses are read only if somebody asks (``normals``)
        self._centres = centres
        self._frame = {self._key(i): k for k, i in enumerate(self.image_ids)}
        self.counts = np.ascontiguousarray(counts, dtype=np.int64)
        self.n_labels = int(self.counts.shape[1])
        self.offsets = np.zeros(self.counts.size + 1, dtype=np.int64)
        np.cumsum(self.counts.reshape(-1), out=self.offsets[1:])
        self.rows, self.pixel, self.lo, self.hi, self.rgb = rows, pixel, lo, hi, rgb
        self.with_color = rows.shape[1] == 6

    @property
    def centres(self) -> Optional[np.ndarray]:
        """[F, 3] host float64 or None: each frame's camera centre in the rows' frame, a NaN row where it is not known.  Taken on the
        first look where ``build`` left a function."""
        if callable(self._centres):
            self._centres = self._centres()
        if self._centres is not None:
            self._centres = np.ascontiguousarray(self._centres, dtype=np.float64).reshape(len(self.image_ids), 3)
        return self._centres

    @staticmethod
    def _key(image_id):
        try:
            return int(image_id)
        except (TypeError, ValueError):
            return image_id

    def _segment(self, image_id, target_id):
        k, v = self._frame[self._key(image_id)], int(target_id) + 1
        if v <= 0 or v >= self.n_labels:
            return k, v, 0, 0
        s = k * self.n_labels + v
        return k, v, int(self.offsets[s]), int(self.offsets[s + 1])

    def cloud(self, image_id, target_id) -> torch.Tensor:
        """[M, 3] or [M, 6] float64 device tensor, a view: ``project_image_to_3d_with_mask(scene, image, get_instance_mask(scene,
        image, target_id), with_color)`` value for value; [0, C] for an object the image does not show."""
        _k, _v, a, b = self._segment(image_id, target_id)
        return self.rows[a:b]

    def count(self, image_id, target_id) -> int:
        _k, _v, a, b = self._segment(image_id, target_id)
        return b - a

    def present(self, image_id) -> List[int]:
        """The target ids with at least one selected pixel in the image, ascending."""
        k = self._frame[self._key(image_id)]
        return [int(v) - 1 for v in np.nonzero(self.counts[k])[0] if v > 0]

    def aabb(self, image_id, target_id) -> torch.Tensor:
        """[cx, cy, cz, dx, dy, dz] of the object's cloud in the image: ``calculate_aabb(cloud(...))`` from the extents the split
        took.  An empty cloud has no box (ValueError, as NumPy's reduction over no rows)."""
        k, v, a, b = self._segment(image_id, target_id)
        if a == b:
            raise ValueError(f"aabb: object {target_id} has no point in image {image_id}")
        lo, hi = self.lo[k, v], self.hi[k, v]
        return torch.cat([(hi + lo) / 2, hi - lo])

    def object_cloud(self, target_id) -> torch.Tensor:
        """The object's rows over all images, in ``image_ids`` order: one device concatenation."""
        return torch.cat([self.cloud(i, target_id) for i in self.image_ids] or [self.rows[:0]])

    # ---- every segment at once (mspa.cloud_segments): launches and read-backs do not depend on the number of segments ----------
    def cleaned(self, nb_neighbors=20, std_ratio=1.0, cluster=None) -> "InstanceClouds":
        """A new ``InstanceClouds`` of the same ``image_ids`` that holds, per (image, object), the rows
        ``ops.remove_statistical_outliers(cloud(image, object), nb_neighbors, std_ratio)`` keeps: ``counts``, ``offsets``, ``rows``,
        ``rgb``, ``lo`` / ``hi`` (and ``pixel``, where this one has it) are those of the kept rows.  One batched pass
        (``cloud_segments.remove_statistical_outliers_segments``: two read-backs, its exceptions).
        With ``cluster=(eps, min_points)`` each cleaned segment is then cut down to its largest DBSCAN cluster
        (``cloud_segments.largest_cluster_segments``: one more read-back, its exceptions) -- the blob a mask's edge bleeds onto the
        wall behind the object is dense, so the statistical rule keeps it, and a box over both blobs is not the object's."""
        from . import cloud_segments
        rows, offsets, lo, hi, index = cloud_segments.clean_segments(self.rows, self.offsets, nb_neighbors, std_ratio)
        if cluster is not None:
            rows, offsets, lo, hi, of_cleaned = cloud_segments.largest_cluster_segments(rows, offsets, *cluster)
            index = index.index_select(0, of_cleaned)
        shape = self.counts.shape
        return InstanceClouds(self.image_ids, np.diff(offsets).reshape(shape), rows, None if self.pixel is None else self.pixel.index_select(0, index),
                              lo.reshape(shape + (3,)), hi.reshape(shape + (3,)), None if self.rgb is None else self.rgb.index_select(0, index),
                              centres=self._centres)

    def normals(self, k=30, max_distance=None) -> dict:
        """``cloud_segments.normals_segments`` of every (image, label) at once -> its dict of device tensors over ``rows``: ``normal``
        [total, 3], ``curvature`` [total], ``used`` [total] int32 and ``status`` [total] uint8 (``cloud_segments.NORMALS_STATUS``); the
        rows of (frame k, label v) are ``offsets[k * L + v] : offsets[k * L + v + 1]`` as everywhere here.  The neighbours of a row
        are the ``k`` nearest rows of its OWN (image, object) cloud, within ``max_distance`` where one is given.  A depth frame samples
        surfaces from its camera centre, so every normal of frame k points towards ``centres[k]`` (the translation of the frame's
        aligned pose, which ``build`` records); it is unoriented -- first non-zero component positive -- where no centre is known: a
        NaN row of ``centres``, or an ``InstanceClouds`` made without them.  One read-back (``normals_segments``'), its ValueError; it
        needs the rows on the device."""
        from . import cloud_segments
        views = None if self.centres is None else np.repeat(self.centres, self.n_labels, axis=0)
        return cloud_segments.normals_segments(self.rows, self.offsets, k, max_distance, views)

    def boxes(self) -> torch.Tensor:
        """[F, L, 6] float64 on the device: ``aabb`` of every (image, label) at once, ``[(hi + lo) / 2, hi - lo]``; NaN where the
        segment is empty.  Enqueue only."""
        from . import cloud_segments
        return cloud_segments.boxes_of(self.lo, self.hi)

    def upright_boxes(self) -> torch.Tensor:
        """[F, L, 8] float64 on the device: the upright minimal box ``[cx, cy, cz, length, width, height, ux, uy]`` of every (image,
        label) at once -- ``ops.calculate_upright_box(cloud(image, object))`` bit for bit; NaN where the segment is empty.  One
        batched pass (``cloud_segments.upright_boxes_segments``: at most two read-backs, its exceptions); it needs the rows on the
        device."""
        from . import cloud_segments
        return cloud_segments.upright_boxes_segments(self.rows, self.offsets).reshape(self.counts.shape + (8,))

    def _object_runs(self):
        """(shift [O * F], lengths [O * F], offsets [O + 1], object_ids [O]) as host int64 arrays: run (j, k) of the regrouped rows is
        object ``object_ids[j]`` = label ``object_ids[j] + 1`` in frame k; regrouped row p of that run is row p + shift of ``rows``.  The
        objects with at least one row, ascending; the frames in ``image_ids`` order."""
        F, L = self.counts.shape
        labels = np.array([v for v in range(1, L) if self.counts[:, v].any()], dtype=np.int64)
        segments = (np.arange(F, dtype=np.int64)[None, :] * L + labels[:, None]).reshape(-1)      # object-major, then frame
        lengths = self.counts.reshape(-1)[segments]
        ends = np.cumsum(lengths)
        offsets = np.zeros((len(labels) + 1,), dtype=np.int64)
        if len(labels):
            offsets[1:] = ends.reshape(len(labels), F)[:, -1]
        return self.offsets[segments] - (ends - lengths), lengths, offsets, labels - 1

    def by_object(self, voxel_size=None):
        """``(rows, offsets, object_ids)``: the same rows regrouped so that the rows of object ``object_ids[j]`` over all images are
        ``rows[offsets[j]:offsets[j + 1]]``, value for value ``object_cloud(object_ids[j])``; the objects with at least one row,
        ascending; ``offsets`` and ``object_ids`` are host int64 arrays.  One device gather whose index is built from the host
        ``offsets``: a run table of O * F entries goes up, the index itself is expanded on the device.  Enqueue only.
        With a ``voxel_size`` the regrouped rows are the voxel means of each object's fused cloud instead, value for value
        ``ops.voxel_down_sample(object_cloud(object_ids[j]), voxel_size)``: every overlapping frame contributes its own sample of
        the same surface, and the grid leaves one row per occupied voxel.  That form makes the one read-back of
        ``cloud_segments.voxel_down_sample_segments`` and raises its exceptions; it needs the rows on the device."""
        shift, lengths, offsets, object_ids = self._object_runs()
        total = int(offsets[-1])
        if self.rows.is_cuda:
            from . import cloud_segments
            shift, lengths = cloud_segments._upload(shift, lengths, device=self.rows.device)
        else:
            shift, lengths = torch.from_numpy(shift), torch.from_numpy(lengths)
        index = torch.arange(total, dtype=torch.int64, device=self.rows.device) + torch.repeat_interleave(shift, lengths, output_size=total)
        rows = self.rows.index_select(0, index)
        if voxel_size is not None:
            from . import cloud_segments
            rows, offsets, _counts = cloud_segments.voxel_down_sample_segments(rows, offsets, voxel_size)
        return rows, offsets, object_ids

    def view_coverage(self, tau, voxel_size=None) -> torch.Tensor:
        """[F, L] float64 on the device: for every (image, label) with rows, the share of that object's fused cloud
        (``by_object(voxel_size)``) that lies within ``tau`` of this image's cloud of the object -- how much of the object the frame
        shows; NaN where the segment is empty.  One index over the per-image batch (``cloud_segments.target_index``: one read-back,
        its ValueError), one pair table (object run, image segment), one query with ``max_distance=tau`` -- a frame that misses the
        object walks a bounded block -- and one summary (``cloud_segments.fit_segments``).  ``tau`` finite and > 0.  It needs the
        rows on the device."""
        from . import cloud_segments
        F, L = self.counts.shape
        fused, fused_offsets, object_ids = self.by_object(voxel_size)
        frames, labels = np.nonzero(self.counts[:, 1:] if L > 1 else self.counts[:, :0])
        labels = labels + 1
        run_of = np.full((L,), -1, dtype=np.int64)
        run_of[np.asarray(object_ids, dtype=np.int64) + 1] = np.arange(len(object_ids), dtype=np.int64)
        pairs = np.stack([run_of[labels], frames.astype(np.int64) * L + labels], axis=1).astype(np.int64)
        out = torch.full((F * L,), float("nan"), dtype=torch.float64, device=self.rows.device)
        if len(pairs) == 0:
            return out.reshape(F, L)
        index = cloud_segments.target_index(self.rows, self.offsets)
        found = index.nearest(fused, fused_offsets, pairs, max_distance=tau, want_index=False)
        fit = cloud_segments.fit_segments(found["distance"], found["offsets"], tau)
        where, = cloud_segments._upload(pairs[:, 1].copy(), device=self.rows.device)
        out[where] = fit["within"].to(torch.float64) / fit["rows"].to(torch.float64)
        return out.reshape(F, L)

    def view_alignment(self, max_distance, voxel_size=None, iterations=30, fused=None) -> dict:
        """For every (image, label) with rows, the rigid transform that carries this image's cloud of the object onto the object's
        fused cloud (``by_object(voxel_size)``), by point-to-point ICP from the identity (``cloud_segments.TargetIndex.register``
        with the cap ``max_distance`` and ``iterations``) -> a dict of device tensors: ``R`` [F, L, 3, 3], ``t`` [F, L, 3], ``angle``
        [F, L] (the rotation's angle in [0, pi]: 2 atan2(|xyz|, w) of its quaternion, taken from R as atan2(sin, cos)), ``shift``
        [F, L] (how far the transform moves the segment's centroid), ``fitness``, ``inlier_rmse`` [F, L] float64 -- NaN where the
        segment is empty -- and ``status`` [F, L] int32 (``cloud_segments.ALIGN_STATUS``; -1 where the segment is empty).  ``angle``
        and ``shift`` are torch expressions.  It says BY WHICH motion a frame's cloud lies off the object: pose drift, or an object
        that moved.  The fused cloud contains the frame's own samples, so a frame that dominates its object is pulled towards itself:
        without a ``voxel_size`` every row finds itself at distance 0 and the answer is the identity exactly; with one, the voxel
        means are drawn towards the frame by its share of the samples, and the motion reported is short by about that share.
        ``fused=(rows, offsets, object_ids)`` -- the ``by_object`` of ANOTHER ``InstanceClouds`` (the other frames, an earlier visit, a
        reference scan) -- replaces the target and has no such pull; a (image, label) whose object it lacks has an empty target and
        is FEW.  One index over the fused clouds (``cloud_segments.target_index``: one read-back, its ValueError) on top of
        ``by_object``'s read-back; it needs the rows on the device."""
        from . import cloud_segments
        F, L = self.counts.shape
        dev = self.rows.device
        nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)      # noqa: E731
        out = {"R": nan(F * L, 3, 3), "t": nan(F * L, 3), "angle": nan(F * L), "shift": nan(F * L), "fitness": nan(F * L), "inlier_rmse": nan(F * L),
               "status": torch.full((F * L,), -1, dtype=torch.int32, device=dev)}
        shaped = lambda: {k: v.reshape((F, L) + tuple(v.shape[1:])) for k, v in out.items()}       # noqa: E731
        target, target_offsets, object_ids = self.by_object(voxel_size) if fused is None else fused
        frames, labels = np.nonzero(self.counts[:, 1:] if L > 1 else self.counts[:, :0])
        labels = labels + 1
        if len(frames) == 0:
            return shaped()
        object_ids = np.asarray(object_ids, dtype=np.int64)
        target_offsets = np.append(np.asarray(target_offsets, dtype=np.int64), target_offsets[-1])  # one empty segment behind the objects
        run_of = np.full((max(L, int(object_ids.max(initial=-1)) + 2),), len(object_ids), dtype=np.int64)
        run_of[object_ids + 1] = np.arange(len(object_ids), dtype=np.int64)
        pairs = np.stack([frames.astype(np.int64) * L + labels, run_of[labels]], axis=1).astype(np.int64)
        reg = cloud_segments.target_index(target, target_offsets).register(self.rows, self.offsets, pairs, max_distance=max_distance, iterations=iterations)
        where, lengths = cloud_segments._upload(pairs[:, 0].copy(), self.counts.reshape(-1), device=dev)
        R, t = reg["R"], reg["t"]
        xyz = self.rows[:, :3].to(torch.float64).contiguous()
        centre = (torch.segment_reduce(xyz, "sum", lengths=lengths, axis=0, unsafe=True) / lengths.to(torch.float64)[:, None]).index_select(0, where)
        moved = (R @ centre[:, :, None])[:, :, 0] + t
        sine = 0.5 * torch.sqrt((R[:, 2, 1] - R[:, 1, 2]) ** 2 + (R[:, 0, 2] - R[:, 2, 0]) ** 2 + (R[:, 1, 0] - R[:, 0, 1]) ** 2)
        cosine = 0.5 * (R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2] - 1.0)
        out["R"][where], out["t"][where], out["status"][where] = R, t, reg["status"]
        out["angle"][where], out["shift"][where] = torch.atan2(sine, cosine), torch.linalg.vector_norm(moved - centre, dim=1)
        out["fitness"][where], out["inlier_rmse"][where] = reg["fitness"], reg["inlier_rmse"]
        return shaped()

    def cleaned_objects(self, nb_neighbors=20, std_ratio=1.0, voxel_size=None, cluster=None, upright=False):
        """``(rows, offsets, object_ids, boxes)``: ``by_object()`` through the same batched cleaning -- per object the rows
        ``ops.remove_statistical_outliers(object_cloud(t), nb_neighbors, std_ratio)`` keeps, back to back, with host ``offsets``
        [O + 1]; ``boxes`` [O, 6] float64 (device) their ``calculate_aabb``, NaN where nothing is kept.  With a ``voxel_size`` each
        fused cloud is down-sampled first (``by_object(voxel_size)``), then cleaned: the neighbours of a point are then other
        places of the surface, not its own copies from other frames.  With ``cluster=(eps, min_points)`` each cleaned cloud is then
        cut down to its largest DBSCAN cluster (``cloud_segments.largest_cluster_segments``), and the boxes are those of what is
        kept.  With ``upright=True`` one more element follows: [O, 8] float64 (device), the upright minimal boxes of what is kept
        (``cloud_segments.upright_boxes_segments``: at most two more read-backs, its exceptions), NaN where nothing is kept."""
        from . import cloud_segments
        rows, offsets, object_ids = self.by_object(voxel_size)
        kept, kept_offsets, lo, hi = cloud_segments.remove_statistical_outliers_segments(rows, offsets, nb_neighbors, std_ratio)
        if cluster is not None:
            kept, kept_offsets, lo, hi, _index = cloud_segments.largest_cluster_segments(kept, kept_offsets, *cluster)
        out = (kept, kept_offsets, object_ids, cloud_segments.boxes_of(lo, hi))
        return out + (cloud_segments.upright_boxes_segments(kept, kept_offsets),) if upright else out


def _mask_path(handler, scene_id, image_id) -> str:
    return os.path.join(handler.mask_image_root, scene_id, "instance-filt", f"{int(image_id)}.png")


def _rows(xyz: torch.Tensor, rgb: Optional[torch.Tensor]) -> torch.Tensor:
    return xyz if rgb is None else torch.cat([xyz, rgb.to(torch.float64)], dim=1)


DECODE_GROUP = 256          # frames decoded in one batch: the decode kernels take one wave per frame, so their time is a frame's, not the batch's


def _decode_group(handler, scene_id, ids, mask_paths, with_color, device, num_workers, images, color_hw):
    """(depth [f, h, w] int16, labels [f, H, W] uint8, rgb [f, H, W, 3] uint8 or None) of a group of posed frames, each decoded once on
    the device.  Raises ValueError where the device path declines."""
    depth_paths = [handler.get_depth_image_path(scene_id, i) for i in ids]
    if any(p in images.MEMORY for p in depth_paths):                       # registered frames (synthetic scenes, tests): host, then upload
        depth = engine.depth_to_device(ingest.read_depth_frames(depth_paths, num_workers, general_reader=images.read_depth,
                                                                memory=images.MEMORY), device)
    else:
        depth = ingest.read_depth_frames_device(depth_paths, device, num_workers, general_reader=images.read_depth)
    labels = ingest.read_label_frames_device(mask_paths, device, num_workers, general_reader=images.read_depth)
    H, W = int(labels.shape[1]), int(labels.shape[2])
    if (H, W) != tuple(color_hw):
        raise ValueError(f"mask of {(H, W)}, colour frames of {tuple(color_hw)}")
    rgb = None
    if with_color:
        color_paths = [handler.get_image_path(scene_id, i) for i in ids]
        if any(p in images.MEMORY for p in color_paths):
            rgb = torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(images.read_color_rgb(p)) for p in color_paths]))).to(device)
        else:
            rgb = handler.color_frames_device(scene_id, ids, device, num_workers)
        if tuple(rgb.shape) != (len(ids), H, W, 3) or rgb.dtype != torch.uint8:
            raise ValueError(f"colour frames of {tuple(rgb.shape)} {rgb.dtype}")
    return depth, labels, rgb


def _split_chunk(handler, scene_id, ids, depth, labels, rgb, device):
    """One chunk of decoded frames through ONE K3 exact launch (pairs (f, f): xyz_f64 + valid_u8 of every pixel) and the split."""
    H, W = int(labels.shape[1]), int(labels.shape[2])
    K = handler.get_intrinsic_matrix(scene_id, ids[0])
    A = handler.get_world_to_axis_align_matrix(scene_id)
    mats = torch.from_numpy(engine.frame_matrices(np.asarray(K, np.float64), np.asarray(A, np.float64),
                                                  [np.asarray(handler.get_extrinsic_matrix(scene_id, i, warning=False), np.float64)
                                                   for i in ids])).to(device)
    pairs = torch.arange(len(ids), dtype=torch.int32, device=device)[:, None].repeat(1, 2).contiguous()
    out = engine.alloc_pair_outputs(len(ids), (H, W), ("xyz_f64", "valid_u8"), device)
    engine.pair_reproject(depth, mats, pairs, (H, W), out)
    return engine.instance_split(labels, out["valid_u8"], out["xyz_f64"], rgb)


def _centres(handler, scene_id, ids) -> np.ndarray:
    """[F, 3]: the camera centre of every posed frame in the clouds' (axis-aligned) frame, the translation of ``A @ E``; a NaN row for a
    frame without a finite pose."""
    out = np.full((len(ids), 3), np.nan)
    A = None
    for k, i in enumerate(ids):
        if handler.is_posed_image_valid(scene_id, i):
            if A is None:
                A = np.asarray(handler.get_world_to_axis_align_matrix(scene_id), np.float64)
            out[k] = (A @ np.asarray(handler.get_extrinsic_matrix(scene_id, i, warning=False), np.float64))[:3, 3]
    return out


def _host_composition(handler, scene_id, ids, with_color, device, images) -> InstanceClouds:
    """The same object from the per-object composition the reference writes: get_instance_mask + project_image_to_3d_with_mask
    per (image, label present in the mask)."""
    per_frame, n_labels = [], 256
    for i in ids:
        clouds = {}
        if handler.is_posed_image_valid(scene_id, i):
            path = _mask_path(handler, scene_id, i)
            try:
                mask_image = images.read_depth(path)
            except Exception:
                mask_image = None
            if mask_image is None:
                raise FileNotFoundError(f"Mask image not found at path: {path}")
            for v in np.unique(np.asarray(mask_image)):
                if int(v) > 0:
                    c = handler.project_image_to_3d_with_mask(scene_id, i, handler.get_instance_mask(scene_id, i, int(v) - 1), with_color)
                    if len(c):
                        clouds[int(v)] = np.asarray(c, dtype=np.float64)
                        n_labels = max(n_labels, int(v) + 1)
        else:
            handler.get_extrinsic_matrix(scene_id, i)                      # (the reference's warning)
        per_frame.append(clouds)
    C = 6 if with_color else 3
    counts = np.zeros((len(ids), n_labels), dtype=np.int64)
    lo = np.full((len(ids), n_labels, 3), np.inf)
    hi = np.full((len(ids), n_labels, 3), -np.inf)
    blocks = []
    for k, clouds in enumerate(per_frame):
        for v in sorted(clouds):
            counts[k, v] = len(clouds[v])
            lo[k, v], hi[k, v] = clouds[v][:, :3].min(axis=0), clouds[v][:, :3].max(axis=0)
            blocks.append(clouds[v])
    rows = np.concatenate(blocks) if blocks else np.zeros((0, C))
    return InstanceClouds(ids, counts, torch.from_numpy(np.ascontiguousarray(rows.reshape(-1, C))).to(device), None,
                          torch.from_numpy(lo).to(device), torch.from_numpy(hi).to(device), centres=lambda: _centres(handler, scene_id, ids))


def build(handler, scene_id, image_ids=None, with_color=False, device="cuda", num_workers=8, max_dense_bytes=1 << 30,
          images=None) -> InstanceClouds:
    """``SceneInfoHandler.instance_clouds``: see there.  ``images`` is the handler's image-I/O module (its in-memory registry and
    general readers)."""
    ids = handler.get_all_image_ids(scene_id) if image_ids is None else list(image_ids)
    LAST_INSTANCE_CLOUDS.clear()
    posed = [i for i in ids if handler.is_posed_image_valid(scene_id, i)]
    mask_paths = {}
    for i in posed:
        p = _mask_path(handler, scene_id, i)
        if p not in images.MEMORY and not os.path.isfile(p):
            raise FileNotFoundError(f"Mask image not found at path: {p}")
        mask_paths[InstanceClouds._key(i)] = p
    reason = ""
    if any(p in images.MEMORY for p in mask_paths.values()):
        reason = "a mask is registered in memory, not a file"
    color_hw = tuple(handler.get_image_shape(scene_id, posed[0])) if posed else (0, 0)
    parts = []
    if not reason and posed:
        per_chunk = max(1, int(max_dense_bytes) // max(1, color_hw[0] * color_hw[1] * 24))
        try:
            group = max(per_chunk, DECODE_GROUP // per_chunk * per_chunk)
            for g in range(0, len(posed), group):
                gids = posed[g:g + group]
                depth, labels, rgb = _decode_group(handler, scene_id, gids, [mask_paths[InstanceClouds._key(i)] for i in gids], with_color,
                                                   device, num_workers, images, color_hw)
                for b in range(0, len(gids), per_chunk):
                    e = b + per_chunk
                    parts.append(_split_chunk(handler, scene_id, gids[b:e], depth[b:e], labels[b:e], None if rgb is None else rgb[b:e],
                                              device))
        except ValueError as e:
            reason = str(e)
    if reason:
        LAST_INSTANCE_CLOUDS.update(path="host", reason=reason)
        return _host_composition(handler, scene_id, ids, with_color, device, images)
    LAST_INSTANCE_CLOUDS.update(path="device", reason="")
    # the chunks' segments back to back, the frames without a finite pose as empty rows of the tables
    L = engine.SPLIT_LABELS
    counts = np.zeros((len(ids), L), dtype=np.int64)
    lo = torch.full((len(ids), L, 3), float("inf"), dtype=torch.float64, device=device)
    hi = torch.full((len(ids), L, 3), float("-inf"), dtype=torch.float64, device=device)
    where = {InstanceClouds._key(i): k for k, i in enumerate(ids)}
    at = [where[InstanceClouds._key(i)] for i in posed]
    for i in ids:
        if InstanceClouds._key(i) not in mask_paths:
            handler.get_extrinsic_matrix(scene_id, i)                      # (the reference's warning for a non-finite pose)
    C = 6 if with_color else 3
    if parts:
        counts[at] = np.concatenate([p[0] for p in parts])
        idx = torch.tensor(at, dtype=torch.int64, device=device)
        lo[idx] = torch.cat([p[5] for p in parts])
        hi[idx] = torch.cat([p[6] for p in parts])
        xyz = parts[0][2] if len(parts) == 1 else torch.cat([p[2] for p in parts])
        rgb = None if not with_color else (parts[0][3] if len(parts) == 1 else torch.cat([p[3] for p in parts]))
        pixel = parts[0][4] if len(parts) == 1 else torch.cat([p[4] for p in parts])
        rows = _rows(xyz, rgb)
    else:
        rows, rgb = torch.zeros((0, C), dtype=torch.float64, device=device), None
        pixel = torch.zeros((0,), dtype=torch.int32, device=device)
    return InstanceClouds(ids, counts, rows, pixel, lo, hi, rgb, centres=lambda: _centres(handler, scene_id, ids))
