"""Freeze the reference's per-object clouds on one synthetic scene into tests/golden/instance_clouds.npz (arrays only).

Runs the unmodified reference through oracle.ref_harness (its in-memory ``cv2.imread``): for every (image, target) the result of
``project_image_to_3d_with_mask(scene, image, get_instance_mask(scene, image, target), with_color)`` with and without colour, and
``calculate_aabb`` of it.  The scene: 3 frames, colour and mask 162 x 121 over depth 80 x 60 (ScanNet's 2.025 / 2.0167 ratios),
7 labels -- label 1 a ring that touches all four borders, label 5 an object whose depth is all zero, label 6 a single pixel with
valid depth, the others rectangles over zero-depth holes -- and target 7 (label 8), which no image shows.

To keep the file small the objects cover about a third of the frame, and a cloud is stored once: ``xyz_<k>_<t>`` float64 plus
``rgb_<k>_<t>`` uint8.  The generator asserts that the reference's colourless result IS ``xyz`` and its coloured result IS
``np.hstack((xyz, rgb))`` bit for bit before it drops the duplicates.  Needs the reference tree (MSPA_REFERENCE_ROOT)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "multi-spatialmllm_amd"), ROOT):
    sys.path.insert(0, p)

from mspa import synth  # noqa: E402
from oracle import ref_harness as RH  # noqa: E402

COLOR_HW, DEPTH_HW, N_FRAMES, SEED = (121, 162), (60, 80), 3, 2207
TARGETS = tuple(range(8))            # labels 1 .. 8; label 8 is in no image


def label_image(k):
    """[121, 162] uint8 labels of frame k (the rectangles move with k)."""
    H, W = COLOR_HW
    s = 3 * k
    a = np.zeros((H, W), np.uint8)
    a[10:40, 10 + s:45 + s] = 2
    a[30:60, 90:130 - s] = 3
    a[80:110, 20:70] = 4
    a[85:100, 100 + s:120 + s] = 5
    a[60 + k, 70] = 6
    a[55:75, 5:40] = 7
    a[:2, :] = a[-2:, :] = 1
    a[:, :2] = a[:, -2:] = 1
    return a


def depth_pixels(my, mx):
    """The depth pixel the reference reads for colour pixel (my, mx): OPS:272-290."""
    dy = np.clip(np.round(my * (DEPTH_HW[0] / COLOR_HW[0])).astype(int), 0, DEPTH_HW[0] - 1)
    dx = np.clip(np.round(mx * (DEPTH_HW[1] / COLOR_HW[1])).astype(int), 0, DEPTH_HW[1] - 1)
    return dy, dx


def main(out_path):
    ns = RH.import_reference()
    sc = synth.make_scene(SEED, n_points=64, n_frames=N_FRAMES, color_hw=COLOR_HW, depth_hw=DEPTH_HW, invalid_pose_frac=0.0,
                          zero_frac=0.07, with_color=True, scene_id="scene0950_00")
    ids = sc.image_ids
    labels = np.stack([label_image(k) for k in range(N_FRAMES)])
    for k, i in enumerate(ids):
        d = sc.depth[i]
        d[depth_pixels(*np.where(labels[k] == 5))] = 0                       # object 4: no valid depth at all
        d[depth_pixels(*np.where(labels[k] == 6))] = 1500 + 10 * k            # object 5: its one pixel is valid
    handler = RH.make_handler(ns, [sc])
    handler.mask_image_root = os.path.join(handler._mspa_root, "scans")
    for k, i in enumerate(ids):
        RH.STORE.images[os.path.join(handler.mask_image_root, sc.scene_id, "instance-filt", f"{int(i)}.png")] = labels[k]
    data = {"image_ids": np.array(ids), "targets": np.array(TARGETS), "depth": np.stack([sc.depth[i] for i in ids]), "labels": labels,
            "color": np.stack([sc.color[i] for i in ids]), "K": sc.K, "A": sc.A, "E": np.stack([sc.E[i] for i in ids])}
    sizes = np.zeros((N_FRAMES, len(TARGETS)), np.int64)
    for k, i in enumerate(ids):
        for t in TARGETS:
            mask = handler.get_instance_mask(sc.scene_id, i, t)
            plain = handler.project_image_to_3d_with_mask(sc.scene_id, i, mask, with_color=False)
            coloured = handler.project_image_to_3d_with_mask(sc.scene_id, i, mask, with_color=True)
            assert plain.dtype == np.float64 and coloured.dtype == np.float64 and plain.shape[1:] == (3,) and coloured.shape[1:] == (6,)
            rgb = coloured[:, 3:].astype(np.uint8)
            assert np.hstack((plain, rgb)).tobytes() == coloured.tobytes()    # so xyz + uint8 rgb IS both results
            data[f"xyz_{k}_{t}"], data[f"rgb_{k}_{t}"] = plain, rgb
            sizes[k, t] = len(plain)
            if len(plain):
                data[f"aabb_{k}_{t}"] = ns.OPS.calculate_aabb(plain)
    data["sizes"] = sizes
    assert (sizes[:, 4] == 0).all() and (sizes[:, 5] == 1).all() and (sizes[:, 7] == 0).all() and (sizes[:, [0, 1, 2, 3, 6]] >= 2).all(), sizes
    np.savez_compressed(out_path, **data)
    print(out_path, os.path.getsize(out_path), "bytes;", int(sizes.sum()), "points")
    assert os.path.getsize(out_path) < (1 << 20)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "instance_clouds.npz"))
