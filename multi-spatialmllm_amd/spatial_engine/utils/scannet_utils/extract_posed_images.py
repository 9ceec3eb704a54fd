"""Mirror of the reference's utils/scannet_utils/extract_posed_images.py on top of ``mspa.sens``: the same ``SensorData``
surface (load with ``frame_skip``, export of depth PNGs, colour JPEGs, pose and intrinsic text files) and the same
``posed_images/<scene>/`` layout.  Differences, both deliberate: skipped frames are seeked over instead of being read, and
the JPEG payloads are written out as stored instead of being decoded and re-encoded.  ``--depth_png device`` encodes the
depth PNGs on the GPU (same pixels and filtered scanlines as Pillow's files, another deflate stream); scenes then run one
after another in this process, with the depth frames inflated on the device, instead of in a process pool."""
from __future__ import annotations

import os
import time
from argparse import ArgumentParser

import numpy as np

from mspa import sens as _sens

COMPRESSION_TYPE_COLOR = dict(_sens.COLOR_COMPRESSION)
COMPRESSION_TYPE_DEPTH = dict(_sens.DEPTH_COMPRESSION)


class RGBDFrame:
    """One kept frame: pose, timestamps and the undecoded payload sizes (reference: :28-56)."""

    def __init__(self, scene: "_sens.SensScene", k: int):
        self.camera_to_world = scene.camera_to_world[k]
        self.timestamp_color, self.timestamp_depth = (int(v) for v in scene.timestamps[k])
        self.color_data = scene.color_jpeg[k] if scene.color_jpeg is not None else b""
        self._scene, self._k = scene, k

    def decompress_depth(self, compression_type):
        assert compression_type in ("zlib_ushort", "raw_ushort")
        s = self._scene
        if s.depth_device is not None:
            return s.depth_device[self._k].cpu().numpy().view(np.uint16).tobytes()
        return s.depth[self._k].tobytes()

    def decompress_color(self, compression_type):
        assert compression_type == "jpeg"
        import io
        from PIL import Image
        return np.asarray(Image.open(io.BytesIO(self.color_data)).convert("RGB"))


class SensorData:
    def __init__(self, filename, frame_skip, want_color=True, depth_to_device=None):
        self.version = _sens.VERSION
        self.load(filename, frame_skip, want_color, depth_to_device)

    def load(self, filename, frame_skip, want_color=True, depth_to_device=None):
        s = self._scene = _sens.read_sens(filename, frame_skip, want_color=want_color, depth_to_device=depth_to_device)
        self.sensor_name = s.sensor_name
        self.intrinsic_color, self.extrinsic_color = s.intrinsic_color, s.extrinsic_color
        self.intrinsic_depth, self.extrinsic_depth = s.intrinsic_depth, s.extrinsic_depth
        self.color_compression_type, self.depth_compression_type = s.color_compression, s.depth_compression
        self.color_height, self.color_width = s.color_hw
        self.depth_height, self.depth_width = s.depth_hw
        self.depth_shift = s.depth_shift
        print(f"Number of total frames: {s.n_frames_total}")
        self.frames = [RGBDFrame(s, k) for k in range(len(s.frame_index))]
        print(f"Exported {len(self.frames)} frames. Frame skip is {frame_skip}.")

    index_to_str = staticmethod(_sens.SensScene.index_to_str)

    @staticmethod
    def save_mat_to_file(matrix, filename):
        with open(filename, "w") as f:
            f.write(_sens.matrix_text(matrix))

    def export_depth_images(self, output_path, depth_png="pillow"):
        assert depth_png in ("pillow", "device")
        os.makedirs(output_path, exist_ok=True)
        paths = [os.path.join(output_path, self.index_to_str(k) + ".png") for k in range(len(self.frames))]
        if depth_png == "device":
            s = self._scene
            _sens.write_depth_pngs_device(s.depth_device if s.depth_device is not None else s.depth, paths)
            return
        from PIL import Image
        for k in range(len(self.frames)):
            Image.fromarray(self._scene.depth[k]).save(os.path.join(output_path, self.index_to_str(k) + ".png"))

    def export_color_images(self, output_path):
        os.makedirs(output_path, exist_ok=True)
        for k, frame in enumerate(self.frames):
            with open(os.path.join(output_path, self.index_to_str(k) + ".jpg"), "wb") as f:
                f.write(frame.color_data)

    def export_poses(self, output_path):
        os.makedirs(output_path, exist_ok=True)
        for k, frame in enumerate(self.frames):
            self.save_mat_to_file(frame.camera_to_world, os.path.join(output_path, self.index_to_str(k) + ".txt"))

    def export_intrinsics(self, output_path):
        os.makedirs(output_path, exist_ok=True)
        self.save_mat_to_file(self.intrinsic_color, os.path.join(output_path, "intrinsic.txt"))


def process_scene(path, frame_skip, idx, depth_png="pillow"):
    """posed_images/<idx>/ from <path>/<idx>/<idx>.sens (reference: :161-178).  ``depth_png="device"``: the depth frames are
    inflated and the PNGs encoded on the GPU."""
    print(f"Processing {idx}.")
    t1 = time.time()
    output_path = os.path.join("posed_images", idx)
    if os.path.exists(output_path):
        print(f"{output_path} already exists. Skip.")
        return
    data = SensorData(os.path.join(path, idx, f"{idx}.sens"), frame_skip,
                      depth_to_device="cuda" if depth_png == "device" else None)
    data.export_color_images(output_path)
    data.export_intrinsics(output_path)
    data.export_poses(output_path)
    data.export_depth_images(output_path, depth_png)
    print(f"Finish processing {idx}. Using {time.time() - t1}s.")


def process_directory(path, frame_skip, nproc, depth_png="pillow"):
    print(f"processing {path}")
    scan_ids = sorted(os.listdir(path))
    if nproc and nproc > 1 and depth_png == "pillow":      # device mode: one process holds the GPU, scenes in turn
        from functools import partial
        from multiprocessing import Pool
        with Pool(nproc) as pool:
            pool.map(partial(process_scene, path, frame_skip), scan_ids)
    else:
        for idx in scan_ids:
            process_scene(path, frame_skip, idx, depth_png)


if __name__ == "__main__":
    parser = ArgumentParser()
    parser.add_argument("--frame_skip", type=int, default=1, help="export every nth frame")
    parser.add_argument("--nproc", type=int, default=20)
    parser.add_argument("--depth_png", choices=("pillow", "device"), default="pillow",
                        help="encode the depth PNGs with Pillow (default) or on the GPU")
    args = parser.parse_args()
    if os.path.exists("scans"):
        process_directory("scans", args.frame_skip, args.nproc, args.depth_png)
    if os.path.exists("scans_test"):
        process_directory("scans_test", args.frame_skip, args.nproc, args.depth_png)
