"""ctypes binding of libmspa.so.  Fails loudly: no library, no engine."""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_double, c_int, c_int32, c_int64, c_uint32, c_void_p, POINTER

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("MSPA_LIB", os.path.join(_PKG_ROOT, "libmspa.so"))

MSPA_OK, MSPA_EINVAL, MSPA_EHIP, MSPA_EUNSUPPORTED = 0, -1, -2, -3
MAT_KINV, MAT_E, MAT_A, MAT_EINV_ALIGNED, MAT_K, MAT_UNPROJ, MAT_REPROJ, MAT_BOUNDS, FRAME_MATS = 0, 1, 2, 3, 4, 5, 6, 7, 8
GUARD_C = 256.0
CAM_EINV, CAM_K, CAM_BOUNDS, CAM_MATS = 0, 1, 2, 3
PAIR_FAST = 1
PAIR_STREAM = 2
PAIR_WORD_STRIPES = 0x200      # retired: accepted and ignored (the word-stripe kernel it selected was removed)
CORR_TILE_W, CORR_TILE_H, CORR_TILE_CAP = 64, 48, 64 * 48
JPEG_DESC_BYTES = 4224
KNN_GRID_BYTES, KNN_MAX_K = 112, 64      # csrc/knn_grid_core.h: sizeof(Grid), kMaxK
SEGMENTS_MAX = 1 << 24                   # csrc/cloud_segments_core.h: kMaxSegments
VOXEL_AXIS_BITS, VOXEL_MAX_COLUMNS = 21, 65536   # csrc/voxel_grid_core.h: kAxisBits; include/mspa.h: MSPA_VOXEL_MAX_COLUMNS
RESIZE_BILINEAR, RESIZE_BICUBIC = 2, 3     # Pillow's Image.Resampling numbers
CLOUD_DISTANCE_GRID_K, CLOUD_DISTANCE_MAX_ROWS, CLOUD_DISTANCE_MAX_PAIRS = 1, 1 << 30, 1 << 24   # csrc/cloud_distance_core.h
CLOUD_ALIGN_OK, CLOUD_ALIGN_FEW, CLOUD_ALIGN_DEGENERATE, CLOUD_ALIGN_SWEEPS, CLOUD_ALIGN_GAP_EXPONENT = 0, 1, 2, 12, -26   # csrc/cloud_align_core.h
CLOUD_ALIGN_ORTHO_BOUND = 32.0 * 2.0 ** -53    # csrc/cloud_align_core.h: kOrthoBound, the derived bound on max |R^T R - I|
CLOUD_NORMALS_OK, CLOUD_NORMALS_FEW, CLOUD_NORMALS_DEGENERATE, CLOUD_NORMALS_SWEEPS, CLOUD_NORMALS_GAP_EXPONENT = 0, 1, 2, 8, -26   # csrc/cloud_normals_core.h
CLOUD_NORMALS_UNIT_BOUND = 8.0 * 2.0 ** -53    # csrc/cloud_normals_core.h: kUnitBound, the derived bound on | |n|^2 - 1 |
UPRIGHT_IOU_PAIRS, UPRIGHT_IOU_MATRIX = 0, 1   # include/mspa.h: the two launch shapes of mspa_upright_iou_device
LINKAGE_MAX_POINTS = 2048
SNAPPY_BLOCK, SNAPPY_SLOT = 65536, 76544   # csrc/snappy_core.h: kBlock, kSlot
# csrc/snappy_core.h: what mspa_snappy_decompress_host returns for, and the device writes as the status of, a stream it declines
SNAPPY_EPREAMBLE, SNAPPY_ETRUNCATED, SNAPPY_EOVERRUN, SNAPPY_EOFFSET, SNAPPY_ETRAILING, SNAPPY_ESHORT = -16, -17, -18, -19, -20, -21
SNAPPY_NOT_BLOCKWISE = -22     # mspa_snappy_block_starts_host alone: a valid stream that does not decode block by block
SNAPPY_SEGMENT = 2048          # csrc/snappy_decode.hip: kSeg, the compressed bytes one wave of the block-start scan takes
# csrc/rle_hybrid_core.h: what mspa_rle_hybrid_take_host returns for, and mspa_parquet_dict_spans_device writes as the code of, runs it declines
RLE_EBITWIDTH, RLE_EHEADER, RLE_EZERORUN, RLE_ETRUNCATED, RLE_ESHORT = -32, -33, -34, -35, -36
# mspa_index_lists_pick_device's per-sample status (csrc/index_rows.hip: kPick*) and the samples one workgroup takes
PICK_OK, PICK_EROW, PICK_EPOSITION, PICK_ERANGE, PICK_EOFFSETS = 0, 1, 2, 4, 8
PICK_BLOCK = 256
# csrc/pair_bins_core.h: the class bytes that are no bin, the most bins a table may have and the entries of a class table;
# csrc/pair_table.hip: the page flags of mspa_parquet_double_layout_device and the rows of its layout table
PAIR_CLASS_ZERO, PAIR_CLASS_DROPPED, PAIR_MAX_BINS, PAIR_CLASSES = 254, 255, 250, 256
PAGE_LEVELS_INLINE, PAGE_DICT_CODED, PAGE_LEVELS_GIVEN = 1, 2, 4
LAYOUT_LEVEL_OFFSET, LAYOUT_LEVEL_BYTES, LAYOUT_VALUE_OFFSET, LAYOUT_VALUE_BYTES, LAYOUT_BIT_WIDTH, LAYOUT_ROWS = range(6)
LINKAGE_OK, LINKAGE_NONFINITE, LINKAGE_ITERATION_CAP = 0, 1, 2
# csrc/track_mining_core.h: a point's statistics record, its flags, the classes of a pick and the longest track
TRACK_STAT_V, TRACK_STAT_STATIC, TRACK_STAT_MOVING, TRACK_STAT_MIN_BITS, TRACK_STAT_MAX_BITS, TRACK_STAT_FLAGS, TRACK_STAT_WORDS = range(7)
TRACK_FLAG_NONFINITE, TRACK_FLAG_BAD_POINT = 1, 2
TRACK_BINS, TRACK_CLASS_STATIC, TRACK_CLASSES, TRACK_MAX_FRAMES = 10, 10, 11, 65535
KERNEL_NONE, KERNEL_PAIR_EXACT, KERNEL_PAIR_FAST, KERNEL_PAIR_FAST_LINEAR, KERNEL_PAIR_FAST_TIGHT, KERNEL_PAIR_FAST_SCALED, KERNEL_PAIR_FAST_RECT = range(7)   # KERNEL_PAIR_FAST_SCALED (5): retired id, never reported


class MspaError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"libmspa error {code}: {message}")
        self.code = code


_lib = None

# name -> (restype, argtypes); mirrors include/mspa.h one to one
_SIGNATURES = {
    "mspa_version": (c_int, []),
    "mspa_last_error_string": (c_char_p, []),
    "mspa_frame_bounds_host": (c_int, [c_void_p, c_int32]),
    "mspa_camera_bounds_host": (c_int, [c_void_p, c_int32]),
    "mspa_device_info": (c_int, [c_int, POINTER(c_int), POINTER(c_int), POINTER(c_int64), POINTER(c_int),
                                 c_char_p, c_int]),
    "mspa_pair_reproject": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int64,
                                    c_int32, c_int32, c_int32, c_int32,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p]),
    "mspa_pair_reproject_last_kernel": (c_int, []),
    "mspa_corr_tiles": (c_int64, [c_int32, c_int32]),
    "mspa_pair_correspondences_workspace_bytes": (c_int64, [c_int64, c_int32, c_int32, c_int32, c_int32, c_uint32]),
    "mspa_pair_correspondences": (c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_uint32, c_void_p]),
    "mspa_compact_correspondences": (c_int, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "mspa_vertex_visibility": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int32, c_void_p,
                                       c_int32, c_int32, c_int32, c_int32,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mspa_vertex_visibility_ex": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int32, c_void_p, c_int32, c_void_p,
                                          c_int32, c_int32, c_int32, c_int32, c_double,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mspa_check_visibility_ex": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_int32, c_int32, c_int32, c_double,
                                         c_void_p, c_void_p, c_void_p, c_void_p]),
    "mspa_project_samples_ex": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int32, c_void_p, c_int32,
                                        c_int32, c_int32, c_int32, c_double, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                        c_void_p]),
    "mspa_pair_overlap": (c_int, [c_void_p, c_int32, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                  c_void_p]),
    "mspa_overlap_workspace_bytes": (c_int64, [c_int32, c_int32, c_int64]),
    "mspa_scene_overlap": (c_int, [c_void_p, c_int32, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mspa_overlap_matrix": (c_int, [c_void_p, c_int32, c_void_p, c_int32, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    "mspa_bits_popcount": (c_int, [c_void_p, c_int64, c_void_p, c_void_p]),
    "mspa_bits_expand": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "mspa_bits_transpose": (c_int, [c_void_p, c_int32, c_int64, c_void_p, c_void_p]),
    "mspa_format_int_lists_host": (c_int64, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    "mspa_format_token_lists_host": (c_int64, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_void_p, c_int64,
                                               c_void_p]),
    "mspa_format_int_keys_host": (c_int64, [c_char_p, c_int64, c_int64, c_void_p, c_int64, c_void_p]),
    "mspa_format_list_costs_device": (c_int, [c_void_p, c_int64, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "mspa_format_lists_device": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                         c_void_p, c_void_p]),
    "mspa_prep_labels": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_void_p]),
    "mspa_prep_align": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "mspa_prep_objects": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p,
                                  c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mspa_parse_int_list_host": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int32]),
    "mspa_parse_int_list_flags_device": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "mspa_parse_int_list_device": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                           c_void_p]),
    "mspa_gather_blocks_host": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int32]),
    "mspa_inflate_blocks_host": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int32]),
    "mspa_read_depth_png_host": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_int32, c_void_p]),
    "mspa_inflate_zlib_fast_host": (c_int, [c_void_p, c_int64, c_void_p, c_int64]),
    "mspa_png_header_host": (c_int, [c_char_p, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), POINTER(c_int32),
                                     POINTER(c_int32)]),
    "mspa_stream_create_reserving": (c_int, [c_int32, POINTER(c_void_p)]),
    "mspa_stream_destroy": (c_int, [c_void_p]),
    "mspa_inflate_blocks_device": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p,
                                           c_void_p, c_void_p]),
    "mspa_png_unfilter_device": (c_int, [c_void_p, c_int64, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "mspa_png_pack_idat_host": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                        POINTER(c_int64), c_int32]),
    "mspa_jpeg_parse_host": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "mspa_jpeg_workspace_bytes": (c_int64, [c_int64, c_int32, c_int32]),
    "mspa_jpeg_decode_device": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p,
                                        c_void_p, c_int64, c_void_p]),
    "mspa_jpeg_encode_capacity": (c_int64, [c_int32, c_int32, c_int32]),
    "mspa_jpeg_encode_workspace_bytes": (c_int64, [c_int64, c_int32, c_int32, c_int32]),
    "mspa_jpeg_encode_header_host": (c_int, [c_int32, c_int32, c_int32, c_int32, c_void_p, c_int64, POINTER(c_int64)]),
    "mspa_jpeg_encode_device": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int64, c_void_p, c_void_p,
                                        c_int64, c_void_p]),
    "mspa_png_encode_capacity": (c_int64, [c_int32, c_int32]),
    "mspa_png_encode_workspace_bytes": (c_int64, [c_int64, c_int32, c_int32]),
    "mspa_png_encode_device": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                                       c_void_p]),
    "mspa_resize_coeffs_host": (c_int, [c_int32, c_int32, c_int32, c_void_p, c_void_p, POINTER(c_int32)]),
    "mspa_resize_workspace_bytes": (c_int64, [c_int64, c_int32, c_int32, c_int32, c_int32]),
    "mspa_resize_rgb_device": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_int64, c_int64, c_void_p, c_int32, c_int32, c_int32,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "mspa_draw_spans_device": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int32, c_void_p]),
    "mspa_blend_masks_device": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int32, c_void_p]),
    "mspa_check_visibility": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                      c_void_p, c_void_p, c_void_p, c_void_p]),
    "mspa_pair_pose": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_void_p,
                               c_void_p]),
    "mspa_extract_yaw_pitch": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "mspa_track_to_world": (c_int, [c_void_p, c_void_p, c_int32, c_int32, POINTER(c_double), c_int32, c_int32,
                                    c_void_p, c_void_p, c_void_p, c_void_p]),
    "mspa_select_common_point": (c_int, [c_void_p, c_int32, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    "mspa_project_samples": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int32, c_void_p, c_int32,
                                     c_int32, c_int32, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                     c_void_p]),
    "mspa_object_extents": (c_int, [c_void_p, c_int32, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int32,
                                    c_void_p, c_void_p, c_void_p, c_void_p]),
    "mspa_track_pair_distances": (c_int, [c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                                          c_void_p, c_void_p, c_void_p]),
    "mspa_track_pair_stats": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_int32, c_double, c_double, c_void_p, c_void_p,
                                      c_void_p, c_void_p]),
    "mspa_track_pair_bin_counts": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_double, c_double, c_void_p,
                                           c_void_p]),
    "mspa_track_pair_sort": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_void_p]),
    "mspa_track_pair_order": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_int64, c_double,
                                      c_double, c_void_p, c_void_p, c_void_p]),
    "mspa_track_pair_resolve": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p,
                                        c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_double, c_double, c_void_p, c_void_p]),
    "mspa_track_rigidity_loss": (c_int, [c_void_p, c_int32, c_int32, c_double, c_void_p, c_void_p]),
    "mspa_track_rigidity_loss_batch": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_double, c_void_p, c_void_p]),
    "mspa_track_linkage_workspace_bytes": (c_int64, [c_int64, c_int32]),
    "mspa_track_linkage": (c_int, [c_void_p, c_int64, c_int32, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                   c_void_p]),
    "mspa_snappy_capacity": (c_int64, [c_int64]),
    "mspa_snappy_compress_host": (c_int64, [c_void_p, c_int64, c_void_p, c_int64]),
    "mspa_snappy_workspace_bytes": (c_int64, [c_int64]),
    "mspa_snappy_compress_device": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                                            c_void_p, c_void_p]),
    "mspa_snappy_compact_device": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                           c_int64, c_void_p, c_void_p]),
    "mspa_parquet_page_cuts_host": (c_int64, [c_void_p, c_int64, c_int64, c_void_p, c_int64]),
    "mspa_parquet_page_payload_bytes_host": (c_int64, [c_void_p, c_int64, c_int64]),
    "mspa_parquet_page_payload_host": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64]),
    "mspa_parquet_string_pages_device": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_void_p,
                                                 c_void_p, c_void_p]),
    "mspa_snappy_decompress_host": (c_int64, [c_void_p, c_int64, c_void_p, c_int64]),
    "mspa_snappy_decompress_device": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p,
                                              c_void_p, c_void_p]),
    "mspa_snappy_block_starts_host": (c_int64, [c_void_p, c_int64, c_int64, c_void_p, c_int64]),
    "mspa_snappy_blocks_workspace_bytes": (c_int64, [c_int64, c_int64, c_int64]),
    "mspa_snappy_block_starts_device": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64,
                                                c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "mspa_snappy_decompress_blocks_device": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p,
                                                     c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "mspa_parquet_plain_spans_device": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p,
                                                c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mspa_rle_hybrid_take_host": (c_int, [c_void_p, c_int64, c_int32, c_int64, c_void_p, c_int64, c_void_p]),
    "mspa_parquet_dict_spans_device": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p,
                                               c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                               c_void_p, c_void_p, c_void_p]),
    "mspa_index_rows_brackets_device": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mspa_index_rows_gather_device": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    "mspa_index_lists_to_bits_device": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    "mspa_index_lists_pick_device": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "mspa_rle_hybrid_runs_device": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64,
                                            c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mspa_rle_hybrid_expand_device": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    "mspa_parquet_double_layout_device": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "mspa_parquet_double_column_device": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                                  c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
                                                  c_void_p, c_void_p]),
    "mspa_pair_tile_rows": (c_int32, []),
    "mspa_pair_bin_codes_host": (c_int, [c_void_p, c_int64, c_void_p, c_int32, c_void_p, c_void_p]),
    "mspa_pair_bin_codes_device": (c_int, [c_void_p, c_int64, c_void_p, c_int32, c_void_p, c_void_p, c_int64, c_void_p]),
    "mspa_pair_partition_device": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    "mspa_track_displacement": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_int64,
                                        c_double, c_double, c_void_p, c_void_p, c_void_p]),
    "mspa_jpeg_decode_luma_device": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p,
                                             c_void_p, c_int64, c_void_p]),
    "mspa_laplacian_blocks": (c_int32, [c_int32, c_int32]),
    "mspa_laplacian_moments_device": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p]),
    "mspa_knn_grid_host": (c_int, [c_void_p, c_void_p, c_int64, c_int32, c_void_p]),
    "mspa_knn_workspace_bytes": (c_int64, [c_int64, c_int32]),
    "mspa_knn_cells_device": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "mspa_knn_mean_distance_device": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "mspa_knn_mean_distance_host": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_void_p]),
    "mspa_knn_segments_tables_host": (c_int, [c_void_p, c_int64, c_int32, c_void_p]),
    "mspa_knn_segments_grids_host": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p]),
    "mspa_knn_segments_workspace_bytes": (c_int64, [c_void_p, c_int64, c_int32]),
    "mspa_knn_segments_cells_device": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mspa_knn_segments_mean_distance_device": (c_int, [c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                       c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "mspa_outlier_segments_device": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_void_p]),
    "mspa_knn_segments_mean_distance_host": (c_int, [c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p]),
    "mspa_outlier_segments_host": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_void_p]),
    "mspa_png_pack_idat8_host": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                         POINTER(c_int64), c_int32]),
    "mspa_png_unfilter8_device": (c_int, [c_void_p, c_int64, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "mspa_png_unfilter8_host": (c_int, [c_void_p, c_int64, c_int64, c_int32, c_int32, c_void_p, c_void_p]),
    "mspa_instance_split_workspace_bytes": (c_int64, [c_int64, c_int64]),
    "mspa_instance_split_count": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
    "mspa_instance_split_scatter": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32, c_void_p, c_void_p,
                                            c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mspa_instance_split_host": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_int32]),
    "mspa_voxel_segments_tables_host": (c_int, [c_void_p, c_int64, c_void_p]),
    "mspa_voxel_segments_workspace_bytes": (c_int64, [c_void_p, c_int64]),
    "mspa_voxel_segments_keys_device": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                c_void_p, c_int64, c_void_p]),
    "mspa_voxel_segments_heads_device": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "mspa_voxel_segments_means_device": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                                 c_int64, c_void_p]),
    "mspa_voxel_segments_host": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_double, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mspa_dbscan_cell_side": (c_double, [c_double]),
    "mspa_dbscan_segments_workspace_bytes": (c_int64, [c_void_p, c_int64]),
    "mspa_dbscan_segments_device": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_double, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "mspa_dbscan_segments_host": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_double, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_void_p]),
    "mspa_upright_filter_workspace_bytes": (c_int64, [c_void_p, c_int64]),
    "mspa_upright_filter_device": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_int64, c_void_p]),
    "mspa_upright_hull_device": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mspa_upright_boxes_workspace_bytes": (c_int64, [c_void_p, c_int64]),
    "mspa_upright_boxes_device": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "mspa_upright_segments_host": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mspa_upright_iou_device": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int32, c_void_p, c_void_p, c_void_p]),
    "mspa_upright_iou_host": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int32, c_void_p, c_void_p]),
    "mspa_upright_iou_bound_host": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "mspa_knn_segments_index_device": (c_int, [c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                               c_void_p, c_void_p, c_int64, c_void_p]),
    "mspa_cloud_distance_device": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                           c_double, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mspa_cloud_distance_keys_device": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                                c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mspa_cloud_distance_fit_device": (c_int, [c_void_p, c_void_p, c_int64, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                               c_void_p, c_void_p]),
    "mspa_cloud_distance_host": (c_int, [c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_double,
                                         c_void_p, c_void_p, c_void_p]),
    "mspa_cloud_distance_fit_host": (c_int, [c_void_p, c_void_p, c_int64, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mspa_cloud_align_transform_device": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                                  c_void_p, c_void_p, c_void_p]),
    "mspa_cloud_align_fit_device": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p,
                                            c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_void_p]),
    "mspa_cloud_align_transform_host": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "mspa_cloud_align_fit_host": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                          c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mspa_cloud_normals_device": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mspa_cloud_normals_host": (c_int, [c_void_p, c_void_p, c_int64, c_int32, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_void_p]),
    "mspa_cloud_align_plane_fit_device": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64,
                                                  c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                  c_void_p, c_void_p]),
    "mspa_cloud_align_plane_fit_host": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p,
                                                c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
}


def load() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"libmspa.so not found at {LIB_PATH}. Build it with `python __graft_entry__.py build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for the geometry kernels.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in _SIGNATURES.items():
        fn = getattr(lib, name)        # AttributeError here = header and library out of sync
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def exported_symbols():
    return list(_SIGNATURES.keys())


def check(rc: int):
    if rc != MSPA_OK:
        msg = load().mspa_last_error_string()
        raise MspaError(rc, msg.decode() if msg else "unknown")


def version() -> int:
    return load().mspa_version()


def device_info(device: int = 0) -> dict:
    n_cu, wave, clock = c_int(0), c_int(0), c_int(0)
    hbm = c_int64(0)
    name = ctypes.create_string_buffer(64)
    check(load().mspa_device_info(device, ctypes.byref(n_cu), ctypes.byref(wave), ctypes.byref(hbm),
                                  ctypes.byref(clock), name, 64))
    return {"name": name.value.decode(), "n_cu": n_cu.value, "wave_size": wave.value,
            "hbm_bytes": hbm.value, "clock_khz": clock.value}


_OWN_STREAMS: dict = {}
_OWN_STREAMS_LOCK = __import__("threading").Lock()


def own_stream(role: str, device):
    """A HIP stream of this process's OWN for a long-lived role (a decode slot, the sweeps' copy stream, an encoder thread's side
    stream), created once per (role, device) through mspa_stream_create_reserving(0) and kept: ``torch.cuda.ExternalStream``.

    ``torch.cuda.Stream()`` is not that: it hands out the next of a pool of 32 streams per device, round robin.  A process that
    sweeps more than once asks for 1 + 8 streams per pass (copy stream, encoder threads) on top of its 8 decode slots -- from the
    third pass on an encoder thread's "own" stream IS a decode slot's stream, its downloads queue behind a 40 ms inflate and the
    slot's next scene behind them (the fourth pass of every multi-pass measurement was the slow one: profiles/r06_sweep_timeline.md)."""
    import torch
    device = torch.device(device)
    index = device.index if device.index is not None else torch.cuda.current_device()
    key = (role, index)
    with _OWN_STREAMS_LOCK:
        st = _OWN_STREAMS.get(key)
        if st is None:
            ptr = ctypes.c_void_p(0)
            with torch.cuda.device(index):
                check(load().mspa_stream_create_reserving(0, ctypes.byref(ptr)))
            st = _OWN_STREAMS[key] = torch.cuda.ExternalStream(ptr.value, device=torch.device("cuda", index))
        return st
