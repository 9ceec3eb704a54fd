/*
 * mspa.h -- C ABI of libmspa.so, the MI355X (gfx950) geometry engine behind the MultiSPA
 * data pipeline of facebookresearch/Multi-SpatialMLLM.
 *
 * The reference is pure Python and has no FFI of its own: its hot path sits behind plain Python
 * callables.  Each entry point below names the reference callable(s) it
 * replaces (paths relative to the reference tree; IH = spatial_engine/utils/scannet_utils/
 * handler/info_handler.py, OPS = .../handler/ops.py, CFR = spatial_engine/camera_movement/
 * calculate_frames_relations.py, MVI = spatial_engine/utils/scannet_utils/make_visibility_info.py,
 * CME = spatial_engine/camera_movement/camera_movement_engine_train_val.py, OM_C =
 * spatial_engine/object_movement/single_object_movement_engine_coord.py).  The ctypes binding a
 * maintainer would add on the reference side is shown in INTEGRATION.md.
 *
 * Conventions
 *  - Every pointer is a DEVICE pointer (HBM) unless the name ends in _host.  The library never
 *    allocates, frees or copies user buffers: the caller (PyTorch-ROCm tensors in the shipped host
 *    layer) owns all memory and passes data_ptr() values plus element counts.
 *  - `stream` is a hipStream_t (NULL = the default stream).  Calls enqueue work and return; they
 *    never synchronise.  Entry points are re-entrant; there is no global mutable state besides the
 *    thread-local error string.
 *  - Matrices are 4x4, row-major, float64, affine (last row exactly 0 0 0 1; the host layer
 *    verifies this and the finiteness of every entry, as the reference's pose-validity filter
 *    IH:409-418 does, before calling).  Inverses are computed by the caller with the same LAPACK
 *    routine the reference uses (numpy.linalg.inv) and passed in ready-made.
 *  - All arithmetic is IEEE float64 in the reference's operation order (each matrix row is the
 *    chain m0*x, fma(m1,y,.), fma(m2,z,.), +m3 -- what NumPy/OpenBLAS computes for K = 4), so
 *    integer outputs and masks are bit-exact and float64 outputs are bit-identical to the C oracle.
 *  - Return value: MSPA_OK or a negative MSPA_E* code; mspa_last_error_string() describes the
 *    last failure on the calling thread.  Nothing throws or aborts.
 */
#ifndef MSPA_H
#define MSPA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSPA_VERSION 260            /* 0.16.0: per-object clouds from instance masks on the device: 8-bit greyscale PNG decode (mspa_png_pack_idat8_host, mspa_png_unfilter8_device / _host) and the stable split by label (mspa_instance_split_count / _scatter); 0.15.0: pair mining of the object-movement head on the device (mspa_track_pair_stats / _bin_counts / _sort / _order / _resolve); 0.14.0: handler ops on the device: grey decode and Laplacian moments (mspa_jpeg_decode_luma_device, mspa_laplacian_moments_device), exact k-nearest mean distance (mspa_knn_*); 0.13.0: parquet data pages of the visibility index on the device (mspa_snappy_*, mspa_parquet_*); 0.12.0: rigid-body track grouping on the device (mspa_track_linkage, mspa_track_rigidity_loss_batch); 0.11.0: image resizing on the device (mspa_resize_coeffs_host, mspa_resize_rgb_device); 0.10.0: ScanNet instance data from raw scans (mspa_prep_labels / _align / _objects, mspa_parse_int_list_*); 0.9.0: depth-PNG writes on the device (mspa_png_encode_device); 0.8.0: annotated-image writes on the device (mspa_jpeg_encode_device, mspa_draw_spans_device,
                                       mspa_blend_masks_device); 0.7.0: colour-frame (baseline JPEG) decode on the device (mspa_jpeg_parse_host, mspa_jpeg_decode_device);
                                       0.6.0: depth-frame decode on the device (mspa_inflate_blocks_device, mspa_png_unfilter_device); 0.5.0: host-side depth-PNG ingest (mspa_read_depth_png_host); 0.4.0: frame records carry
                                       guard-bound coefficients (slot MSPA_MAT_BOUNDS, MSPA_FRAME_MATS 7 -> 8) */

#define MSPA_OK 0
#define MSPA_EINVAL (-1)            /* bad argument (null pointer, size out of range, ...) */
#define MSPA_EHIP (-2)              /* a HIP runtime call failed; see mspa_last_error_string() */
#define MSPA_EUNSUPPORTED (-3)      /* valid request this build has no kernel for */

typedef void *mspa_stream_t;        /* hipStream_t */

/* Matrix slots of one frame record in `frame_mats` ([n_frames][MSPA_FRAME_MATS][16] float64). */
#define MSPA_MAT_KINV 0             /* inv(K)            OPS:313 */
#define MSPA_MAT_E 1                /* E, camera->world  OPS:316 */
#define MSPA_MAT_A 2                /* A, world->aligned OPS:319-320 (identity when absent) */
#define MSPA_MAT_EINV_ALIGNED 3     /* inv(A @ E)        IH:113-124, IH:57 */
#define MSPA_MAT_K 4                /* K                 IH:66 */
#define MSPA_MAT_UNPROJ 5           /* A @ E @ inv(K)    composed on the host (fast path only) */
#define MSPA_MAT_REPROJ 6           /* K @ inv(A @ E)    composed on the host (fast path only) */
#define MSPA_MAT_BOUNDS 7           /* not a matrix: the frame's guard-bound coefficients (fast path only), filled by
                                       mspa_frame_bounds_host from slots 0-4.  With |.| entrywise, Uabs = |A| |E| |inv(K)|,
                                       Nabs = |K| |inv(A @ E)| and c = MSPA_GUARD_C * 2^-53:
                                         [0..2]  max over rows r < 3 of Uabs[r][j], j = 0, 1, 2      [3]  1000 * max_r Uabs[r][3]
                                         [4..6]  c * (Nabs[k][0] + Nabs[k][1] + Nabs[k][2]), k = 0, 1, 2
                                         [8..10] c * 1000 * Nabs[k][3]                              (other entries 0)
                                       For a pixel block with columns <= X, rows <= Y and depth samples <= D millimetres,
                                       w = D * ([0] X + [1] Y + [2]) + [3] bounds the aligned-world coordinates (mm) and
                                       B_k = [4 + k] * w + [8 + k] bounds the difference between ANY two float64 evaluation
                                       orders of the k-th homogeneous image coordinate (pixel * millimetre; k = 2: the
                                       camera-2 depth in mm) -- the reference's five products vs the composed 3x4 of the
                                       fast kernels.  The guard band of MSPA_PAIR_FAST is derived from B_k per tile. */
#define MSPA_FRAME_MATS 8
#define MSPA_GUARD_C 256.0          /* >= the roundings of either evaluation order (89 counted) */

/* Slots of one image record in `cam_mats` ([n_images][MSPA_CAM_MATS][16] float64) of K1 / K6b. */
#define MSPA_CAM_EINV 0             /* inv(A @ E)        IH:57 */
#define MSPA_CAM_K 1                /* K                 IH:66 */
#define MSPA_CAM_BOUNDS 2           /* not a matrix: guard-bound coefficients of the composed K1 kernels, filled by
                                       mspa_camera_bounds_host from slots 0-1.  Nabs = |K| |inv(A @ E)|, c = MSPA_GUARD_C * 2^-53 * 1000:
                                         [0] c (nr_0 + nr_1)   [1] c nr_2   [2] c (Nabs[0][3] + Nabs[1][3])   [3] c Nabs[2][3]
                                       with nr_k = Nabs[k][0] + Nabs[k][1] + Nabs[k][2] (other entries 0).  For a vertex with
                                       s = |x| + |y| + |z| (metres), [0] s + [2] bounds the difference between any two float64
                                       evaluation orders of the homogeneous image x and y (summed; pixel * millimetre) and
                                       [1] s + [3] that of the camera depth (millimetres). */
#define MSPA_CAM_MATS 3

/* flags of mspa_pair_reproject */
#define MSPA_PAIR_FAST 1u           /* composed-matrix evaluation with exact re-evaluation of every
                                       lane near a decision boundary: masks, pixel indices and counters
                                       stay bit-exact, float32 points agree to ~1e-12 relative.  Needs
                                       slots 5-7 filled and K's third row == 0 0 1 0 (pinhole); ignored
                                       (the exact kernel runs) when any float64 output is requested.  A bitset
                                       output on a width that is not a multiple of 64 takes a linear pixel mapping
                                       (64 consecutive pixel indices per wave) so that ballots stay whole words. */
#define MSPA_PAIR_STREAM 2u         /* caller's hint: the frames of this launch are (mostly) not revisited by other pairs of
                                       the same launch -- frame 1 is read with the non-temporal hint so that it does not
                                       displace frame-2 lines that ARE revisited (gathers).  Results are identical with or
                                       without it; measured +3 % with distinct frames, -10 % when 48 frames serve 1000 pairs */

#define MSPA_PAIR_WORD_STRIPES 0x200u /* retired: accepted and ignored, the kernel it selected was removed (rounds 2-3's word-stripe
                                       kernel for ScanNet's shape; the rectangular-tile kernel has been the default there since
                                       round 4).  A call does exactly what it does without the bit. */

int mspa_version(void);
const char *mspa_last_error_string(void);

/*
 * Host-side: fills slot MSPA_MAT_BOUNDS of n_frames frame records from their slots 0-4 (HOST pointer to the
 * [n_frames, MSPA_FRAME_MATS, 16] table, before it is uploaded).  The shipped host layer computes the same numbers in NumPy
 * (mspa.engine.frame_bounds); a C caller that builds its own table calls this once per table.
 */
int mspa_frame_bounds_host(double *frame_mats_host, int32_t n_frames);
/* The same for K1's image records: fills slot MSPA_CAM_BOUNDS of [n_images, MSPA_CAM_MATS, 16] from slots 0-1 (HOST pointer). */
int mspa_camera_bounds_host(double *cam_mats_host, int32_t n_images);

/* Device facts the host layer reports next to measurements.  Any out pointer may be NULL. */
int mspa_device_info(int device, int *n_cu, int *wave_size, int64_t *hbm_bytes, int *clock_khz,
                     char *name_host, int name_len);

/*
 * K3 -- the frame-pair pipe (BASELINE.json north_star).  For every pair (f1, f2) and every colour
 * pixel (mx, my) of frame f1:
 *   project_mask_to_3d          OPS:235-329   depth -> camera -> world -> aligned point
 *   project_3d_point_to_image   IH:313-335, project_points IH:46-72   into frame f2
 *   check_point_visibility      IH:337-386    bounds + strict depth-buffer test in frame f2
 *
 *   depth       [n_frames, dh, dw] uint16 millimetres
 *   rgb         [n_frames, H, W, 3] uint8 or NULL (needed only for out_rgba)
 *   frame_mats  [n_frames, MSPA_FRAME_MATS, 16] float64
 *   pairs       [n_pairs, 2] int32 frame indices (f1, f2)
 * Outputs, each optional (NULL = not produced), P = H*W pixels in row-major order:
 *   out_vis_bits  [n_pairs, ceil(P/64)] uint64   bit (i & 63) of word (i >> 6) = pixel i visible
 *   out_vis_u8    [n_pairs, P] uint8             1 = visible in f2, 0 otherwise
 *   out_valid_u8  [n_pairs, P] uint8             1 = depth sample of f1 > 0 (OPS:297)
 *   out_pix_i16   [n_pairs, P, 2] int16          depth-pixel index (xi, yi) in f2 (IH:362-366) where the
 *                                                point lands inside f2 in front of its camera (the
 *                                                candidate correspondence); (-1,-1) otherwise
 *   out_xyz_f32   [n_pairs, P, 3] float32        aligned world point, NaN where invalid
 *   out_rgba      [n_pairs, P] uint32            r | g<<8 | b<<16 | (valid ? 255 : 0)<<24
 *   out_xyz_f64   [n_pairs, P, 3], out_uv_f64 [n_pairs, P, 2], out_depth_f64 [n_pairs, P]
 *                                                full-precision point, un-rounded (u, v) in f2
 *                                                and camera-2 depth; NaN where invalid
 *   out_counts    [n_pairs, 2] int32             (#valid, #visible); zeroed by the call
 * Requires 2 <= dw,dh,W,H <= 32767 and H*W*W < 2^32.
 * Alignment: out_pix_i16 must be 4-byte aligned (MSPA_EINVAL otherwise): every kernel stores an (xi, yi) pair as one 32-bit
 * word.  Every other pointer needs its element's alignment only (rgb: any; the whole-tile kernel reads a row's colour bytes
 * as one 32-bit word per pixel at byte 3 x - 1 of the row, at every residue mod 4 wherever rgb starts, and never in front of
 * it).  The whole-tile and rectangular-tile kernels (MSPA_KERNEL_PAIR_FAST_TIGHT / _RECT) additionally want depth and
 * out_vis_u8 4-byte, out_vis_bits 8-byte and out_pix_i16, out_xyz_f32 and out_rgba 16-byte aligned; a launch with one of them
 * elsewhere takes the general kernel of its mode.
 */
int mspa_pair_reproject(const uint16_t *depth, const uint8_t *rgb, const double *frame_mats,
                        int32_t n_frames, const int32_t *pairs, int64_t n_pairs,
                        int32_t dh, int32_t dw, int32_t H, int32_t W,
                        uint64_t *out_vis_bits, uint8_t *out_vis_u8, uint8_t *out_valid_u8,
                        int16_t *out_pix_i16, float *out_xyz_f32, uint32_t *out_rgba,
                        double *out_xyz_f64, double *out_uv_f64, double *out_depth_f64,
                        int32_t *out_counts, uint32_t flags, mspa_stream_t stream);

/* Which kernel the most recent mspa_pair_reproject call OF THE CALLING THREAD enqueued (a diagnostic the parity tests
 * use to prove that the instantiation they mean to check is the one that ran; no effect on results). */
#define MSPA_KERNEL_NONE 0
#define MSPA_KERNEL_PAIR_EXACT 1          /* reference operation order */
#define MSPA_KERNEL_PAIR_FAST 2           /* composed + guarded, any shape, stripe mapping */
#define MSPA_KERNEL_PAIR_FAST_LINEAR 3    /* the same with the linear pixel mapping (bitset, W % 64 != 0) */
#define MSPA_KERNEL_PAIR_FAST_TIGHT 4     /* whole-tile images (W % 64 == 0, H % 48 == 0, colour == depth grid), output set
                                             corr / dense / dense without colour / minimal / compact */
#define MSPA_KERNEL_PAIR_FAST_SCALED 5    /* retired id, never returned: rounds 2-3's word-stripe kernel for ScanNet's shape was removed
                                             (the ids are not renumbered) */
#define MSPA_KERNEL_PAIR_FAST_RECT 6      /* the tight kernel on rectangular tiles of a colour / depth grid pair with dw <= W, dh <= H,
                                             W % 16 == 0, H % 4 == 0, dw % 4 == 0, dh % 2 == 0, H * W * 4 < 2^31 and
                                             dh * dw * 2 < 2^31 that is not a whole-tile shape (ScanNet's shape included):
                                             correspondence / minimal / compacted sets */
int mspa_pair_reproject_last_kernel(void);

/*
 * K3, compacted correspondence output -- "overlap + correspondence extraction" of the frame-pair pipe without the dense
 * [P, 2] table, three quarters of which is (-1, -1) fill on overlap-sampled pairs: per pair the visibility bitset and, per
 * 64 x 48-pixel tile of frame f1, the (xi, yi) of its VISIBLE pixels only.
 *
 *   Tiles: n_stripes = ceil(W / 64) across, ceil(H / 48) down, tile t = band * n_stripes + stripe (ragged at the right /
 *   bottom edge); mspa_corr_tiles(H, W) returns their number.
 *   out_vis_bits     [n_pairs, ceil(P/64)] uint64   as in mspa_pair_reproject
 *   out_cpix_i16     [n_pairs, n_tiles, MSPA_CORR_TILE_CAP, 2] int16   tile t's segment holds, for its visible pixels in
 *                    (row, column) order, the depth-pixel index (xi, yi) in f2 (IH:362-366) -- the k-th set bit of the
 *                    tile's part of the bitset <-> entry k; entries beyond the tile's count are unspecified (the fused
 *                    kernel writes 4 bytes per VISIBLE pixel and nothing else; only a tile in which the exact re-evaluation
 *                    of a guarded pixel took a pixel OUT of the visible set may keep stale entries behind its count)
 *   out_tile_counts  [n_pairs, n_tiles] int32       visible pixels per tile (= entries of its segment)
 *   out_counts       [n_pairs, 2] int32 or NULL     (#valid, #visible); zeroed by the call
 * With MSPA_PAIR_FAST on a whole-tile shape (W % 64 == 0, H % 48 == 0, colour grid == depth grid: BASELINE's 640x480) and on
 * every shape with dw <= W, dh <= H, W % 16 == 0, H % 4 == 0, dw % 4 == 0, dh % 2 == 0, H * W * 4 < 2^31 and dh * dw * 2 < 2^31
 * (the predicate of MSPA_KERNEL_PAIR_FAST_RECT: ScanNet's own 1296x968 colour over 640x480 depth; ragged tiles hold fewer
 * pixels, same indexing) one fused kernel produces all of it -- mspa_pair_correspondences_workspace_bytes() is the authority
 * on which shapes those are (it returns 0 for them); every other shape / mode runs mspa_pair_reproject into a dense table in
 * `workspace` (caller-owned, 16-byte aligned, at least mspa_pair_correspondences_workspace_bytes(...) bytes; NULL / 0 when
 * that returns 0) and compacts it with mspa_compact_correspondences.  Identical results either way (bit-exact integers).
 * out_cpix_i16 must be 16-byte aligned.  MSPA_PAIR_STREAM as in mspa_pair_reproject.  The fused kernel additionally needs
 * `depth` 4-byte aligned (any allocator's base address is): a table at an odd 2-byte offset takes the dense route as well,
 * i.e. needs the workspace although mspa_pair_correspondences_workspace_bytes, which cannot see the pointer, returned 0
 * (the error string says so).  Depth samples are millimetres here and in mspa_pair_reproject (project_mask_to_3d's literal
 * 0.001, OPS:292-294): a handler's depth_value_scale applies to K1 / K6b / the predicates only.
 */
#define MSPA_CORR_TILE_W 64
#define MSPA_CORR_TILE_H 48
#define MSPA_CORR_TILE_CAP (MSPA_CORR_TILE_W * MSPA_CORR_TILE_H)
int64_t mspa_corr_tiles(int32_t H, int32_t W);
int64_t mspa_pair_correspondences_workspace_bytes(int64_t n_pairs, int32_t dh, int32_t dw, int32_t H, int32_t W,
                                                  uint32_t flags);
int mspa_pair_correspondences(const uint16_t *depth, const double *frame_mats, int32_t n_frames,
                              const int32_t *pairs, int64_t n_pairs, int32_t dh, int32_t dw, int32_t H, int32_t W,
                              uint64_t *out_vis_bits, int16_t *out_cpix_i16, int32_t *out_tile_counts,
                              int32_t *out_counts, void *workspace, int64_t workspace_bytes, uint32_t flags,
                              mspa_stream_t stream);
/* The compaction step on its own: (vis_bits, dense pix_i16 [n_pairs, P, 2]) of mspa_pair_reproject -> segments + counts.
 * pix_i16 and out_cpix_i16 must be 4-byte aligned (MSPA_EINVAL otherwise): an (xi, yi) pair moves as one 32-bit word. */
int mspa_compact_correspondences(const uint64_t *vis_bits, const int16_t *pix_i16, int64_t n_pairs, int32_t H, int32_t W,
                                 int16_t *out_cpix_i16, int32_t *out_tile_counts, mspa_stream_t stream);

/*
 * K1 -- vertex visibility, HOT LOOP 1 of CFR.process_scene (CFR:152-164) and
 * MVI.process_scene (MVI:93-100): project_3d_point_to_image (IH:313-335) + check_point_visibility
 * (IH:375-386) of all scene vertices into a batch of images.
 *
 *   xyz         vertex coordinates, element (i, c) at xyz[i*point_stride + c*comp_stride]
 *               ([N,3] rows: 3,1;  aligned_points.npy [N,6] rows: 6,1;  SoA [3,N]: 1,N)
 *   cam_mats    [n_images, MSPA_CAM_MATS, 16] float64: inv(A @ E), K, guard-bound coefficients (mspa_camera_bounds_host), per image
 *   depth       [n_images, dh, dw] uint16
 * Outputs, each optional:
 *   out_bits    [n_images, ceil(n_points/64)] uint64  visibility bitset (tail bits zero)
 *   out_mask    [n_images, n_points] uint8
 *   out_uv      [n_images, n_points, 2] float64        un-rounded projection (IH:72)
 *   out_depth   [n_images, n_points] float64           signed camera depth (IH:63)
 *   out_count   [n_images] int32                       visible vertices per image; zeroed by the call
 */
int mspa_vertex_visibility(const double *xyz, int64_t n_points, int64_t point_stride,
                           int64_t comp_stride, const double *cam_mats, int32_t n_images,
                           const uint16_t *depth, int32_t dh, int32_t dw, int32_t H, int32_t W,
                           uint64_t *out_bits, uint8_t *out_mask, double *out_uv, double *out_depth,
                           int32_t *out_count, mspa_stream_t stream);

/*
 * The same with the two parameters the reference's interface leaves open:
 *   homogeneous != 0   the points are general homogeneous rows (x, y, z, w), the fourth coordinate at
 *                      xyz[i*point_stride + 3*comp_stride] -- project_points (IH:46-72) takes any [N, 4] array; both 4x4
 *                      products are then evaluated in full (w == 1 gives the bits of the affine form)
 *   depth_value_scale  metres per depth-image unit (SceneInfoHandler(depth_value_scale=...), IH:76, applied at IH:368);
 *                      0.001 in mspa_vertex_visibility.  Positive and finite.
 * Either one selects the reference-order kernel (the composed kernels fold w == 1 and the millimetre in).
 */
int mspa_vertex_visibility_ex(const double *xyz, int64_t n_points, int64_t point_stride, int64_t comp_stride,
                              int32_t homogeneous, const double *cam_mats, int32_t n_images, const uint16_t *depth,
                              int32_t dh, int32_t dw, int32_t H, int32_t W, double depth_value_scale,
                              uint64_t *out_bits, uint8_t *out_mask, double *out_uv, double *out_depth,
                              int32_t *out_count, mspa_stream_t stream);

/*
 * The three predicates of the reference on already-projected points, for callers that hold (uv, depth)
 * from an earlier projection: check_point_in_image_boundary (IH:337-344),
 * check_point_visibility_by_depth (IH:346-373), check_point_visibility (IH:375-386).
 *   uv [n, 2] f64, point_depth [n] f64, depth_image [dh, dw] u16 (may be NULL for the bounds test alone)
 *   out_in_bounds / out_by_depth / out_visible [n] u8, each optional
 */
int mspa_check_visibility(const double *uv, const double *point_depth, int64_t n,
                          const uint16_t *depth_image, int32_t dh, int32_t dw, int32_t H, int32_t W,
                          uint8_t *out_in_bounds, uint8_t *out_by_depth, uint8_t *out_visible,
                          mspa_stream_t stream);
/* ... with the handler's depth_value_scale (IH:368) instead of the default 0.001 */
int mspa_check_visibility_ex(const double *uv, const double *point_depth, int64_t n,
                             const uint16_t *depth_image, int32_t dh, int32_t dw, int32_t H, int32_t W,
                             double depth_value_scale, uint8_t *out_in_bounds, uint8_t *out_by_depth,
                             uint8_t *out_visible, mspa_stream_t stream);

/*
 * K2 -- pair overlap, HOT LOOP 2 of CFR.process_scene: calculate_camera_overlap (CFR:102-137)
 * on K1's bitsets.  overlap = |a & b| / |a | b| * 100 in float64 (NaN for an empty union).
 *
 *   bits        [n_images, n_words] uint64
 *   pairs       [n_pairs, 2] int32 image indices
 *   out_overlap [n_pairs] float64;  out_inter / out_union [n_pairs] int32, optional
 */
int mspa_pair_overlap(const uint64_t *bits, int32_t n_images, int64_t n_words, const int32_t *pairs,
                      int64_t n_pairs, double *out_overlap, int32_t *out_inter, int32_t *out_union,
                      mspa_stream_t stream);

/*
 * K2, tiled forms.  The reference visits every pair of a scene (CFR:176-189: F(F-1)/2 calls of
 * calculate_camera_overlap) and, for object visibility, every (object, image) combination
 * (compute_object_visibility.py:72-152).  These two entry points do a whole scene / rectangle in one pass: 32 x 32
 * blocks of rows, bitset chunks staged in LDS, only |a & b| counted (|a | b| = |a| + |b| - |a & b|).  Results are
 * identical to mspa_pair_overlap's.  `workspace` is caller-owned scratch of at least
 * mspa_overlap_workspace_bytes(n_a, n_b, n_words) bytes (4-byte aligned); its contents are undefined afterwards.
 *
 * mspa_scene_overlap: all pairs i < j of one scene in the reference's nested-loop order (CFR:176-178),
 *   out_overlap [F(F-1)/2] float64 (NaN for an empty union, CFR:136), out_inter / out_union [F(F-1)/2] int32 optional.
 * mspa_overlap_matrix: out_inter [n_a, n_b] int32 = |a_i & b_j| (bits_a == bits_b with n_a == n_b is recognised as
 *   symmetric: half the blocks are computed, the matrix is returned full; its diagonal holds the row popcounts).
 */
int64_t mspa_overlap_workspace_bytes(int32_t n_a, int32_t n_b, int64_t n_words);
int mspa_scene_overlap(const uint64_t *bits, int32_t n_images, int64_t n_words, void *workspace,
                       int64_t workspace_bytes, double *out_overlap, int32_t *out_inter, int32_t *out_union,
                       mspa_stream_t stream);
int mspa_overlap_matrix(const uint64_t *bits_a, int32_t n_a, const uint64_t *bits_b, int32_t n_b, int64_t n_words,
                        void *workspace, int64_t workspace_bytes, int32_t *out_inter, mspa_stream_t stream);

/*
 * K9 -- visibility bitsets -> index lists on the device: what MVI.process_scene (make_visibility_info.py:103-118) builds as
 * Python lists -- np.where(mask)[0].tolist() per image, and per vertex the sorted ids of the images that see it -- as CSR
 * tables.  The second table is the compaction of the TRANSPOSED bit matrix.
 *   mspa_bits_popcount   out_counts[i] = popcount(bits[i]) over a flat table of n_words_total words
 *   mspa_bits_expand     bits [n_rows, n_words]; word_offsets [n_rows * n_words] int64 = exclusive prefix sum of the
 *                        popcounts (row r's list starts at word_offsets[r * n_words]); out_indices[k] int32 = position of
 *                        the k-th set bit WITHIN ITS ROW, rows back to back, ascending within a row
 *   mspa_bits_transpose  bits [n_rows, n_words] -> out [n_words * 64, ceil(n_rows / 64)]: bit (r & 63) of
 *                        out[c, r >> 6] = bit (c & 63) of bits[r, c >> 6]; padding bits are zero
 */
int mspa_bits_popcount(const uint64_t *bits, int64_t n_words_total, int32_t *out_counts, mspa_stream_t stream);
int mspa_bits_expand(const uint64_t *bits, int64_t n_rows, int64_t n_words, const int64_t *word_offsets,
                     int32_t *out_indices, mspa_stream_t stream);
int mspa_bits_transpose(const uint64_t *bits, int32_t n_rows, int64_t n_words, uint64_t *out, mspa_stream_t stream);

/*
 * Host-side text formatting of index columns (HOST pointers).  The visibility parquet stores each list as its JSON text
 * (json.dumps form: "[1, 2, 3]", "[\"00000\", \"00005\"]", "[]"; make_visibility_info.py:38-73) under keys
 * "scene:point_to_images:idx"; these write that text straight into arrow's string layout (int32 offsets + UTF-8 data) from
 * the CSR tables K9 produces.  Each returns the number of bytes written (>= 0) or a negative MSPA_E* code;
 * out_text_offsets_host has n + 1 entries.  A buffer of 2 + 13 * len bytes per integer list, 2 + (longest token + 2) * len
 * per token list and strlen(prefix) + 21 per key is always large enough.
 *   mspa_format_int_lists_host    list k = values[offsets[k] .. offsets[k+1])
 *   mspa_format_token_lists_host  list k = tokens named by token_ids[offsets[k] .. offsets[k+1]); token t is the text
 *                                 tokens[token_offsets[t] .. token_offsets[t+1]) (e.g. an already quoted image id)
 *   mspa_format_int_keys_host     key k = prefix followed by the decimal text of first + k
 */
int64_t mspa_format_int_lists_host(const int64_t *offsets_host, const int32_t *values_host, int64_t n_lists,
                                   char *out_text_host, int64_t capacity, int32_t *out_text_offsets_host);
int64_t mspa_format_token_lists_host(const int64_t *offsets_host, const int32_t *token_ids_host, int64_t n_lists,
                                     const char *tokens_host, const int32_t *token_offsets_host, int32_t n_tokens,
                                     char *out_text_host, int64_t capacity, int32_t *out_text_offsets_host);
int64_t mspa_format_int_keys_host(const char *prefix_host, int64_t first, int64_t n, char *out_text_host,
                                  int64_t capacity, int32_t *out_text_offsets_host);

/*
 * The same text written ON the device (round 6, K10: csrc/format_lists.hip) -- every list item formatted by its own lane at its
 * final byte position -- for the visibility-index sweep, whose encoder threads spent half of their time per scene in the host
 * loops above (make_visibility_info.py:38-73: json.dumps per key).  DEVICE pointers; two launches around two prefix sums
 * that are the caller's plumbing (as for mspa_bits_popcount -> prefix sum -> mspa_bits_expand):
 *   mspa_format_list_costs_device  out_cost[e] = bytes of item e's text + 2.  token_offsets_dev NULL: items are integers
 *                                  (decimal, '-' for negatives); else item e is token values[e] of n_tokens tokens
 *                                  (token t = tokens[token_offsets[t] .. token_offsets[t+1])); an id outside sets *bad_flag_dev
 *   mspa_format_lists_device       cost_prefix_dev: exclusive prefix sum of out_cost as int64, nnz + 1 entries;
 *                                  nonempty_prefix_dev[r]: lists q < r with offsets[q+1] > offsets[q], n_lists + 1 int64 entries;
 *                                  text_bytes = 2 n_lists + cost_prefix[nnz] - 2 nonempty_prefix[n_lists] (< 2 GiB);
 *                                  writes the text and arrow's int32 string offsets (n_lists + 1 entries).
 * Bit-exact with the host formatters (and json.dumps).
 */
int mspa_format_list_costs_device(const int32_t *values_dev, int64_t nnz, const int32_t *token_offsets_dev, int32_t n_tokens,
                                  int32_t *out_cost_dev, int32_t *bad_flag_dev, mspa_stream_t stream);
int mspa_format_lists_device(const int64_t *offsets_dev, const int32_t *values_dev, int64_t n_lists, int64_t nnz,
                             const int64_t *cost_prefix_dev, const int64_t *nonempty_prefix_dev, const char *tokens_dev,
                             const int32_t *token_offsets_dev, char *out_text_dev, int64_t text_bytes,
                             int32_t *out_text_offsets_dev, mspa_stream_t stream);

/*
 * K11 -- ScanNet instance data from raw scans (batch_load_scannet_data.py export(), scannet_utils.py extract_bbox), batched:
 * one launch serves n_scenes scenes whose vertices lie back to back.  DEVICE pointers.  Offset tables shared by the three calls
 * (int64, n_scenes + 1 entries each): vert_off = prefix sum of the scenes' vertex counts, word_off = prefix sum of
 * ceil(N_s / 64) (a wave works on 64 consecutive vertices of ONE scene); n_vertices = vert_off[n_scenes], n_waves = word_off[n_scenes].
 *   mspa_prep_labels   seg [n_vertices] int32 = the scans' segIndices.  Scene s owns rows tab_off[s] .. tab_off[s+1] of seg2inst /
 *                      seg2label (indexed by segment id; a segment id outside reads as 0 = unannotated) and entries
 *                      lab_off[s] .. lab_off[s+1] of label_value (entry 0 of every scene: 0).  Writes
 *                      instance_ids[v] = seg2inst[seg[v]], label_index[v] = seg2label[seg[v]], label_ids[v] = label_value[label_index[v]].
 *   mspa_prep_align    vertices [n_vertices, 6] float32 (x y z r g b) -> out_aligned [n_vertices, 6] float64; x y z through scene s's
 *                      row-major 4x4 axis_align[s] in the order m0*x, fma(m1,y,.), fma(m2,z,.), fma(m3,1.0,.) -- the bits of
 *                      np.dot(pts, A.T) (BL:66-69) for N >= 2; a scene of one vertex takes the order of the
 *                      vector path np.dot takes then, (m0*x + m2*z) + (m1*y + m3) with every product rounded; colours widened.
 *   mspa_prep_objects  scene s owns object slots obj_off[s] .. obj_off[s+1] (slot obj_off[s] + k - 1 <-> instance id k); n_objects =
 *                      obj_off[n_scenes].  Per slot: out_count = vertices with that id, out_lo / out_hi_unaligned [n_objects, 3] = min /
 *                      max of the float32 x y z (as float64: exact), out_lo / out_hi_aligned the same over out_aligned (+inf / -inf
 *                      for an object without vertices); out_bits [n_objects, n_words] = the object's membership bitset over its
 *                      scene's vertices (n_words >= the longest scene's word count; mspa_bits_popcount -> prefix sum ->
 *                      mspa_bits_expand turn the rows into vertex lists in vertex order: the stable split).  Per scene:
 *                      out_zero_count = vertices with id 0, out_unique = len(np.unique(instance_ids)).
 */
int mspa_prep_labels(const int32_t *seg, const int64_t *vert_off, const int64_t *word_off, int64_t n_scenes, int64_t n_vertices,
                     int64_t n_waves, const int64_t *tab_off, const int32_t *seg2inst, const int32_t *seg2label,
                     const int64_t *lab_off, const uint32_t *label_value, uint32_t *out_instance_ids, uint32_t *out_label_ids,
                     int32_t *out_label_index, mspa_stream_t stream);
int mspa_prep_align(const float *vertices, const int64_t *vert_off, const int64_t *word_off, int64_t n_scenes, int64_t n_vertices,
                    int64_t n_waves, const double *axis_align, double *out_aligned, mspa_stream_t stream);
int mspa_prep_objects(const uint32_t *instance_ids, const float *vertices, const double *aligned, const int64_t *vert_off,
                      const int64_t *word_off, int64_t n_scenes, int64_t n_vertices, int64_t n_waves, const int64_t *obj_off,
                      int64_t n_objects, uint64_t *out_bits, int64_t n_words, int32_t *out_count, double *out_lo_unaligned,
                      double *out_hi_unaligned, double *out_lo_aligned, double *out_hi_aligned, int32_t *out_zero_count,
                      int32_t *out_unique, mspa_stream_t stream);

/*
 * JSON integer lists -> int32 (the "segIndices" array of *.segs.json; the inverse of the formatters above).  Array a is the text
 * BETWEEN its brackets, bytes text_offsets[a] .. text_offsets[a+1] of one concatenated buffer.
 *   mspa_parse_int_list_host          HOST pointers, up to n_threads pool threads, one array each.  JSON's grammar: white space,
 *                                     -?(0|[1-9][0-9]*), commas.  Array a's values go to out_values[out_offsets[a] ..], at most
 *                                     out_offsets[a+1] - out_offsets[a] of them; out_counts[a] = how many.  status[a]: 0 parsed;
 *                                     1 not such a list; 2 a value outside int32; 16 more values than room.
 *   mspa_parse_int_list_flags_device  DEVICE pointers; one lane per byte: out_flags[i] = 1 where a number ends, 1 << 32 for a
 *                                     comma; clears status and raises bit 1 of status[a] for a byte that is no digit, comma
 *                                     or JSON white space.
 *   mspa_parse_int_list_device        flags_prefix: exclusive prefix sum of out_flags, n_bytes + 1 entries (the caller's plumbing).
 *                                     The lane at a number's last digit assembles it from at most 10 digits and stores it at
 *                                     out_values[numbers in front of it] (arrays back to back; nothing is stored at or beyond
 *                                     out_capacity); out_offsets [n_arrays + 1] = where each array's values start.  status bits:
 *                                     2 more than 10 digits or above INT32_MAX, 4 a leading zero, 8 commas and numbers do not
 *                                     alternate, 16 the count differs from expected_counts[a] (NULL or < 0: not checked).
 *                                     Non-negative lists only: a '-' declines.  A declined array (status != 0) is the host
 *                                     parser's; its neighbours' values are intact.
 */
int mspa_parse_int_list_host(const char *text_host, const int64_t *text_offsets_host, int64_t n_arrays, int32_t *out_values_host,
                             const int64_t *out_offsets_host, int64_t *out_counts_host, int32_t *status_host, int32_t n_threads);
int mspa_parse_int_list_flags_device(const char *text_dev, const int64_t *text_offsets_dev, int64_t n_arrays, int64_t n_bytes,
                                     int64_t *out_flags_dev, int32_t *status_dev, mspa_stream_t stream);
int mspa_parse_int_list_device(const char *text_dev, const int64_t *text_offsets_dev, int64_t n_arrays, int64_t n_bytes,
                               const int64_t *flags_prefix_dev, const int64_t *expected_counts_dev, int32_t *out_values_dev,
                               int64_t out_capacity, int64_t *out_offsets_dev, int32_t *status_dev, mspa_stream_t stream);

/*
 * Host-side staging of a scene's depth frames (the loop that fills the frame stack in the reference: CFR / MVI read one
 * image per frame into its own array): n_blocks equally sized host blocks are gathered into one contiguous destination
 * -- the pinned buffer the H2D copy reads -- by up to n_threads copy threads.  Host pointers only; no device work.
 */
int mspa_gather_blocks_host(const void *const *src_blocks_host, int64_t n_blocks, int64_t block_bytes, void *dst_host,
                            int32_t n_threads);

/*
 * Host-side ingest of zlib-compressed frames: the depth payloads of a ScanNet .sens stream (`zlib_ushort`,
 * extract_posed_images.py:49-57 inflates them one by one).  Block k (src_bytes_host[k] bytes at src_blocks_host[k], e.g.
 * inside a memory-mapped file) is inflated into dst_host + k * block_bytes by up to n_threads threads.  Every block
 * must inflate to exactly block_bytes; otherwise MSPA_EINVAL and the error string names the block.
 */
int mspa_inflate_blocks_host(const void *const *src_blocks_host, const int64_t *src_bytes_host, int64_t n_blocks,
                             int64_t block_bytes, void *dst_host, int32_t n_threads);

/*
 * Host-side ingest of a scene's depth frames from disk: the per-frame `cv2.imread(depth_png, -1)` of
 * SceneInfoHandler.get_depth_image (info_handler.py:149-155), which CFR.process_scene / MVI.process_scene call once per
 * image (CFR:152-157, MVI:93-100) and which the reference hides behind a process pool over scenes (CFR:222-229,
 * MVI:151-156).  The n_files files named by paths_host (NUL-terminated) are read and decoded into
 * dst_host[k * h * w ...] (host byte order) by up to n_threads native threads; no interpreter lock is involved.
 * Decoded natively: PNG, 16-bit greyscale, non-interlaced, of exactly h x w pixels (what extract_posed_images.py:118-123
 * writes).  status_host[k]: 0 decoded; 1 file unreadable; 2 a PNG of another pixel format or size (decode that frame with
 * a general reader); 3 corrupt.  Returns MSPA_OK when the call ran (the per-file status tells), MSPA_EINVAL on a bad argument.
 *   mspa_png_header_host   (h, w, bit depth, colour type, interlace flag) of one file's IHDR; each output optional
 */
int mspa_read_depth_png_host(const char *const *paths_host, int64_t n_files, int32_t h, int32_t w, uint16_t *dst_host,
                             int32_t n_threads, int32_t *status_host);
int mspa_png_header_host(const char *path_host, int32_t *h, int32_t *w, int32_t *bit_depth, int32_t *color_type,
                         int32_t *interlace);
/*
 * The table-driven zlib decoder the two ingest entry points above try first (csrc/inflate_fast.h; the from-disk sweep is bound
 * by the inflate of its depth frames -- zlib's own delivers ~155 MB/s per thread on them).  One whole zlib stream in host memory
 * -> exactly dst_bytes of output.  Returns 0 when the stream was decoded (output size AND Adler-32 match), 1 when the decoder
 * declines it (damaged or truncated stream, other output size, preset dictionary): the callers above then use zlib itself.
 */
int mspa_inflate_zlib_fast_host(const void *src_host, int64_t src_bytes, void *dst_host, int64_t dst_bytes);

/*
 * Depth-frame decode ON THE DEVICE (csrc/device_ingest.hip): the same two reference stages -- `cv2.imread(depth_png, -1)` per
 * frame (info_handler.py:149-155) and `zlib.decompress` per .sens frame (extract_posed_images.py:49-57) -- with the COMPRESSED
 * bytes crossing PCIe and the frames landing in HBM as the [F, h, w] uint16 block K1 / K3 read.
 *
 * mspa_inflate_blocks_device   n_blocks zlib streams (RFC 1950 / 1951: stored, fixed and dynamic blocks, 32 K window), stream k =
 *   src_bytes_dev[k] bytes at src_dev + src_offsets_dev[k] (offsets multiples of 8; the buffer src_dev .. + src_capacity must
 *   hold every stream and may be read up to the 8-byte unit a stream ends in), each inflated by ONE wave into dst_dev + k *
 *   dst_pitch.  status_dev[k] (int32, written for every k): 0 the stream inflated to EXACTLY block_bytes, ended inside its
 *   input and the Adler-32 of the output equals its trailer; 1 not a valid / supported stream or another size; 2 checksum
 *   mismatch.  A block with a non-zero status holds garbage: decode that frame on the host (mspa_inflate_blocks_host /
 *   mspa_read_depth_png_host) -- the same "accept only what verifies, hand the rest on" contract as csrc/inflate_fast.h.
 *   work_dev: n_blocks uint32 of scratch.  src_dev 16-byte, dst_dev and dst_pitch 256-byte aligned; block_bytes <= 64 MiB.
 * mspa_png_unfilter_device     n_images inflated scanline blocks (h rows of 1 filter byte + 2 w sample bytes, image k at raw_dev +
 *   k * raw_pitch) -> out_dev[k, h, w] uint16 in host byte order: the five PNG row filters (None / Sub / Up / Average / Paeth)
 *   undone, big-endian samples swapped.  Images whose status_dev[k] is non-zero on entry are skipped; an image with a filter
 *   byte > 4 gets status 3.  raw_pitch >= h * (2 w + 1) and a multiple of 4, raw_dev 4-byte aligned (MSPA_EINVAL otherwise);
 *   out_dev needs no more than the 2-byte alignment of uint16.
 * mspa_png_pack_idat_host      the host half: the n_files 16-bit greyscale non-interlaced h x w PNG files are read by up to
 *   n_threads threads and the payloads of their IDAT chunks -- the scanlines' zlib stream -- packed into dst_host (pinned memory
 *   the H2D copy reads) at offsets_host[k] (multiples of 16), bytes_host[k] long.  Call with dst_host == NULL first: only the
 *   files' sizes are looked up and *capacity_needed is set (offsets are assigned from the file sizes, so both calls agree).
 *   status_host[k]: 0 packed; 1 unreadable; 2 another pixel format or size; 3 corrupt chunk structure.
 */
/*
 * A stream for long-running background kernels (the depth decode above) that leaves `reserve_cus` compute units alone, spread
 * over the device (every (n_cu / reserve_cus)-th unit; hipExtStreamCreateWithCUMask): kernels launched on other streams always
 * find free LDS and wave slots there instead of waiting for a 100 ms decode wave to retire.  reserve_cus = 0: a plain
 * non-blocking stream.  *stream_out is a hipStream_t; release it with mspa_stream_destroy.
 */
int mspa_stream_create_reserving(int32_t reserve_cus, void **stream_out);
int mspa_stream_destroy(void *stream);

int mspa_inflate_blocks_device(const void *src_dev, const int64_t *src_offsets_dev, const int64_t *src_bytes_dev,
                               int64_t src_capacity, int64_t n_blocks, int64_t block_bytes, void *dst_dev, int64_t dst_pitch,
                               int32_t *status_dev, uint32_t *work_dev, void *stream);
int mspa_png_unfilter_device(const void *raw_dev, int64_t raw_pitch, int64_t n_images, int32_t h, int32_t w, uint16_t *out_dev,
                             int32_t *status_dev, void *stream);
int mspa_png_pack_idat_host(const char *const *paths_host, int64_t n_files, int32_t h, int32_t w, void *dst_host,
                            int64_t dst_capacity, int64_t *offsets_host, int64_t *bytes_host, int32_t *status_host,
                            int64_t *capacity_needed, int32_t n_threads);

/*
 * Colour-frame decode ON THE DEVICE (csrc/jpeg_decode.hip, arithmetic in csrc/jpeg_core.h): the per-frame JPEG decode of
 * SceneInfoHandler.get_color_image (`cv2.imread` + BGR -> RGB, ops.py:265-266) and of the .sens colour payloads
 * (extract_posed_images.py), with the COMPRESSED bytes crossing PCIe and [H, W, 3] uint8 RGB landing in HBM -- the layout
 * mspa_pair_reproject's `rgb` reads.  Output is bit-identical to libjpeg-turbo's default decompression (JDCT_ISLOW, fancy
 * upsampling) for every image that gets status 0.
 *
 * mspa_jpeg_parse_host     n payloads (nbytes_host[k] bytes at src_host[k]) -> n descriptors of MSPA_JPEG_DESC_BYTES each at
 *   desc_host, and status_host[k]: 0 decodable on the device; 1 not a JPEG, truncated or malformed header, invalid table;
 *   2 a JPEG outside the accepted subset.  Accepted: SOF0 (baseline, 8-bit, Huffman), one scan holding every component,
 *   greyscale, or YCbCr (JFIF, or no Adobe marker and component ids other than 'R','G','B') with luma sampling 1x1, 2x1 or 2x2
 *   and chroma 1x1; any DQT / DHT / APPn / COM / DRI segments before SOS.  Reads only [src, src + nbytes).
 *   Descriptor fields (little endian; the rest is the kernel's tables):
 *     int32 [0] status [1] h [2] w [3] components [4] restart interval (MCUs; 0 none) [5] max h sampling [6] max v sampling
 *           [7] MCUs per row [8] MCU rows [9] coefficient blocks
 *     int64 at byte 48: offset of the entropy-coded segment in the payload; at byte 56: its length (to the payload's end)
 *     int32 at byte 64: h sampling[3], v sampling[3], quantisation table id[3], DC table id[3], AC table id[3]
 *     uint16 at byte 192: [3][64] each component's quantisation table in natural (row-major) order
 * mspa_jpeg_workspace_bytes  bytes of scratch a decode of n_images h x w images needs (coefficients and component planes).
 * mspa_jpeg_decode_device  n_images payloads resident on the device (payload k = src_bytes_dev[k] bytes at src_dev +
 *   src_offsets_dev[k]; src_dev 4-byte aligned; the kernel reads the aligned 4-byte words that hold a payload's bytes, all of
 *   which must lie inside src_capacity) with their descriptors (desc_dev, 16-byte aligned) -> out_dev[k] = [h, w, 3] uint8 RGB
 *   (greyscale: R = G = B).  status_dev[k] (written for every k): 0 decoded exactly -- every MCU from real data, restart markers
 *   present and in sequence, valid codes only, no coefficient past index 63, the segment consumed up to EOI with at most seven
 *   1-bits of padding, every block inside the range in which all forms of the IDCT agree; otherwise the parse status, 3 another
 *   size than h x w, 4 bad entropy-coded data, 5 a restart marker missing or out of sequence, 6 data after the last MCU or no
 *   EOI, 7 a block out of range.  A non-zero image's output is unspecified: decode that frame on the host.  Images of one
 *   call share (h, w); sampling and tables may differ.  workspace: caller-owned, 16-byte aligned, at least
 *   mspa_jpeg_workspace_bytes(n_images, h, w) bytes; contents undefined afterwards.  n_images <= 65 535.
 */
#define MSPA_JPEG_DESC_BYTES 4224
int mspa_jpeg_parse_host(const void *const *src_host, const int64_t *nbytes_host, int64_t n, void *desc_host, int32_t *status_host);
int64_t mspa_jpeg_workspace_bytes(int64_t n_images, int32_t h, int32_t w);
int mspa_jpeg_decode_device(const void *src_dev, const int64_t *src_offsets_dev, const int64_t *src_bytes_dev, int64_t src_capacity,
                            const void *desc_dev, int64_t n_images, int32_t h, int32_t w, uint8_t *out_dev, int32_t *status_dev,
                            void *workspace, int64_t workspace_bytes, void *stream);

/*
 * Annotated-image writes ON THE DEVICE (csrc/jpeg_encode.hip, arithmetic in csrc/jpeg_encode_core.h): the drawing and the
 * JPEG encode of mspa/annotate.py's PillowAnnotator, byte for byte.
 *
 * mspa_jpeg_encode_capacity  worst-case bytes of one file of h x w at `subsampling` (0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0, Pillow's
 *   numbering); -1 for a bad argument.  1 <= h, w <= 65535.
 * mspa_jpeg_encode_workspace_bytes  bytes of scratch an encode of n_images h x w images needs; -1 for a bad argument.
 * mspa_jpeg_encode_header_host  the file's bytes up to the end of SOS (SOI, APP0 JFIF 1.1 with density 1:1 and no units, DQT
 *   luma, DQT chroma, SOF0, DHT DC0 / AC0 / DC1 / AC1, SOS) into dst (capacity >= 623); *nbytes = its length.
 * mspa_jpeg_encode_device  rgb_dev = [n_images, h, w, 3] uint8 RGB -> out_dev + k * out_pitch = image k's whole file (header,
 *   entropy-coded data, EOI), equal to Pillow 12 / libjpeg-turbo `Image.fromarray(rgb).save(f, "JPEG", quality=quality,
 *   subsampling=subsampling)`: standard Huffman tables, JDCT_ISLOW, no restart markers.  out_bytes_dev[k] (int64) = the file's
 *   length; a file longer than out_pitch is written up to out_pitch only (a pitch of mspa_jpeg_encode_capacity never
 *   truncates).  quality 1..100.  workspace: caller-owned, 16-byte aligned, at least mspa_jpeg_encode_workspace_bytes bytes;
 *   contents undefined afterwards.  n_images <= 65 535.  Only enqueues on `stream`.
 * mspa_draw_spans_device  n_spans int32 records (image, y, x0, x1, 0xRRGGBB) painted into images_dev = [n_images, h, w, 3] uint8:
 *   pixels x0..x1 (inclusive, clipped) of row y take the colour.  Records must be grouped by (image, y) with call order kept
 *   inside a group; the last record of a group that covers a pixel wins.  Records outside the images are ignored.
 * mspa_blend_masks_device  n_labels int64 records (image, x, y, mask w, mask h, 0xRRGGBB ink, mask offset, 0): the 8-bit mask at
 *   masks_dev + offset ([mask h, mask w], row-major) blended onto the image at (x, y), clipped at the borders, with Pillow's
 *   arithmetic t = ink * m + px * (255 - m) + 128, px' = ((t >> 8) + t) >> 8.  Records must be grouped by image with call order
 *   kept inside a group; overlapping labels blend in that order.  A record whose mask lies outside [0, masks_bytes) is ignored.
 */
int64_t mspa_jpeg_encode_capacity(int32_t h, int32_t w, int32_t subsampling);
int64_t mspa_jpeg_encode_workspace_bytes(int64_t n_images, int32_t h, int32_t w, int32_t subsampling);
int mspa_jpeg_encode_header_host(int32_t h, int32_t w, int32_t quality, int32_t subsampling, uint8_t *dst, int64_t capacity,
                                 int64_t *nbytes);
int mspa_jpeg_encode_device(const uint8_t *rgb_dev, int64_t n_images, int32_t h, int32_t w, int32_t quality, int32_t subsampling,
                            uint8_t *out_dev, int64_t out_pitch, int64_t *out_bytes_dev, void *workspace, int64_t workspace_bytes,
                            void *stream);
int mspa_draw_spans_device(const int32_t *spans_dev, int64_t n_spans, uint8_t *images_dev, int64_t n_images, int32_t h, int32_t w,
                           void *stream);
int mspa_blend_masks_device(const int64_t *labels_dev, int64_t n_labels, const uint8_t *masks_dev, int64_t masks_bytes,
                            uint8_t *images_dev, int64_t n_images, int32_t h, int32_t w, void *stream);

/*
 * Depth-PNG writes ON THE DEVICE (csrc/png_encode.hip, arithmetic in csrc/png_encode_core.h): 16-bit greyscale, non-interlaced
 * PNG files whose pixels equal the input and whose filtered scanlines are Pillow's (`Image.fromarray(depth).save(path)`); the
 * deflate stream is the encoder's own, so the files are not Pillow's byte for byte.  A g++ build of png_encode_core.h is the
 * reference the device equals byte for byte.
 *
 * mspa_png_encode_capacity  worst-case bytes of one file of h x w; -1 for a bad size (1 <= h, w <= 8192).  The bound: the
 *   filtered stream has N = h (1 + 2 w) bytes in ceil(N / 32768) deflate blocks; a block is written dynamic only when that is
 *   shorter than 42 + 8 L bits (L its bytes), otherwise stored, which is 3 + <= 7 padding + 32 + 8 L bits; so the deflate stream
 *   has at most N + ceil(42 blocks / 8) bytes, the zlib stream 6 more (header and Adler-32), and the file adds 33 (signature,
 *   IHDR), 12 per IDAT chunk of at most 16 384 zlib bytes, and 12 (IEND).
 * mspa_png_encode_workspace_bytes  bytes of scratch an encode of n frames of h x w needs (about 7 h (2 w + 1) n); -1 for a bad
 *   argument (n outside 0..65535 or a bad size).
 * mspa_png_encode_device  depth_dev = [n, h, w] uint16 values stored as int16 (the layout of depth_device /
 *   read_depth_frames_device), contiguous -> out_dev + k * out_pitch = frame k's whole file, nbytes_dev[k] (int64) = its length.
 *   Bytes [0, nbytes rounded up to 4) of a row are written (the padding bytes are 0); the rest of the row is left as it was.
 *   Limits: 1 <= h, w <= 8192, 0 <= n <= 65535 (n = 0 writes nothing and returns MSPA_OK).
 *   Alignment: depth_dev 2 bytes, out_dev 4 bytes, nbytes_dev 8 bytes, workspace 16 bytes; out_pitch a multiple of 4 and
 *   >= mspa_png_encode_capacity(h, w).  workspace: caller-owned, >= mspa_png_encode_workspace_bytes(n, h, w); contents
 *   undefined afterwards.  Anything else (a null pointer included) returns MSPA_EINVAL before anything is enqueued, so the
 *   outputs are left unwritten.  Only enqueues on `stream`.
 */
int64_t mspa_png_encode_capacity(int32_t h, int32_t w);
int64_t mspa_png_encode_workspace_bytes(int64_t n, int32_t h, int32_t w);
int mspa_png_encode_device(const int16_t *depth_dev, int64_t n, int32_t h, int32_t w, uint8_t *out_dev, int64_t out_pitch,
                           int64_t *nbytes_dev, void *workspace, int64_t workspace_bytes, void *stream);

/*
 * The visibility index's `values` column chunk ON THE DEVICE (csrc/parquet_pages.hip, K12; arithmetic in csrc/snappy_core.h):
 * parquet v1 data pages -- PLAIN BYTE_ARRAY, RLE definition levels, Snappy -- from arrow's string layout (int32 offsets
 * [rows + 1], uint8 data) as mspa_format_lists_device leaves it.  The compressor is the library's own deterministic algorithm
 * (any Snappy decoder reads its streams; the bytes are not Google's): a stream is varint(n) and the elements of the input's
 * independent 64 KiB blocks.  A g++ build of snappy_core.h is the reference the device equals byte for byte.
 *
 * mspa_snappy_capacity  worst-case bytes of the stream of n input bytes, 32 + n + n / 6; -1 for n outside 0 .. 2^31 - 1.
 * mspa_snappy_compress_host  the reference: src[0, n) -> dst (dst_capacity >= mspa_snappy_capacity(n)); returns the stream's
 *   length, or MSPA_EINVAL.
 * mspa_snappy_workspace_bytes  bytes of block slots for n_blocks blocks (76 544 each); -1 for a bad count.
 * mspa_snappy_compress_device  a batch of streams: stream s is src_dev[offsets_dev[s], + nbytes_dev[s]) (int64; streams may be
 *   empty, overlap or leave gaps; every one must lie inside [0, src_bytes)), block_prefix_dev [n_streams + 1] the exclusive
 *   prefix sum of ceil(nbytes / 65536) and n_blocks its last entry (the caller's plumbing, as for mspa_format_lists_device).
 *   Block b's elements go to slots_dev + 76 544 b, their byte count to out_block_sizes_dev[b] (int64); -1 there marks a block
 *   whose table entries do not describe a stream inside src (nothing was read for it).
 * mspa_snappy_compact_device  the streams, back to back, into out_dev: size_prefix_dev [n_blocks + 1] is the exclusive prefix
 *   sum of the block sizes, preamble_prefix_dev [n_streams + 1] that of the preambles' lengths (varint(nbytes): 1 .. 5 bytes).
 *   Stream s occupies out_dev[size_prefix[block_prefix[s]] + preamble_prefix[s], size_prefix[block_prefix[s + 1]] +
 *   preamble_prefix[s + 1]).  bad_flag_dev (int32, zeroed by the caller) is raised when a destination falls outside out_bytes;
 *   such bytes are not written.
 * mspa_parquet_page_cuts_host  the page-cut rule on host offsets: a page ends after the first value at which its PLAIN bytes
 *   (4 + len per value) reach page_bytes.  out_cuts [pages + 1] (first value of each page, then rows) when not null; returns
 *   the page count, MSPA_EINVAL for decreasing offsets or a cuts_capacity that is too small.
 * mspa_parquet_page_payload_bytes_host / mspa_parquet_page_payload_host  the reference of one page's uncompressed payload for
 *   the values [v0, v1): u32le(L), L bytes of levels (varint(num_values << 1), 0x01), the PLAIN values.
 * mspa_parquet_string_pages_device  all pages' payloads back to back: cuts_dev [n_pages + 1] (int64, as above) and
 *   payload_offsets_dev [n_pages + 1] (int64, exclusive prefix sum of the payload lengths; last entry payload_bytes) ->
 *   out_payload_dev [payload_bytes].  The kernel checks the tables against the offsets and every index against rows and
 *   data_bytes; bad_flag_dev (int32, zeroed by the caller) is raised on a mismatch and the bytes concerned are not written.
 * All device calls only enqueue on `stream`; the caller owns every buffer; a wrong argument (a null pointer included) returns
 * MSPA_EINVAL before anything is enqueued.
 */
int64_t mspa_snappy_capacity(int64_t n);
int64_t mspa_snappy_compress_host(const uint8_t *src, int64_t n, uint8_t *dst, int64_t dst_capacity);
int64_t mspa_snappy_workspace_bytes(int64_t n_blocks);
int mspa_snappy_compress_device(const uint8_t *src_dev, int64_t src_bytes, const int64_t *offsets_dev, const int64_t *nbytes_dev,
                                int64_t n_streams, const int64_t *block_prefix_dev, int64_t n_blocks, uint8_t *slots_dev,
                                int64_t slots_bytes, int64_t *out_block_sizes_dev, void *stream);
int mspa_snappy_compact_device(const int64_t *nbytes_dev, int64_t n_streams, const int64_t *block_prefix_dev, int64_t n_blocks,
                               const uint8_t *slots_dev, int64_t slots_bytes, const int64_t *size_prefix_dev,
                               const int64_t *preamble_prefix_dev, uint8_t *out_dev, int64_t out_bytes, int32_t *bad_flag_dev,
                               void *stream);
int64_t mspa_parquet_page_cuts_host(const int32_t *offsets, int64_t rows, int64_t page_bytes, int64_t *out_cuts, int64_t cuts_capacity);
int64_t mspa_parquet_page_payload_bytes_host(const int32_t *offsets, int64_t v0, int64_t v1);
int mspa_parquet_page_payload_host(const int32_t *offsets, const uint8_t *data, int64_t v0, int64_t v1, uint8_t *dst,
                                   int64_t dst_capacity);
int mspa_parquet_string_pages_device(const int32_t *text_offsets_dev, int64_t rows, const uint8_t *data_dev, int64_t data_bytes,
                                     const int64_t *cuts_dev, const int64_t *payload_offsets_dev, int64_t n_pages, int64_t payload_bytes,
                                     uint8_t *out_payload_dev, int32_t *bad_flag_dev, void *stream);

/*
 * The way back -- a `values` column chunk's pages to the image_to_points rows' bitsets ON THE DEVICE (csrc/snappy_decode.hip,
 * csrc/index_rows.hip; the Snappy decoder's rules in csrc/snappy_core.h).  What a reader of the index otherwise does on the
 * host: decompress, walk the PLAIN values, json.loads every list, pack the bits.
 *
 * mspa_snappy_decompress_host  the reference: one raw Snappy stream src[0, src_len) (varint(n), then literals with 0 .. 4
 *   length bytes, copy-1 / copy-2 / copy-4 elements, overlapping copies included; any writer's) -> dst[0, expected).  Returns
 *   `expected`, or a negative code: -16 the preamble is not varint(expected); -17 an element runs past the input; -18 the
 *   output would pass `expected`; -19 a copy with offset 0 or one that reaches in front of the output; -20 input left over
 *   after `expected` bytes; -21 the input ended early; MSPA_EINVAL for a null pointer or a size outside 0 .. 2^31 - 1.
 *   Nothing outside [src, src + src_len) is read and nothing outside [dst, dst + expected) written, whatever the stream.
 * mspa_snappy_decompress_device  a batch: stream s is src_dev[offsets_dev[s], + nbytes_dev[s]) (int64; streams may be empty,
 *   overlap or leave gaps) and decodes to out_dev[out_offsets_dev[s], + out_bytes_dev[s]).  status_dev[s] (int32): 0 decoded,
 *   byte for byte the host's output; otherwise declined with the host's code, or MSPA_EINVAL for a table entry that does not
 *   lie inside [0, src_bytes) / [0, out_bytes) (nothing is touched then).  A declined stream's output bytes are unspecified
 *   but stay inside its own span.  One wave per stream; no copy offset is refused.
 * Decoding by blocks -- a second route with the same results.  Both writers (this library's, and Google's, which pyarrow uses)
 * compress the input in independent blocks of 64 KiB, so in their streams every multiple of 65 536 output bytes is an element
 * start, no element straddles one and no copy reaches in front of its block: such a stream is BLOCKWISE and every block decodes
 * alone, one wave per block, once the blocks' positions in the compressed bytes are known.
 * mspa_snappy_block_starts_host  the serial definition: out_starts[b] = the compressed position of the element that begins at
 *   output 65 536 b, for b < ceil(expected / 65536), and one more entry, src_len (starts_capacity >= that many).  Returns the
 *   block count; mspa_snappy_decompress_host's code for a stream that it declines; -22 for a stream that it decodes but that is
 *   not blockwise; MSPA_EINVAL as above.
 * mspa_snappy_blocks_workspace_bytes  bytes of workspace for a batch: stream_bytes >= the sum of the streams' compressed sizes
 *   (src_bytes when they do not overlap), n_streams, n_blocks = the sum of ceil(out_bytes / 65536).  About 8 bytes per compressed
 *   byte (the segment tables of the scan); -1 for a bad argument.
 * mspa_snappy_block_starts_device  the scan alone, for a batch as above: block_prefix_dev [n_streams + 1] is the exclusive prefix
 *   sum of ceil(out_bytes_dev / 65536) and n_blocks its last entry (the caller's plumbing, as for mspa_snappy_compress_device).
 *   Stream s's starts go to starts_dev[block_prefix[s] + s ..], one more than its blocks (the last is nbytes[s]); starts_dev
 *   has n_blocks + n_streams entries.  route_dev[s] (int32) = the stream's block count when it is blockwise and decodable, and
 *   then its starts are mspa_snappy_block_starts_host's; 0 otherwise (its starts are unspecified).  The scan cuts a stream into
 *   segments of 2 KiB of compressed bytes, one wave each; the only serial chain over a stream has one step per segment.
 * mspa_snappy_decompress_blocks_device  mspa_snappy_decompress_device's arguments and results -- status_dev and the bytes are
 *   the same for every input -- through the scan, one wave per block of every blockwise stream of two blocks or more, and then
 *   the one-wave kernel for every other stream and for every stream with anything the matter with it.  route_dev[s] = the number
 *   of blocks decoded in parallel, or 0 when the one-wave kernel decoded (or declined) the stream.  Nothing is read back in
 *   between.  workspace: caller-owned, 16-byte aligned, >= mspa_snappy_blocks_workspace_bytes; a stream whose tables do not fit
 *   stream_bytes takes the one-wave kernel.
 * mspa_parquet_plain_spans_device  pages_dev holds the needed pages' uncompressed payloads; page p is page_offsets_dev[p] +
 *   page_bytes_dev[p] (int64) and holds page_values_dev[p] values.  has_levels = 1: the payload opens with u32le(L) and L bytes
 *   of RLE definition levels, which must be ONE run of ones (varint(num_values << 1), 0x01: no nulls); 0: a required column,
 *   the values open the payload.  Rows row_begin_dev[p] .. row_begin_dev[p + 1] of the row table (int64, n_pages + 1 entries)
 *   belong to page p; row_index_dev[r] is the row's value number inside its page, ascending within a page.  Writes
 *   out_start_dev[r] (position of the value's text in pages_dev) and out_len_dev[r]; page_status_dev[p]: 0, 1 a length or a
 *   table entry outside the page, 2 levels that are not a run of ones (the rows of such a page get 0 / 0).
 * mspa_rle_hybrid_take_host  the reference of parquet's RLE / bit-packed hybrid (csrc/rle_hybrid_core.h), the encoding of a
 *   dictionary-coded page's indices: src[0, src_len) is runs, each behind a ULEB128 header h -- h & 1 == 0: h >> 1 times ONE
 *   value of ceil(bit_width / 8) little-endian bytes; h & 1 == 1: h >> 1 groups of 8 values of bit_width bits, LSB first (the
 *   last group may be padding beyond n_values).  out[i] (int32) = value rows[i]; rows (int64) ascend strictly and are
 *   < n_values.  The walk stops at the last needed row and reads nothing outside [src, src + src_len).  Returns 0, or: -32 a
 *   bit width outside 0 .. 32; -33 a header of more than 5 bytes or one that runs past the input; -34 a run of zero values;
 *   -35 a run whose bytes pass the input's end; -36 the runs end before a needed row; MSPA_EINVAL for rows that do not ascend
 *   or are >= n_values, a null pointer or a size outside 0 .. 2^31 - 1.
 * mspa_parquet_dict_spans_device  mspa_parquet_plain_spans_device for dictionary-coded data pages (RLE_DICTIONARY,
 *   PLAIN_DICTIONARY), with the same page and row tables: behind the levels (has_levels, as above) a page is one byte of bit
 *   width and a hybrid stream of indices.  The page's dictionary is entries dict_begin_dev[p] .. + dict_count_dev[p] of a span
 *   table dict_start_dev / dict_len_dev (int64, n_dict entries) -- what mspa_parquet_plain_spans_device writes for the
 *   decompressed dictionary page (has_levels = 0, every entry a row), so pages of several row groups each name their own.
 *   Writes out_index_dev[r] (int32, the row's index), out_start_dev[r] / out_len_dev[r] (the entry's span);
 *   page_status_dev[p]: 0, 1 a table entry outside the page (or rows that do not ascend), 2 levels, 3 malformed runs --
 *   page_code_dev[p] (int32) then holds mspa_rle_hybrid_take_host's code, else 0 --, 4 an index >= dict_count_dev[p]; the
 *   rows of a declined page get -1 and 0 / 0.  One lane per page: a chain of one step per run in front of the last needed row.
 * mspa_index_rows_brackets_device  row r's text must be '[' ... ']' with JSON white space around: out_inner_start_dev /
 *   out_inner_len_dev = what lies between; row_status_dev[r] = 1 and an empty span otherwise.
 * mspa_index_rows_gather_device  the spans back to back: inner_prefix_dev [n_rows + 1] is the exclusive prefix sum of the
 *   inner lengths and text_bytes its last entry (< 2 GiB) -> out_text_dev, the layout mspa_parse_int_list_flags_device and
 *   mspa_parse_int_list_device take (with inner_prefix_dev as their text_offsets).
 * mspa_index_lists_to_bits_device  values_dev (int32) / offsets_dev [n_rows + 1] as mspa_parse_int_list_device leaves them ->
 *   out_bits_dev [n_rows, n_words] uint64, bit i of word w = vertex 64 w + i (scene.pack_index_lists' layout), rows zeroed
 *   first; n_points <= 64 n_words.  Lists ascend: a value below its predecessor raises 32 in row_status_dev[r] (cleared by the
 *   call), a value outside [0, n_points) 64 -- such a row's bits are unspecified; a duplicate is harmless, an empty list a zero row.
 * mspa_index_lists_pick_device  the same values_dev / offsets_dev read as LISTS (duplicates count, the order is the text's):
 *   samples_dev [n_samples, 2] int64 (row, position) -> out_vertex_dev[s] (int32) = values[offsets[row] + position] and
 *   out_status_dev[s] (int32) = 0; otherwise out_vertex_dev[s] = -1 and the status says why: 1 the row lies outside
 *   [0, n_rows), 2 the position outside [0, offsets[row + 1] - offsets[row]), 4 the value outside [0, n_points), 8 offsets[row]
 *   or offsets[row + 1] outside [0, n_values] or descending.  n_points < 2^31; n_samples = 0 enqueues nothing.  A vertex with a
 *   non-zero status must not reach mspa_project_samples_ex, which indexes xyz with what it is given.
 * All device calls only enqueue on `stream`; a wrong argument (a null pointer included) returns MSPA_EINVAL before anything is
 * enqueued; no kernel uses atomics.
 */
int64_t mspa_snappy_decompress_host(const uint8_t *src, int64_t src_len, uint8_t *dst, int64_t expected);
int mspa_snappy_decompress_device(const uint8_t *src_dev, int64_t src_bytes, const int64_t *offsets_dev, const int64_t *nbytes_dev,
                                  int64_t n_streams, uint8_t *out_dev, int64_t out_bytes, const int64_t *out_offsets_dev,
                                  const int64_t *out_bytes_dev, int32_t *status_dev, void *stream);
int64_t mspa_snappy_block_starts_host(const uint8_t *src, int64_t src_len, int64_t expected, int64_t *out_starts, int64_t starts_capacity);
int64_t mspa_snappy_blocks_workspace_bytes(int64_t stream_bytes, int64_t n_streams, int64_t n_blocks);
int mspa_snappy_block_starts_device(const uint8_t *src_dev, int64_t src_bytes, const int64_t *offsets_dev, const int64_t *nbytes_dev,
                                    int64_t n_streams, const int64_t *out_bytes_dev, const int64_t *block_prefix_dev, int64_t n_blocks,
                                    int64_t stream_bytes, void *workspace, int64_t workspace_bytes, int64_t *starts_dev, int32_t *route_dev,
                                    void *stream);
int mspa_snappy_decompress_blocks_device(const uint8_t *src_dev, int64_t src_bytes, const int64_t *offsets_dev, const int64_t *nbytes_dev,
                                         int64_t n_streams, uint8_t *out_dev, int64_t out_bytes, const int64_t *out_offsets_dev,
                                         const int64_t *out_bytes_dev, const int64_t *block_prefix_dev, int64_t n_blocks, int64_t stream_bytes,
                                         void *workspace, int64_t workspace_bytes, int32_t *status_dev, int32_t *route_dev, void *stream);
int mspa_parquet_plain_spans_device(const uint8_t *pages_dev, int64_t pages_bytes, const int64_t *page_offsets_dev,
                                    const int64_t *page_bytes_dev, const int64_t *page_values_dev, int64_t n_pages, int32_t has_levels,
                                    const int64_t *row_begin_dev, const int64_t *row_index_dev, int64_t n_rows, int64_t *out_start_dev,
                                    int64_t *out_len_dev, int32_t *page_status_dev, void *stream);
int mspa_rle_hybrid_take_host(const uint8_t *src, int64_t src_len, int32_t bit_width, int64_t n_values, const int64_t *rows, int64_t n_rows,
                              int32_t *out);
int mspa_parquet_dict_spans_device(const uint8_t *pages_dev, int64_t pages_bytes, const int64_t *page_offsets_dev,
                                   const int64_t *page_bytes_dev, const int64_t *page_values_dev, int64_t n_pages, int32_t has_levels,
                                   const int64_t *row_begin_dev, const int64_t *row_index_dev, int64_t n_rows,
                                   const int64_t *dict_begin_dev, const int64_t *dict_count_dev, const int64_t *dict_start_dev,
                                   const int64_t *dict_len_dev, int64_t n_dict, int32_t *out_index_dev, int64_t *out_start_dev,
                                   int64_t *out_len_dev, int32_t *page_status_dev, int32_t *page_code_dev, void *stream);
int mspa_index_rows_brackets_device(const uint8_t *pages_dev, int64_t pages_bytes, const int64_t *start_dev, const int64_t *len_dev,
                                    int64_t n_rows, int64_t *out_inner_start_dev, int64_t *out_inner_len_dev, int32_t *row_status_dev,
                                    void *stream);
int mspa_index_rows_gather_device(const uint8_t *pages_dev, int64_t pages_bytes, const int64_t *inner_start_dev,
                                  const int64_t *inner_prefix_dev, int64_t n_rows, uint8_t *out_text_dev, int64_t text_bytes, void *stream);
int mspa_index_lists_to_bits_device(const int32_t *values_dev, int64_t n_values, const int64_t *offsets_dev, int64_t n_rows,
                                    int64_t n_points, uint64_t *out_bits_dev, int64_t n_words, int32_t *row_status_dev, void *stream);
int mspa_index_lists_pick_device(const int32_t *values_dev, int64_t n_values, const int64_t *offsets_dev, int64_t n_rows,
                                 const int64_t *samples_dev, int64_t n_samples, int64_t n_points, int32_t *out_vertex_dev,
                                 int32_t *out_status_dev, void *stream);

/*
 * The pair table sampled ON THE DEVICE (csrc/pair_table.hip; the bin rule in csrc/pair_bins_core.h): the DOUBLE column chunks of
 * `*_camera_info_D5.parquet` from decompressed pages to float64 columns, `overlap` to one class byte per row and the classes to
 * lists of ascending file rows -- what mspa/pairtable.py draws its sample from.
 *
 * mspa_rle_hybrid_runs_device  a batch of RLE / bit-packed hybrid streams (csrc/rle_hybrid_core.h), ALL values wanted: stream s
 *   is src_dev[stream_offsets_dev[s], + stream_bytes_dev[s]) with bit width stream_bit_width_dev[s] and stream_values_dev[s]
 *   values (all int64); its values go to out[out_begin_dev[s] ..] of the expansion (out_begin_dev [n_streams + 1]: the exclusive
 *   prefix sum of the value counts, the caller's plumbing).  One lane per stream walks the run headers, one step per run, until
 *   the values are covered.  Always written: run_count_dev[s] (int64), status_dev[s] (int32: 0, or
 *   mspa_rle_hybrid_take_host's code, MSPA_EINVAL for a table entry outside src) and const_value_dev[s] (int32: the value when
 *   the stream is ONE RLE run over all its values, else -1).  With run_begin_dev (int64 [n_streams + 1], the exclusive prefix
 *   sum of a first call's run_count_dev; n_runs its last entry) the run table is written too: run_first_dev[r] (int64, where
 *   run r's first value goes in the expansion), run_pos_dev[r] (int64, where its bytes lie in src) and run_info_dev[r] (int32:
 *   bit 0 bit-packed, bit 1 a hole, bits 8.. the bit width).  A declined stream's runs end with one hole over the values it did
 *   not give (counted in run_count_dev).  run_begin_dev null or n_runs = 0: a counting call.
 * mspa_rle_hybrid_expand_device  the run table -> out_dev [n_values] int32, one lane per value: mspa_rle_hybrid_take_host's
 *   values for rows 0 .. n - 1 of every stream, -1 inside a hole.
 * mspa_parquet_double_layout_device  one lane per decompressed page of a DOUBLE chunk (page p: pages_dev[page_offsets_dev[p], +
 *   page_bytes_dev[p])): page_flags_dev[p] (int32) bit 0 a v1 page whose payload opens with u32le(L) and L bytes of RLE
 *   definition levels, bit 1 dictionary-coded values (a byte of bit width, then hybrid indices), bit 2 a v2 page whose level
 *   bytes the caller has put into rows 0 / 1 of layout_dev.  layout_dev [5, n_pages] int64: level offset, level bytes, value
 *   offset, value bytes (positions in pages_dev), bit width.  page_status_dev[p] (int32): 0, or 1 when the tables do not
 *   describe the page or a length runs past it (its layout is then empty).
 * mspa_parquet_double_column_device  out_dev [n_out] float64, one lane per row: page_first_dev [n_pages] (int64, ascending,
 *   first entry 0) says where each page's first row goes in out_dev, page_values_dev its rows.  With levels_dev (int32, the
 *   expansion of the level streams, level_begin_dev[p] where page p's open; level_rank_dev the exclusive running sum of
 *   levels_dev) a row of level 0 reads as NaN (0x7ff8000000000000) and the others take value k, k = the non-null rows of the
 *   page in front; levels_dev null: no page has a null.  A PLAIN page gives the 8 bytes at value offset + 8 k; a dictionary-
 *   coded page entry indices_dev[index_begin_dev[p] + k] of the dictionary at pages_dev[dict_offsets_dev[p], + 8
 *   dict_count_dev[p]) (a decompressed PLAIN dictionary page).  value_status_dev[p] (int32, cleared by the call): 5 when a
 *   level, an index or a value lies outside what the page holds; such rows read as NaN.
 * mspa_pair_bin_codes_host / _device  the sampler's bin rule (mspa/sampling.py: pd.cut(x, edges, include_lowest=True) behind
 *   the `== 0` split): edges [n_edges] float64, strictly ascending, 2 <= n_edges <= 251.  codes[i] (uint8) = the row's bin,
 *   254 for x == 0 (-0.0 too) or 255 for a row the sampler drops (NaN, outside the edges).  Host: out_counts [256] int64.
 *   Device: a wave per tile of mspa_pair_tile_rows() rows; out_tile_counts_dev [n_tiles, 256] int32, n_tiles =
 *   ceil(n / tile rows); n < 2^31.
 * mspa_pair_partition_device  codes_dev -> out_order_dev [n] int32: per class the ascending file rows, back to back.
 *   tile_offsets_dev [n_tiles, 256] int32: where tile t's first row of class c goes -- the exclusive prefix sum of the tile
 *   counts in (class, tile) order (the caller's plumbing).  Offsets that are not write nothing outside out_order_dev.
 * All device calls only enqueue on `stream`; a wrong argument returns MSPA_EINVAL before anything is enqueued; no atomics.
 */
#define MSPA_PAIR_CLASS_ZERO 254
#define MSPA_PAIR_CLASS_DROPPED 255
#define MSPA_PAIR_MAX_BINS 250
int mspa_rle_hybrid_runs_device(const uint8_t *src_dev, int64_t src_bytes, const int64_t *stream_offsets_dev,
                                const int64_t *stream_bytes_dev, const int64_t *stream_bit_width_dev, const int64_t *stream_values_dev,
                                const int64_t *out_begin_dev, const int64_t *run_begin_dev, int64_t n_streams, int64_t n_runs,
                                int64_t *run_count_dev, int32_t *status_dev, int32_t *const_value_dev, int64_t *run_first_dev,
                                int64_t *run_pos_dev, int32_t *run_info_dev, void *stream);
int mspa_rle_hybrid_expand_device(const uint8_t *src_dev, int64_t src_bytes, const int64_t *run_first_dev, const int64_t *run_pos_dev,
                                  const int32_t *run_info_dev, int64_t n_runs, int32_t *out_dev, int64_t n_values, void *stream);
int mspa_parquet_double_layout_device(const uint8_t *pages_dev, int64_t pages_bytes, const int64_t *page_offsets_dev,
                                      const int64_t *page_bytes_dev, const int32_t *page_flags_dev, int64_t n_pages, int64_t *layout_dev,
                                      int32_t *page_status_dev, void *stream);
int mspa_parquet_double_column_device(const uint8_t *pages_dev, int64_t pages_bytes, const int64_t *layout_dev,
                                      const int64_t *page_values_dev, const int32_t *page_flags_dev, const int64_t *page_first_dev,
                                      int64_t n_pages, const int32_t *levels_dev, const int64_t *level_rank_dev,
                                      const int64_t *level_begin_dev, int64_t n_levels, const int32_t *indices_dev,
                                      const int64_t *index_begin_dev, int64_t n_indices, const int64_t *dict_offsets_dev,
                                      const int64_t *dict_count_dev, double *out_dev, int64_t n_out, int32_t *value_status_dev,
                                      void *stream);
int32_t mspa_pair_tile_rows(void);
int mspa_pair_bin_codes_host(const double *x, int64_t n, const double *edges, int32_t n_edges, uint8_t *out_codes, int64_t *out_counts);
int mspa_pair_bin_codes_device(const double *x_dev, int64_t n, const double *edges_dev, int32_t n_edges, uint8_t *out_codes_dev,
                               int32_t *out_tile_counts_dev, int64_t n_tiles, void *stream);
int mspa_pair_partition_device(const uint8_t *codes_dev, int64_t n, const int32_t *tile_offsets_dev, int64_t n_tiles,
                               int32_t *out_order_dev, void *stream);

/*
 * Image resizing ON THE DEVICE (csrc/resize.hip, arithmetic in csrc/resize_core.h): n 8-bit RGB images of one shape resampled
 * to one target shape, bit-identical to Pillow's `Image.resize((W, H), resample)` for resample = BILINEAR (filter 2) and
 * BICUBIC (filter 3, Pillow's default): float64 weights per axis turned into 22-bit fixed point, a horizontal pass rounded to
 * 8 bits, then a vertical pass; a pass whose size does not change is skipped.  A g++ build of resize_core.h is the reference.
 *
 * mspa_resize_coeffs_host  the tables of one axis of `in` samples resampled to `out` (host pointers only): bounds = [out, 2]
 *   int32 (first tap, tap count), coeffs = [out, *ksize] int32 (zero past the tap count), *ksize = taps per row.  With bounds
 *   and coeffs both null only *ksize is written (a sizing call); coeffs alone may be null.  1 <= in, out <= 65535.  A table
 *   with a row whose sum of |coefficient| would let the 32-bit accumulator wrap returns MSPA_EUNSUPPORTED (none does for a
 *   factor within 1/8 .. 8).
 * mspa_resize_workspace_bytes  bytes of scratch a resize of n images of h x w to H x W needs (0 when at most one pass runs);
 *   -1 for a bad argument.
 * mspa_resize_rgb_device  src_dev + k * src_image_pitch + y * src_row_pitch = row y of image k ([w, 3] uint8; pitches in
 *   bytes, any alignment) -> dst_dev = [n_images, H, W, 3] uint8, contiguous.  The four tables are DEVICE copies of what
 *   mspa_resize_coeffs_host gives for (w, W, filter) and (h, H, filter); the tables of a pass that does not run may be null.
 *   The kernels clamp every table entry to the data they hold, so a damaged table gives wrong pixels, never a wild access.
 *   workspace: caller-owned, 16-byte aligned, >= mspa_resize_workspace_bytes (may be null when that is 0); contents
 *   undefined afterwards.  n_images = 0 returns MSPA_OK and enqueues nothing; sizes outside 1..65535, more than 65535 images,
 *   a null pointer, a pitch smaller than a row or a bad filter return MSPA_EINVAL.  A per-axis factor below 1/8 or above 8
 *   returns MSPA_EUNSUPPORTED (there Pillow's pass order is not the one restated here); inside that range nothing is
 *   declined.  Only enqueues on `stream`.
 */
int mspa_resize_coeffs_host(int32_t in, int32_t out, int32_t filter, int32_t *bounds, int32_t *coeffs, int32_t *ksize);
int64_t mspa_resize_workspace_bytes(int64_t n_images, int32_t h, int32_t w, int32_t H, int32_t W);
int mspa_resize_rgb_device(const uint8_t *src_dev, int64_t n_images, int32_t h, int32_t w, int64_t src_row_pitch,
                           int64_t src_image_pitch, uint8_t *dst_dev, int32_t H, int32_t W, int32_t filter,
                           const int32_t *bounds_x_dev, const int32_t *coeffs_x_dev, const int32_t *bounds_y_dev,
                           const int32_t *coeffs_y_dev, void *workspace, int64_t workspace_bytes, void *stream);

/*
 * K4 -- per-pair camera relations: the distance / yaw / pitch columns of CFR.process_scene's pair
 * table (CFR:176-189) and the relative-pose translation of CME.build_training_sample (CME:185-190).
 *
 *   E_aligned, Einv_aligned  [n_frames, 16] float64: A @ E and its inverse (host, numpy.linalg.inv)
 *   yaw, pitch               [n_frames] float64 degrees, extract_yaw_pitch (CFR:86-100) on the host
 *   pairs                    [n_pairs, 2] int32 (i, j)
 *   out                      [n_pairs, 6] float64: ||t_j - t_i||, yaw_j - yaw_i, pitch_j - pitch_i,
 *                            then the translation column of inv(E_i) @ E_j (camera-i axes)
 */
int mspa_pair_pose(const double *E_aligned, const double *Einv_aligned, const double *yaw,
                   const double *pitch, int32_t n_frames, const int32_t *pairs, int64_t n_pairs,
                   double *out, mspa_stream_t stream);

/*
 * extract_yaw_pitch (CFR:86-100) for a batch of frames: yaw = degrees(atan2(z_y, z_x)), pitch = degrees(asin(z_z / |z|)) of
 * the rotated z axis z = E[:3, 2].   E_aligned [n_frames, 16] f64  ->  out_yaw, out_pitch [n_frames] f64 (degrees).
 * Device libm: within a few ulp of NumPy, not bit-identical (float64 quantity; the host layer keeps a NumPy path for
 * callers that need the reference's exact bits).
 */
int mspa_extract_yaw_pitch(const double *E_aligned, int32_t n_frames, double *out_yaw, double *out_pitch,
                           mspa_stream_t stream);

/*
 * K5a -- TAPVid-3D tracks: camera->world (OM_C:446-454) and the normalised pinhole projection with
 * its validity test (TwoFrameVideoQAEngine.project_point, OM_C:293-315) for every (frame, point).
 *
 *   tracks_xyz  [T, P, 3] float64 camera-space      c2w  [T, 16] float64 = inv(extrinsics_w2c) (host)
 *   fx_fy_cx_cy_host  4 float64 on the HOST          H, W image size
 *   out_world [T, P, 3] f64,  out_uvn [T, P, 2] f64 (u/W, v/H),  out_ok [T, P] u8
 *   (1 = the reference would return coordinates, 0 = it returns None); each optional.
 */
int mspa_track_to_world(const double *tracks_xyz, const double *c2w, int32_t T, int32_t P,
                        const double *fx_fy_cx_cy_host, int32_t H, int32_t W, double *out_world,
                        double *out_uvn, uint8_t *out_ok, mspa_stream_t stream);

/*
 * K5b -- object displacement between two frames of one track point (OM_C:324-356) and the pair
 * distance used for binning (OM_C:484-498), for a list of (frame1, frame2, point) triples.
 *
 *   world [T, P, 3] f64 (K5a),  w2c / c2w [T, 16] f64,  triples [n, 3] int32
 *   out   [n, 5] f64: distance (0 when below obj_threshold), displacement in camera-1 axes (x, y, z;
 *         zeroed likewise), np.linalg.norm(axis=1)-form pair distance
 *   out_flags [n, 2] u8: point_moving, cam_moving
 */
int mspa_track_displacement(const double *world, const double *w2c, const double *c2w, int32_t T,
                            int32_t P, const int32_t *triples, int64_t n, double obj_threshold,
                            double cam_threshold, double *out, uint8_t *out_flags, mspa_stream_t stream);

/*
 * K5c -- pair mining of the object-movement head (OM_C:484-498): for each selected track point, the distance
 * between its world positions in every two of the frames it is visible in,
 * np.linalg.norm(points2 - points1, axis=1) over frame_pairs = [(i, j) for i < j] in that order.
 *   world [T, P, 3] f64 (K5a);  points [n_selected] i32;  frames = the points' visible-frame lists, concatenated,
 *   frame_offsets [n_selected+1] i32 into it;  n_frames_max = longest list;
 *   out_offsets [n_selected+1] i64 with out_offsets[s+1]-out_offsets[s] = n_s (n_s - 1) / 2  ->  out f64
 */
int mspa_track_pair_distances(const double *world, int32_t T, int32_t P, const int32_t *points,
                              const int32_t *frame_offsets, const int32_t *frames, int32_t n_selected,
                              int32_t n_frames_max, const int64_t *out_offsets, double *out, mspa_stream_t stream);

/*
 * K5d -- the pair mining itself (OM_C:465-567) on the device: csrc/track_mining.hip, rule in csrc/track_mining_core.h.  The
 * draws stay on the host (mspa/heads.py: plan_track_draws); the device counts, orders and resolves.  For a point, `frames` is
 * the ascending list of the frames it is visible in (V of them) and its pairs are (i, j), i < j, in row-major order, with K5c's
 * distance d.  A pair is dropped when (double)frames[i] > d + future_frame_windows (OM_C:505-507 as written), else static when
 * d < object_not_moving_threshold, else moving.  T <= 65535 throughout.
 *
 *   mspa_track_pair_stats       world [T, P, 3] f64, visibility [T, P] u8, points [n_points] i32 -> out_frames [n_points, T] i32
 *                               and out_positions [n_points, T, 3] f64 (the first V entries of a row), out_stats
 *                               [n_points, MSPA_TRACK_STAT_WORDS] i64: V, static pairs, moving pairs, the bit patterns of the
 *                               smallest and the largest moving distance, flags (1: a moving distance is not finite, 2: the point
 *                               lies outside the track).  The three outputs are what the calls below read.
 *   mspa_track_pair_bin_counts  edges [n_points, 11] f64 -> out_bin_counts [n_points, 10] i32 of the moving pairs, bin =
 *                               min(#{e : e <= d} - 1, 9) (np.digitize, then min(.., 9)).
 *   mspa_track_pair_sort        the segmented sort on its own: segment s is [seg_offsets[s], seg_offsets[s+1]) of keys
 *                               [2, n_total] u64 and payload [2, n_total] u32 (row 0 holds the data and the result, row 1 is the
 *                               other half of the ping-pong), each segment shorter than 2^31, sorted by (key, payload).
 *                               payload_ordered != 0: every segment ascends in its payload already, so only the key is sorted.
 *   mspa_track_pair_order       rows [n_selected] i32 (rows of the statistics), seg_offsets [n_selected + 1] i64 with segment
 *                               lengths = the rows' moving counts -> every selected point's moving pairs in keys / payload as
 *                               above: key = the bits of d, payload = (i << 16) | j, sorted by (key, payload).
 *   mspa_track_pair_resolve     picks [n_picks, 3] i32 (selected point, class, rank; class 0..9 a bin, 10 the static pairs) ->
 *                               out_frame_pairs [n_picks, 2] i32 (frames[i], frames[j]).  A bin pick is entry (bin start + rank) of
 *                               the point's sorted segment, a static pick the rank-th static pair in row-major order.  picks_host
 *                               is the same table in host memory and class_counts_host [n_selected, 11] i32 the classes' sizes:
 *                               a pick outside them is MSPA_EINVAL, and nothing is launched.
 */
#define MSPA_TRACK_STAT_WORDS 6
#define MSPA_TRACK_CLASS_STATIC 10
int mspa_track_pair_stats(const double *world, const uint8_t *visibility, int32_t T, int32_t P, const int32_t *points,
                          int32_t n_points, double object_not_moving_threshold, double future_frame_windows,
                          int32_t *out_frames, double *out_positions, int64_t *out_stats, mspa_stream_t stream);
int mspa_track_pair_bin_counts(const int32_t *frames, const double *positions, const int64_t *stats, int32_t T, int32_t n_points,
                               const double *edges, double object_not_moving_threshold, double future_frame_windows,
                               int32_t *out_bin_counts, mspa_stream_t stream);
int mspa_track_pair_sort(uint64_t *keys, uint32_t *payload, const int64_t *seg_offsets, int64_t n_segments, int64_t n_total,
                         int32_t payload_ordered, mspa_stream_t stream);
int mspa_track_pair_order(const int32_t *frames, const double *positions, const int64_t *stats, int32_t T, int32_t n_points,
                          const int32_t *rows, const int64_t *seg_offsets, int32_t n_selected, int64_t n_total,
                          double object_not_moving_threshold, double future_frame_windows, uint64_t *keys, uint32_t *payload,
                          mspa_stream_t stream);
int mspa_track_pair_resolve(const int32_t *frames, const double *positions, const int64_t *stats, const int32_t *bin_counts, int32_t T,
                            int32_t n_points, const int32_t *rows, const int64_t *seg_offsets, int32_t n_selected,
                            const uint32_t *payload, int64_t n_total, const int32_t *picks_host, const int32_t *class_counts_host,
                            const int32_t *picks, int64_t n_picks, double object_not_moving_threshold, double future_frame_windows,
                            int32_t *out_frame_pairs, mspa_stream_t stream);

/*
 * K7 -- the accumulation inside rigid_body_segmentation (OM_C:49-92): cumulative_loss[i, j] = sum over
 * frames t >= 1 of |d_t(i,j) - d_{t-1}(i,j)| where that change exceeds smoothing_factor, d_t the Euclidean
 * distance between track points i and j at frame t.  The linkage / fcluster step that consumes it is
 * mspa_track_linkage below.   tracks_xyz [T, P, 3] f64 -> out_loss [P, P] f64 (symmetric, zero diagonal)
 * The batch form runs n_blocks equal-shape track blocks in one launch: tracks_xyz [n_blocks, T, P, 3] ->
 * out_loss [n_blocks, P, P], each block's matrix the one the single form writes.  n_blocks <= 65 535.
 */
int mspa_track_rigidity_loss(const double *tracks_xyz, int32_t T, int32_t P, double smoothing_factor,
                             double *out_loss, mspa_stream_t stream);
int mspa_track_rigidity_loss_batch(const double *tracks_xyz, int32_t n_blocks, int32_t T, int32_t P,
                                   double smoothing_factor, double *out_loss, mspa_stream_t stream);

/*
 * K7b -- the second half of rigid_body_segmentation (OM_C:80-92) for a batch of K7 matrices: SciPy's
 * linkage(squareform(loss, checks=False), method='average') (the nearest-neighbour chain, its tie rules, its
 * stable sort by height and its union-find relabelling) and fcluster(Z, threshold, criterion='distance'),
 * one workgroup per block.  Only the strict upper triangle of a block is read, as squareform does.
 *   loss [n_blocks, P, P] f64 (left untouched)  ->  out_Z [n_blocks, P-1, 4] f64, bit for bit SciPy's;
 *   out_labels [n_blocks, P] i32, value for value fcluster's;  out_status [n_blocks] i32:
 *   MSPA_LINKAGE_OK, MSPA_LINKAGE_NONFINITE (a NaN / inf in the block: SciPy raises ValueError there) or
 *   MSPA_LINKAGE_ITERATION_CAP (the chain loop reached 4 P scans: a bug indicator, never a normal outcome).
 *   A block whose status is not 0 has zeros in out_Z and out_labels; the other blocks are unaffected.
 * 2 <= P <= MSPA_LINKAGE_MAX_POINTS; P < 2 or n_blocks == 0 returns MSPA_OK with nothing written.
 * workspace: caller-owned, 16-byte aligned, >= mspa_track_linkage_workspace_bytes(n_blocks, P) bytes (the
 * working copy of every matrix; -1 for a bad argument); contents undefined afterwards.
 */
#define MSPA_LINKAGE_MAX_POINTS 2048
#define MSPA_LINKAGE_OK 0
#define MSPA_LINKAGE_NONFINITE 1
#define MSPA_LINKAGE_ITERATION_CAP 2
int64_t mspa_track_linkage_workspace_bytes(int64_t n_blocks, int32_t P);
int mspa_track_linkage(const double *loss, int64_t n_blocks, int32_t P, double threshold, double *out_Z,
                       int32_t *out_labels, int32_t *out_status, void *workspace, int64_t workspace_bytes,
                       mspa_stream_t stream);

/*
 * K8 -- per (object, image) extent of the object's visible vertices: what compute_coverage
 * (object_perception/single_object_coverage_finder.py:56-65) takes off `image mask & object mask`, for all
 * three axes at once.  The coverage of a union of images is max-of-max minus min-of-min of these, so the
 * minimal-combination search (COV:76-220) runs on them without ever forming a union mask.
 *   vis_bits [n_images, n_words] u64 (K1's bitsets, or rows packed from the visibility parquet),
 *   xyz [n_vertices, 3] f64 (axis-aligned scene points), objects as CSR: obj_offsets [n_objects+1] i32 into
 *   obj_vertices [n_list_entries] (vertex ids, each < n_vertices; n_list_entries = obj_offsets[n_objects])
 *   -> out_lo / out_hi [n_objects, n_images, 3] f64 (+inf / -inf where the image sees none of the object),
 *      out_count [n_objects, n_images] i32 (= intersection_count of compute_object_visibility.py:119-121)
 */
int mspa_object_extents(const uint64_t *vis_bits, int32_t n_images, int64_t n_words, const double *xyz,
                        int64_t n_vertices, const int32_t *obj_offsets, const int32_t *obj_vertices,
                        int64_t n_list_entries, int32_t n_objects, double *out_lo, double *out_hi, int32_t *out_count,
                        mspa_stream_t stream);

/*
 * K6a -- correspondence extraction on K1's bitsets: for every selection (image1, image2, j) the j-th
 * vertex (ascending index) visible in both images, i.e. element j of np.intersect1d(points1, points2)
 * (visual correspondence, VC_C:303-313); with image1 == image2 it is element j of that image's
 * visible-vertex list (depth heads, DE_C:190-198).  -1 when fewer than j+1 vertices qualify.
 *   bits [n_images, n_words] uint64,  selections [n, 3] int32,  out_vertex [n] int32
 */
int mspa_select_common_point(const uint64_t *bits, int32_t n_images, int64_t n_words,
                             const int32_t *selections, int64_t n, int32_t *out_vertex,
                             mspa_stream_t stream);

/*
 * K6b -- SceneInfoHandler.get_point_2d_coordinates_in_image (IH:291-305) for a batch of
 * (vertex, image) samples: un-rounded (u, v), camera depth and the check_point_visibility flag.
 *   xyz as in mspa_vertex_visibility; cam_mats [n_images, MSPA_CAM_MATS, 16]; depth [n_images, dh, dw]
 *   samples [n, 2] int32 (vertex, image);  out_uv [n, 2] f64, out_depth [n] f64, out_visible [n] u8
 */
int mspa_project_samples(const double *xyz, int64_t n_points, int64_t point_stride, int64_t comp_stride,
                         const double *cam_mats, int32_t n_images, const uint16_t *depth, int32_t dh,
                         int32_t dw, int32_t H, int32_t W, const int32_t *samples, int64_t n,
                         double *out_uv, double *out_depth, uint8_t *out_visible, mspa_stream_t stream);
/* ... with the handler's depth_value_scale (IH:368) instead of the default 0.001 */
int mspa_project_samples_ex(const double *xyz, int64_t n_points, int64_t point_stride, int64_t comp_stride,
                            const double *cam_mats, int32_t n_images, const uint16_t *depth, int32_t dh,
                            int32_t dw, int32_t H, int32_t W, double depth_value_scale, const int32_t *samples, int64_t n,
                            double *out_uv, double *out_depth, uint8_t *out_visible, mspa_stream_t stream);

/*
 * Frame sharpness (the reference's calculate_image_sharpness, OPS:22-34) -- csrc/image_ops.hip.
 *
 * mspa_jpeg_decode_luma_device   arguments, workspace (mspa_jpeg_workspace_bytes) and status codes of mspa_jpeg_decode_device,
 *                                but out_dev[k] is [h, w] uint8: component 0 after the IDCT at the image's size -- libjpeg's
 *                                JCS_GRAYSCALE output, what cv2.imread(IMREAD_GRAYSCALE) and Pillow's draft("L") return for a
 *                                baseline greyscale or YCbCr file.
 * mspa_laplacian_blocks          the number of row blocks B of one [h, w] image (-1: bad size).
 * mspa_laplacian_moments_device  luma_dev [n, h, w] uint8 -> partials_dev [n, B, 2] int64: per image and row block the sum and
 *                                the sum of squares of L = I(y-1,x) + I(y+1,x) + I(y,x-1) + I(y,x+1) - 4 I(y,x), borders
 *                                reflect-101 (cv2.Laplacian(img, CV_64F) with its defaults).  Exact integers, no atomics.
 */
int mspa_jpeg_decode_luma_device(const void *src_dev, const int64_t *src_offsets_dev, const int64_t *src_bytes_dev, int64_t src_capacity,
                                 const void *desc_dev, int64_t n_images, int32_t h, int32_t w, uint8_t *out_dev, int32_t *status_dev,
                                 void *workspace, int64_t workspace_bytes, mspa_stream_t stream);
int32_t mspa_laplacian_blocks(int32_t h, int32_t w);
int mspa_laplacian_moments_device(const uint8_t *luma_dev, int64_t n, int32_t h, int32_t w, int64_t *partials_dev, mspa_stream_t stream);

/*
 * Exact k-nearest mean distance (the quantity behind Open3D's remove_statistical_outlier, OPS:138-160) -- csrc/cloud_ops.hip,
 * rule in csrc/knn_grid_core.h.  mean[i] = the mean of the Euclidean distances from point i to its min(k, n) nearest points,
 * point i itself included at distance 0, summed in ascending order in float64.  1 <= k <= MSPA_KNN_MAX_K, n <= 2^30, finite
 * coordinates.  The ordering of the points by cell is the caller's sort, so the device form is three calls:
 *   mspa_knn_grid_host             box lo[3] <= hi[3] (per-axis order statistics of the cloud), n, k -> grid record
 *                                  (MSPA_KNN_GRID_BYTES, host memory); points outside the box fall into its border cells.
 *   mspa_knn_cells_device          xyz_dev [n, 3] f64 -> cells_dev [n] int32.  The caller sorts them STABLY and passes the
 *                                  permutation on as order_dev [n] int64.
 *   mspa_knn_mean_distance_device  -> mean_dev [n] f64 and, when evals_dev is not null, the distances evaluated per point
 *                                  [n] int32.  An order_dev that is no such permutation gives wrong means, never an access
 *                                  outside the buffers.  workspace: mspa_knn_workspace_bytes(n, k), 16-byte aligned.
 *   mspa_knn_mean_distance_host    the same search on the CPU through the same header (box: ranks n / 100 and n - 1 - n / 100).
 */
#define MSPA_KNN_GRID_BYTES 112
#define MSPA_KNN_MAX_K 64
int mspa_knn_grid_host(const double *lo, const double *hi, int64_t n, int32_t k, void *grid_out);
int64_t mspa_knn_workspace_bytes(int64_t n, int32_t k);
int mspa_knn_cells_device(const double *xyz_dev, int64_t n, const void *grid_host, int32_t *cells_dev, mspa_stream_t stream);
int mspa_knn_mean_distance_device(const double *xyz_dev, int64_t n, int32_t k, const void *grid_host, const int64_t *order_dev,
                                  double *mean_dev, int32_t *evals_dev, void *workspace, int64_t workspace_bytes, mspa_stream_t stream);
int mspa_knn_mean_distance_host(const double *xyz_host, int64_t n, int32_t k, double *mean_host, int32_t *evals_host);

/*
 * The same search and the statistical-outlier rule for a RAGGED BATCH of clouds in a fixed number of launches -- csrc/cloud_segments.hip,
 * rule in csrc/cloud_segments_core.h on top of csrc/knn_grid_core.h.  A batch is xyz [N, 3] f64 plus offsets [S + 1] int64
 * (offsets[0] = 0, ascending, offsets[S] = N <= 2^30, S <= MSPA_SEGMENTS_MAX); segment s is the rows offsets[s] .. offsets[s + 1],
 * empty segments allowed anywhere.  Per segment the grid is the one mspa_knn_grid_host builds for that cloud alone, so mean and
 * evals equal mspa_knn_mean_distance_device's on the segment bit for bit.  Every device entry point takes the offsets (and the
 * grids) TWICE: the host copy, which it checks before anything is enqueued, and the device copy the kernels read, which the caller
 * uploads and which must hold the same bytes.
 *   mspa_knn_segments_tables_host          offsets, k -> cell_base [S + 1] int64: the exclusive prefix of the most cells a
 *                                          non-empty segment's grid can have.  A row's sort key is cell_base[s] + its cell.
 *   mspa_knn_segments_grids_host           boxes lo / hi [S, 3] (per-axis order statistics of rank n_s / 100 and n_s - 1 - n_s / 100
 *                                          of each segment; an empty segment's box is not read) -> grids [S] records of
 *                                          MSPA_KNN_GRID_BYTES (an empty segment's: zeros).
 *   mspa_knn_segments_cells_device         -> keys_dev [N] int64, monotone in the segment.  The caller sorts them STABLY and passes
 *                                          the permutation on as order_dev [N] int64.
 *   mspa_knn_segments_mean_distance_device -> mean_dev [N] f64 and, when evals_dev is not null, the distances evaluated per row
 *                                          [N] int32.  Every entry of order_dev is clamped into [0, N) and then into the segment
 *                                          of its slot: an order_dev that is no such permutation gives wrong means, never an access
 *                                          outside the buffers.  workspace: mspa_knn_segments_workspace_bytes(), 16-byte aligned.
 *   mspa_outlier_segments_device           avg_dev [N], xyz_dev [N, 3] -> keep_dev [N] uint8 (1: the row stays) and per segment
 *                                          kept_dev [S] int64, mean_dev / sd_dev / thr_dev [S] f64, lo_dev / hi_dev [S, 3] f64, the
 *                                          extents of the kept rows (+inf / -inf where none stays).  With P the rows of a segment of
 *                                          n whose avg > 0: mean = sum_P avg / n, sd = sqrt(sum_P (avg - mean)^2 / (n - 1)), thr =
 *                                          mean + std_ratio * sd, a row stays iff 0 < avg < thr; n = 0 has no mean, n < 2 no sd and no
 *                                          thr (one quiet NaN) and keeps nothing.  The two sums are taken in the order
 *                                          csrc/cloud_segments_core.h states (256 lane sums, folded by halving strides): not
 *                                          torch.sum's.  One workgroup per segment, no atomics.
 *   mspa_knn_segments_mean_distance_host,
 *   mspa_outlier_segments_host             the same two steps on the CPU through the same headers: the device's twins for tests on a
 *                                          machine without a GPU, not a fallback.
 */
#define MSPA_SEGMENTS_MAX (1 << 24)
int mspa_knn_segments_tables_host(const int64_t *offsets_host, int64_t S, int32_t k, int64_t *cell_base_out);
int mspa_knn_segments_grids_host(const double *lo, const double *hi, const int64_t *offsets_host, int64_t S, int32_t k, void *grids_out);
int64_t mspa_knn_segments_workspace_bytes(const int64_t *offsets_host, int64_t S, int32_t k);
int mspa_knn_segments_cells_device(const double *xyz_dev, const int64_t *offsets_host, int64_t S, const void *grids_host,
                                   const int64_t *offsets_dev, const void *grids_dev, const int64_t *cell_base_dev, int64_t *keys_dev,
                                   mspa_stream_t stream);
int mspa_knn_segments_mean_distance_device(const double *xyz_dev, const int64_t *offsets_host, int64_t S, int32_t k, const void *grids_host,
                                           const int64_t *offsets_dev, const void *grids_dev, const int64_t *cell_base_dev,
                                           const int64_t *order_dev, double *mean_dev, int32_t *evals_dev, void *workspace,
                                           int64_t workspace_bytes, mspa_stream_t stream);
int mspa_outlier_segments_device(const double *avg_dev, const double *xyz_dev, const int64_t *offsets_host, int64_t S, double std_ratio,
                                 const int64_t *offsets_dev, uint8_t *keep_dev, int64_t *kept_dev, double *mean_dev, double *sd_dev,
                                 double *thr_dev, double *lo_dev, double *hi_dev, mspa_stream_t stream);
int mspa_knn_segments_mean_distance_host(const double *xyz_host, const int64_t *offsets_host, int64_t S, int32_t k, double *mean_host,
                                         int32_t *evals_host);
int mspa_outlier_segments_host(const double *avg_host, const double *xyz_host, const int64_t *offsets_host, int64_t S, double std_ratio,
                               uint8_t *keep_host, int64_t *kept_host, double *mean_host, double *sd_host, double *thr_host,
                               double *lo_host, double *hi_host);

/*
 * NEAREST-POINT DISTANCES BETWEEN THE CLOUDS OF TWO RAGGED BATCHES -- csrc/cloud_distance.hip, rule in csrc/cloud_distance_core.h on top
 * of csrc/cloud_segments_core.h and csrc/knn_grid_core.h.  The targets are one batch (t_xyz [Nt, 3] f64, t_offsets [St + 1]), the
 * queries another (q_xyz [Nq, 3] f64, q_offsets [Sq + 1]); pairs [P, 2] int64 names, per pair, the query segment and the target
 * segment it is searched in (null: Sq == St == P and pair s is (s, s)); a segment may stand in any number of pairs.  The output rows
 * lie back to back by pair: out_offsets [P + 1] with out_offsets[p + 1] - out_offsets[p] = the rows of query segment pairs[p][0], at
 * most MSPA_CLOUD_DISTANCE_MAX_ROWS rows and MSPA_CLOUD_DISTANCE_MAX_PAIRS pairs.  Per output row: distance = sqrt(min over the target
 * segment of (dx * dx + dy * dy) + dz * dz), index = the row of t_xyz that attains it, the lowest among equal ones; +inf and -1 for an
 * empty target segment; NaN and -1 for a query row with a non-finite coordinate.  max_distance (finite, > 0; +inf: no cap): a row
 * whose minimum squared distance exceeds max_distance * max_distance reports +inf and -1, every other row what it reports without a
 * cap.  The bits are those of a brute force over all rows.  Every device entry point takes each host table TWICE, as the entries
 * above do, and checks all arguments before it enqueues anything; zero output rows enqueue nothing.
 *   mspa_knn_segments_index_device   the search structure of a batch, in caller-owned buffers: pts_dev [N, 3] (the rows by key),
 *                                    sorted_keys_dev [N] and starts_dev [starts_slots] int32, starts_slots >= the batch's cell_base[S] +
 *                                    S.  order_dev is the stable sort of mspa_knn_segments_cells_device's keys; the grids are
 *                                    mspa_knn_segments_grids_host's for k.  The gather and the starts launches of
 *                                    mspa_knn_segments_mean_distance_device, nothing else.
 *   mspa_cloud_distance_device       -> distance_dev [M] f64 and, where not null, index_dev [M] int64 and evals_dev [M] int32 (the
 *                                    distances each row evaluated).  t_pts_dev, t_starts_dev [t_starts_slots], t_order_dev: an index built with grid_k
 *                                    (MSPA_CLOUD_DISTANCE_GRID_K is the library's choice; results do not depend on it).  MSPA_EINVAL
 *                                    for a null pointer where a count is positive, bad offsets, a pair outside [0, Sq) x [0, St),
 *                                    out_offsets that do not follow from the pairs, grids that are not grids_host's, a cap outside
 *                                    its domain or a misaligned buffer.  Every device table entry a lane indexes with is clamped:
 *                                    corrupt device tables give wrong distances, never an access outside the buffers.
 *                                    perm_dev [M] (null: lane i takes output row i): a permutation of the output rows, the sort
 *                                    of mspa_cloud_distance_keys_device's keys; it decides which lane computes a row, never what the
 *                                    row holds.  Its entries are clamped into [0, M).
 *   mspa_cloud_distance_keys_device  -> keys_dev [M] int64: (pair << 31) + the query row's cell in its target segment's grid.
 *   mspa_cloud_distance_fit_device   distance_dev [M], out_offsets [P + 1] -> per pair rows_dev, finite_dev (d < inf), within_dev
 *                                    (d <= tau; tau finite, >= 0) [P] int64 and sum_dev, sum_sq_dev (of d and d * d over the finite
 *                                    rows, in the order csrc/cloud_segments_core.h states: 256 lane sums folded by halving strides),
 *                                    max_dev (the largest finite d, -inf where none) [P] f64.  One workgroup per pair, no atomics.
 *   mspa_cloud_distance_host,
 *   mspa_cloud_distance_fit_host     the same two steps on the CPU through the same headers, from the unsorted targets: the device's
 *                                    twins for tests on a machine without a GPU, not a fallback.
 */
#define MSPA_CLOUD_DISTANCE_MAX_ROWS (1 << 30)
#define MSPA_CLOUD_DISTANCE_MAX_PAIRS (1 << 24)
#define MSPA_CLOUD_DISTANCE_GRID_K 1
int mspa_knn_segments_index_device(const double *xyz_dev, const int64_t *offsets_host, int64_t S, int32_t k, const void *grids_host,
                                   const int64_t *offsets_dev, const void *grids_dev, const int64_t *cell_base_dev, const int64_t *order_dev,
                                   double *pts_dev, int64_t *sorted_keys_dev, int32_t *starts_dev, int64_t starts_slots, mspa_stream_t stream);
int mspa_cloud_distance_device(const double *t_pts_dev, const int32_t *t_starts_dev, int64_t t_starts_slots, const int64_t *t_order_dev,
                               const int64_t *t_offsets_host, int64_t St, int32_t grid_k, const void *grids_host, const int64_t *t_offsets_dev, const void *grids_dev,
                               const int64_t *cell_base_dev, const double *q_xyz_dev, const int64_t *q_offsets_host, int64_t Sq,
                               const int64_t *q_offsets_dev, const int64_t *pairs_host, const int64_t *pairs_dev, int64_t P,
                               const int64_t *out_offsets_host, const int64_t *out_offsets_dev, const int64_t *perm_dev, double max_distance,
                               double *distance_dev, int64_t *index_dev, int32_t *evals_dev, mspa_stream_t stream);
int mspa_cloud_distance_keys_device(const int64_t *t_offsets_host, int64_t St, int32_t grid_k, const void *grids_host, const void *grids_dev,
                                    const double *q_xyz_dev, const int64_t *q_offsets_host, int64_t Sq, const int64_t *q_offsets_dev,
                                    const int64_t *pairs_host, const int64_t *pairs_dev, int64_t P, const int64_t *out_offsets_host,
                                    const int64_t *out_offsets_dev, int64_t *keys_dev, mspa_stream_t stream);
int mspa_cloud_distance_fit_device(const double *distance_dev, const int64_t *out_offsets_host, int64_t P, double tau,
                                   const int64_t *out_offsets_dev, int64_t *rows_dev, int64_t *finite_dev, int64_t *within_dev, double *sum_dev,
                                   double *sum_sq_dev, double *max_dev, mspa_stream_t stream);
int mspa_cloud_distance_host(const double *t_xyz_host, const int64_t *t_offsets_host, int64_t St, int32_t grid_k, const double *q_xyz_host,
                             const int64_t *q_offsets_host, int64_t Sq, const int64_t *pairs_host, int64_t P, const int64_t *out_offsets_host,
                             double max_distance, double *distance_host, int64_t *index_host, int32_t *evals_host);
int mspa_cloud_distance_fit_host(const double *distance_host, const int64_t *out_offsets_host, int64_t P, double tau, int64_t *rows_host,
                                 int64_t *finite_host, int64_t *within_host, double *sum_host, double *sum_sq_host, double *max_host);

/*
 * RIGID ALIGNMENT OF THE CLOUDS OF TWO RAGGED BATCHES (Kabsch / Horn, and the two steps point-to-point ICP adds to the search above) --
 * csrc/cloud_align.hip, rule in csrc/cloud_align_core.h on top of csrc/cloud_distance_core.h.  The batches, pairs [P, 2] and out_offsets
 * [P + 1] are the search's.  A transform is 12 f64: R row-major, then t; y_a = ((R_a0 * x + R_a1 * y) + R_a2 * z) + t_a.  Output row i of
 * pair p carries index[i], a row of t_xyz [Nt, 3] or -1 (clamped into [-1, Nt) before use); it is used when that is >= 0 and its query
 * row is finite.  Per pair: the counts and centroids of the used rows, the nine centred sums S_ab (both passes in the order
 * csrc/cloud_segments_core.h states), Horn's symmetric 4 x 4 matrix, MSPA_CLOUD_ALIGN_SWEEPS cyclic Jacobi sweeps in a fixed pivot
 * order, R from the unit quaternion of the largest eigenvalue and t = pc - R qc.  status: MSPA_CLOUD_ALIGN_OK; _FEW (fewer than 3 used
 * rows); _DEGENERATE (l1 - l2 <= 2^MSPA_CLOUD_ALIGN_GAP_EXPONENT * (l1 - l4): collinear or coincident rows).  A pair that is not OK
 * leaves with the transform of init.  Equal correspondences give equal bits.  Every device entry point takes each host table TWICE
 * and checks all arguments before it enqueues anything; every device table entry a lane indexes with is clamped.
 *   mspa_cloud_align_transform_device  -> out_dev [M, 3] f64, the query rows of every pair under transform_dev [P, 12], in output-row
 *                                      order.  One launch; nothing is enqueued for M == 0.  St only bounds the pairs' second column.
 *   mspa_cloud_align_fit_device        index_dev [M], init_dev [P, 12] -> transform_dev [P, 12] (may be init_dev), used_dev [P] int64,
 *                                      status_dev [P] int32 and, where not null, eigen_dev [P, 4] (descending) and converged_dev [P]
 *                                      int64, in and out: an entry of -1 becomes `iteration` where the transform written equals init
 *                                      bit for bit.  moments_dev [P, 16] f64 is workspace (used, qc, pc, S afterwards).  Two launches:
 *                                      one workgroup of 256 per pair for the sums, one lane per pair for the solve; no atomics.
 *                                      Nothing is enqueued for P == 0.  MSPA_EINVAL for a null pointer where a count is positive,
 *                                      bad offsets, a pair outside [0, Sq) x [0, St), out_offsets that do not follow from the pairs,
 *                                      Nt outside [0, 2^30], a negative iteration or a misaligned buffer.
 *   mspa_cloud_align_transform_host,
 *   mspa_cloud_align_fit_host          the same on the CPU through the same header: the device's twins for tests, not a fallback.
 */
#define MSPA_CLOUD_ALIGN_OK 0
#define MSPA_CLOUD_ALIGN_FEW 1
#define MSPA_CLOUD_ALIGN_DEGENERATE 2
#define MSPA_CLOUD_ALIGN_SWEEPS 12
#define MSPA_CLOUD_ALIGN_GAP_EXPONENT (-26)
int mspa_cloud_align_transform_device(const double *q_xyz_dev, const int64_t *q_offsets_host, int64_t Sq, const int64_t *q_offsets_dev, int64_t St,
                                      const int64_t *pairs_host, const int64_t *pairs_dev, int64_t P, const int64_t *out_offsets_host,
                                      const int64_t *out_offsets_dev, const double *transform_dev, double *out_dev, mspa_stream_t stream);
int mspa_cloud_align_fit_device(const double *q_xyz_dev, const int64_t *q_offsets_host, int64_t Sq, const int64_t *q_offsets_dev,
                                const double *t_xyz_dev, int64_t Nt, int64_t St, const int64_t *pairs_host, const int64_t *pairs_dev, int64_t P,
                                const int64_t *out_offsets_host, const int64_t *out_offsets_dev, const int64_t *index_dev, const double *init_dev,
                                int64_t iteration, double *moments_dev, double *transform_dev, int64_t *used_dev, int32_t *status_dev,
                                double *eigen_dev, int64_t *converged_dev, mspa_stream_t stream);
int mspa_cloud_align_transform_host(const double *q_xyz_host, const int64_t *q_offsets_host, int64_t Sq, int64_t St, const int64_t *pairs_host,
                                    int64_t P, const int64_t *out_offsets_host, const double *transform_host, double *out_host);
int mspa_cloud_align_fit_host(const double *q_xyz_host, const int64_t *q_offsets_host, int64_t Sq, const double *t_xyz_host, int64_t Nt, int64_t St,
                              const int64_t *pairs_host, int64_t P, const int64_t *out_offsets_host, const int64_t *index_host,
                              const double *init_host, int64_t iteration, double *transform_host, int64_t *used_host, int32_t *status_host,
                              double *eigen_host, int64_t *converged_host);

/*
 * THE K NEAREST ROWS AND THE NORMAL OF EVERY ROW OF A RAGGED BATCH -- csrc/cloud_normals.hip, rule in csrc/cloud_normals_core.h on top of
 * csrc/cloud_distance_core.h.  The batch is xyz [N, 3] f64 with offsets [S + 1]; 1 <= k <= 64.  The neighbours of a row are the
 * min(k, n_s) rows of its own segment with the smallest (d2, row), d2 = (dx * dx + dy * dy) + dz * dz, the row itself among them;
 * with max_distance (finite, > 0; +inf: no cap) only rows with d2 <= max_distance * max_distance.  used [N] int32 is their number.
 * The neighbour table (nbr_index [N, k] int64, rows of the batch, -1 behind used; nbr_distance [N, k] f64 = sqrt(d2), +inf behind
 * used) holds them in ascending (d2, row) order: the bits of a brute force.  The fit: the centroid and the six centred sums over the
 * neighbours in that order, MSPA_CLOUD_NORMALS_SWEEPS cyclic Jacobi sweeps over (0,1) (0,2) (1,2), the normalised column of the
 * smallest eigenvalue with its first non-zero component positive, negated where a viewpoint of the segment (viewpoints [S, 3], a
 * non-finite row: none; null: none anywhere) sees it from behind: ((v - p) . n) < 0.  curvature [N] = l0 / ((l0 + l1) + l2).  status
 * [N] uint8: MSPA_CLOUD_NORMALS_OK; _FEW (used < 3); _DEGENERATE (l1 - l0 <= 2^MSPA_CLOUD_NORMALS_GAP_EXPONENT * (l2 - l0): collinear,
 * coincident or isotropic neighbours); a row that is not OK has a NaN normal and curvature.  The two output groups -- normal, curvature
 * and status; nbr_index and nbr_distance -- are null together or not at all, and at least one is asked for.
 *   mspa_cloud_normals_device  pts_dev, starts_dev [starts_slots], order_dev: mspa_knn_segments_index_device's tables for the same k.
 *                              One launch, one lane per row, no atomics; the table is a second output of the same walk.  Takes each
 *                              host table TWICE and checks all arguments before it enqueues anything; nothing is enqueued for N == 0.
 *                              MSPA_EINVAL for a null pointer where a count is positive, bad offsets, k outside its range, grids that
 *                              are not grids_host's, a cap outside its domain, too few starts slots or a misaligned buffer.  Every
 *                              device table entry a lane indexes with is clamped: corrupt device tables give wrong normals, never an
 *                              access outside the buffers.
 *   mspa_cloud_normals_host    the same on the CPU through the same headers, from the unsorted rows (non-finite coordinates are
 *                              MSPA_EINVAL): the device's twin for tests on a machine without a GPU, not a fallback.
 */
#define MSPA_CLOUD_NORMALS_OK 0
#define MSPA_CLOUD_NORMALS_FEW 1
#define MSPA_CLOUD_NORMALS_DEGENERATE 2
#define MSPA_CLOUD_NORMALS_SWEEPS 8
#define MSPA_CLOUD_NORMALS_GAP_EXPONENT (-26)
int mspa_cloud_normals_device(const double *pts_dev, const int32_t *starts_dev, int64_t starts_slots, const int64_t *order_dev,
                              const int64_t *offsets_host, int64_t S, int32_t k, const void *grids_host, const int64_t *offsets_dev,
                              const void *grids_dev, const int64_t *cell_base_dev, double max_distance, const double *viewpoints_dev,
                              double *normal_dev, double *curvature_dev, int32_t *used_dev, uint8_t *status_dev, int64_t *nbr_index_dev,
                              double *nbr_distance_dev, mspa_stream_t stream);
int mspa_cloud_normals_host(const double *xyz_host, const int64_t *offsets_host, int64_t S, int32_t k, double max_distance,
                            const double *viewpoints_host, double *normal_host, double *curvature_host, int32_t *used_host,
                            uint8_t *status_host, int64_t *nbr_index_host, double *nbr_distance_host);

/*
 * ONE LINEARISED POINT-TO-PLANE STEP PER PAIR -- csrc/cloud_align_plane.hip, rule in csrc/cloud_align_plane_core.h on top of
 * csrc/cloud_align_core.h: what point-to-plane ICP puts in the place of mspa_cloud_align_fit_*.  The batches, pairs, out_offsets, index
 * and the 12 f64 of a transform are that entry's; t_normals [Nt, 3] f64 are the targets' normals (mspa_cloud_normals_*).  With T = init
 * of the pair, y = T q; a row is used when its clamped index is >= 0, its query row is finite and its target row's normal is finite.
 * Per pair: used and the centroid c of the used y; with a = [(y - c) x n, n] and r = (y - p) . n the 21 + 6 + 1 sums of a a^T, a r
 * and r r (both passes in the order csrc/cloud_segments_core.h states); (A^T A) x = -(A^T r) by a written-out L D L^T; the new rotation
 * from the unit quaternion of init's R multiplied by the step's (1, x0 / 2, x1 / 2, x2 / 2) and normalised -- max |R^T R - I| stays
 * within 32 * 2^-53 after any number of steps -- and the translation about c.  status: MSPA_CLOUD_ALIGN_OK; _FEW (fewer than 6 used
 * rows); _DEGENERATE (a pivot <= 2^MSPA_CLOUD_ALIGN_GAP_EXPONENT * the largest diagonal entry, or not finite: a flat target).  A pair
 * that is not OK, and a step that is exactly zero, leave with the 12 f64 of init bit for bit.
 *   mspa_cloud_align_plane_fit_device  index_dev [M], init_dev [P, 12] -> transform_dev [P, 12] (may be init_dev), used_dev [P] int64,
 *                                      status_dev [P] int32 and, where not null, rmse_dev [P] (sqrt(r r / used) under init, NaN where
 *                                      nothing is used) and converged_dev [P] int64, in and out, as mspa_cloud_align_fit_device's.
 *                                      moments_dev [P, 32] f64 is workspace, a buffer of its own.  Two launches: one workgroup of 256
 *                                      per pair for the sums, one lane per pair for the solve; no atomics.  Takes each host table
 *                                      TWICE and checks all arguments before it enqueues anything; nothing is enqueued for P == 0;
 *                                      every device table entry a lane indexes with is clamped.  MSPA_EINVAL as
 *                                      mspa_cloud_align_fit_device's.
 *   mspa_cloud_align_plane_fit_host    the same on the CPU through the same header: the device's twin for tests, not a fallback.
 */
int mspa_cloud_align_plane_fit_device(const double *q_xyz_dev, const int64_t *q_offsets_host, int64_t Sq, const int64_t *q_offsets_dev,
                                      const double *t_xyz_dev, const double *t_normals_dev, int64_t Nt, int64_t St, const int64_t *pairs_host,
                                      const int64_t *pairs_dev, int64_t P, const int64_t *out_offsets_host, const int64_t *out_offsets_dev,
                                      const int64_t *index_dev, const double *init_dev, int64_t iteration, double *moments_dev,
                                      double *transform_dev, int64_t *used_dev, int32_t *status_dev, double *rmse_dev, int64_t *converged_dev,
                                      mspa_stream_t stream);
int mspa_cloud_align_plane_fit_host(const double *q_xyz_host, const int64_t *q_offsets_host, int64_t Sq, const double *t_xyz_host,
                                    const double *t_normals_host, int64_t Nt, int64_t St, const int64_t *pairs_host, int64_t P,
                                    const int64_t *out_offsets_host, const int64_t *index_host, const double *init_host, int64_t iteration,
                                    double *transform_host, int64_t *used_host, int32_t *status_host, double *rmse_host, int64_t *converged_host);

/*
 * Instance-mask decode ON THE DEVICE (csrc/mask_ingest.hip, rule in csrc/png_unfilter8_core.h): the 8-bit twin of the depth-frame
 * decode above, for ScanNet's `instance-filt/<image>.png` label images (`cv2.imread(path, -1)` per (image, object) in the
 * reference's get_instance_mask).  The inflate in front of the un-filter is mspa_inflate_blocks_device with block_bytes = h * (w + 1).
 *
 * mspa_png_pack_idat8_host    mspa_png_pack_idat_host for 8-bit greyscale (bit depth 8, colour type 0), non-interlaced h x w PNG
 *   files: the same two-call contract, offsets and status codes (0 packed; 1 unreadable; 2 another pixel format or size; 3 corrupt
 *   chunk structure).
 * mspa_png_unfilter8_device   n_images inflated scanline blocks (h rows of 1 filter byte + w sample bytes, image k at raw_dev + k *
 *   raw_pitch) -> out_dev[k, h, w] uint8: the five PNG row filters undone with bytes-per-pixel 1.  Images whose status_dev[k] is
 *   non-zero on entry are skipped; an image with a filter byte > 4 gets status 3 and is not written.  raw_pitch >= h * (w + 1) and a
 *   multiple of 4, raw_dev 4-byte aligned (MSPA_EINVAL otherwise).  Every well-formed image is decoded: nothing is declined.
 * mspa_png_unfilter8_host     the same rule from the same header on the CPU (no alignment requirement).
 */
int mspa_png_pack_idat8_host(const char *const *paths_host, int64_t n_files, int32_t h, int32_t w, void *dst_host,
                             int64_t dst_capacity, int64_t *offsets_host, int64_t *bytes_host, int32_t *status_host,
                             int64_t *capacity_needed, int32_t n_threads);
int mspa_png_unfilter8_device(const void *raw_dev, int64_t raw_pitch, int64_t n_images, int32_t h, int32_t w, uint8_t *out_dev,
                              int32_t *status_dev, mspa_stream_t stream);
int mspa_png_unfilter8_host(const void *raw_host, int64_t raw_pitch, int64_t n_images, int32_t h, int32_t w, uint8_t *out_host,
                            int32_t *status_host);

/*
 * Stable split of a batch of frames' valid pixels by instance label (csrc/instance_split.hip, rule and decomposition in
 * csrc/instance_split_core.h): the per-object clouds of `project_image_to_3d_with_mask(get_instance_mask(...))` for EVERY object
 * of every frame from one K3 exact pass per frame.  labels [F, P] uint8 (P = H * W colour pixels, row-major; 0 = nothing, object
 * `target_id` is label `target_id + 1`), valid = K3 exact's valid_u8 [F, P], xyz_f64 = its [F, P, 3], rgb optionally [F, H, W, 3]
 * uint8.  A pixel is selected when label != 0 and valid != 0.  F <= 65535, P < 2^31.  All buffers are the caller's:
 *   mspa_instance_split_workspace_bytes   the workspace of both calls (4-byte aligned); -1 for sizes out of range.
 *   mspa_instance_split_count             out_counts [F, 256] int32: selected pixels per (frame, label); the workspace receives
 *                                         what the second call needs (per-tile positions).
 *   mspa_instance_split_scatter           offsets [F * 256 + 1] int64 = the exclusive prefix of out_counts in (frame, label) order
 *                                         (the caller's scan), workspace as the first call left it.  Writes out_xyz [total, 3] f64,
 *                                         out_rgb [total, 3] u8 (rgb and out_rgb both given or both null) and out_pixel [total]
 *                                         int32 (the pixel index my * W + mx).  THE ORDER IS THE CONTRACT: segment (f, v) occupies
 *                                         rows offsets[f * 256 + v] .. and holds its pixels in ascending pixel index (np.where(mask)
 *                                         order), whatever order the hardware runs the workgroups in.  out_lo / out_hi [F, 256, 3]
 *                                         f64: the segment's per-axis minimum / maximum, +inf / -inf where it is empty (the sign of
 *                                         a zero extremum is unspecified when both zeros occur).
 *   mspa_instance_split_host              the same decomposition on the CPU through the same header (tests; the arrays are host
 *                                         memory).  Fills out_counts, out_offsets [F * 256 + 1] and, unless out_xyz is null (the
 *                                         size-only first call), everything the scatter writes.  workspace: the same size, int32.
 *                                         reversed != 0 walks tiles and waves in the opposite order: the output does not change.
 */
int64_t mspa_instance_split_workspace_bytes(int64_t F, int64_t P);
int mspa_instance_split_count(const uint8_t *labels, const uint8_t *valid, int64_t F, int64_t P, int32_t *out_counts, void *workspace,
                              int64_t workspace_bytes, mspa_stream_t stream);
int mspa_instance_split_scatter(const uint8_t *labels, const uint8_t *valid, const double *xyz_f64, const uint8_t *rgb_or_null,
                                int64_t F, int64_t P, int32_t H, int32_t W, const int64_t *offsets, const void *workspace,
                                double *out_xyz, uint8_t *out_rgb, int32_t *out_pixel, double *out_lo, double *out_hi,
                                mspa_stream_t stream);
int mspa_instance_split_host(const uint8_t *labels, const uint8_t *valid, const double *xyz_f64, const uint8_t *rgb_or_null, int64_t F,
                             int64_t P, int32_t *out_counts, int64_t *out_offsets, int32_t *workspace, double *out_xyz,
                             uint8_t *out_rgb, int32_t *out_pixel, double *out_lo, double *out_hi, int32_t reversed);

/*
 * Voxel-grid down-sampling of a RAGGED BATCH of clouds (csrc/voxel_segments.hip, rule in csrc/voxel_grid_core.h): one output row
 * per occupied voxel of every segment, every column the mean over the voxel's rows, plus the voxel's row count.  The rule restates
 * Open3D's voxel_down_sample as the maintainers recall it and is NOT checked against Open3D.  A batch is rows [N, C] f64 (xyz
 * first, 3 <= C <= MSPA_VOXEL_MAX_COLUMNS) plus offsets [S + 1] int64 (offsets[0] = 0, ascending, offsets[S] = N <= 2^30, S <=
 * MSPA_SEGMENTS_MAX).  Per segment and axis: min_bound = lo - voxel_size * 0.5 (lo the segment's minimum), idx = floor((p -
 * min_bound) / voxel_size) < 2^21, key = ix << 42 | iy << 21 | iz.  Output: segments in order, voxels in ascending key order; a
 * voxel's rows are summed in ascending input row index, sequentially for a run of m <= 64 rows and, for m > 64, as 64 lane sums
 * (lane j: rows j, j + 64, ...) folded by strides 32 .. 1; mean = sum / m.  The same bits on every run: no atomic places a row or
 * takes part in a sum.
 * Every device entry point takes the offsets TWICE, as the segmented search does: the host copy, which it checks together with all
 * other arguments before anything is enqueued (MSPA_EINVAL: null pointer, offsets that descend or do not start at 0, N > 2^30,
 * S > 2^24, C out of range, voxel_size not positive and finite, workspace too small or misaligned), and the device copy the
 * kernels read.  ALIGNMENT: workspace 16 bytes; every other buffer its element's size (f64 and int64: 8, int32: 4).
 *   mspa_voxel_segments_tables_host    offsets -> tile_base [S + 1] int64: the exclusive prefix of ceil(n_s / 4096), the tiles the
 *                                      extents pass cuts each segment into (so one huge segment does not serialise it).
 *   mspa_voxel_segments_workspace_bytes  the one workspace of the three device calls (-1 for offsets that are no batch).  The
 *                                      calls hand their intermediate tables to each other in it: pass the same bytes on.
 *   mspa_voxel_segments_keys_device    -> keys_dev [N] int64 and segment_dev [N] int32 (the row's segment), and seg_voxels_dev
 *                                      [S + 1] int32 zeroed, whose LAST word is the flag word: bit 0 a non-finite xyz, bit 1 an
 *                                      index >= 2^21.  Such a row gets a clamped key, so nothing downstream indexes outside a
 *                                      buffer.  The caller sorts the rows STABLY by key and then STABLY by segment and passes the
 *                                      permutation on as order_dev [N] int64.
 *   mspa_voxel_segments_heads_device   keys_dev, order_dev -> seg_voxels_dev[0 .. S): the occupied voxels of each segment.  A sorted
 *                                      slot opens a voxel when it is the first of its segment or its key differs from its
 *                                      predecessor's.  Every entry of order_dev is clamped into [0, N) and then into the segment
 *                                      of its slot: an order_dev that is no such permutation gives wrong voxels, never an access
 *                                      outside the buffers.  The caller reads seg_voxels_dev back (counts and flag word at once);
 *                                      M is the sum of the counts.
 *   mspa_voxel_segments_means_device   the same order_dev and workspace, M -> out_rows_dev [M, C] f64 and out_counts_dev [M] int32.
 *                                      Voxels beyond those the heads call found (an M that is too large) are not written.
 *   mspa_voxel_segments_host           the whole op on the CPU through the same header: the device's twin for tests and for
 *                                      NumPy input, not a fallback.  out_rows_host [N, C] and out_counts_host [N] are sized for
 *                                      the worst case and receive M = out_offsets_host[S] rows; out_offsets_host [S + 1];
 *                                      *flags_out the flag word (non-zero: the caller refuses the batch).
 */
#define MSPA_VOXEL_MAX_COLUMNS 65536
int mspa_voxel_segments_tables_host(const int64_t *offsets_host, int64_t S, int64_t *tile_base_out);
int64_t mspa_voxel_segments_workspace_bytes(const int64_t *offsets_host, int64_t S);
int mspa_voxel_segments_keys_device(const double *rows_dev, int64_t C, const int64_t *offsets_host, int64_t S, double voxel_size,
                                    const int64_t *offsets_dev, const int64_t *tile_base_dev, int64_t *keys_dev, int32_t *segment_dev,
                                    int32_t *seg_voxels_dev, void *workspace, int64_t workspace_bytes, mspa_stream_t stream);
int mspa_voxel_segments_heads_device(const int64_t *offsets_host, int64_t S, const int64_t *offsets_dev, const int64_t *keys_dev,
                                     const int64_t *order_dev, int32_t *seg_voxels_dev, void *workspace, int64_t workspace_bytes,
                                     mspa_stream_t stream);
int mspa_voxel_segments_means_device(const double *rows_dev, int64_t C, const int64_t *offsets_host, int64_t S, const int64_t *offsets_dev,
                                     const int64_t *order_dev, int64_t M, double *out_rows_dev, int32_t *out_counts_dev, void *workspace,
                                     int64_t workspace_bytes, mspa_stream_t stream);
int mspa_voxel_segments_host(const double *rows_host, int64_t C, const int64_t *offsets_host, int64_t S, double voxel_size,
                             double *out_rows_host, int64_t *out_offsets_host, int32_t *out_counts_host, int32_t *flags_out);

/*
 * DBSCAN of a RAGGED BATCH of clouds (csrc/dbscan_segments.hip, rule in csrc/dbscan_core.h): per segment the labels of
 * sklearn.cluster.DBSCAN(eps, min_samples = min_points, algorithm = "kd_tree"), value for value, and the rows of the largest
 * cluster.  The batch is the down-sample's: rows [N, C] f64 (xyz first, 3 <= C <= MSPA_VOXEL_MAX_COLUMNS) plus offsets [S + 1].
 * near(i, j) <=> (dx * dx + dy * dy) + dz * dz <= eps * eps in float64, i near itself; a row is core with min_points near rows;
 * clusters are the components of the core rows under near, numbered in ascending order of their lowest core row; a row that is not
 * core takes the lowest cluster number among its near core rows, or -1; the largest cluster has the most rows, a tie going to the
 * lowest number.  The same values on every run: the union-find hooks the larger root under the smaller by compare-and-swap, whose
 * result no arrival order changes; no atomic places a row or takes part in a floating-point sum.
 * The cells are the down-sample's at voxel size mspa_dbscan_cell_side(eps): the caller runs mspa_voxel_segments_keys_device with
 * that size and seg_voxels_dev = seg_dev + S (which zeroes the flag word seg_dev[2 S]), sorts as for the down-sample, and passes
 * keys_dev and order_dev on.  The device entry point takes the offsets TWICE, as the down-sample does, and checks every argument
 * from the host copy before anything is enqueued (MSPA_EINVAL: null pointer, offsets that descend or do not start at 0, N > 2^30,
 * S > 2^24, C out of range, eps or its square not positive, normal and finite, min_points < 1, workspace too small or
 * misaligned).  ALIGNMENT: workspace 16 bytes; every other buffer its element's size (f64 and int64: 8, int32: 4, uint8: 1).
 *   mspa_dbscan_cell_side              eps -> the cell side, eps * (1 + 2^-20): any near pair then lies in cells whose indices
 *                                      differ by at most 1 per axis (the argument is in csrc/dbscan_core.h); -1 for a bad eps.
 *   mspa_dbscan_segments_workspace_bytes  the workspace of the device call (-1 for offsets that are no batch).
 *   mspa_dbscan_segments_device        -> labels_dev [N] int32 in input row order, seg_dev [2 S + 1] int32: [0, S) the rows of each
 *                                      segment's largest cluster (written where keep_dev is given, else zero), [S, 2 S) the
 *                                      clusters of each segment, and the flag word seg_dev[2 S], into which bit 2 is ORed where a
 *                                      union-find loop reached its cap (the keys call's bits 0 and 1 stay).  keep_dev [N] uint8 or
 *                                      null: 1 for the rows of the largest cluster; with it kept_lo_dev and kept_hi_dev [S, 3] f64
 *                                      receive the kept rows' extents (+inf / -inf where nothing is kept) and tile_base_dev is
 *                                      mspa_voxel_segments_tables_host's table on the device; without it the three may be null.
 *                                      Every entry of order_dev is clamped into [0, N) and then into the segment of its slot, and
 *                                      a negative key counts as 0: arguments that are not the keys call's and its sort give wrong
 *                                      labels, never an access outside the buffers.  Thirteen launches with keep_dev, nine
 *                                      without, whatever S is; with N = 0 only the counts of seg_dev are written.
 *   mspa_dbscan_segments_host          the whole op on the CPU through the same header: the device's twin for tests and for
 *                                      NumPy input, not a fallback.  labels_host [N] int32, clusters_host [S] int32, keep_host [N]
 *                                      uint8 and kept_host [S] int32 (both or neither may be null), *flags_out the flag word.
 */
double mspa_dbscan_cell_side(double eps);
int64_t mspa_dbscan_segments_workspace_bytes(const int64_t *offsets_host, int64_t S);
int mspa_dbscan_segments_device(const double *rows_dev, int64_t C, const int64_t *offsets_host, int64_t S, double eps, int64_t min_points,
                                const int64_t *offsets_dev, const int64_t *keys_dev, const int64_t *order_dev, const int64_t *tile_base_dev,
                                int32_t *labels_dev, uint8_t *keep_dev, double *kept_lo_dev, double *kept_hi_dev, int32_t *seg_dev,
                                void *workspace, int64_t workspace_bytes, mspa_stream_t stream);
int mspa_dbscan_segments_host(const double *rows_host, int64_t C, const int64_t *offsets_host, int64_t S, double eps, int64_t min_points,
                              int32_t *labels_host, int32_t *clusters_host, uint8_t *keep_host, int32_t *kept_host, int32_t *flags_out);

/*
 * The UPRIGHT MINIMAL BOX of every cloud of a RAGGED BATCH (csrc/upright_segments.hip, rule in csrc/upright_box_core.h): per segment
 * the strict convex hull of its distinct (x, y) pairs -- counter-clockwise from the lexicographically smallest vertex, collinear
 * boundary points left out, a vertex reported as the lowest row that holds its coordinates, the orientation test EXACT (a floating
 * filter, then the six products as error-free pairs summed as an expansion) -- the minimum-area rectangle around it by the
 * all-edges rule (m_k = (along_k * across_k) / (d . d), the lowest k with the smallest m_k) and the z extent, as 8 f64:
 * [cx, cy, cz, length, width, height, ux, uy], length >= width, (ux, uy) the unit direction of the length with ux > 0, or ux == 0
 * and uy > 0; no hull vertex: eight NaN; one: sizes 0 and axis (1, 0).  The batch is the down-sample's: rows [N, C] f64 (xyz
 * first, 3 <= C <= MSPA_VOXEL_MAX_COLUMNS) plus offsets [S + 1].  The same bits on every run: minima, maxima and an integer minimum
 * over row indices only; no atomic places a row or takes part in a floating-point operation.
 * FLAGS (a flag word that is not zero refuses the call): bit 0 a non-finite x, y or z; bit 1 a non-zero |x| or |y| outside
 * [2^-200, 2^200] (the window that keeps the rule's products clear of overflow and underflow); bit 2 a hull chain that popped more
 * often than its segment has survivors.
 * Three device stages, because the caller sorts between them; each takes its offsets TWICE (host and device) and checks every
 * argument from the host copy before anything is enqueued (MSPA_EINVAL: null pointer, offsets that descend or do not start at 0,
 * more than 2^30 rows, S > 2^24, C out of range, more hull vertices than survivors in a segment, workspace too small or
 * misaligned).  Twelve launches in all, whatever S is.  ALIGNMENT: workspace 16 bytes; every other buffer its element's size
 * (f64 and int64: 8, int32: 4).
 *   mspa_upright_filter_workspace_bytes   the workspace of the filter stage (-1 for offsets that are no batch).
 *   mspa_upright_filter_device         8 launches.  -> list_dev [N] int64: in front the SURVIVORS' rows, ascending (a row is dropped only
 *                                      where a floating test with its error bound proves it strictly inside a triangle of three
 *                                      rows of its segment, so no hull vertex is ever dropped); ext_dev [S, 10] f64: the minima
 *                                      of the negated supports in the 8 directions k * 45 degrees, then min z and min -z; seg_dev
 *                                      [S + 1] int32: the survivors of each segment and the flag word (bits 0 and 1).
 *                                      tile_base_dev is mspa_voxel_segments_tables_host's table on the device.
 *   mspa_upright_hull_device           1 launch.  pts_dev [M, 2] f64: the survivors' (x, y) sorted by (segment, x, y), ties in row
 *                                      order; kept_offsets [S + 1]: the survivors' offsets.  -> stack_dev [2, M] int32: the lower and
 *                                      the upper chain of each segment (slots), seg_dev [2 S + 1] int32: the two chains' lengths
 *                                      per segment (lower, upper) and the flag word (bit 2).  A segment's hull has 0 vertices
 *                                      without survivors, 1 where the lower chain holds one slot, else lower + upper - 2.
 *   mspa_upright_boxes_workspace_bytes the workspace of the boxes stage (-1 for hull offsets that are no batch).
 *   mspa_upright_boxes_device          3 launches.  row_dev [M] int64: the input row of each sorted survivor; hull_offsets [S + 1]: the
 *                                      hull vertices' offsets; edge_base_dev [S + 1] int64: the exclusive prefix of
 *                                      ceil(vertices / 256) per segment; counts_dev: the hull stage's seg_dev.  -> hull_index_dev
 *                                      [H] int64 the hull rows, edge_dev [S] int32 the chosen edge (-1 without a vertex),
 *                                      boxes_dev [S, 8] f64.  Slots read from stack_dev are clamped into their segment: arguments
 *                                      that are not the hull stage's give wrong boxes, never an access outside the buffers.
 *   mspa_upright_segments_host         the whole op on the CPU through the same header: the device's twin for tests and for
 *                                      NumPy input, not a fallback.  hull_index_host has room for N rows, hull_offsets_host
 *                                      [S + 1], edges_host [S] int32, boxes_host [S, 8], *flags_out the flag word.
 */
int64_t mspa_upright_filter_workspace_bytes(const int64_t *offsets_host, int64_t S);
int mspa_upright_filter_device(const double *rows_dev, int64_t C, const int64_t *offsets_host, int64_t S, const int64_t *offsets_dev,
                               const int64_t *tile_base_dev, int64_t *list_dev, double *ext_dev, int32_t *seg_dev, void *workspace,
                               int64_t workspace_bytes, mspa_stream_t stream);
int mspa_upright_hull_device(const double *pts_dev, const int64_t *kept_offsets_host, int64_t S, const int64_t *kept_offsets_dev,
                             int32_t *stack_dev, int32_t *seg_dev, mspa_stream_t stream);
int64_t mspa_upright_boxes_workspace_bytes(const int64_t *hull_offsets_host, int64_t S);
int mspa_upright_boxes_device(const double *pts_dev, const int64_t *row_dev, const int64_t *kept_offsets_host,
                              const int64_t *hull_offsets_host, int64_t S, const int64_t *kept_offsets_dev, const int64_t *hull_offsets_dev,
                              const int64_t *edge_base_dev, const int32_t *stack_dev, const int32_t *counts_dev, const double *ext_dev,
                              int64_t *hull_index_dev, int32_t *edge_dev, double *boxes_dev, void *workspace, int64_t workspace_bytes,
                              mspa_stream_t stream);
int mspa_upright_segments_host(const double *rows_host, int64_t C, const int64_t *offsets_host, int64_t S, int64_t *hull_index_host,
                               int64_t *hull_offsets_host, int32_t *edges_host, double *boxes_host, int32_t *flags_out);

/*
 * The INTERSECTION OVER UNION of UPRIGHT BOXES (csrc/upright_iou.hip, rule in csrc/upright_iou_core.h): boxes are 8 f64
 * [cx, cy, cz, length, width, height, ux, uy] as the upright block above emits them; a pair gives one f64, the volume of the
 * intersection over that of the union, the footprints (rectangles c +- (length / 2) u +- (width / 2) n, n = (-uy, ux)) clipped by
 * Sutherland-Hodgman in the frame of the box with the larger length * width.  Every step is one rounded f64 operation in the
 * header's order: the device gives the host twin's bits, the same bits on every run, and iou(a, b) and iou(b, a) are the same
 * bits.  A box with a non-finite value, a negative size, |ux^2 + uy^2 - 1| > 2^-20, or a non-zero centre or size outside
 * [2^-200, 2^200] is REFUSED: its pairs give NaN; no flag word is kept and nothing is read back.  Two boxes equal in all eight
 * values give exactly 1.0 (NaN with zero volume).  Otherwise 0 <= IoU <= 1, or NaN where both volumes are zero.
 *   mode MSPA_UPRIGHT_IOU_PAIRS    a [Pa, 8], b [Pb, 8] with Pa == Pb, or either of them 1 (one box against many); G = A = B = 0;
 *                                  out [P], P the larger count (0 if either is 0).
 *   mode MSPA_UPRIGHT_IOU_MATRIX   a [G, A, 8], b [G, B, 8] (Pa == G * A, Pb == G * B); out [G, A, B].
 * parts (may be null) [.., 2] takes per output the footprint intersection area and the z overlap (zero or negative where the boxes
 * do not overlap in z).  One launch on the caller's stream; every argument is checked before anything is enqueued (MSPA_EINVAL:
 * a null pointer where a count is positive, a negative count, counts that do not fit the mode, more than 2^31 outputs, a
 * misaligned buffer); a call with zero outputs enqueues nothing.  This entry point only enqueues.  ALIGNMENT: every buffer its
 * element's size (f64: 8).
 *   mspa_upright_iou_host          the same op on the CPU through the same header: the device's twin for tests and for NumPy
 *                                  input, not a fallback.
 *   mspa_upright_iou_bound_host    a [P, 8], b [P, 8] -> per pair the header's forward-error bounds of the footprint area and of
 *                                  the IoU against the exact rational values (NaN for a refused pair).
 */
#define MSPA_UPRIGHT_IOU_PAIRS 0
#define MSPA_UPRIGHT_IOU_MATRIX 1
int mspa_upright_iou_device(const double *a_dev, int64_t Pa, const double *b_dev, int64_t Pb, int64_t G, int64_t A, int64_t B, int32_t mode,
                            double *out_dev, double *parts_dev, mspa_stream_t stream);
int mspa_upright_iou_host(const double *a_host, int64_t Pa, const double *b_host, int64_t Pb, int64_t G, int64_t A, int64_t B, int32_t mode,
                          double *out_host, double *parts_host);
int mspa_upright_iou_bound_host(const double *a_host, const double *b_host, int64_t P, double *area_bound_out, double *iou_bound_out);

#ifdef __cplusplus
}
#endif
#endif /* MSPA_H */
