// The upright minimal box of every cloud of a RAGGED BATCH ON the MI355X: the exact convex hull of each segment's (x, y) footprint,
// the minimum-area rectangle around it and the z extent, in a number of launches that does not depend on the number of segments and
// with the same bits on every run.  The rule, its window and its two floating-point arguments are csrc/upright_box_core.h; this file
// holds the op's own kernels, the host twin's entry point and the C ABI; the compaction is the batch's shared pass
// (csrc/segments_device.h).
//
// Three stages, because two of the caller's steps lie between them (the sort of the survivors, which is torch's as in sections
// 0.24 and 0.25, and the sizing of the hull list); 12 launches in all, whatever S is:
//   mspa_upright_filter_device   8 launches
//     1. up_extremes_tiles_kernel   one workgroup per tile of 4 096 rows of ONE segment (the extents pass's tiling): the segment's
//        support in 8 fixed directions (0, 45, ..., 315 degrees) and z's two ends as ten running minima per lane, folded through
//        wave shuffles and LDS -> part [T, 10]; the refusal bits of every row are ORed into the flag word (an integer atomic).
//     2. up_extremes_fold_kernel    one wave per segment over its tiles (min is order-independent) -> ext [S, 10].
//     3. up_corner_rows_kernel      the tiles again: a row whose support value EQUALS its segment's extreme in a direction enters an
//        integer atomicMin over row indices -> corner [S, 8], the lowest such row.  The corners are rows of the segment.
//     4. up_filter_kernel           the tiles again: a row is a survivor unless the floating filter, with its error bound, proves it
//        strictly inside one of the six triangles corner 0, corner i, corner i + 1.  A point strictly inside a triangle of three
//        rows is no hull vertex, whatever the corners are, so the filter cannot change the hull.  One byte per row, written once.
//     5. flag_count_kernel<KeepFlag>, tile_scan_kernel, flag_place_kernel<KeepFlag>   the survivors' rows ascending (compact()).
//     6. up_survivor_counts_kernel  one thread per segment: its survivors, by two binary searches in the list.
//   mspa_upright_hull_device     1 launch
//     7. up_chain_kernel            one lane per (segment, lower / upper chain): Andrew's scan over the sorted survivors with the exact
//        predicate; the pops are capped by the segment's survivor count, reaching the cap ORs kCapReached and the lane stops.  No
//        lane waits for another.
//   mspa_upright_boxes_device    3 launches
//     8. up_hull_gather_kernel      one thread per hull vertex: its row and its (x, y), lower chain then upper chain.
//     9. up_edge_kernel             one workgroup per (segment, tile of 256 edges): the segment's hull vertices pass through LDS in
//        chunks of 256, each lane owns an edge and keeps four running extremes -> m [H].
//    10. up_box_kernel              one wave per segment: the arg-min over its edges with the tie rule, the chosen edge's spans once
//        more (wave minima), the box.
#include "mspa_common.h"
#include "upright_box_core.h"
#include "segments_device.h"

namespace mspa {
namespace upright {

using segs::kBlock;
using segs::kExtentTile;
using segs::kFlagTile;
using segs::kWaves;

constexpr int kDirs = 8;                                         // support directions, counter-clockwise from +x in steps of 45 degrees
constexpr int kExt = kDirs + 2;                                  // and z, -z behind them
constexpr int kEdgeTile = 256;
constexpr int32_t kNoRow = 0x7f7f7f7f;                           // what the corner table is filled with (above any row: N <= 2^30)

// w [kExt]: the NEGATED support of (x, y) in direction e, so that a minimum finds the extreme; then z and -z.
__device__ __forceinline__ void negated_supports(double x, double y, double z, double w[kExt]) {
    const double s = x + y, d = x - y;
    w[0] = -x;
    w[1] = -s;
    w[2] = -y;
    w[3] = d;
    w[4] = x;
    w[5] = s;
    w[6] = y;
    w[7] = -d;
    w[8] = z;
    w[9] = -z;
}

struct Tile {                                                    // rows [a, b) of segment s
    int64_t s, a, b;
};

__device__ __forceinline__ Tile tile_of(const int64_t *__restrict__ offsets, const int64_t *__restrict__ tile_base, int64_t S, int64_t t) {
    Tile tile;
    tile.s = segment_of(tile_base, S, t);
    tile.a = offsets[tile.s] + (t - tile_base[tile.s]) * kExtentTile;
    const int64_t end = offsets[tile.s + 1];
    tile.b = tile.a + kExtentTile < end ? tile.a + kExtentTile : end;
    return tile;
}

__global__ void __launch_bounds__(kBlock) up_extremes_tiles_kernel(const double *__restrict__ rows, int64_t C, const int64_t *__restrict__ offsets,
                                                                   const int64_t *__restrict__ tile_base, int64_t S, double *__restrict__ part,
                                                                   int32_t *__restrict__ flag_word) {
    __shared__ double mins[kWaves][kExt];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const Tile tile = tile_of(offsets, tile_base, S, blockIdx.x);
    double m[kExt];
#pragma unroll
    for (int e = 0; e < kExt; ++e) m[e] = INFINITY;
    int32_t refused = 0;
    for (int64_t i = tile.a + tid; i < tile.b; i += kBlock) {
        const double x = rows[i * C], y = rows[i * C + 1], z = rows[i * C + 2];
        refused |= refusal_of(x, y, z);
        double v[kExt];
        negated_supports(x, y, z, v);
#pragma unroll
        for (int e = 0; e < kExt; ++e) m[e] = v[e] < m[e] ? v[e] : m[e];
    }
    if (refused) atomicOr(flag_word, refused);
#pragma unroll
    for (int e = 0; e < kExt; ++e) {
        const double v = wave_min(m[e]);
        if (lane == 0) mins[w][e] = v;
    }
    __syncthreads();
    if (tid < kExt) {
        double v = mins[0][tid];
#pragma unroll
        for (int e = 1; e < kWaves; ++e) v = mins[e][tid] < v ? mins[e][tid] : v;
        part[(int64_t)blockIdx.x * kExt + tid] = v;
    }
}

__global__ void __launch_bounds__(kWave) up_extremes_fold_kernel(const double *__restrict__ part, const int64_t *__restrict__ tile_base,
                                                                 double *__restrict__ ext) {
    const int lane = (int)threadIdx.x;
    const int64_t s = blockIdx.x;
    const int64_t a = tile_base[s], b = tile_base[s + 1];
    double m[kExt];
#pragma unroll
    for (int e = 0; e < kExt; ++e) m[e] = INFINITY;
    for (int64_t t = a + lane; t < b; t += kWave) {
#pragma unroll
        for (int e = 0; e < kExt; ++e) m[e] = part[t * kExt + e] < m[e] ? part[t * kExt + e] : m[e];
    }
#pragma unroll
    for (int e = 0; e < kExt; ++e) {
        const double v = wave_min(m[e]);
        if (lane == e) ext[s * kExt + e] = v;
    }
}

__global__ void __launch_bounds__(kBlock) up_corner_rows_kernel(const double *__restrict__ rows, int64_t C, const int64_t *__restrict__ offsets,
                                                                const int64_t *__restrict__ tile_base, int64_t S, const double *__restrict__ ext,
                                                                int32_t *__restrict__ corner) {
    const int tid = (int)threadIdx.x;
    const Tile tile = tile_of(offsets, tile_base, S, blockIdx.x);
    double extreme[kDirs];
#pragma unroll
    for (int e = 0; e < kDirs; ++e) extreme[e] = ext[tile.s * kExt + e];
    for (int64_t i = tile.a + tid; i < tile.b; i += kBlock) {
        double v[kExt];
        negated_supports(rows[i * C], rows[i * C + 1], 0.0, v);
#pragma unroll
        for (int e = 0; e < kDirs; ++e)
            if (v[e] == extreme[e]) atomicMin(corner + tile.s * kDirs + e, (int32_t)i);
    }
}

__global__ void __launch_bounds__(kBlock) up_filter_kernel(const double *__restrict__ rows, int64_t C, const int64_t *__restrict__ offsets,
                                                           const int64_t *__restrict__ tile_base, int64_t S, int64_t N,
                                                           const int32_t *__restrict__ corner, uint8_t *__restrict__ keep) {
    const int tid = (int)threadIdx.x;
    const Tile tile = tile_of(offsets, tile_base, S, blockIdx.x);
    const int64_t a = offsets[tile.s], b = offsets[tile.s + 1];
    double cx[kDirs], cy[kDirs];
#pragma unroll
    for (int e = 0; e < kDirs; ++e) {
        const int64_t r = segs::row_in_segment(corner[tile.s * kDirs + e], N, a, b);      // (a corner nobody wrote: a segment with a NaN row)
        cx[e] = rows[r * C];
        cy[e] = rows[r * C + 1];
    }
    for (int64_t i = tile.a + tid; i < tile.b; i += kBlock) {
        const double x = rows[i * C], y = rows[i * C + 1];
        bool inside = false;
#pragma unroll
        for (int e = 1; e + 1 < kDirs; ++e) inside = inside || proved_inside(cx[0], cy[0], cx[e], cy[e], cx[e + 1], cy[e + 1], x, y);
        keep[i] = inside ? 0 : 1;
    }
}

struct KeepFlag {                                                // row i survives the filter
    const uint8_t *keep;
    __device__ __forceinline__ bool operator()(int64_t i) const { return keep[i] != 0; }
};

__global__ void __launch_bounds__(kBlock) up_survivor_counts_kernel(const int64_t *__restrict__ list, const int64_t *__restrict__ total,
                                                                    const int64_t *__restrict__ offsets, int64_t S, int32_t *__restrict__ seg) {
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= S) return;
    const int64_t M = *total;
    seg[s] = (int32_t)(first_at_or_above(list, 0, M, offsets[s + 1]) - first_at_or_above(list, 0, M, offsets[s]));
}

__global__ void __launch_bounds__(kBlock) up_chain_kernel(const double *__restrict__ pts, const int64_t *__restrict__ kept_offsets, int64_t S, int64_t M,
                                                          int32_t *__restrict__ stack, int32_t *__restrict__ seg) {
    const int64_t lane = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (lane >= 2 * S) return;
    const int64_t s = lane >> 1;
    const bool upper = (lane & 1) != 0;
    int64_t a = kept_offsets[s], b = kept_offsets[s + 1];
    a = a < 0 ? 0 : a > M ? M : a;                               // (offsets that are the host's: already inside)
    b = b < a ? a : b > M ? M : b;
    bool capped = false;
    const int64_t count = chain(pts, a, b, upper, stack + (upper ? M : 0), b - a, capped);
    seg[lane] = (int32_t)count;
    if (capped) atomicOr(seg + 2 * S, kCapReached);
}

__global__ void __launch_bounds__(kBlock) up_hull_gather_kernel(const double *__restrict__ pts, const int64_t *__restrict__ row,
                                                                const int64_t *__restrict__ kept_offsets, const int64_t *__restrict__ hull_offsets,
                                                                int64_t S, int64_t M, int64_t H, const int32_t *__restrict__ stack,
                                                                const int32_t *__restrict__ counts, int64_t *__restrict__ hull_index,
                                                                double *__restrict__ hull_xy) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= H) return;
    const int64_t s = segment_of(hull_offsets, S, j);
    const int64_t a = kept_offsets[s], m = kept_offsets[s + 1] - a;          // m >= the segment's hull vertices >= 1: the entry point checked
    int64_t lower_count = counts[2 * s];
    lower_count = lower_count < 1 ? 1 : lower_count > m ? m : lower_count;
    int64_t slot = hull_slot(stack, stack + M, a, lower_count, j - hull_offsets[s]);
    slot = slot < a ? a : slot >= a + m ? a + m - 1 : slot;      // a slot of the segment, whatever the stacks hold
    hull_index[j] = row[slot];
    hull_xy[2 * j] = pts[2 * slot];
    hull_xy[2 * j + 1] = pts[2 * slot + 1];
}

__global__ void __launch_bounds__(kEdgeTile) up_edge_kernel(const double *__restrict__ hull_xy, const int64_t *__restrict__ hull_offsets,
                                                            const int64_t *__restrict__ edge_base, int64_t S, double *__restrict__ measure) {
    __shared__ double vx[kEdgeTile], vy[kEdgeTile];
    const int tid = (int)threadIdx.x;
    const int64_t t = blockIdx.x;
    const int64_t s = segment_of(edge_base, S, t);
    const int64_t first = hull_offsets[s], h = hull_offsets[s + 1] - first;
    const int64_t k = (t - edge_base[s]) * kEdgeTile + tid;
    const bool owns = k < h;
    double ax = 0.0, ay = 0.0, dx = 0.0, dy = 0.0;
    if (owns) {
        const int64_t k1 = k + 1 < h ? k + 1 : 0;
        ax = hull_xy[2 * (first + k)];
        ay = hull_xy[2 * (first + k) + 1];
        dx = hull_xy[2 * (first + k1)] - ax;
        dy = hull_xy[2 * (first + k1) + 1] - ay;
    }
    Spans sp = no_spans();
    for (int64_t base = 0; base < h; base += kEdgeTile) {
        const int64_t n = h - base < kEdgeTile ? h - base : kEdgeTile;
        __syncthreads();
        if (tid < n) {
            vx[tid] = hull_xy[2 * (first + base + tid)];
            vy[tid] = hull_xy[2 * (first + base + tid) + 1];
        }
        __syncthreads();
        for (int j = 0; j < (int)n; ++j) project(ax, ay, dx, dy, vx[j], vy[j], sp);
    }
    if (owns) measure[first + k] = edge_measure(sp, length_sq(dx, dy));
}

__global__ void __launch_bounds__(kWave) up_box_kernel(const double *__restrict__ hull_xy, const int64_t *__restrict__ hull_offsets,
                                                       const double *__restrict__ measure, const double *__restrict__ ext,
                                                       int32_t *__restrict__ edge_out, double *__restrict__ boxes) {
    const int lane = (int)threadIdx.x;
    const int64_t s = blockIdx.x;
    const int64_t first = hull_offsets[s], h = hull_offsets[s + 1] - first;
    const double z_lo = ext[s * kExt + 8], z_hi = -ext[s * kExt + 9];
    double *box = boxes + s * kBoxValues;
    if (h < 2) {
        if (lane == 0) {
            edge_out[s] = h == 1 ? 0 : -1;
            if (h == 1) point_box(hull_xy[2 * first], hull_xy[2 * first + 1], z_lo, z_hi, box);
            else no_box(box);
        }
        return;
    }
    double best = 0.0;
    int64_t best_k = -1;
    for (int64_t k = lane; k < h; k += kWave) {
        const double m = measure[first + k];
        if (better_edge(best, best_k, m, k)) {
            best = m;
            best_k = k;
        }
    }
#pragma unroll
    for (int t = 32; t >= 1; t >>= 1) {
        const double m = __shfl_xor(best, t, 64);
        const int64_t k = __shfl_xor(best_k, t, 64);
        if (better_edge(best, best_k, m, k)) {
            best = m;
            best_k = k;
        }
    }
    best_k = best_k < 0 ? 0 : best_k;                            // (every lane of a wave with h >= 2 holds an edge by now)
    const int64_t k1 = best_k + 1 < h ? best_k + 1 : 0;
    const double ax = hull_xy[2 * (first + best_k)], ay = hull_xy[2 * (first + best_k) + 1];
    const double dx = hull_xy[2 * (first + k1)] - ax, dy = hull_xy[2 * (first + k1) + 1] - ay;
    Spans sp = no_spans();
    for (int64_t j = lane; j < h; j += kWave) project(ax, ay, dx, dy, hull_xy[2 * (first + j)], hull_xy[2 * (first + j) + 1], sp);
    sp.t_min = wave_min(sp.t_min);
    sp.t_max = -wave_min(-sp.t_max);
    sp.c_min = wave_min(sp.c_min);
    sp.c_max = -wave_min(-sp.c_max);
    if (lane == 0) {
        edge_out[s] = (int32_t)best_k;
        box_of(ax, ay, dx, dy, sp, z_lo, z_hi, box);
    }
}

// The workspace of the filter stage for a batch of N rows in S segments and T tiles, cut into its parts.
struct FilterWorkspace {
    int64_t part, corner, keep, tile_counts, total, bytes;
    FilterWorkspace(int64_t N, int64_t S, int64_t T) {
        part = 0;
        corner = part + align16(T * kExt * 8);
        keep = corner + align16(S * kDirs * 4);
        tile_counts = keep + align16(N);
        total = tile_counts + align16(((N + kFlagTile - 1) / kFlagTile + 1) * 4);
        bytes = total + 16;
    }
};

// The workspace of the boxes stage for H hull vertices.
struct BoxesWorkspace {
    int64_t hull_xy, measure, bytes;
    explicit BoxesWorkspace(int64_t H) {
        hull_xy = 0;
        measure = hull_xy + align16(H * 16);
        bytes = measure + align16(H * 8);
    }
};

int64_t edge_tiles(const int64_t *hull_offsets, int64_t S) {
    int64_t T = 0;
    for (int64_t s = 0; s < S; ++s) T += (hull_offsets[s + 1] - hull_offsets[s] + kEdgeTile - 1) / kEdgeTile;
    return T;
}

// N of a batch the entry points take with its columns, or -1 with the error text set.
int64_t checked_batch(const char *who, const int64_t *offsets_host, int64_t S, int64_t C) {
    const int64_t N = segs::checked_rows(who, offsets_host, S);
    if (N < 0) return -1;
    if (C < 3 || C > MSPA_VOXEL_MAX_COLUMNS) {
        fail(MSPA_EINVAL, std::string(who) + ": C must be between 3 and 65536 columns");
        return -1;
    }
    return N;
}

}  // namespace upright
}  // namespace mspa

using namespace mspa;

extern "C" int64_t mspa_upright_filter_workspace_bytes(const int64_t *offsets_host, int64_t S) {
    const int64_t N = upright::batch_rows(offsets_host, S);
    if (N < 0) return -1;
    return upright::FilterWorkspace(N, S, segs::extent_tiles(offsets_host, S)).bytes;
}

extern "C" int mspa_upright_filter_device(const double *rows_dev, int64_t C, const int64_t *offsets_host, int64_t S, const int64_t *offsets_dev,
                                          const int64_t *tile_base_dev, int64_t *list_dev, double *ext_dev, int32_t *seg_dev, void *workspace,
                                          int64_t workspace_bytes, void *stream) {
    const char *who = "mspa_upright_filter_device";
    const int64_t N = upright::checked_batch(who, offsets_host, S, C);
    if (N < 0) return MSPA_EINVAL;
    if (!seg_dev || (S > 0 && !ext_dev) || (N > 0 && (!rows_dev || !offsets_dev || !tile_base_dev || !list_dev)))
        return fail(MSPA_EINVAL, std::string(who) + ": null pointer");
    const int64_t T = segs::extent_tiles(offsets_host, S);
    if (N > 0 && (!workspace || workspace_bytes < upright::FilterWorkspace(N, S, T).bytes))
        return fail(MSPA_EINVAL, std::string(who) + ": workspace null or smaller than mspa_upright_filter_workspace_bytes()");
    if (N > 0 && ((uintptr_t)workspace & 15u)) return fail(MSPA_EINVAL, std::string(who) + ": workspace must be 16-byte aligned");
    if (segs::misaligned(rows_dev, 8) || segs::misaligned(offsets_dev, 8) || segs::misaligned(tile_base_dev, 8) || segs::misaligned(list_dev, 8) ||
        segs::misaligned(ext_dev, 8) || segs::misaligned(seg_dev, 4))
        return fail(MSPA_EINVAL, std::string(who) + ": a buffer is not aligned to its element");
    hipStream_t st = (hipStream_t)stream;
    if (check_hip(hipMemsetAsync(seg_dev, 0, (size_t)(S + 1) * 4, st), who) != MSPA_OK) return MSPA_EHIP;       // the counts and the flag word
    if (N == 0) {                                                // no rows: every segment's extremes are those of nothing
        if (S > 0 && check_hip(hipMemsetAsync(ext_dev, 0, (size_t)S * upright::kExt * 8, st), who) != MSPA_OK) return MSPA_EHIP;
        return MSPA_OK;
    }
    const upright::FilterWorkspace ws(N, S, T);
    uint8_t *base = (uint8_t *)workspace;
    double *part = (double *)(base + ws.part);
    int32_t *corner = (int32_t *)(base + ws.corner), *tile_counts = (int32_t *)(base + ws.tile_counts);
    uint8_t *keep = base + ws.keep;
    int64_t *total = (int64_t *)(base + ws.total);
    int32_t *flag_word = seg_dev + S;
    const dim3 block(upright::kBlock), tiles((unsigned)T);
    if (check_hip(hipMemsetAsync(corner, 0x7f, (size_t)S * upright::kDirs * 4, st), who) != MSPA_OK) return MSPA_EHIP;
    static_assert(upright::kNoRow == 0x7f7f7f7f, "the corner table is filled bytewise");
    hipLaunchKernelGGL(upright::up_extremes_tiles_kernel, tiles, block, 0, st, rows_dev, C, offsets_dev, tile_base_dev, S, part, flag_word);
    hipLaunchKernelGGL(upright::up_extremes_fold_kernel, dim3((unsigned)S), dim3(kWave), 0, st, (const double *)part, tile_base_dev, ext_dev);
    hipLaunchKernelGGL(upright::up_corner_rows_kernel, tiles, block, 0, st, rows_dev, C, offsets_dev, tile_base_dev, S, (const double *)ext_dev,
                       corner);
    hipLaunchKernelGGL(upright::up_filter_kernel, tiles, block, 0, st, rows_dev, C, offsets_dev, tile_base_dev, S, N, (const int32_t *)corner, keep);
    segs::compact(upright::KeepFlag{keep}, N, tile_counts, total, list_dev, false, st);
    hipLaunchKernelGGL(upright::up_survivor_counts_kernel, dim3((unsigned)((S + upright::kBlock - 1) / upright::kBlock)), block, 0, st,
                       (const int64_t *)list_dev, (const int64_t *)total, offsets_dev, S, seg_dev);
    return check_hip(hipGetLastError(), who);
}

extern "C" int mspa_upright_hull_device(const double *pts_dev, const int64_t *kept_offsets_host, int64_t S, const int64_t *kept_offsets_dev,
                                        int32_t *stack_dev, int32_t *seg_dev, void *stream) {
    const char *who = "mspa_upright_hull_device";
    const int64_t M = segs::checked_rows(who, kept_offsets_host, S);
    if (M < 0) return MSPA_EINVAL;
    if (!seg_dev || (M > 0 && (!pts_dev || !kept_offsets_dev || !stack_dev))) return fail(MSPA_EINVAL, std::string(who) + ": null pointer");
    if (segs::misaligned(pts_dev, 8) || segs::misaligned(kept_offsets_dev, 8) || segs::misaligned(stack_dev, 4) || segs::misaligned(seg_dev, 4))
        return fail(MSPA_EINVAL, std::string(who) + ": a buffer is not aligned to its element");
    hipStream_t st = (hipStream_t)stream;
    if (check_hip(hipMemsetAsync(seg_dev, 0, (size_t)(2 * S + 1) * 4, st), who) != MSPA_OK) return MSPA_EHIP;   // the counts and the flag word
    if (M == 0) return MSPA_OK;
    hipLaunchKernelGGL(upright::up_chain_kernel, dim3((unsigned)((2 * S + upright::kBlock - 1) / upright::kBlock)), dim3(upright::kBlock), 0, st, pts_dev,
                       kept_offsets_dev, S, M, stack_dev, seg_dev);
    return check_hip(hipGetLastError(), who);
}

extern "C" int64_t mspa_upright_boxes_workspace_bytes(const int64_t *hull_offsets_host, int64_t S) {
    const int64_t H = upright::batch_rows(hull_offsets_host, S);
    if (H < 0) return -1;
    return upright::BoxesWorkspace(H).bytes;
}

extern "C" int mspa_upright_boxes_device(const double *pts_dev, const int64_t *row_dev, const int64_t *kept_offsets_host,
                                         const int64_t *hull_offsets_host, int64_t S, const int64_t *kept_offsets_dev,
                                         const int64_t *hull_offsets_dev, const int64_t *edge_base_dev, const int32_t *stack_dev,
                                         const int32_t *counts_dev, const double *ext_dev, int64_t *hull_index_dev, int32_t *edge_dev,
                                         double *boxes_dev, void *workspace, int64_t workspace_bytes, void *stream) {
    const char *who = "mspa_upright_boxes_device";
    const int64_t M = segs::checked_rows(who, kept_offsets_host, S);
    if (M < 0) return MSPA_EINVAL;
    const int64_t H = segs::checked_rows(who, hull_offsets_host, S);
    if (H < 0) return MSPA_EINVAL;
    for (int64_t s = 0; s < S; ++s)
        if (hull_offsets_host[s + 1] - hull_offsets_host[s] > kept_offsets_host[s + 1] - kept_offsets_host[s])
            return fail(MSPA_EINVAL, std::string(who) + ": a segment has more hull vertices than survivors");
    if ((S > 0 && (!hull_offsets_dev || !ext_dev || !edge_dev || !boxes_dev)) ||
        (H > 0 && (!pts_dev || !row_dev || !kept_offsets_dev || !edge_base_dev || !stack_dev || !counts_dev || !hull_index_dev)))
        return fail(MSPA_EINVAL, std::string(who) + ": null pointer");
    if (H > 0 && (!workspace || workspace_bytes < upright::BoxesWorkspace(H).bytes))
        return fail(MSPA_EINVAL, std::string(who) + ": workspace null or smaller than mspa_upright_boxes_workspace_bytes()");
    if (H > 0 && ((uintptr_t)workspace & 15u)) return fail(MSPA_EINVAL, std::string(who) + ": workspace must be 16-byte aligned");
    if (segs::misaligned(pts_dev, 8) || segs::misaligned(row_dev, 8) || segs::misaligned(kept_offsets_dev, 8) || segs::misaligned(hull_offsets_dev, 8) ||
        segs::misaligned(edge_base_dev, 8) || segs::misaligned(stack_dev, 4) || segs::misaligned(counts_dev, 4) || segs::misaligned(ext_dev, 8) ||
        segs::misaligned(hull_index_dev, 8) || segs::misaligned(edge_dev, 4) || segs::misaligned(boxes_dev, 8))
        return fail(MSPA_EINVAL, std::string(who) + ": a buffer is not aligned to its element");
    if (S == 0) return MSPA_OK;
    hipStream_t st = (hipStream_t)stream;
    const upright::BoxesWorkspace ws(H);
    uint8_t *base = (uint8_t *)workspace;
    double *hull_xy = (double *)(base + ws.hull_xy), *measure = (double *)(base + ws.measure);
    if (H > 0) {
        const int64_t T = upright::edge_tiles(hull_offsets_host, S);
        hipLaunchKernelGGL(upright::up_hull_gather_kernel, dim3((unsigned)((H + upright::kBlock - 1) / upright::kBlock)), dim3(upright::kBlock), 0, st,
                           pts_dev, row_dev, kept_offsets_dev, hull_offsets_dev, S, M, H, stack_dev, counts_dev, hull_index_dev, hull_xy);
        hipLaunchKernelGGL(upright::up_edge_kernel, dim3((unsigned)T), dim3(upright::kEdgeTile), 0, st, (const double *)hull_xy, hull_offsets_dev,
                           edge_base_dev, S, measure);
    }
    hipLaunchKernelGGL(upright::up_box_kernel, dim3((unsigned)S), dim3(kWave), 0, st, (const double *)hull_xy, hull_offsets_dev,
                       (const double *)measure, ext_dev, edge_dev, boxes_dev);
    return check_hip(hipGetLastError(), who);
}

extern "C" int mspa_upright_segments_host(const double *rows_host, int64_t C, const int64_t *offsets_host, int64_t S, int64_t *hull_index_host,
                                          int64_t *hull_offsets_host, int32_t *edges_host, double *boxes_host, int32_t *flags_out) {
    const char *who = "mspa_upright_segments_host";
    const int64_t N = upright::checked_batch(who, offsets_host, S, C);
    if (N < 0) return MSPA_EINVAL;
    if (!flags_out || !hull_offsets_host || (S > 0 && (!edges_host || !boxes_host)) || (N > 0 && (!rows_host || !hull_index_host)))
        return fail(MSPA_EINVAL, std::string(who) + ": null pointer");
    *flags_out = upright::upright_all(rows_host, C, offsets_host, S, hull_index_host, hull_offsets_host, edges_host, boxes_host);
    return MSPA_OK;
}
