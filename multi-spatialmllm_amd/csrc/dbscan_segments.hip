// DBSCAN of a RAGGED BATCH of clouds ON the MI355X: a label per row of every segment, the per-segment cluster counts and, where
// asked, the rows of each segment's largest cluster, in a number of launches that does not depend on the number of segments and
// with labels that are the same values on every run.  The rule and its two floating-point arguments are csrc/dbscan_core.h; this
// file holds the op's own kernels, the host twin's entry point and the C ABI; the compaction and the extents pass are the batch's
// shared passes (csrc/segments_device.h).
//
// The cells are section 0.24's: the caller runs mspa_voxel_segments_keys_device at voxel size mspa_dbscan_cell_side(eps) (the
// segments' extents, the 63-bit keys, the flag word) and sorts the keys stably by (segment, key), exactly as for the down-sample.
// A segment's range of the sorted keys IS its sorted cell table: a cell is found by binary search in it, and the three cells
// iz - 1 .. iz + 1 of a column are one run, so the 27 cells cost nine searches.  One entry point, mspa_dbscan_segments_device:
//     1. db_gather_kernel     one thread per sorted slot: its row (the order entry clamped into the slot's segment), the row's xyz
//        and key gathered once, so the walks read points and keys in sorted order.
//     2. db_core_kernel       one thread per sorted slot: the near points in the 27 cells, the count stopped at min_points -> core
//        [slot], and parent[row] = row for a core row, -1 for any other.
//     3. db_link_kernel       one thread per core slot: every near core slot in front of it is hooked to it (union-find on parent
//        by compare-and-swap, the larger root under the smaller; agent-scope atomic loads; capped loops, no lane waits).
//     4. db_roots_kernel      one thread per row, a launch of its own after the linking: root[row], the lowest core row of its
//        component (-1 for a row that is not core).
//     5. flag_count_kernel<RepFlag>, tile_scan_kernel, flag_place_kernel<RepFlag>   the representatives (root[row] == row) in input
//        row order (compact(): per tile a count from wave ballots, one workgroup's scan, positions from ballots).
//        The rank of a representative in that list, less the rank of its segment's first, is the cluster's number.
//     6. db_segment_clusters_kernel   one thread per segment: its clusters, by two binary searches in the list.
//     7. db_labels_kernel     one thread per sorted slot: a core row's root, or for any other row the lowest root among the near
//        core slots (a second walk) -> its rank by binary search -> labels[row]; the row is counted into its cluster's size (an
//        integer add: no order changes a count).
//     8. db_largest_kernel    one wave per segment: the cluster with the most rows, a tie to the lowest number -> best, kept.
//     9. db_keep_kernel       one thread per row: keep = the row's label is its segment's best.
//    10. extent_tiles_kernel<2, KeptFlag>, extent_fold_kernel<2>   the extents of the kept rows per segment by the down-sample's
//        extents pass: one workgroup per tile of 4 096 rows of ONE segment, then one wave per segment over its tiles (min and max
//        are order-independent) -> kept_lo, kept_hi [S, 3], +inf / -inf where nothing is kept.
// Steps 8 to 10 run only where the caller passes keep_dev.
#include "mspa_common.h"
#include "dbscan_core.h"
#include "segments_device.h"

namespace mspa {
namespace dbscan {

using segs::kBlock;
using segs::kFlagTile;

// parent through agent-scope atomics: a load sees what any workgroup of the launch has stored.
struct DeviceMemory {
    int32_t *parent;
    __device__ __forceinline__ int32_t load(int32_t i) const { return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ void lower(int32_t i, int32_t v) const { atomicMin(parent + i, v); }
    __device__ __forceinline__ int32_t compare_and_swap(int32_t i, int32_t expected, int32_t desired) const {
        return atomicCAS(parent + i, expected, desired);
    }
};

__global__ void __launch_bounds__(kBlock) db_gather_kernel(const double *__restrict__ rows, int64_t C, const int64_t *__restrict__ offsets, int64_t S,
                                                           int64_t N, const int64_t *__restrict__ keys_in, const int64_t *__restrict__ order,
                                                           double *__restrict__ pts, int64_t *__restrict__ keys, int32_t *__restrict__ row) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const int64_t s = segment_of(offsets, S, i);
    const int64_t o = row_in_segment(order[i], N, offsets[s], offsets[s + 1]);
    pts[3 * i] = rows[o * C];
    pts[3 * i + 1] = rows[o * C + 1];
    pts[3 * i + 2] = rows[o * C + 2];
    const int64_t key = keys_in[o];
    keys[i] = key < 0 ? 0 : key;                                 // a key that is not the keys pass's decodes into [0, 2^21) anyway
    row[i] = (int32_t)o;
}

__global__ void __launch_bounds__(kBlock) db_core_kernel(const double *__restrict__ pts, const int64_t *__restrict__ keys,
                                                         const int32_t *__restrict__ row, const int64_t *__restrict__ offsets, int64_t S, int64_t N,
                                                         double eps_sq, int64_t min_points, uint8_t *__restrict__ core,
                                                         int32_t *__restrict__ parent) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const int64_t s = segment_of(offsets, S, i);
    const bool is = is_core(pts, keys, offsets[s], offsets[s + 1], i, eps_sq, min_points);
    core[i] = is ? 1 : 0;
    parent[row[i]] = is ? row[i] : -1;
}

__global__ void __launch_bounds__(kBlock) db_link_kernel(const double *__restrict__ pts, const int64_t *__restrict__ keys,
                                                         const int32_t *__restrict__ row, const uint8_t *__restrict__ core,
                                                         const int64_t *__restrict__ offsets, int64_t S, int64_t N, double eps_sq,
                                                         int32_t *parent, int32_t *__restrict__ flag_word) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= N || !core[i]) return;
    const int64_t s = segment_of(offsets, S, i);
    const int64_t a = offsets[s], b = offsets[s + 1];
    bool capped = false;
    link_point(DeviceMemory{parent}, pts, keys, row, core, a, b, i, eps_sq, cap_of(b - a), capped);
    if (capped) atomicOr(flag_word, kCapReached);
}

__global__ void __launch_bounds__(kBlock) db_roots_kernel(int32_t *parent, const int64_t *__restrict__ offsets, int64_t S, int64_t N,
                                                          int32_t *__restrict__ root, int32_t *__restrict__ flag_word) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= N) return;
    const int64_t s = segment_of(offsets, S, r);
    const int64_t a = offsets[s], b = offsets[s + 1];
    bool capped = false;
    int32_t top = -1;
    if (parent[r] >= 0) {
        top = read_root(DeviceMemory{parent}, (int32_t)r, cap_of(b - a), capped);
        top = top < a ? (int32_t)a : top > r ? (int32_t)r : top;  // a root is a row of the segment at or below the row
    }
    root[r] = top;
    if (capped) atomicOr(flag_word, kCapReached);
}

__global__ void __launch_bounds__(kBlock) db_segment_clusters_kernel(const int64_t *__restrict__ reps, const int64_t *__restrict__ total,
                                                                     const int64_t *__restrict__ offsets, int64_t S,
                                                                     int32_t *__restrict__ seg_clusters) {
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= S) return;
    const int64_t M = *total;
    seg_clusters[s] = (int32_t)(first_at_or_above(reps, 0, M, offsets[s + 1]) - first_at_or_above(reps, 0, M, offsets[s]));
}

__global__ void __launch_bounds__(kBlock) db_labels_kernel(const double *__restrict__ pts, const int64_t *__restrict__ keys,
                                                           const int32_t *__restrict__ row, const uint8_t *__restrict__ core,
                                                           const int32_t *__restrict__ root, const int64_t *__restrict__ reps,
                                                           const int64_t *__restrict__ total, const int64_t *__restrict__ offsets, int64_t S,
                                                           int64_t N, double eps_sq, int32_t *__restrict__ labels, int32_t *__restrict__ sizes) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const int64_t s = segment_of(offsets, S, i);
    const int64_t a = offsets[s], b = offsets[s + 1], M = *total;
    const int32_t o = row[i];
    const int32_t r = core[i] ? root[o] : border_root(pts, keys, row, core, root, a, b, i, eps_sq);
    int32_t label = -1;
    if (r >= 0) {
        const int64_t first = first_at_or_above(reps, 0, M, a), at = first_at_or_above(reps, 0, M, (int64_t)r);
        if (at < M && reps[at] == r) {                           // (always, for a root the roots pass wrote)
            label = (int32_t)(at - first);
            atomicAdd(sizes + at, 1);
        }
    }
    labels[o] = label;
}

__global__ void __launch_bounds__(kWave) db_largest_kernel(const int32_t *__restrict__ sizes, const int64_t *__restrict__ reps,
                                                           const int64_t *__restrict__ total, const int64_t *__restrict__ offsets,
                                                           int32_t *__restrict__ best_out, int32_t *__restrict__ seg_kept) {
    const int lane = (int)threadIdx.x;
    const int64_t s = blockIdx.x, M = *total;
    const int64_t first = first_at_or_above(reps, 0, M, offsets[s]), count = first_at_or_above(reps, 0, M, offsets[s + 1]) - first;
    int32_t best = -1, size = 0;
    for (int64_t c = lane; c < count; c += kWave) {
        const int32_t n = sizes[first + c];
        if (better_of(size, best, n, (int32_t)c)) {
            best = (int32_t)c;
            size = n;
        }
    }
#pragma unroll
    for (int t = 32; t >= 1; t >>= 1) {
        const int32_t other = __shfl_xor(best, t, 64), n = __shfl_xor(size, t, 64);
        if (better_of(size, best, n, other)) {
            best = other;
            size = n;
        }
    }
    if (lane == 0) {
        best_out[s] = best;
        seg_kept[s] = best >= 0 ? size : 0;
    }
}

__global__ void __launch_bounds__(kBlock) db_keep_kernel(const int32_t *__restrict__ labels, const int32_t *__restrict__ best,
                                                         const int64_t *__restrict__ offsets, int64_t S, int64_t N, uint8_t *__restrict__ keep) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= N) return;
    const int32_t label = labels[r];
    keep[r] = label >= 0 && label == best[segment_of(offsets, S, r)] ? 1 : 0;
}

struct RepFlag {                                                 // row i is its component's representative
    const int32_t *root;
    __device__ __forceinline__ bool operator()(int64_t i) const { return root[i] == i; }
};

struct KeptFlag {                                                // row i is kept
    const uint8_t *keep;
    __device__ __forceinline__ bool operator()(int64_t i) const { return keep[i] != 0; }
};

// The workspace of a batch of N rows in S segments, cut into its parts.
struct Workspace {
    int64_t pts, keys, reps, row, parent, root, sizes, core, tile_counts, totals, best, part, bytes;
    Workspace(int64_t N, int64_t S, int64_t T) {
        pts = 0;
        keys = pts + align16(N * 24);
        reps = keys + align16(N * 8);
        row = reps + align16((N + 1) * 8);
        parent = row + align16(N * 4);
        root = parent + align16(N * 4);
        sizes = root + align16(N * 4);
        core = sizes + align16(N * 4);
        tile_counts = core + align16(N);
        totals = tile_counts + align16(((N + kFlagTile - 1) / kFlagTile + 1) * 4);
        best = totals + 16;
        part = best + align16((S + 1) * 4);
        bytes = part + align16(T * 48);
    }
};

// N of a batch the entry points take with their parameters, or -1 with the error text set.
int64_t checked_batch(const char *who, const int64_t *offsets_host, int64_t S, int64_t C, double eps, int64_t min_points) {
    const std::string name(who);
    const int64_t N = segs::checked_rows(who, offsets_host, S);
    if (N < 0) return -1;
    if (C < 3 || C > MSPA_VOXEL_MAX_COLUMNS) {
        fail(MSPA_EINVAL, name + ": C must be between 3 and 65536 columns");
        return -1;
    }
    if (!eps_ok(eps)) {
        fail(MSPA_EINVAL, name + ": eps must be positive and finite, and so must its square");
        return -1;
    }
    if (min_points < 1) {
        fail(MSPA_EINVAL, name + ": min_points must be at least 1");
        return -1;
    }
    return N;
}

}  // namespace dbscan
}  // namespace mspa

using namespace mspa;

extern "C" double mspa_dbscan_cell_side(double eps) { return dbscan::eps_ok(eps) ? dbscan::cell_side(eps) : -1.0; }

extern "C" int64_t mspa_dbscan_segments_workspace_bytes(const int64_t *offsets_host, int64_t S) {
    const int64_t N = dbscan::batch_rows(offsets_host, S);
    if (N < 0) return -1;
    return dbscan::Workspace(N, S, segs::extent_tiles(offsets_host, S)).bytes;
}

extern "C" int mspa_dbscan_segments_device(const double *rows_dev, int64_t C, const int64_t *offsets_host, int64_t S, double eps,
                                           int64_t min_points, const int64_t *offsets_dev, const int64_t *keys_dev, const int64_t *order_dev,
                                           const int64_t *tile_base_dev, int32_t *labels_dev, uint8_t *keep_dev, double *kept_lo_dev,
                                           double *kept_hi_dev, int32_t *seg_dev, void *workspace, int64_t workspace_bytes, void *stream) {
    const char *who = "mspa_dbscan_segments_device";
    const int64_t N = dbscan::checked_batch(who, offsets_host, S, C, eps, min_points);
    if (N < 0) return MSPA_EINVAL;
    if (!seg_dev || (N > 0 && (!rows_dev || !offsets_dev || !keys_dev || !order_dev || !labels_dev)) ||
        (keep_dev && S > 0 && (!kept_lo_dev || !kept_hi_dev || (N > 0 && !tile_base_dev))))
        return fail(MSPA_EINVAL, std::string(who) + ": null pointer");
    const int64_t T = segs::extent_tiles(offsets_host, S);
    if (N > 0 && (!workspace || workspace_bytes < dbscan::Workspace(N, S, T).bytes))
        return fail(MSPA_EINVAL, std::string(who) + ": workspace null or smaller than mspa_dbscan_segments_workspace_bytes()");
    if (N > 0 && ((uintptr_t)workspace & 15u)) return fail(MSPA_EINVAL, std::string(who) + ": workspace must be 16-byte aligned");
    if (segs::misaligned(rows_dev, 8) || segs::misaligned(offsets_dev, 8) || segs::misaligned(keys_dev, 8) ||
        segs::misaligned(order_dev, 8) || segs::misaligned(labels_dev, 4) || segs::misaligned(seg_dev, 4) ||
        segs::misaligned(tile_base_dev, 8) || segs::misaligned(kept_lo_dev, 8) || segs::misaligned(kept_hi_dev, 8))
        return fail(MSPA_EINVAL, std::string(who) + ": a buffer is not aligned to its element");
    hipStream_t st = (hipStream_t)stream;
    if (S > 0 && check_hip(hipMemsetAsync(seg_dev, 0, (size_t)S * 8, st), who) != MSPA_OK) return MSPA_EHIP;   // kept and clusters; not the flag word
    if (N == 0) return MSPA_OK;                                  // (no rows: the counts are zero and nothing else is written)
    const dbscan::Workspace ws(N, S, T);
    uint8_t *base = (uint8_t *)workspace;
    double *pts = (double *)(base + ws.pts);
    int64_t *keys = (int64_t *)(base + ws.keys), *reps = (int64_t *)(base + ws.reps), *totals = (int64_t *)(base + ws.totals);
    int32_t *row = (int32_t *)(base + ws.row), *parent = (int32_t *)(base + ws.parent), *root = (int32_t *)(base + ws.root);
    int32_t *sizes = (int32_t *)(base + ws.sizes), *tile_counts = (int32_t *)(base + ws.tile_counts), *best = (int32_t *)(base + ws.best);
    uint8_t *core = base + ws.core;
    int32_t *seg_kept = seg_dev, *seg_clusters = seg_dev + S, *flag_word = seg_dev + 2 * S;
    const double eps_sq = eps * eps;
    const dim3 per_row((unsigned)((N + dbscan::kBlock - 1) / dbscan::kBlock)), per_segment((unsigned)((S + dbscan::kBlock - 1) / dbscan::kBlock));
    const dim3 block(dbscan::kBlock);
    // sizes from 0; parent and labels from -1, so that an order_dev that is no permutation leaves "not core" and "noise", not stale bytes
    if (check_hip(hipMemsetAsync(sizes, 0, (size_t)N * 4, st), who) != MSPA_OK ||
        check_hip(hipMemsetAsync(parent, 0xff, (size_t)N * 4, st), who) != MSPA_OK ||
        check_hip(hipMemsetAsync(labels_dev, 0xff, (size_t)N * 4, st), who) != MSPA_OK)
        return MSPA_EHIP;
    hipLaunchKernelGGL(dbscan::db_gather_kernel, per_row, block, 0, st, rows_dev, C, offsets_dev, S, N, keys_dev, order_dev, pts, keys, row);
    hipLaunchKernelGGL(dbscan::db_core_kernel, per_row, block, 0, st, (const double *)pts, (const int64_t *)keys, (const int32_t *)row, offsets_dev, S,
                       N, eps_sq, min_points, core, parent);
    hipLaunchKernelGGL(dbscan::db_link_kernel, per_row, block, 0, st, (const double *)pts, (const int64_t *)keys, (const int32_t *)row,
                       (const uint8_t *)core, offsets_dev, S, N, eps_sq, parent, flag_word);
    hipLaunchKernelGGL(dbscan::db_roots_kernel, per_row, block, 0, st, parent, offsets_dev, S, N, root, flag_word);
    segs::compact(dbscan::RepFlag{root}, N, tile_counts, totals, reps, false, st);
    hipLaunchKernelGGL(dbscan::db_segment_clusters_kernel, per_segment, block, 0, st, (const int64_t *)reps, (const int64_t *)totals, offsets_dev, S,
                       seg_clusters);
    hipLaunchKernelGGL(dbscan::db_labels_kernel, per_row, block, 0, st, (const double *)pts, (const int64_t *)keys, (const int32_t *)row,
                       (const uint8_t *)core, (const int32_t *)root, (const int64_t *)reps, (const int64_t *)totals, offsets_dev, S, N, eps_sq,
                       labels_dev, sizes);
    if (keep_dev) {
        hipLaunchKernelGGL(dbscan::db_largest_kernel, dim3((unsigned)S), dim3(kWave), 0, st, (const int32_t *)sizes, (const int64_t *)reps,
                           (const int64_t *)totals, offsets_dev, best, seg_kept);
        hipLaunchKernelGGL(dbscan::db_keep_kernel, per_row, block, 0, st, (const int32_t *)labels_dev, (const int32_t *)best, offsets_dev, S, N,
                           keep_dev);
        double *part = (double *)(base + ws.part);
        hipLaunchKernelGGL((segs::extent_tiles_kernel<2, dbscan::KeptFlag>), dim3((unsigned)T), block, 0, st, rows_dev, C, offsets_dev,
                           tile_base_dev, S, part, dbscan::KeptFlag{keep_dev});
        hipLaunchKernelGGL(segs::extent_fold_kernel<2>, dim3((unsigned)S), dim3(kWave), 0, st, (const double *)part, tile_base_dev, kept_lo_dev,
                           kept_hi_dev);
    }
    return check_hip(hipGetLastError(), who);
}

extern "C" int mspa_dbscan_segments_host(const double *rows_host, int64_t C, const int64_t *offsets_host, int64_t S, double eps,
                                         int64_t min_points, int32_t *labels_host, int32_t *clusters_host, uint8_t *keep_host,
                                         int32_t *kept_host, int32_t *flags_out) {
    const char *who = "mspa_dbscan_segments_host";
    const int64_t N = dbscan::checked_batch(who, offsets_host, S, C, eps, min_points);
    if (N < 0) return MSPA_EINVAL;
    if (!flags_out || (S > 0 && !clusters_host) || (N > 0 && (!rows_host || !labels_host)) || (keep_host && S > 0 && !kept_host))
        return fail(MSPA_EINVAL, std::string(who) + ": null pointer");
    *flags_out = dbscan::dbscan_all(rows_host, C, offsets_host, S, eps, min_points, labels_host, clusters_host, keep_host, kept_host);
    return MSPA_OK;
}
