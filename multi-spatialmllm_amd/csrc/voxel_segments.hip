// Voxel-grid down-sampling of a RAGGED BATCH of clouds ON the MI355X: one output row per occupied voxel of every segment, the mean
// of each column over the voxel's rows, in a number of launches that does not depend on the number of segments and with results
// that are the same bits on every run.  The rule -- grid origin, index, key, the order of the sums -- is csrc/voxel_grid_core.h;
// this file holds the op's own kernels, the host twin's entry point and the C ABI; the extents pass and the compaction are the
// batch's shared passes (csrc/segments_device.h).
//
// Three entry points around two torch.sorts (plumbing: stably by key, then stably by segment) and one read-back:
//   mspa_voxel_segments_keys_device
//     1. extent_tiles_kernel<1, TakeAll>  one workgroup per tile of 4 096 rows of ONE segment (tile_base: the host's prefix of the
//        segments' tiles): the per-axis minimum of the tile.  A segment of 1.5 M rows is 367 workgroups, not one.
//     2. extent_fold_kernel<1>    one wave per segment: the minimum over its tiles -> lo [S, 3] (min is order-independent).
//     3. vox_keys_kernel          one thread per row: its segment (binary search in the offsets), its 63-bit key, its segment id
//        beside it; a non-finite or out-of-range row ORs its bit into the flag word (an integer OR does not depend on arrival order).
//   mspa_voxel_segments_heads_device
//     4. vox_heads_kernel         one thread per sorted slot: the slot opens a voxel when it is the first of its segment or its key
//        differs from its predecessor's.  Order entries are clamped into [0, N) and into the slot's segment.
//     5. flag_count_kernel<HeadFlag>, tile_scan_kernel, flag_place_kernel<HeadFlag>   the heads' slots, compacted in ascending order
//        (compact(): per tile of 2 048 slots a count, one workgroup's exclusive scan, positions from ballots; no atomics)
//        -> run_start [M + 1] (run_start[M] = N), so run v has run_start[v + 1] - run_start[v] rows.
//     6. vox_segment_counts_kernel  one thread per segment: its voxels, by two binary searches in run_start.
//   mspa_voxel_segments_means_device  (after the read-back of the counts: M is the host's)
//     7. the same compaction over the voxels with the flag "run longer than 64" -> the list of long runs.
//     8. vox_short_means_kernel   one lane per voxel: counts, and for a run of m <= 64 the sequential sums of every column.
//     9. vox_long_means_kernel    one wave per long run, waves striding over the list: 64 lane sums, folded by strides 32 .. 1.
#include "mspa_common.h"
#include "voxel_grid_core.h"
#include "segments_device.h"

namespace mspa {
namespace voxel {

using segs::kBlock;
using segs::kFlagTile;
using segs::kWaves;

static_assert(kLanes == kWave, "the strided order has one lane per lane of a wave");

__global__ void __launch_bounds__(kBlock) vox_keys_kernel(const double *__restrict__ rows, int64_t C, const int64_t *__restrict__ offsets, int64_t S,
                                                          int64_t N, const double *__restrict__ lo, double voxel_size, int64_t *__restrict__ keys,
                                                          int32_t *__restrict__ segment, int32_t *__restrict__ flag_word) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const int64_t s = segment_of(offsets, S, i);
    const double p[3] = {rows[i * C], rows[i * C + 1], rows[i * C + 2]};
    const double l[3] = {lo[s * 3], lo[s * 3 + 1], lo[s * 3 + 2]};
    int32_t flags = 0;
    keys[i] = row_key(p, l, voxel_size, flags);
    segment[i] = (int32_t)s;
    const uint64_t raised = __ballot(flags != 0);
    if (raised) {                                                // (wave-uniform)
        const int32_t all = (__ballot(flags & kNonFinite) ? kNonFinite : 0) | (__ballot(flags & kOutOfRange) ? kOutOfRange : 0);
        if ((int)(threadIdx.x & 63) == __builtin_ctzll(raised)) atomicOr(flag_word, all);
    }
}

__global__ void __launch_bounds__(kBlock) vox_heads_kernel(const int64_t *__restrict__ keys, const int64_t *__restrict__ order,
                                                           const int64_t *__restrict__ offsets, int64_t S, int64_t N, uint8_t *__restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const int64_t s = segment_of(offsets, S, i);
    const int64_t a = offsets[s], b = offsets[s + 1];
    bool opens = i == a;
    if (!opens) opens = keys[row_in_segment(order[i], N, a, b)] != keys[row_in_segment(order[i - 1], N, a, b)];
    head[i] = opens ? 1 : 0;
}

struct HeadFlag {                                                // slot i opens a voxel
    const uint8_t *head;
    __device__ __forceinline__ bool operator()(int64_t i) const { return head[i] != 0; }
};

struct LongFlag {                                                // voxel v of the runs that exist has more than kSequential rows
    const int64_t *run_start, *total;
    __device__ __forceinline__ bool operator()(int64_t v) const { return v < *total && is_long(run_start[v + 1] - run_start[v]); }
};

__global__ void __launch_bounds__(kBlock) vox_segment_counts_kernel(const int64_t *__restrict__ run_start, const int64_t *__restrict__ total,
                                                                    const int64_t *__restrict__ offsets, int64_t S, int32_t *__restrict__ seg_voxels) {
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= S) return;
    const int64_t a = offsets[s], b = offsets[s + 1], M = *total;
    seg_voxels[s] = b > a ? (int32_t)(first_at_or_above(run_start, 0, M, b) - first_at_or_above(run_start, 0, M, a)) : 0;
}

__global__ void __launch_bounds__(kBlock) vox_short_means_kernel(const double *__restrict__ rows, int64_t C, const int64_t *__restrict__ offsets,
                                                                 int64_t S, int64_t N, const int64_t *__restrict__ order,
                                                                 const int64_t *__restrict__ run_start, const int64_t *__restrict__ total, int64_t M,
                                                                 double *__restrict__ out_rows, int32_t *__restrict__ out_counts) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= M || v >= *total) return;
    const int64_t start = run_start[v], m = run_start[v + 1] - start;
    out_counts[v] = (int32_t)m;
    if (is_long(m)) return;
    const int64_t s = segment_of(offsets, S, start);
    const int64_t a = offsets[s], b = offsets[s + 1];
    for (int64_t c0 = 0; c0 < C; c0 += 3) {                      // three columns per walk over the run: the sums stay in registers
        const int width = C - c0 < 3 ? (int)(C - c0) : 3;
        double sum[3] = {0.0, 0.0, 0.0};
        for (int64_t i = 0; i < m; ++i) {                        // sequential_sum, three columns abreast
            const double *__restrict__ p = rows + row_in_segment(order[start + i], N, a, b) * C + c0;
#pragma unroll
            for (int e = 0; e < 3; ++e)
                if (e < width) sum[e] += p[e];
        }
#pragma unroll
        for (int e = 0; e < 3; ++e)
            if (e < width) out_rows[v * C + c0 + e] = mean_of(sum[e], m);
    }
}

__global__ void __launch_bounds__(kBlock) vox_long_means_kernel(const double *__restrict__ rows, int64_t C, const int64_t *__restrict__ offsets,
                                                                int64_t S, int64_t N, const int64_t *__restrict__ order,
                                                                const int64_t *__restrict__ run_start, const int64_t *__restrict__ long_list,
                                                                const int64_t *__restrict__ n_long, double *__restrict__ out_rows) {
    const int lane = (int)threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * kWaves;
    const int64_t count = *n_long;
    for (int64_t w = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); w < count; w += waves) {
        const int64_t v = long_list[w];
        const int64_t start = run_start[v], m = run_start[v + 1] - start;
        const int64_t s = segment_of(offsets, S, start);
        const int64_t a = offsets[s], b = offsets[s + 1];
        for (int64_t c = 0; c < C; ++c) {
            double p = lane_sum(lane, m, [&](int64_t i) { return rows[row_in_segment(order[start + i], N, a, b) * C + c]; });
#pragma unroll
            for (int t = kLanes / 2; t >= 1; t >>= 1) p += __shfl_down(p, t, 64);       // lane j < t: partial[j] += partial[j + t]
            if (lane == 0) out_rows[v * C + c] = mean_of(p, m);
        }
    }
}

// The workspace of a batch of N rows in S segments whose extents pass has T tiles, cut into its parts.
struct Workspace {
    int64_t lo, part, head, run_start, tile_counts, totals, long_list, bytes;
    Workspace(int64_t N, int64_t S, int64_t T) {
        lo = 0;
        part = lo + align16(S * 24);
        head = part + align16(T * 24);
        run_start = head + align16(N);
        tile_counts = run_start + align16((N + 1) * 8);
        totals = tile_counts + align16(((N + kFlagTile - 1) / kFlagTile + 1) * 4);
        long_list = totals + 16;
        bytes = long_list + align16((N / (kSequential + 1) + 1) * 8);
    }
};

// N of a batch the entry points take with their column count and workspace, or -1 with the error text set.
int64_t checked_batch(const char *who, const int64_t *offsets_host, int64_t S, int64_t C, bool with_workspace, const void *workspace,
                      int64_t workspace_bytes) {
    const std::string name(who);
    const int64_t N = segs::checked_rows(who, offsets_host, S);
    if (N < 0) return -1;
    if (C < 3 || C > MSPA_VOXEL_MAX_COLUMNS) {
        fail(MSPA_EINVAL, name + ": C must be between 3 and 65536 columns");
        return -1;
    }
    if (with_workspace && N > 0) {
        if (!workspace || workspace_bytes < Workspace(N, S, segs::extent_tiles(offsets_host, S)).bytes) {
            fail(MSPA_EINVAL, name + ": workspace null or smaller than mspa_voxel_segments_workspace_bytes()");
            return -1;
        }
        if ((uintptr_t)workspace & 15u) {
            fail(MSPA_EINVAL, name + ": workspace must be 16-byte aligned");
            return -1;
        }
    }
    return N;
}

}  // namespace voxel
}  // namespace mspa

using namespace mspa;

extern "C" int mspa_voxel_segments_tables_host(const int64_t *offsets_host, int64_t S, int64_t *tile_base_out) {
    if (!tile_base_out) return fail(MSPA_EINVAL, "mspa_voxel_segments_tables_host: null pointer");
    if (voxel::checked_batch("mspa_voxel_segments_tables_host", offsets_host, S, 3, false, nullptr, 0) < 0) return MSPA_EINVAL;
    voxel::tile_table(offsets_host, S, tile_base_out);
    return MSPA_OK;
}

extern "C" int64_t mspa_voxel_segments_workspace_bytes(const int64_t *offsets_host, int64_t S) {
    const int64_t N = voxel::batch_rows(offsets_host, S);
    if (N < 0) return -1;
    return voxel::Workspace(N, S, segs::extent_tiles(offsets_host, S)).bytes;
}

extern "C" int mspa_voxel_segments_keys_device(const double *rows_dev, int64_t C, const int64_t *offsets_host, int64_t S, double voxel_size,
                                               const int64_t *offsets_dev, const int64_t *tile_base_dev, int64_t *keys_dev,
                                               int32_t *segment_dev, int32_t *seg_voxels_dev, void *workspace, int64_t workspace_bytes,
                                               void *stream) {
    const char *who = "mspa_voxel_segments_keys_device";
    if (!voxel::size_ok(voxel_size)) return fail(MSPA_EINVAL, std::string(who) + ": voxel_size must be positive and finite");
    const int64_t N = voxel::checked_batch(who, offsets_host, S, C, true, workspace, workspace_bytes);
    if (N < 0) return MSPA_EINVAL;
    if (!seg_voxels_dev || (N > 0 && (!rows_dev || !offsets_dev || !tile_base_dev || !keys_dev || !segment_dev)))
        return fail(MSPA_EINVAL, std::string(who) + ": null pointer");
    if (segs::misaligned(rows_dev, 8) || segs::misaligned(offsets_dev, 8) || segs::misaligned(tile_base_dev, 8) ||
        segs::misaligned(keys_dev, 8) || segs::misaligned(segment_dev, 4) || segs::misaligned(seg_voxels_dev, 4))
        return fail(MSPA_EINVAL, std::string(who) + ": a buffer is not aligned to its element");
    hipStream_t st = (hipStream_t)stream;
    if (check_hip(hipMemsetAsync(seg_voxels_dev, 0, (size_t)(S + 1) * 4, st), who) != MSPA_OK) return MSPA_EHIP;
    if (N == 0) return MSPA_OK;
    const int64_t T = segs::extent_tiles(offsets_host, S);
    const voxel::Workspace ws(N, S, T);
    double *lo = (double *)((uint8_t *)workspace + ws.lo), *part = (double *)((uint8_t *)workspace + ws.part);
    hipLaunchKernelGGL((segs::extent_tiles_kernel<1, segs::TakeAll>), dim3((unsigned)T), dim3(segs::kBlock), 0, st, rows_dev, C, offsets_dev,
                       tile_base_dev, S, part, segs::TakeAll{});
    hipLaunchKernelGGL(segs::extent_fold_kernel<1>, dim3((unsigned)S), dim3(kWave), 0, st, (const double *)part, tile_base_dev, lo,
                       (double *)nullptr);
    hipLaunchKernelGGL(voxel::vox_keys_kernel, dim3((unsigned)((N + voxel::kBlock - 1) / voxel::kBlock)), dim3(voxel::kBlock), 0, st, rows_dev, C,
                       offsets_dev, S, N, (const double *)lo, voxel_size, keys_dev, segment_dev, seg_voxels_dev + S);
    return check_hip(hipGetLastError(), who);
}

extern "C" int mspa_voxel_segments_heads_device(const int64_t *offsets_host, int64_t S, const int64_t *offsets_dev, const int64_t *keys_dev,
                                                const int64_t *order_dev, int32_t *seg_voxels_dev, void *workspace, int64_t workspace_bytes,
                                                void *stream) {
    const char *who = "mspa_voxel_segments_heads_device";
    const int64_t N = voxel::checked_batch(who, offsets_host, S, 3, true, workspace, workspace_bytes);
    if (N < 0) return MSPA_EINVAL;
    if (N == 0) return MSPA_OK;
    if (!offsets_dev || !keys_dev || !order_dev || !seg_voxels_dev) return fail(MSPA_EINVAL, std::string(who) + ": null pointer");
    if (segs::misaligned(offsets_dev, 8) || segs::misaligned(keys_dev, 8) || segs::misaligned(order_dev, 8) ||
        segs::misaligned(seg_voxels_dev, 4))
        return fail(MSPA_EINVAL, std::string(who) + ": a buffer is not aligned to its element");
    hipStream_t st = (hipStream_t)stream;
    const voxel::Workspace ws(N, S, segs::extent_tiles(offsets_host, S));
    uint8_t *base = (uint8_t *)workspace;
    uint8_t *head = base + ws.head;
    int64_t *run_start = (int64_t *)(base + ws.run_start), *totals = (int64_t *)(base + ws.totals);
    hipLaunchKernelGGL(voxel::vox_heads_kernel, dim3((unsigned)((N + voxel::kBlock - 1) / voxel::kBlock)), dim3(voxel::kBlock), 0, st, keys_dev,
                       order_dev, offsets_dev, S, N, head);
    segs::compact(voxel::HeadFlag{head}, N, (int32_t *)(base + ws.tile_counts), totals, run_start, true, st);
    hipLaunchKernelGGL(voxel::vox_segment_counts_kernel, dim3((unsigned)((S + voxel::kBlock - 1) / voxel::kBlock)), dim3(voxel::kBlock), 0, st,
                       (const int64_t *)run_start, (const int64_t *)totals, offsets_dev, S, seg_voxels_dev);
    return check_hip(hipGetLastError(), who);
}

extern "C" int mspa_voxel_segments_means_device(const double *rows_dev, int64_t C, const int64_t *offsets_host, int64_t S,
                                                const int64_t *offsets_dev, const int64_t *order_dev, int64_t M, double *out_rows_dev,
                                                int32_t *out_counts_dev, void *workspace, int64_t workspace_bytes, void *stream) {
    const char *who = "mspa_voxel_segments_means_device";
    const int64_t N = voxel::checked_batch(who, offsets_host, S, C, true, workspace, workspace_bytes);
    if (N < 0) return MSPA_EINVAL;
    if (M < 0 || M > N) return fail(MSPA_EINVAL, std::string(who) + ": M must be between 0 and the number of rows");
    if (M == 0) return MSPA_OK;
    if (!rows_dev || !offsets_dev || !order_dev || !out_rows_dev || !out_counts_dev) return fail(MSPA_EINVAL, std::string(who) + ": null pointer");
    if (segs::misaligned(rows_dev, 8) || segs::misaligned(offsets_dev, 8) || segs::misaligned(order_dev, 8) ||
        segs::misaligned(out_rows_dev, 8) || segs::misaligned(out_counts_dev, 4))
        return fail(MSPA_EINVAL, std::string(who) + ": a buffer is not aligned to its element");
    hipStream_t st = (hipStream_t)stream;
    const voxel::Workspace ws(N, S, segs::extent_tiles(offsets_host, S));
    uint8_t *base = (uint8_t *)workspace;
    const int64_t *run_start = (const int64_t *)(base + ws.run_start);
    int64_t *totals = (int64_t *)(base + ws.totals), *long_list = (int64_t *)(base + ws.long_list);
    segs::compact(voxel::LongFlag{run_start, totals}, M, (int32_t *)(base + ws.tile_counts), totals + 1, long_list, false, st);
    hipLaunchKernelGGL(voxel::vox_short_means_kernel, dim3((unsigned)((M + voxel::kBlock - 1) / voxel::kBlock)), dim3(voxel::kBlock), 0, st, rows_dev,
                       C, offsets_dev, S, N, order_dev, run_start, (const int64_t *)totals, M, out_rows_dev, out_counts_dev);
    const int64_t most_long = N / (voxel::kSequential + 1);
    if (most_long > 0) {
        const int64_t blocks = (most_long + voxel::kWaves - 1) / voxel::kWaves;
        hipLaunchKernelGGL(voxel::vox_long_means_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(voxel::kBlock), 0, st, rows_dev, C,
                           offsets_dev, S, N, order_dev, run_start, (const int64_t *)long_list, (const int64_t *)(totals + 1), out_rows_dev);
    }
    return check_hip(hipGetLastError(), who);
}

extern "C" int mspa_voxel_segments_host(const double *rows_host, int64_t C, const int64_t *offsets_host, int64_t S, double voxel_size,
                                        double *out_rows_host, int64_t *out_offsets_host, int32_t *out_counts_host, int32_t *flags_out) {
    const char *who = "mspa_voxel_segments_host";
    if (!voxel::size_ok(voxel_size)) return fail(MSPA_EINVAL, std::string(who) + ": voxel_size must be positive and finite");
    const int64_t N = voxel::checked_batch(who, offsets_host, S, C, false, nullptr, 0);
    if (N < 0) return MSPA_EINVAL;
    if (!out_offsets_host || !flags_out || (N > 0 && (!rows_host || !out_rows_host || !out_counts_host)))
        return fail(MSPA_EINVAL, std::string(who) + ": null pointer");
    *flags_out = voxel::down_sample_all(rows_host, C, offsets_host, S, voxel_size, out_rows_host, out_offsets_host, out_counts_host);
    return MSPA_OK;
}
