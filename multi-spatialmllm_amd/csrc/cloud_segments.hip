// Cleaning and boxing a RAGGED BATCH of clouds ON the MI355X: the k-nearest mean distance of cloud_ops.hip and the statistical
// outlier rule for every segment of a batch at once, in a number of launches that does not depend on the number of segments.
// The rule -- a row's segment, its global key, the order of the sums -- is csrc/cloud_segments_core.h on top of
// csrc/knn_grid_core.h; this file holds the kernels, the host twins and the C ABI.
//
// Four kernels around one torch.sort (plumbing, between mspa_knn_segments_cells_device and mspa_knn_segments_mean_distance_device),
// the segmented twins of cloud_ops.hip's, and one more behind them:
//   1. seg_cells_kernel  -- one thread per row: its segment (binary search in the offsets), that segment's grid record from the
//      device table, the key cell_base[s] + cell.
//   2. seg_gather_kernel -- one thread per sorted slot: the row the order names, clamped into [0, N) and then into the slot's own
//      segment, copied next to its neighbours, and its key computed again from the copy.
//   3. seg_starts_kernel -- one thread per slot of the table of starts: the first sorted slot of its segment at or above its
//      cell, by binary search inside the segment, as a segment-local index.
//   4. seg_knn_kernel    -- one lane per sorted slot; each lane loads its own segment's grid record, so a wave may hold rows of
//      several segments.  The k best squared distances are an ascending list in LDS, interleaved by lane, as in knn_kernel.
//   5. seg_stats_kernel  -- one workgroup of 256 per segment, three passes over its avg: sum -> mean, squared deviations -> sd and
//      thr, keep flags with the kept count and the kept rows' extents.  No atomics: lane sums, then folds through LDS.
// Kernels 2 and 3 alone, into caller-owned buffers, are mspa_knn_segments_index_device: the search structure csrc/cloud_distance.hip
// queries from another batch.
#include "mspa_common.h"
#include "segments_device.h"

namespace mspa {
namespace segs {

using knn::Grid;

static_assert(sizeof(Grid) == MSPA_KNN_GRID_BYTES, "include/mspa.h and knn_grid_core.h disagree on the grid record");
static_assert(kMaxSegments == MSPA_SEGMENTS_MAX, "include/mspa.h and cloud_segments_core.h disagree on the most segments");

__global__ void __launch_bounds__(256) seg_cells_kernel(const double *__restrict__ xyz, const int64_t *__restrict__ offsets, int64_t S,
                                                        const Grid *__restrict__ grids, const int64_t *__restrict__ cell_base,
                                                        int64_t *__restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= offsets[S]) return;
    const int64_t s = segment_of(offsets, S, i);
    const Grid g = grids[s];
    keys[i] = key_of(g, cell_base[s], xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
}

__global__ void __launch_bounds__(256) seg_gather_kernel(const double *__restrict__ xyz, const int64_t *__restrict__ offsets, int64_t S,
                                                         const Grid *__restrict__ grids, const int64_t *__restrict__ cell_base,
                                                         const int64_t *__restrict__ order, double *__restrict__ pts,
                                                         int64_t *__restrict__ sorted_keys) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t N = offsets[S];
    if (i >= N) return;
    const int64_t s = segment_of(offsets, S, i);
    const int64_t o = row_in_segment(order[i], N, offsets[s], offsets[s + 1]);
    const double x = xyz[3 * o], y = xyz[3 * o + 1], z = xyz[3 * o + 2];
    pts[3 * i] = x;
    pts[3 * i + 1] = y;
    pts[3 * i + 2] = z;
    const Grid g = grids[s];
    sorted_keys[i] = key_of(g, cell_base[s], x, y, z);
}

__global__ void __launch_bounds__(256) seg_starts_kernel(const int64_t *__restrict__ sorted_keys, const int64_t *__restrict__ offsets, int64_t S,
                                                         const Grid *__restrict__ grids, const int64_t *__restrict__ cell_base,
                                                         int32_t *__restrict__ starts) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= cell_base[S] + S) return;
    int64_t lo = 0, hi = S;                                      // the segment of slot t: starts_base(lo) <= t < starts_base(hi)
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (starts_base(cell_base, mid) <= t) lo = mid;
        else hi = mid;
    }
    const int64_t c = t - starts_base(cell_base, lo);
    if (c > grids[lo].cells) return;                             // slots behind the segment's cells: never read
    const int64_t a = offsets[lo], b = offsets[lo + 1];
    starts[t] = (int32_t)(first_at_or_above(sorted_keys, a, b, cell_base[lo] + c) - a);
}

struct LdsList {
    double *base;
    __device__ __forceinline__ double &operator[](int32_t j) const { return base[j * kWave]; }
};

__global__ void __launch_bounds__(kWave) seg_knn_kernel(const double *__restrict__ pts, const int32_t *__restrict__ starts,
                                                        const int64_t *__restrict__ offsets, int64_t S, const Grid *__restrict__ grids,
                                                        const int64_t *__restrict__ cell_base, const int64_t *__restrict__ order, int32_t k,
                                                        double *__restrict__ mean, int32_t *__restrict__ evals) {
    extern __shared__ double lists[];                            // [k][kWave]
    const int64_t i = (int64_t)blockIdx.x * kWave + threadIdx.x;
    const int64_t N = offsets[S];
    if (i >= N) return;
    const int64_t s = segment_of(offsets, S, i);
    const int64_t a = offsets[s], n = offsets[s + 1] - a;
    const int32_t kk = (int32_t)(k < n ? k : n);
    const Grid g = grids[s];
    const double q[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    const LdsList best{lists + threadIdx.x};
    const int64_t e = knn::walk(g, pts + 3 * a, starts + starts_base(cell_base, s), q, kk, best);
    const int64_t o = row_in_segment(order[i], N, a, a + n);
    mean[o] = knn::mean_root(best, kk);
    if (evals) evals[o] = (int32_t)e;
}

// partial[] of kLanes entries, every thread's own written: the fold of cloud_segments_core.h's stated order, the result in every thread.
__device__ __forceinline__ double fold_sum(double *partial, int32_t j) {
    __syncthreads();
    for (int32_t t = kLanes / 2; t >= 1; t >>= 1) {
        if (j < t) partial[j] += partial[j + t];
        __syncthreads();
    }
    const double total = partial[0];
    __syncthreads();                                             // partial[] is free again
    return total;
}

template <bool kMin>
__device__ __forceinline__ double fold_extent(double *partial, int32_t j, double mine) {
    partial[j] = mine;
    __syncthreads();
    for (int32_t t = kLanes / 2; t >= 1; t >>= 1) {
        if (j < t) {
            const double other = partial[j + t];
            if (kMin ? other < partial[j] : other > partial[j]) partial[j] = other;
        }
        __syncthreads();
    }
    const double total = partial[0];
    __syncthreads();
    return total;
}

__global__ void __launch_bounds__(kLanes) seg_stats_kernel(const double *__restrict__ avg, const double *__restrict__ xyz,
                                                           const int64_t *__restrict__ offsets, double std_ratio, uint8_t *__restrict__ keep,
                                                           int64_t *__restrict__ kept, double *__restrict__ mean, double *__restrict__ sd,
                                                           double *__restrict__ thr, double *__restrict__ lo, double *__restrict__ hi) {
    __shared__ double partial[kLanes];
    __shared__ int64_t counts[kLanes];
    const int64_t s = blockIdx.x;
    const int32_t j = threadIdx.x;
    const int64_t a = offsets[s], n = offsets[s + 1] - a;
    const double *__restrict__ v = avg + a;
    partial[j] = lane_sum(j, n, [&](int64_t i) { return positive_term(v[i]); });
    const double m = mean_of(fold_sum(partial, j), n);
    partial[j] = lane_sum(j, n, [&](int64_t i) { return deviation_term(v[i], m); });
    const double d = sd_of(fold_sum(partial, j), n);
    const double t = threshold_of(m, d, std_ratio, n);
    int64_t count = 0;
    double l[3] = {INFINITY, INFINITY, INFINITY}, h[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = j; i < n; i += kLanes) {
        const bool in = stays(v[i], t);
        keep[a + i] = in ? 1 : 0;
        if (!in) continue;
        ++count;
        for (int ax = 0; ax < 3; ++ax) {
            const double x = xyz[3 * (a + i) + ax];
            l[ax] = x < l[ax] ? x : l[ax];
            h[ax] = x > h[ax] ? x : h[ax];
        }
    }
    counts[j] = count;
    __syncthreads();
    for (int32_t w = kLanes / 2; w >= 1; w >>= 1) {
        if (j < w) counts[j] += counts[j + w];
        __syncthreads();
    }
    for (int ax = 0; ax < 3; ++ax) {
        l[ax] = fold_extent<true>(partial, j, l[ax]);
        h[ax] = fold_extent<false>(partial, j, h[ax]);
    }
    if (j == 0) {
        kept[s] = counts[0];
        mean[s] = m;
        sd[s] = d;
        thr[s] = t;
        for (int ax = 0; ax < 3; ++ax) {
            lo[3 * s + ax] = l[ax];
            hi[3 * s + ax] = h[ax];
        }
    }
}

}  // namespace segs
}  // namespace mspa

using namespace mspa;

extern "C" int mspa_knn_segments_tables_host(const int64_t *offsets_host, int64_t S, int32_t k, int64_t *cell_base_out) {
    if (!cell_base_out) return fail(MSPA_EINVAL, "mspa_knn_segments_tables_host: null pointer");
    if (k < 1 || k > knn::kMaxK) return fail(MSPA_EINVAL, "mspa_knn_segments_tables_host: k outside [1, 64]");
    if (segs::checked_rows("mspa_knn_segments_tables_host", offsets_host, S) < 0) return MSPA_EINVAL;
    segs::cell_tables(offsets_host, S, k, cell_base_out);
    return MSPA_OK;
}

extern "C" int mspa_knn_segments_grids_host(const double *lo, const double *hi, const int64_t *offsets_host, int64_t S, int32_t k,
                                            void *grids_out) {
    if (k < 1 || k > knn::kMaxK) return fail(MSPA_EINVAL, "mspa_knn_segments_grids_host: k outside [1, 64]");
    if (segs::checked_rows("mspa_knn_segments_grids_host", offsets_host, S) < 0) return MSPA_EINVAL;
    if (S == 0) return MSPA_OK;
    if (!lo || !hi || !grids_out) return fail(MSPA_EINVAL, "mspa_knn_segments_grids_host: null pointer");
    if (!segs::make_grids(lo, hi, offsets_host, S, k, (knn::Grid *)grids_out))
        return fail(MSPA_EINVAL, "mspa_knn_segments_grids_host: a non-empty segment's box must be finite with lo <= hi and have a grid");
    return MSPA_OK;
}

extern "C" int64_t mspa_knn_segments_workspace_bytes(const int64_t *offsets_host, int64_t S, int32_t k) {
    if (k < 1 || k > knn::kMaxK) return -1;
    const int64_t N = segs::batch_rows(offsets_host, S);
    if (N < 0) return -1;
    int64_t cells = 0;
    for (int64_t s = 0; s < S; ++s)
        if (offsets_host[s + 1] > offsets_host[s]) cells += knn::max_cells(offsets_host[s + 1] - offsets_host[s], k);
    return align16(N * 24) + align16(N * 8) + align16((cells + S) * 4);
}

extern "C" int mspa_knn_segments_cells_device(const double *xyz_dev, const int64_t *offsets_host, int64_t S, const void *grids_host,
                                              const int64_t *offsets_dev, const void *grids_dev, const int64_t *cell_base_dev,
                                              int64_t *keys_dev, void *stream) {
    const int64_t N = segs::checked_rows("mspa_knn_segments_cells_device", offsets_host, S);
    if (N < 0) return MSPA_EINVAL;
    if (N == 0) return MSPA_OK;
    if (!xyz_dev || !grids_host || !offsets_dev || !grids_dev || !cell_base_dev || !keys_dev)
        return fail(MSPA_EINVAL, "mspa_knn_segments_cells_device: null pointer");
    if (!segs::grids_ok((const knn::Grid *)grids_host, offsets_host, S, 1))
        return fail(MSPA_EINVAL, "mspa_knn_segments_cells_device: not the grids of mspa_knn_segments_grids_host");
    hipLaunchKernelGGL(segs::seg_cells_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, xyz_dev, offsets_dev, S,
                       (const knn::Grid *)grids_dev, cell_base_dev, keys_dev);
    return check_hip(hipGetLastError(), "mspa_knn_segments_cells_device");
}

// The slots of a batch's table of starts: one more than its cells per segment, also for an empty one.
static int64_t index_slots(const int64_t *offsets_host, int64_t S, int32_t k) {
    int64_t slots = S;
    for (int64_t s = 0; s < S; ++s)
        if (offsets_host[s + 1] > offsets_host[s]) slots += knn::max_cells(offsets_host[s + 1] - offsets_host[s], k);
    return slots;
}

// The gather and the starts of a sorted batch of N >= 1 rows: the two launches every search of a batch is built on.
static void launch_index(const double *xyz_dev, int64_t N, int64_t S, int64_t slots, const int64_t *offsets_dev, const knn::Grid *grids,
                         const int64_t *cell_base_dev, const int64_t *order_dev, double *pts, int64_t *sorted_keys, int32_t *starts,
                         hipStream_t st) {
    hipLaunchKernelGGL(segs::seg_gather_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, xyz_dev, offsets_dev, S, grids, cell_base_dev,
                       order_dev, pts, sorted_keys);
    hipLaunchKernelGGL(segs::seg_starts_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, (const int64_t *)sorted_keys, offsets_dev,
                       S, grids, cell_base_dev, starts);
}

extern "C" int mspa_knn_segments_index_device(const double *xyz_dev, const int64_t *offsets_host, int64_t S, int32_t k, const void *grids_host,
                                              const int64_t *offsets_dev, const void *grids_dev, const int64_t *cell_base_dev,
                                              const int64_t *order_dev, double *pts_dev, int64_t *sorted_keys_dev, int32_t *starts_dev,
                                              int64_t starts_slots, void *stream) {
    const char *who = "mspa_knn_segments_index_device";
    if (k < 1 || k > knn::kMaxK) return fail(MSPA_EINVAL, std::string(who) + ": k outside [1, 64]");
    const int64_t N = segs::checked_rows(who, offsets_host, S);
    if (N < 0) return MSPA_EINVAL;
    if (N == 0) return MSPA_OK;
    if (!xyz_dev || !grids_host || !offsets_dev || !grids_dev || !cell_base_dev || !order_dev || !pts_dev || !sorted_keys_dev || !starts_dev)
        return fail(MSPA_EINVAL, std::string(who) + ": null pointer");
    if (!segs::grids_ok((const knn::Grid *)grids_host, offsets_host, S, k))
        return fail(MSPA_EINVAL, std::string(who) + ": not the grids of mspa_knn_segments_grids_host for these offsets and k");
    const int64_t slots = index_slots(offsets_host, S, k);
    if (starts_slots < slots) return fail(MSPA_EINVAL, std::string(who) + ": starts_dev holds fewer slots than the batch's cells plus S");
    if (segs::misaligned(xyz_dev, 8) || segs::misaligned(pts_dev, 8) || segs::misaligned(sorted_keys_dev, 8) || segs::misaligned(order_dev, 8) ||
        segs::misaligned(starts_dev, 4))
        return fail(MSPA_EINVAL, std::string(who) + ": a buffer is not aligned to its element");
    launch_index(xyz_dev, N, S, slots, offsets_dev, (const knn::Grid *)grids_dev, cell_base_dev, order_dev, pts_dev, sorted_keys_dev, starts_dev,
                 (hipStream_t)stream);
    return check_hip(hipGetLastError(), who);
}

extern "C" int mspa_knn_segments_mean_distance_device(const double *xyz_dev, const int64_t *offsets_host, int64_t S, int32_t k,
                                                      const void *grids_host, const int64_t *offsets_dev, const void *grids_dev,
                                                      const int64_t *cell_base_dev, const int64_t *order_dev, double *mean_dev,
                                                      int32_t *evals_dev, void *workspace, int64_t workspace_bytes, void *stream) {
    if (k < 1 || k > knn::kMaxK) return fail(MSPA_EINVAL, "mspa_knn_segments_mean_distance_device: k outside [1, 64]");
    const int64_t N = segs::checked_rows("mspa_knn_segments_mean_distance_device", offsets_host, S);
    if (N < 0) return MSPA_EINVAL;
    if (N == 0) return MSPA_OK;
    if (!xyz_dev || !grids_host || !offsets_dev || !grids_dev || !cell_base_dev || !order_dev || !mean_dev || !workspace)
        return fail(MSPA_EINVAL, "mspa_knn_segments_mean_distance_device: null pointer");
    if (!segs::grids_ok((const knn::Grid *)grids_host, offsets_host, S, k))
        return fail(MSPA_EINVAL, "mspa_knn_segments_mean_distance_device: not the grids of mspa_knn_segments_grids_host for these offsets and k");
    if (workspace_bytes < mspa_knn_segments_workspace_bytes(offsets_host, S, k))
        return fail(MSPA_EINVAL, "mspa_knn_segments_mean_distance_device: workspace smaller than mspa_knn_segments_workspace_bytes()");
    if ((uintptr_t)workspace & 15u) return fail(MSPA_EINVAL, "mspa_knn_segments_mean_distance_device: workspace must be 16-byte aligned");
    const int64_t slots = index_slots(offsets_host, S, k);
    hipStream_t st = (hipStream_t)stream;
    const knn::Grid *grids = (const knn::Grid *)grids_dev;
    double *pts = (double *)workspace;
    int64_t *sorted_keys = (int64_t *)((uint8_t *)workspace + align16(N * 24));
    int32_t *starts = (int32_t *)((uint8_t *)sorted_keys + align16(N * 8));
    launch_index(xyz_dev, N, S, slots, offsets_dev, grids, cell_base_dev, order_dev, pts, sorted_keys, starts, st);
    hipLaunchKernelGGL(segs::seg_knn_kernel, dim3((unsigned)((N + kWave - 1) / kWave)), dim3(kWave), (size_t)k * kWave * sizeof(double), st,
                       (const double *)pts, (const int32_t *)starts, offsets_dev, S, grids, cell_base_dev, order_dev, k, mean_dev, evals_dev);
    return check_hip(hipGetLastError(), "mspa_knn_segments_mean_distance_device");
}

extern "C" int mspa_outlier_segments_device(const double *avg_dev, const double *xyz_dev, const int64_t *offsets_host, int64_t S,
                                            double std_ratio, const int64_t *offsets_dev, uint8_t *keep_dev, int64_t *kept_dev,
                                            double *mean_dev, double *sd_dev, double *thr_dev, double *lo_dev, double *hi_dev, void *stream) {
    if (!(fabs(std_ratio) < INFINITY)) return fail(MSPA_EINVAL, "mspa_outlier_segments_device: std_ratio must be finite");
    const int64_t N = segs::checked_rows("mspa_outlier_segments_device", offsets_host, S);
    if (N < 0) return MSPA_EINVAL;
    if (S == 0) return MSPA_OK;
    if (!offsets_dev || !kept_dev || !mean_dev || !sd_dev || !thr_dev || !lo_dev || !hi_dev || (N > 0 && (!avg_dev || !xyz_dev || !keep_dev)))
        return fail(MSPA_EINVAL, "mspa_outlier_segments_device: null pointer");
    hipLaunchKernelGGL(segs::seg_stats_kernel, dim3((unsigned)S), dim3(segs::kLanes), 0, (hipStream_t)stream, avg_dev, xyz_dev, offsets_dev,
                       std_ratio, keep_dev, kept_dev, mean_dev, sd_dev, thr_dev, lo_dev, hi_dev);
    return check_hip(hipGetLastError(), "mspa_outlier_segments_device");
}

extern "C" int mspa_knn_segments_mean_distance_host(const double *xyz_host, const int64_t *offsets_host, int64_t S, int32_t k,
                                                    double *mean_host, int32_t *evals_host) {
    if (k < 1 || k > knn::kMaxK) return fail(MSPA_EINVAL, "mspa_knn_segments_mean_distance_host: k outside [1, 64]");
    const int64_t N = segs::checked_rows("mspa_knn_segments_mean_distance_host", offsets_host, S);
    if (N < 0) return MSPA_EINVAL;
    if (N == 0) return MSPA_OK;
    if (!xyz_host || !mean_host) return fail(MSPA_EINVAL, "mspa_knn_segments_mean_distance_host: null pointer");
    for (int64_t i = 0; i < 3 * N; ++i)
        if (!(fabs(xyz_host[i]) < INFINITY)) return fail(MSPA_EINVAL, "mspa_knn_segments_mean_distance_host: non-finite coordinate");
    if (!segs::mean_distance_segments_all(xyz_host, offsets_host, S, k, mean_host, evals_host))
        return fail(MSPA_EINVAL, "mspa_knn_segments_mean_distance_host: no grid for a segment");
    return MSPA_OK;
}

extern "C" int mspa_outlier_segments_host(const double *avg_host, const double *xyz_host, const int64_t *offsets_host, int64_t S,
                                          double std_ratio, uint8_t *keep_host, int64_t *kept_host, double *mean_host, double *sd_host,
                                          double *thr_host, double *lo_host, double *hi_host) {
    if (!(fabs(std_ratio) < INFINITY)) return fail(MSPA_EINVAL, "mspa_outlier_segments_host: std_ratio must be finite");
    const int64_t N = segs::checked_rows("mspa_outlier_segments_host", offsets_host, S);
    if (N < 0) return MSPA_EINVAL;
    if (S == 0) return MSPA_OK;
    if (!kept_host || !mean_host || !sd_host || !thr_host || !lo_host || !hi_host || (N > 0 && (!avg_host || !xyz_host || !keep_host)))
        return fail(MSPA_EINVAL, "mspa_outlier_segments_host: null pointer");
    segs::outlier_segments_all(avg_host, xyz_host, offsets_host, S, std_ratio, keep_host, kept_host, mean_host, sd_host, thr_host, lo_host, hi_host);
    return MSPA_OK;
}
