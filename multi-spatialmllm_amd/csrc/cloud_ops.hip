// Point-cloud cleaning ON the MI355X: the mean distance of every point to its k nearest points (itself included, at distance
// 0), exact, in float64 -- the quantity behind Open3D's remove_statistical_outlier, which the reference's
// remove_statistical_outliers (handler/ops.py:138-160) runs through a KD-tree on one core.  The rule -- cell of a point, bound
// of a visited block, the walk -- is csrc/knn_grid_core.h; this file holds the kernels, the host twin and the C ABI.
//
// Four kernels around one torch.sort (plumbing, between mspa_knn_cells_device and mspa_knn_mean_distance_device):
//   1. cells_kernel  -- one thread per point: its cell id.
//   2. gather_kernel -- one thread per sorted slot: the point the order names, copied next to its neighbours, and its cell id
//      computed again (the order is the caller's: whatever it holds, every index used below stays inside the buffers).
//   3. starts_kernel -- one thread per cell: the first sorted slot at or above it, by binary search.
//   4. knn_kernel    -- one lane per query, in sorted order, so a wave's lanes walk the same few cells.  The k best squared
//      distances are an ascending list in LDS, interleaved by lane (entry j of lane l at j * 64 + l: conflict-free).
#include "mspa_common.h"
#include "knn_grid_core.h"

namespace mspa {
namespace knn {

static_assert(sizeof(Grid) == MSPA_KNN_GRID_BYTES, "include/mspa.h and knn_grid_core.h disagree on the grid record");
static_assert(kMaxK == MSPA_KNN_MAX_K, "include/mspa.h and knn_grid_core.h disagree on the largest k");

__global__ void __launch_bounds__(256) cells_kernel(Grid g, const double *__restrict__ xyz, int64_t n, int32_t *__restrict__ cells) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    cells[i] = cell_of(g, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
}

__global__ void __launch_bounds__(256) gather_kernel(Grid g, const double *__restrict__ xyz, const int64_t *__restrict__ order, int64_t n,
                                                     double *__restrict__ pts, int32_t *__restrict__ sorted_cells) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int64_t o = order[i];
    o = o < 0 ? 0 : o >= n ? n - 1 : o;
    const double x = xyz[3 * o], y = xyz[3 * o + 1], z = xyz[3 * o + 2];
    pts[3 * i] = x;
    pts[3 * i + 1] = y;
    pts[3 * i + 2] = z;
    sorted_cells[i] = cell_of(g, x, y, z);
}

__global__ void __launch_bounds__(256) starts_kernel(const int32_t *__restrict__ sorted_cells, int64_t n, int32_t cells,
                                                     int32_t *__restrict__ starts) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c > cells) return;
    int64_t lo = 0, hi = n;                                      // sorted_cells[lo - 1] < c <= sorted_cells[hi]
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (sorted_cells[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    starts[c] = (int32_t)lo;
}

struct LdsList {
    double *base;
    __device__ __forceinline__ double &operator[](int32_t j) const { return base[j * kWave]; }
};

__global__ void __launch_bounds__(kWave) knn_kernel(Grid g, const double *__restrict__ pts, const int32_t *__restrict__ starts,
                                                    const int64_t *__restrict__ order, int64_t n, int32_t k, double *__restrict__ mean,
                                                    int32_t *__restrict__ evals) {
    extern __shared__ double lists[];                            // [k][kWave]
    const int64_t i = (int64_t)blockIdx.x * kWave + threadIdx.x;
    if (i >= n) return;
    const double q[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    const LdsList best{lists + threadIdx.x};
    const int64_t e = walk(g, pts, starts, q, k, best);
    int64_t o = order[i];
    o = o < 0 ? 0 : o >= n ? n - 1 : o;
    mean[o] = mean_root(best, (int32_t)(k < n ? k : n));
    if (evals) evals[o] = (int32_t)e;
}

}  // namespace knn
}  // namespace mspa

using namespace mspa;

extern "C" int mspa_knn_grid_host(const double *lo, const double *hi, int64_t n, int32_t k, void *grid_out) {
    if (!lo || !hi || !grid_out) return fail(MSPA_EINVAL, "mspa_knn_grid_host: null pointer");
    if (n < 1 || n > knn::kMaxPoints || k < 1 || k > knn::kMaxK) return fail(MSPA_EINVAL, "mspa_knn_grid_host: n outside [1, 2^30] or k outside [1, 64]");
    for (int a = 0; a < 3; ++a)
        if (!(fabs(lo[a]) < INFINITY) || !(fabs(hi[a]) < INFINITY) || !(lo[a] <= hi[a]))
            return fail(MSPA_EINVAL, "mspa_knn_grid_host: the box must be finite with lo <= hi");
    knn::Grid g;
    memset(&g, 0, sizeof(g));
    knn::make_grid(lo, hi, n, k, g);
    if (!knn::grid_ok(g, n, k)) return fail(MSPA_EINVAL, "mspa_knn_grid_host: no grid for this box");
    memcpy(grid_out, &g, sizeof(g));
    return MSPA_OK;
}

extern "C" int64_t mspa_knn_workspace_bytes(int64_t n, int32_t k) {
    if (n < 0 || n > knn::kMaxPoints || k < 1 || k > knn::kMaxK) return -1;
    return align16(n * 24) + align16(n * 4) + align16((knn::max_cells(n, k) + 1) * 4);
}

extern "C" int mspa_knn_cells_device(const double *xyz_dev, int64_t n, const void *grid_host, int32_t *cells_dev, void *stream) {
    if (n < 0 || n > knn::kMaxPoints) return fail(MSPA_EINVAL, "mspa_knn_cells_device: bad size");
    if (n == 0) return MSPA_OK;
    if (!xyz_dev || !grid_host || !cells_dev) return fail(MSPA_EINVAL, "mspa_knn_cells_device: null pointer");
    knn::Grid g;
    memcpy(&g, grid_host, sizeof(g));
    if (!knn::grid_ok(g, n, 1)) return fail(MSPA_EINVAL, "mspa_knn_cells_device: not a grid of mspa_knn_grid_host");
    hipLaunchKernelGGL(knn::cells_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, xyz_dev, n, cells_dev);
    return check_hip(hipGetLastError(), "mspa_knn_cells_device");
}

extern "C" int mspa_knn_mean_distance_device(const double *xyz_dev, int64_t n, int32_t k, const void *grid_host, const int64_t *order_dev,
                                             double *mean_dev, int32_t *evals_dev, void *workspace, int64_t workspace_bytes, void *stream) {
    if (n < 0 || n > knn::kMaxPoints) return fail(MSPA_EINVAL, "mspa_knn_mean_distance_device: bad size");
    if (k < 1 || k > knn::kMaxK) return fail(MSPA_EINVAL, "mspa_knn_mean_distance_device: k outside [1, 64]");
    if (n == 0) return MSPA_OK;
    if (!xyz_dev || !grid_host || !order_dev || !mean_dev || !workspace) return fail(MSPA_EINVAL, "mspa_knn_mean_distance_device: null pointer");
    knn::Grid g;
    memcpy(&g, grid_host, sizeof(g));
    if (!knn::grid_ok(g, n, k)) return fail(MSPA_EINVAL, "mspa_knn_mean_distance_device: not a grid of mspa_knn_grid_host for this n and k");
    if (workspace_bytes < mspa_knn_workspace_bytes(n, k))
        return fail(MSPA_EINVAL, "mspa_knn_mean_distance_device: workspace smaller than mspa_knn_workspace_bytes()");
    if ((uintptr_t)workspace & 15u) return fail(MSPA_EINVAL, "mspa_knn_mean_distance_device: workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    double *pts = (double *)workspace;
    int32_t *sorted_cells = (int32_t *)((uint8_t *)workspace + align16(n * 24));
    int32_t *starts = (int32_t *)((uint8_t *)sorted_cells + align16(n * 4));
    hipLaunchKernelGGL(knn::gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g, xyz_dev, order_dev, n, pts, sorted_cells);
    hipLaunchKernelGGL(knn::starts_kernel, dim3((unsigned)(((int64_t)g.cells + 1 + 255) / 256)), dim3(256), 0, st,
                       (const int32_t *)sorted_cells, n, g.cells, starts);
    hipLaunchKernelGGL(knn::knn_kernel, dim3((unsigned)((n + kWave - 1) / kWave)), dim3(kWave), (size_t)k * kWave * sizeof(double), st, g,
                       (const double *)pts, (const int32_t *)starts, order_dev, n, k, mean_dev, evals_dev);
    return check_hip(hipGetLastError(), "mspa_knn_mean_distance_device");
}

// The same search on the CPU, through the same header: box from the order statistics of rank n / 100 and n - 1 - n / 100 per
// axis (what mspa.engine.knn_mean_distance reads off a device sort), a stable order by cell, the walk per point.
extern "C" int mspa_knn_mean_distance_host(const double *xyz_host, int64_t n, int32_t k, double *mean_host, int32_t *evals_host) {
    if (n < 0 || n > knn::kMaxPoints) return fail(MSPA_EINVAL, "mspa_knn_mean_distance_host: bad size");
    if (k < 1 || k > knn::kMaxK) return fail(MSPA_EINVAL, "mspa_knn_mean_distance_host: k outside [1, 64]");
    if (n == 0) return MSPA_OK;
    if (!xyz_host || !mean_host) return fail(MSPA_EINVAL, "mspa_knn_mean_distance_host: null pointer");
    for (int64_t i = 0; i < 3 * n; ++i)
        if (!(fabs(xyz_host[i]) < INFINITY)) return fail(MSPA_EINVAL, "mspa_knn_mean_distance_host: non-finite coordinate");
    if (!knn::mean_distance_all(xyz_host, n, k, mean_host, evals_host)) return fail(MSPA_EINVAL, "mspa_knn_mean_distance_host: no grid for this cloud");
    return MSPA_OK;
}
