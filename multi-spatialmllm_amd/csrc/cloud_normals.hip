// The k nearest rows and the normal of every row of a ragged batch of clouds ON the MI355X.  The rule -- the neighbours and why the walk
// may stop at the k-th, the moments, the Jacobi sweeps, the sign, the status -- is csrc/cloud_normals_core.h on top of
// csrc/cloud_distance_core.h, csrc/cloud_segments_core.h and csrc/knn_grid_core.h; this file holds the kernel, the host twin's entry
// point and the C ABI.  The search structure of the batch (sorted points, order, starts) is built by mspa_knn_segments_index_device
// (csrc/cloud_segments.hip) with the gather and the starts kernels every batched search uses.
//
//   seg_normals_kernel<kFit, kTable>  seg_knn_kernel's form: one lane per sorted slot, workgroups of one wave, the list in dynamic LDS
//     laid out [k][kWave] (the k squared distances as doubles, then the k sorted slots as int32: 12 k kWave bytes, 48 KiB at k = 64), so
//     a lane's walk over its own list is free of bank conflicts.  With kFit the lane goes on from its list: the moments gather the
//     neighbours from the SORTED points (rows the walk has just touched), the 3 x 3 Jacobi solve runs as the tail of the same lane
//     (DESIGN.md section 0.30 has the register counts that decided it) and normal, curvature and status go to the lane's ORIGINAL row
//     through order.  With kTable the list itself goes out as the neighbour table of that row: a second output of the same walk, not a
//     second search.  No atomic, no barrier, no lane reads another's state; the lanes of a wave may belong to different segments.
//     Every table entry a lane indexes with -- its segment's offsets, cell_base, starts, order, the grid's dims, a list slot -- is
//     clamped first: corrupt device tables give wrong normals, never an access outside a buffer.
#include "mspa_common.h"
#include "segments_device.h"
#include "cloud_normals_core.h"

namespace mspa {
namespace cnorm {

static_assert(kOk == MSPA_CLOUD_NORMALS_OK && kFew == MSPA_CLOUD_NORMALS_FEW && kDegenerate == MSPA_CLOUD_NORMALS_DEGENERATE,
              "include/mspa.h and cloud_normals_core.h disagree on the status values");
static_assert(kSweeps == MSPA_CLOUD_NORMALS_SWEEPS && kGapExponent == MSPA_CLOUD_NORMALS_GAP_EXPONENT,
              "include/mspa.h and cloud_normals_core.h disagree on the solver's constants");

struct Tables {                                                  // what the kernel reads, all on the device
    const double *pts;                                           // [N, 3] the rows, sorted
    const int32_t *starts;                                       // [slots]
    const int64_t *order;                                        // [N]
    const int64_t *offsets;                                      // [S + 1]
    const Grid *grids;                                           // [S]
    const int64_t *cell_base;                                    // [S + 1]
    const double *viewpoints;                                    // [S, 3] or null
    int64_t N, S, slots;
    int32_t k;
};

struct Outputs {
    double *normal;                                              // [N, 3]  \.
    double *curvature;                                           // [N]      > with kFit
    uint8_t *status;                                             // [N]     /
    int32_t *used;                                               // [N]
    int64_t *nbr_index;                                          // [N, k]  \  with kTable
    double *nbr_distance;                                        // [N, k]  /
};

struct LdsPairs {
    double *d;
    int32_t *s;
    __device__ __forceinline__ double &d2(int32_t j) const { return d[j * kWave]; }
    __device__ __forceinline__ int32_t &slot(int32_t j) const { return s[j * kWave]; }
};

template <bool kFit, bool kTable>
__global__ void __launch_bounds__(kWave) seg_normals_kernel(Tables t, double cap2, Outputs out) {
    extern __shared__ double lists[];                            // [k][kWave] doubles, then [k][kWave] int32
    const int64_t i = (int64_t)blockIdx.x * kWave + threadIdx.x;
    if (i >= t.N) return;
    const int64_t s = segs::segment_of(t.offsets, t.S, i);
    const int64_t a = cdist::clamp_to(t.offsets[s], 0, i), b = cdist::clamp_to(t.offsets[s + 1], i + 1, t.N);   // slot i lies inside
    const int64_t n = b - a;
    const int32_t kk = (int32_t)(t.k < n ? t.k : n);
    Grid g = t.grids[s];
    for (int ax = 0; ax < 3; ++ax) g.dim[ax] = (int32_t)cdist::clamp_to(g.dim[ax], 1, knn::kMaxAxisCells);
    const int64_t sb = cdist::clamp_to(segs::starts_base(t.cell_base, s), 0, t.slots - 1);
    const double *__restrict__ pts = t.pts + 3 * a;
    const double q[3] = {t.pts[3 * i], t.pts[3 * i + 1], t.pts[3 * i + 2]};
    const LdsPairs list{lists + threadIdx.x, (int32_t *)(lists + (size_t)t.k * kWave) + threadIdx.x};
    int32_t count = 0;
    neighbours(g, pts, t.starts + sb, t.slots - sb, t.order + a, t.N, a, n, q, kk, cap2, list, count);
    const int64_t o = segs::row_in_segment(t.order[i], t.N, a, b);
    out.used[o] = count;
    if constexpr (kTable) {
        for (int32_t j = 0; j < t.k; ++j) {
            const bool in = j < count;
            const int64_t at = in ? cdist::clamp_to(list.slot(j), 0, n - 1) : 0;
            out.nbr_index[o * t.k + j] = in ? segs::row_in_segment(t.order[a + at], t.N, a, b) : -1;
            out.nbr_distance[o * t.k + j] = reported_distance(in ? list.d2(j) : 0.0, j, count);
        }
    }
    if constexpr (kFit) {
        Fit f;
        double c[3], m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (count > 0) moments(pts, n, list, count, c, m);
        solve(m, count, q, t.viewpoints ? t.viewpoints + 3 * s : nullptr, f);
        for (int ax = 0; ax < 3; ++ax) out.normal[3 * o + ax] = f.normal[ax];
        out.curvature[o] = f.curvature;
        out.status[o] = (uint8_t)f.status;
    }
}

// The host arguments of either entry, checked: N, or -1 with the error text set.
int64_t checked_batch(const std::string &who, const int64_t *offsets_host, int64_t S, int32_t k, double max_distance) {
    if (k < 1 || k > knn::kMaxK) return fail(MSPA_EINVAL, who + ": k outside [1, 64]"), -1;
    if (!cdist::cap_ok(max_distance)) return fail(MSPA_EINVAL, who + ": max_distance must be finite and > 0 (+inf: no cap)"), -1;
    return segs::checked_rows(who.c_str(), offsets_host, S);
}

}  // namespace cnorm
}  // namespace mspa

using namespace mspa;

extern "C" int mspa_cloud_normals_device(const double *pts_dev, const int32_t *starts_dev, int64_t starts_slots, const int64_t *order_dev,
                                         const int64_t *offsets_host, int64_t S, int32_t k, const void *grids_host, const int64_t *offsets_dev,
                                         const void *grids_dev, const int64_t *cell_base_dev, double max_distance, const double *viewpoints_dev,
                                         double *normal_dev, double *curvature_dev, int32_t *used_dev, uint8_t *status_dev,
                                         int64_t *nbr_index_dev, double *nbr_distance_dev, void *stream) {
    const std::string who = "mspa_cloud_normals_device";
    const int64_t N = cnorm::checked_batch(who, offsets_host, S, k, max_distance);
    if (N < 0) return MSPA_EINVAL;
    const bool fit = normal_dev || curvature_dev || status_dev, table = nbr_index_dev || nbr_distance_dev;
    if (!fit && !table) return fail(MSPA_EINVAL, who + ": neither the normals nor the neighbour table is asked for");
    if (N == 0) return MSPA_OK;
    if (!pts_dev || !starts_dev || !order_dev || !grids_host || !offsets_dev || !grids_dev || !cell_base_dev || !used_dev ||
        (fit && (!normal_dev || !curvature_dev || !status_dev)) || (table && (!nbr_index_dev || !nbr_distance_dev)))
        return fail(MSPA_EINVAL, who + ": null pointer");
    if (!segs::grids_ok((const knn::Grid *)grids_host, offsets_host, S, k))
        return fail(MSPA_EINVAL, who + ": not the grids of mspa_knn_segments_grids_host for these offsets and k");
    const void *eight[] = {pts_dev, order_dev, offsets_dev, grids_dev, cell_base_dev, viewpoints_dev, normal_dev, curvature_dev, nbr_index_dev,
                           nbr_distance_dev};
    for (const void *ptr : eight)
        if (segs::misaligned(ptr, 8)) return fail(MSPA_EINVAL, who + ": a buffer is not aligned to its element");
    if (segs::misaligned(starts_dev, 4) || segs::misaligned(used_dev, 4)) return fail(MSPA_EINVAL, who + ": a buffer is not aligned to its element");
    int64_t slots = S;
    for (int64_t s = 0; s < S; ++s)
        if (offsets_host[s + 1] > offsets_host[s]) slots += knn::max_cells(offsets_host[s + 1] - offsets_host[s], k);
    if (starts_slots < slots) return fail(MSPA_EINVAL, who + ": starts_dev holds fewer slots than the batch's cells plus S");
    const cnorm::Tables t{pts_dev, starts_dev, order_dev, offsets_dev, (const knn::Grid *)grids_dev, cell_base_dev, viewpoints_dev, N, S, slots, k};
    const cnorm::Outputs out{normal_dev, curvature_dev, status_dev, used_dev, nbr_index_dev, nbr_distance_dev};
    const dim3 grid((unsigned)((N + kWave - 1) / kWave)), block(kWave);
    const size_t lds = (size_t)k * kWave * (sizeof(double) + sizeof(int32_t));
    const double cap2 = cdist::cap2_of(max_distance);
    hipStream_t st = (hipStream_t)stream;
    if (fit && table)
        hipLaunchKernelGGL((cnorm::seg_normals_kernel<true, true>), grid, block, lds, st, t, cap2, out);
    else if (fit)
        hipLaunchKernelGGL((cnorm::seg_normals_kernel<true, false>), grid, block, lds, st, t, cap2, out);
    else
        hipLaunchKernelGGL((cnorm::seg_normals_kernel<false, true>), grid, block, lds, st, t, cap2, out);
    return check_hip(hipGetLastError(), who.c_str());
}

extern "C" int mspa_cloud_normals_host(const double *xyz_host, const int64_t *offsets_host, int64_t S, int32_t k, double max_distance,
                                       const double *viewpoints_host, double *normal_host, double *curvature_host, int32_t *used_host,
                                       uint8_t *status_host, int64_t *nbr_index_host, double *nbr_distance_host) {
    const std::string who = "mspa_cloud_normals_host";
    const int64_t N = cnorm::checked_batch(who, offsets_host, S, k, max_distance);
    if (N < 0) return MSPA_EINVAL;
    const bool fit = normal_host || curvature_host || status_host, table = nbr_index_host || nbr_distance_host;
    if (!fit && !table) return fail(MSPA_EINVAL, who + ": neither the normals nor the neighbour table is asked for");
    if (N == 0) return MSPA_OK;
    if (!xyz_host || !used_host || (fit && (!normal_host || !curvature_host || !status_host)) || (table && (!nbr_index_host || !nbr_distance_host)))
        return fail(MSPA_EINVAL, who + ": null pointer");
    for (int64_t i = 0; i < 3 * N; ++i)
        if (!(fabs(xyz_host[i]) < INFINITY)) return fail(MSPA_EINVAL, who + ": non-finite coordinate");
    if (!cnorm::normals_all(xyz_host, offsets_host, S, k, cdist::cap2_of(max_distance), viewpoints_host, normal_host, curvature_host, used_host,
                            status_host, nbr_index_host, nbr_distance_host))
        return fail(MSPA_EINVAL, who + ": no grid for a segment");
    return MSPA_OK;
}
