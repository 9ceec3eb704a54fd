// Nearest-point distances between the clouds of two ragged batches ON the MI355X: for every row of a query segment the distance to,
// and the row of, the nearest point of the target segment its pair names, and a per-pair summary of those distances.  The rule -- the
// pairs, the distance, the cap, the walk and why it may stop, the order of the sums -- is csrc/cloud_distance_core.h on top of
// csrc/knn_grid_core.h and csrc/cloud_segments_core.h; this file holds the two kernels, the host twins' entry points and the C ABI.
// The search structure of the targets (sorted points, order, starts) is built by mspa_knn_segments_index_device
// (csrc/cloud_segments.hip) with the gather and the starts kernels every batched search uses.
//
//   nearest_pairs_kernel  one lane per output row, workgroups of 256.  The lane finds its pair by binary search in out_offsets,
//     derives its query row and the target segment's grid record, starts base and pts base from the pair, and calls nearest(): the
//     best squared distance, its slot and its row stay in registers.  No LDS, no atomic, no lane reads another's state; lanes of one
//     wave may belong to different pairs.  Every table entry a lane indexes with -- the pair's two segments, the offsets of both
//     batches, cell_base, starts, order, the grid's dims -- is clamped first: corrupt device tables give wrong distances, never an
//     access outside a buffer.
//   query_keys_kernel     one lane per output row: the key (pair << 31) + the query's cell in its target segment's grid.  The caller
//     sorts the keys and hands the permutation to nearest_pairs_kernel, whose lane i then takes output row perm[i]: the lanes of a
//     wave walk neighbouring cells of one grid.  The outputs are the same bytes at the same places.
//   fit_pairs_kernel      one workgroup of 256 per pair: lane sums of d and d * d over the finite rows, folded through LDS by halving
//     strides (segs::ordered_sum's order, as seg_stats_kernel's), the three counts and the largest finite d folded the same way.
#include "mspa_common.h"
#include "segments_device.h"
#include "cloud_distance_core.h"

namespace mspa {
namespace cdist {

static_assert(kMaxRows == MSPA_CLOUD_DISTANCE_MAX_ROWS, "include/mspa.h and cloud_distance_core.h disagree on the most output rows");
static_assert(kMaxPairs == MSPA_CLOUD_DISTANCE_MAX_PAIRS, "include/mspa.h and cloud_distance_core.h disagree on the most pairs");
static_assert(kGridK == MSPA_CLOUD_DISTANCE_GRID_K, "include/mspa.h and cloud_distance_core.h disagree on the grid's neighbour count");

constexpr int kNearestBlock = 256;

struct Tables {                                                  // what the search kernel reads, all on the device
    const double *pts;                                           // [Nt, 3] the targets, sorted
    const int32_t *starts;                                       // [slots]
    const int64_t *order;                                        // [Nt]
    const int64_t *t_offsets;                                    // [St + 1]
    const Grid *grids;                                           // [St]
    const int64_t *cell_base;                                    // [St + 1]
    const double *q_xyz;                                         // [Nq, 3]
    const int64_t *q_offsets;                                    // [Sq + 1]
    const int64_t *pairs;                                        // [P, 2] or null: the identity
    const int64_t *out_offsets;                                  // [P + 1]
    const int64_t *perm;                                         // [M] the output row lane i takes, or null: row i
    int64_t Nt, St, slots, Nq, Sq, P, M;
};

// Output row i of the tables: its pair's target segment ts, its query q and the segment's grid record with the dims clamped.  Every
// entry indexed with is clamped first.  Returns the pair.
__device__ __forceinline__ int64_t row_of(const Tables &t, int64_t i, int64_t &ts, double q[3], Grid &g) {
    const int64_t p = segs::segment_of(t.out_offsets, t.P, i);
    const int64_t qs = clamp_to(pair_side(t.pairs, p, 0), 0, t.Sq - 1);
    ts = clamp_to(pair_side(t.pairs, p, 1), 0, t.St - 1);
    const int64_t row = clamp_to(t.q_offsets[qs] + (i - t.out_offsets[p]), 0, t.Nq - 1);
    g = t.grids[ts];
    for (int ax = 0; ax < 3; ++ax) g.dim[ax] = (int32_t)clamp_to(g.dim[ax], 1, knn::kMaxAxisCells);
    for (int ax = 0; ax < 3; ++ax) q[ax] = t.q_xyz[3 * row + ax];
    return p;
}

__global__ void __launch_bounds__(kNearestBlock) query_keys_kernel(Tables t, int64_t *__restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * kNearestBlock + threadIdx.x;
    if (i >= t.M) return;
    int64_t ts;
    double q[3];
    Grid g;
    const int64_t p = row_of(t, i, ts, q, g);
    keys[i] = (p << 31) + knn::cell_of(g, q[0], q[1], q[2]);     // a cell is below 2^30, a pair below 2^24
}

__global__ void __launch_bounds__(kNearestBlock) nearest_pairs_kernel(Tables t, double cap2, double *__restrict__ distance,
                                                                      int64_t *__restrict__ index, int32_t *__restrict__ evals) {
    const int64_t lane = (int64_t)blockIdx.x * kNearestBlock + threadIdx.x;
    if (lane >= t.M) return;
    const int64_t i = t.perm ? clamp_to(t.perm[lane], 0, t.M - 1) : lane;
    int64_t ts;
    double q[3];
    Grid g;
    row_of(t, i, ts, q, g);
    const int64_t a = clamp_to(t.t_offsets[ts], 0, t.Nt), n = clamp_to(t.t_offsets[ts + 1] - a, 0, t.Nt - a);
    const int64_t sb = clamp_to(segs::starts_base(t.cell_base, ts), 0, t.slots - 1);
    double d;
    int64_t at;
    const int64_t e = nearest_row(g, t.pts, t.starts + sb, t.slots - sb, t.order, t.Nt, a, n, q, cap2, d, at);
    distance[i] = d;
    if (index) index[i] = at;
    if (evals) evals[i] = (int32_t)e;
}

// partial[] of kLanes entries, every thread's own written: segs::ordered_sum's fold, the result in every thread.
template <typename T, typename Join>
__device__ __forceinline__ T fold(T *partial, int32_t j, Join join) {
    __syncthreads();
    for (int32_t s = segs::kLanes / 2; s >= 1; s >>= 1) {
        if (j < s) partial[j] = join(partial[j], partial[j + s]);
        __syncthreads();
    }
    const T total = partial[0];
    __syncthreads();                                             // partial[] is free again
    return total;
}

__global__ void __launch_bounds__(segs::kLanes) fit_pairs_kernel(const double *__restrict__ distance, const int64_t *__restrict__ out_offsets,
                                                                 int64_t M, double tau, int64_t *__restrict__ rows, int64_t *__restrict__ finite,
                                                                 int64_t *__restrict__ within, double *__restrict__ sum,
                                                                 double *__restrict__ sum_sq, double *__restrict__ largest) {
    __shared__ double partial[segs::kLanes];
    __shared__ int64_t counts[segs::kLanes];
    const int64_t p = blockIdx.x;
    const int32_t j = threadIdx.x;
    const int64_t a = clamp_to(out_offsets[p], 0, M), n = clamp_to(out_offsets[p + 1] - a, 0, M - a);
    const double *__restrict__ d = distance + a;
    auto plus = [](double x, double y) { return x + y; };
    auto count = [](int64_t x, int64_t y) { return x + y; };
    partial[j] = segs::lane_sum(j, n, [&](int64_t i) { return finite_term(d[i]); });
    const double s1 = fold(partial, j, plus);
    partial[j] = segs::lane_sum(j, n, [&](int64_t i) { return square_term(d[i]); });
    const double s2 = fold(partial, j, plus);
    int64_t nf = 0, nw = 0;
    double m = -INFINITY;
    for (int64_t i = j; i < n; i += segs::kLanes) {
        const double v = d[i];
        if (v < INFINITY) {
            ++nf;
            m = v > m ? v : m;
        }
        if (v <= tau) ++nw;
    }
    counts[j] = nf;
    nf = fold(counts, j, count);
    counts[j] = nw;
    nw = fold(counts, j, count);
    partial[j] = m;
    m = fold(partial, j, [](double x, double y) { return y > x ? y : x; });
    if (j == 0) {
        rows[p] = n;
        finite[p] = nf;
        within[p] = nw;
        sum[p] = s1;
        sum_sq[p] = s2;
        largest[p] = m;
    }
}

// The host tables of a search, checked: the output rows M, or -1 with the error text set.
int64_t checked_search(const std::string &who, const int64_t *t_offsets, int64_t St, const int64_t *q_offsets, int64_t Sq, const int64_t *pairs,
                       int64_t P, const int64_t *out_offsets, int32_t grid_k, double max_distance, int64_t &Nt, int64_t &Nq) {
    if (grid_k < 1 || grid_k > knn::kMaxK) return fail(MSPA_EINVAL, who + ": grid_k outside [1, 64]"), -1;
    if (!cap_ok(max_distance)) return fail(MSPA_EINVAL, who + ": max_distance must be finite and > 0 (+inf: no cap)"), -1;
    Nt = segs::checked_rows(who.c_str(), t_offsets, St);
    Nq = Nt < 0 ? -1 : segs::checked_rows(who.c_str(), q_offsets, Sq);
    if (Nt < 0 || Nq < 0) return -1;
    if (P > 0 && !out_offsets) return fail(MSPA_EINVAL, who + ": null pointer"), -1;
    const int64_t M = pair_rows(q_offsets, Sq, St, pairs, P, nullptr);
    if (M < 0)
        return fail(MSPA_EINVAL, who + ": pairs must be [P, 2] inside [0, Sq) x [0, St) (none: Sq == St == P), at most 2^24 pairs and 2^30 output rows"), -1;
    int64_t run = 0;
    for (int64_t p = 0; p < P; ++p) {
        const int64_t qs = pair_side(pairs, p, 0);
        if (out_offsets[p] != run) return fail(MSPA_EINVAL, who + ": out_offsets do not follow from the pairs"), -1;
        run += q_offsets[qs + 1] - q_offsets[qs];
    }
    if (P > 0 && out_offsets[P] != run) return fail(MSPA_EINVAL, who + ": out_offsets do not follow from the pairs"), -1;
    return M;
}

// The output offsets of a summary, checked: M, or -1 with the error text set.
int64_t checked_fit(const std::string &who, const int64_t *out_offsets, int64_t P, double tau) {
    if (!tau_ok(tau)) return fail(MSPA_EINVAL, who + ": tau must be finite and >= 0"), -1;
    if (P > kMaxPairs) return fail(MSPA_EINVAL, who + ": at most 2^24 pairs"), -1;
    return segs::checked_rows(who.c_str(), out_offsets, P);
}

}  // namespace cdist
}  // namespace mspa

using namespace mspa;

extern "C" int mspa_cloud_distance_device(const double *t_pts_dev, const int32_t *t_starts_dev, int64_t t_starts_slots, const int64_t *t_order_dev,
                                          const int64_t *t_offsets_host, int64_t St, int32_t grid_k, const void *grids_host,
                                          const int64_t *t_offsets_dev, const void *grids_dev, const int64_t *cell_base_dev,
                                          const double *q_xyz_dev, const int64_t *q_offsets_host, int64_t Sq, const int64_t *q_offsets_dev,
                                          const int64_t *pairs_host, const int64_t *pairs_dev, int64_t P, const int64_t *out_offsets_host,
                                          const int64_t *out_offsets_dev, const int64_t *perm_dev, double max_distance, double *distance_dev,
                                          int64_t *index_dev, int32_t *evals_dev, void *stream) {
    const std::string who = "mspa_cloud_distance_device";
    int64_t Nt, Nq;
    const int64_t M = cdist::checked_search(who, t_offsets_host, St, q_offsets_host, Sq, pairs_host, P, out_offsets_host, grid_k, max_distance, Nt, Nq);
    if (M < 0) return MSPA_EINVAL;
    if (M == 0) return MSPA_OK;
    if (!t_offsets_dev || !grids_host || !grids_dev || !cell_base_dev || !q_xyz_dev || !q_offsets_dev || !out_offsets_dev || !distance_dev ||
        (pairs_host && !pairs_dev) || (Nt > 0 && (!t_pts_dev || !t_starts_dev || !t_order_dev)))
        return fail(MSPA_EINVAL, who + ": null pointer");
    if (!segs::grids_ok((const knn::Grid *)grids_host, t_offsets_host, St, grid_k))
        return fail(MSPA_EINVAL, who + ": not the grids of mspa_knn_segments_grids_host for the targets' offsets and grid_k");
    const void *eight[] = {t_pts_dev, t_order_dev, t_offsets_dev, grids_dev, cell_base_dev, q_xyz_dev, q_offsets_dev, pairs_dev, out_offsets_dev,
                           perm_dev, distance_dev, index_dev};
    for (const void *ptr : eight)
        if (segs::misaligned(ptr, 8)) return fail(MSPA_EINVAL, who + ": a buffer is not aligned to its element");
    if (segs::misaligned(t_starts_dev, 4) || segs::misaligned(evals_dev, 4)) return fail(MSPA_EINVAL, who + ": a buffer is not aligned to its element");
    int64_t slots = St;
    for (int64_t s = 0; s < St; ++s)
        if (t_offsets_host[s + 1] > t_offsets_host[s]) slots += knn::max_cells(t_offsets_host[s + 1] - t_offsets_host[s], grid_k);
    if (Nt > 0 && t_starts_slots < slots) return fail(MSPA_EINVAL, who + ": t_starts_dev holds fewer slots than the targets' cells plus St");
    const cdist::Tables t{t_pts_dev, t_starts_dev, t_order_dev, t_offsets_dev, (const knn::Grid *)grids_dev, cell_base_dev, q_xyz_dev, q_offsets_dev,
                          pairs_dev, out_offsets_dev, perm_dev, Nt, St, slots, Nq, Sq, P, M};
    hipLaunchKernelGGL(cdist::nearest_pairs_kernel, dim3((unsigned)((M + cdist::kNearestBlock - 1) / cdist::kNearestBlock)),
                       dim3(cdist::kNearestBlock), 0, (hipStream_t)stream, t, cdist::cap2_of(max_distance), distance_dev, index_dev, evals_dev);
    return check_hip(hipGetLastError(), who.c_str());
}

extern "C" int mspa_cloud_distance_keys_device(const int64_t *t_offsets_host, int64_t St, int32_t grid_k, const void *grids_host, const void *grids_dev,
                                               const double *q_xyz_dev, const int64_t *q_offsets_host, int64_t Sq, const int64_t *q_offsets_dev,
                                               const int64_t *pairs_host, const int64_t *pairs_dev, int64_t P, const int64_t *out_offsets_host,
                                               const int64_t *out_offsets_dev, int64_t *keys_dev, void *stream) {
    const std::string who = "mspa_cloud_distance_keys_device";
    int64_t Nt, Nq;
    const int64_t M = cdist::checked_search(who, t_offsets_host, St, q_offsets_host, Sq, pairs_host, P, out_offsets_host, grid_k, INFINITY, Nt, Nq);
    if (M < 0) return MSPA_EINVAL;
    if (M == 0) return MSPA_OK;
    if (!grids_host || !grids_dev || !q_xyz_dev || !q_offsets_dev || !out_offsets_dev || !keys_dev || (pairs_host && !pairs_dev))
        return fail(MSPA_EINVAL, who + ": null pointer");
    if (!segs::grids_ok((const knn::Grid *)grids_host, t_offsets_host, St, grid_k))
        return fail(MSPA_EINVAL, who + ": not the grids of mspa_knn_segments_grids_host for the targets' offsets and grid_k");
    const void *eight[] = {grids_dev, q_xyz_dev, q_offsets_dev, pairs_dev, out_offsets_dev, keys_dev};
    for (const void *ptr : eight)
        if (segs::misaligned(ptr, 8)) return fail(MSPA_EINVAL, who + ": a buffer is not aligned to its element");
    const cdist::Tables t{nullptr, nullptr, nullptr, nullptr, (const knn::Grid *)grids_dev, nullptr, q_xyz_dev, q_offsets_dev, pairs_dev, out_offsets_dev,
                          nullptr, Nt, St, 0, Nq, Sq, P, M};
    hipLaunchKernelGGL(cdist::query_keys_kernel, dim3((unsigned)((M + cdist::kNearestBlock - 1) / cdist::kNearestBlock)), dim3(cdist::kNearestBlock),
                       0, (hipStream_t)stream, t, keys_dev);
    return check_hip(hipGetLastError(), who.c_str());
}

extern "C" int mspa_cloud_distance_fit_device(const double *distance_dev, const int64_t *out_offsets_host, int64_t P, double tau,
                                              const int64_t *out_offsets_dev, int64_t *rows_dev, int64_t *finite_dev, int64_t *within_dev,
                                              double *sum_dev, double *sum_sq_dev, double *max_dev, void *stream) {
    const std::string who = "mspa_cloud_distance_fit_device";
    const int64_t M = cdist::checked_fit(who, out_offsets_host, P, tau);
    if (M < 0) return MSPA_EINVAL;
    if (P == 0) return MSPA_OK;
    if (!out_offsets_dev || !rows_dev || !finite_dev || !within_dev || !sum_dev || !sum_sq_dev || !max_dev || (M > 0 && !distance_dev))
        return fail(MSPA_EINVAL, who + ": null pointer");
    const void *eight[] = {distance_dev, out_offsets_dev, rows_dev, finite_dev, within_dev, sum_dev, sum_sq_dev, max_dev};
    for (const void *ptr : eight)
        if (segs::misaligned(ptr, 8)) return fail(MSPA_EINVAL, who + ": a buffer is not aligned to its element");
    hipLaunchKernelGGL(cdist::fit_pairs_kernel, dim3((unsigned)P), dim3(segs::kLanes), 0, (hipStream_t)stream, distance_dev, out_offsets_dev, M, tau,
                       rows_dev, finite_dev, within_dev, sum_dev, sum_sq_dev, max_dev);
    return check_hip(hipGetLastError(), who.c_str());
}

extern "C" int mspa_cloud_distance_host(const double *t_xyz_host, const int64_t *t_offsets_host, int64_t St, int32_t grid_k,
                                        const double *q_xyz_host, const int64_t *q_offsets_host, int64_t Sq, const int64_t *pairs_host, int64_t P,
                                        const int64_t *out_offsets_host, double max_distance, double *distance_host, int64_t *index_host,
                                        int32_t *evals_host) {
    const std::string who = "mspa_cloud_distance_host";
    int64_t Nt, Nq;
    const int64_t M = cdist::checked_search(who, t_offsets_host, St, q_offsets_host, Sq, pairs_host, P, out_offsets_host, grid_k, max_distance, Nt, Nq);
    if (M < 0) return MSPA_EINVAL;
    if (M == 0) return MSPA_OK;
    if (!q_xyz_host || !distance_host || (Nt > 0 && !t_xyz_host)) return fail(MSPA_EINVAL, who + ": null pointer");
    for (int64_t i = 0; i < 3 * Nt; ++i)
        if (!(fabs(t_xyz_host[i]) < INFINITY)) return fail(MSPA_EINVAL, who + ": non-finite target coordinate");
    if (!cdist::nearest_segments_all(t_xyz_host, t_offsets_host, St, q_xyz_host, q_offsets_host, pairs_host, P, out_offsets_host, grid_k,
                                     cdist::cap2_of(max_distance), distance_host, index_host, evals_host))
        return fail(MSPA_EINVAL, who + ": no grid for a target segment");
    return MSPA_OK;
}

extern "C" int mspa_cloud_distance_fit_host(const double *distance_host, const int64_t *out_offsets_host, int64_t P, double tau, int64_t *rows_host,
                                            int64_t *finite_host, int64_t *within_host, double *sum_host, double *sum_sq_host, double *max_host) {
    const std::string who = "mspa_cloud_distance_fit_host";
    const int64_t M = cdist::checked_fit(who, out_offsets_host, P, tau);
    if (M < 0) return MSPA_EINVAL;
    if (P == 0) return MSPA_OK;
    if (!rows_host || !finite_host || !within_host || !sum_host || !sum_sq_host || !max_host || (M > 0 && !distance_host))
        return fail(MSPA_EINVAL, who + ": null pointer");
    cdist::fit_segments_all(distance_host, out_offsets_host, P, tau, rows_host, finite_host, within_host, sum_host, sum_sq_host, max_host);
    return MSPA_OK;
}
