// Rigid alignment of the clouds of two ragged batches ON the MI355X: the transform of every query row by its pair's R and t, and the
// rigid fit (Kabsch / Horn) of every pair's matched rows -- the two steps a point-to-point ICP iteration adds to the search of
// cloud_distance.hip.  The rule -- which rows are used, the order of the sums, Horn's matrix, the Jacobi sweeps, the statuses, the
// fixed point -- is csrc/cloud_align_core.h; this file holds the three kernels, the host twins' entry points and the C ABI.
//
//   transform_pairs_kernel   one lane per output row, workgroups of 256.  The lane finds its pair by binary search in out_offsets,
//     reads the 12 doubles of its pair's transform and its query row, and writes y = R q + t to row i of out [M, 3]: the rows in
//     OUTPUT-ROW order, a batch whose offsets are out_offsets, which the search then takes with the pair table (p, target of p).
//   rigid_moments_kernel     one workgroup of 256 per pair, fit_pairs_kernel's form.  Pass 1: every lane's sums of 1, q and p over the
//     used rows, the 7 folded through LDS together (segs::fold_sums of segments_device.h: partial[j] += partial[j + stride] for every
//     sum at every stride, one barrier per stride); the centroids in every lane.  Pass 2: the 9 lane sums of (q - qc)_a (p - pc)_b,
//     folded the same way.  The gather t_xyz[index[i]] is a scattered 24-byte read of rows the search has just touched.  Lane 0
//     writes the pair's record of 16 doubles.  No atomics; no lane reads another's registers.
//   rigid_solve_kernel       one lane per pair: Horn's matrix of the record, the Jacobi sweeps, R and t, the status, the eigenvalues
//     and the loop's counter.  It is a kernel of its own because its 32 doubles of matrix and vectors would set the register count of
//     the summing kernel, whose loops need a fraction of that (Resources).
// Every table entry a lane indexes with is clamped first.
#include "mspa_common.h"
#include "segments_device.h"
#include "cloud_align_core.h"

namespace mspa {
namespace calign {

static_assert(kSweeps == MSPA_CLOUD_ALIGN_SWEEPS, "include/mspa.h and cloud_align_core.h disagree on the Jacobi sweeps");
static_assert(kGapExponent == MSPA_CLOUD_ALIGN_GAP_EXPONENT, "include/mspa.h and cloud_align_core.h disagree on the gap");
static_assert(kOk == MSPA_CLOUD_ALIGN_OK && kFew == MSPA_CLOUD_ALIGN_FEW && kDegenerate == MSPA_CLOUD_ALIGN_DEGENERATE,
              "include/mspa.h and cloud_align_core.h disagree on the statuses");

using cdist::clamp_to;
using cdist::pair_side;
constexpr int kBlock = 256;

struct Tables {                                                  // the pair table of a launch, all on the device
    const double *q_xyz;                                         // [Nq, 3]
    const int64_t *q_offsets;                                    // [Sq + 1]
    const int64_t *pairs;                                        // [P, 2] or null: the identity
    const int64_t *out_offsets;                                  // [P + 1]
    int64_t Nq, Sq, P, M;
};

// The first query row of pair p, clamped; the pair's output rows are [a, a + n).
__device__ __forceinline__ int64_t pair_rows_of(const Tables &t, int64_t p, int64_t &a, int64_t &n) {
    a = clamp_to(t.out_offsets[p], 0, t.M);
    n = clamp_to(t.out_offsets[p + 1] - a, 0, t.M - a);
    const int64_t qs = clamp_to(pair_side(t.pairs, p, 0), 0, t.Sq - 1);
    return clamp_to(t.q_offsets[qs], 0, t.Nq);
}

__global__ void __launch_bounds__(kBlock) transform_pairs_kernel(Tables t, const double *__restrict__ transform, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= t.M) return;
    const int64_t p = segs::segment_of(t.out_offsets, t.P, i);
    int64_t a, n;
    const int64_t row = clamp_to(pair_rows_of(t, p, a, n) + (i - a), 0, t.Nq - 1);
    double T[12], y[3];
    for (int k = 0; k < 12; ++k) T[k] = transform[12 * p + k];
    const double q[3] = {t.q_xyz[3 * row], t.q_xyz[3 * row + 1], t.q_xyz[3 * row + 2]};
    transform_row(T, q, y);
    for (int ax = 0; ax < 3; ++ax) out[3 * i + ax] = y[ax];
}

__global__ void __launch_bounds__(segs::kLanes) rigid_moments_kernel(Tables t, const double *__restrict__ t_xyz, int64_t Nt,
                                                                     const int64_t *__restrict__ index, double *__restrict__ moments) {
    __shared__ double partial[kSecond][segs::kLanes];
    const int64_t p = blockIdx.x;
    const int32_t j = threadIdx.x;
    int64_t a, n;
    const int64_t first_row = pair_rows_of(t, p, a, n);
    auto row = [&](int64_t i, double q[3], double r[3]) {
        return used_row(t.q_xyz, clamp_to(first_row + i, 0, t.Nq - 1), t_xyz, clamped_index(index[a + i], Nt), q, r);
    };
    double sum[kSecond], first[kFirst], qc[3], pc[3];
    for (int k = 0; k < kFirst; ++k) sum[k] = 0.0;
    for (int64_t i = j; i < n; i += segs::kLanes) {
        double q[3] = {0.0, 0.0, 0.0}, r[3] = {0.0, 0.0, 0.0}, term[kFirst];
        first_terms(row(i, q, r), q, r, term);
        for (int k = 0; k < kFirst; ++k) sum[k] = sum[k] + term[k];
    }
    for (int k = 0; k < kFirst; ++k) partial[k][j] = sum[k];
    segs::fold_sums<kFirst>(partial, j, first);
    centroids(first, qc, pc);
    for (int k = 0; k < kSecond; ++k) sum[k] = 0.0;
    for (int64_t i = j; i < n; i += segs::kLanes) {
        double q[3] = {0.0, 0.0, 0.0}, r[3] = {0.0, 0.0, 0.0}, term[kSecond];
        second_terms(row(i, q, r), q, r, qc, pc, term);
        for (int k = 0; k < kSecond; ++k) sum[k] = sum[k] + term[k];
    }
    for (int k = 0; k < kSecond; ++k) partial[k][j] = sum[k];
    segs::fold_sums<kSecond>(partial, j, sum);
    if (j == 0) {
        double *m = moments + kMoments * p;
        m[0] = first[0];
        for (int ax = 0; ax < 3; ++ax) m[1 + ax] = qc[ax], m[4 + ax] = pc[ax];
        for (int k = 0; k < kSecond; ++k) m[7 + k] = sum[k];
    }
}

__global__ void __launch_bounds__(kBlock) rigid_solve_kernel(const double *__restrict__ moments, const double *__restrict__ init, int64_t P,
                                                             int64_t iteration, double *__restrict__ transform, int64_t *__restrict__ used,
                                                             int32_t *__restrict__ status, double *__restrict__ eigen,
                                                             int64_t *__restrict__ converged) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= P) return;
    double m[kMoments], T0[12], T[12], e[4];
    for (int k = 0; k < kMoments; ++k) m[k] = moments[kMoments * p + k];
    for (int k = 0; k < 12; ++k) T0[k] = init[12 * p + k];      // all of init is read before anything is written: the two may be one buffer
    const int32_t st = solve(m, T0, T, e);
    for (int k = 0; k < 12; ++k) transform[12 * p + k] = T[k];
    used[p] = (int64_t)m[0];
    status[p] = st;
    if (eigen)
        for (int k = 0; k < 4; ++k) eigen[4 * p + k] = e[k];
    if (converged) converged[p] = converged_now(converged[p], iteration, T0, T);
}

// The host tables of either entry, checked: the output rows M, or -1 with the error text set.
int64_t checked_pairs(const std::string &who, const int64_t *q_offsets, int64_t Sq, int64_t St, const int64_t *pairs, int64_t P,
                      const int64_t *out_offsets, int64_t &Nq) {
    if (St < 0 || St > segs::kMaxSegments) return fail(MSPA_EINVAL, who + ": St outside [0, 2^24]"), -1;
    Nq = segs::checked_rows(who.c_str(), q_offsets, Sq);
    if (Nq < 0) return -1;
    if (P > 0 && !out_offsets) return fail(MSPA_EINVAL, who + ": null pointer"), -1;
    const int64_t M = cdist::pair_rows(q_offsets, Sq, St, pairs, P, nullptr);
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

bool fit_knobs_ok(const std::string &who, int64_t Nt, int64_t iteration) {
    if (Nt < 0 || Nt > cdist::kMaxRows) return fail(MSPA_EINVAL, who + ": Nt outside [0, 2^30]"), false;
    if (iteration < 0) return fail(MSPA_EINVAL, who + ": iteration must be >= 0"), false;
    return true;
}

}  // namespace calign
}  // namespace mspa

using namespace mspa;

extern "C" int mspa_cloud_align_transform_device(const double *q_xyz_dev, const int64_t *q_offsets_host, int64_t Sq, const int64_t *q_offsets_dev,
                                                 int64_t St, const int64_t *pairs_host, const int64_t *pairs_dev, int64_t P,
                                                 const int64_t *out_offsets_host, const int64_t *out_offsets_dev, const double *transform_dev,
                                                 double *out_dev, void *stream) {
    const std::string who = "mspa_cloud_align_transform_device";
    int64_t Nq;
    const int64_t M = calign::checked_pairs(who, q_offsets_host, Sq, St, pairs_host, P, out_offsets_host, Nq);
    if (M < 0) return MSPA_EINVAL;
    if (M == 0) return MSPA_OK;
    if (!q_xyz_dev || !q_offsets_dev || !out_offsets_dev || !transform_dev || !out_dev || (pairs_host && !pairs_dev))
        return fail(MSPA_EINVAL, who + ": null pointer");
    const void *eight[] = {q_xyz_dev, q_offsets_dev, pairs_dev, out_offsets_dev, transform_dev, out_dev};
    for (const void *ptr : eight)
        if (segs::misaligned(ptr, 8)) return fail(MSPA_EINVAL, who + ": a buffer is not aligned to its element");
    const calign::Tables t{q_xyz_dev, q_offsets_dev, pairs_dev, out_offsets_dev, Nq, Sq, P, M};
    hipLaunchKernelGGL(calign::transform_pairs_kernel, dim3((unsigned)((M + calign::kBlock - 1) / calign::kBlock)), dim3(calign::kBlock), 0,
                       (hipStream_t)stream, t, transform_dev, out_dev);
    return check_hip(hipGetLastError(), who.c_str());
}

extern "C" int mspa_cloud_align_fit_device(const double *q_xyz_dev, const int64_t *q_offsets_host, int64_t Sq, const int64_t *q_offsets_dev,
                                           const double *t_xyz_dev, int64_t Nt, int64_t St, const int64_t *pairs_host, const int64_t *pairs_dev,
                                           int64_t P, const int64_t *out_offsets_host, const int64_t *out_offsets_dev, const int64_t *index_dev,
                                           const double *init_dev, int64_t iteration, double *moments_dev, double *transform_dev,
                                           int64_t *used_dev, int32_t *status_dev, double *eigen_dev, int64_t *converged_dev, void *stream) {
    const std::string who = "mspa_cloud_align_fit_device";
    int64_t Nq;
    const int64_t M = calign::checked_pairs(who, q_offsets_host, Sq, St, pairs_host, P, out_offsets_host, Nq);
    if (M < 0 || !calign::fit_knobs_ok(who, Nt, iteration)) return MSPA_EINVAL;
    if (P == 0) return MSPA_OK;
    if (!q_offsets_dev || !out_offsets_dev || !init_dev || !moments_dev || !transform_dev || !used_dev || !status_dev || (pairs_host && !pairs_dev) ||
        (M > 0 && (!q_xyz_dev || !index_dev)) || (Nt > 0 && !t_xyz_dev))
        return fail(MSPA_EINVAL, who + ": null pointer");
    const void *eight[] = {q_xyz_dev, q_offsets_dev, t_xyz_dev, pairs_dev, out_offsets_dev, index_dev, init_dev, moments_dev, transform_dev, used_dev,
                           eigen_dev, converged_dev};
    for (const void *ptr : eight)
        if (segs::misaligned(ptr, 8)) return fail(MSPA_EINVAL, who + ": a buffer is not aligned to its element");
    if (segs::misaligned(status_dev, 4)) return fail(MSPA_EINVAL, who + ": a buffer is not aligned to its element");
    const calign::Tables t{q_xyz_dev, q_offsets_dev, pairs_dev, out_offsets_dev, Nq, Sq, P, M};
    hipLaunchKernelGGL(calign::rigid_moments_kernel, dim3((unsigned)P), dim3(segs::kLanes), 0, (hipStream_t)stream, t, t_xyz_dev, Nt, index_dev,
                       moments_dev);
    hipLaunchKernelGGL(calign::rigid_solve_kernel, dim3((unsigned)((P + calign::kBlock - 1) / calign::kBlock)), dim3(calign::kBlock), 0,
                       (hipStream_t)stream, (const double *)moments_dev, init_dev, P, iteration, transform_dev, used_dev, status_dev, eigen_dev,
                       converged_dev);
    return check_hip(hipGetLastError(), who.c_str());
}

extern "C" int mspa_cloud_align_transform_host(const double *q_xyz_host, const int64_t *q_offsets_host, int64_t Sq, int64_t St,
                                               const int64_t *pairs_host, int64_t P, const int64_t *out_offsets_host, const double *transform_host,
                                               double *out_host) {
    const std::string who = "mspa_cloud_align_transform_host";
    int64_t Nq;
    const int64_t M = calign::checked_pairs(who, q_offsets_host, Sq, St, pairs_host, P, out_offsets_host, Nq);
    if (M < 0) return MSPA_EINVAL;
    if (M == 0) return MSPA_OK;
    if (!q_xyz_host || !transform_host || !out_host) return fail(MSPA_EINVAL, who + ": null pointer");
    calign::transform_all(q_xyz_host, q_offsets_host, pairs_host, P, out_offsets_host, transform_host, out_host);
    return MSPA_OK;
}

extern "C" int mspa_cloud_align_fit_host(const double *q_xyz_host, const int64_t *q_offsets_host, int64_t Sq, const double *t_xyz_host, int64_t Nt,
                                         int64_t St, const int64_t *pairs_host, int64_t P, const int64_t *out_offsets_host, const int64_t *index_host,
                                         const double *init_host, int64_t iteration, double *transform_host, int64_t *used_host, int32_t *status_host,
                                         double *eigen_host, int64_t *converged_host) {
    const std::string who = "mspa_cloud_align_fit_host";
    int64_t Nq;
    const int64_t M = calign::checked_pairs(who, q_offsets_host, Sq, St, pairs_host, P, out_offsets_host, Nq);
    if (M < 0 || !calign::fit_knobs_ok(who, Nt, iteration)) return MSPA_EINVAL;
    if (P == 0) return MSPA_OK;
    if (!init_host || !transform_host || !used_host || !status_host || (M > 0 && (!q_xyz_host || !index_host)) || (Nt > 0 && !t_xyz_host))
        return fail(MSPA_EINVAL, who + ": null pointer");
    calign::fit_all(q_xyz_host, q_offsets_host, t_xyz_host, Nt, pairs_host, P, out_offsets_host, index_host, init_host, iteration, transform_host,
                    used_host, status_host, eigen_host, converged_host);
    return MSPA_OK;
}
