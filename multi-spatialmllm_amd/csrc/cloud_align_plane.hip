// One linearised point-to-plane step per pair of two ragged batches ON the MI355X: what point-to-plane ICP puts in the place of the
// rigid fit of cloud_align.hip.  The rule -- which rows are used, the order of the sums, the L D L^T solve, the statuses, the
// quaternion update that keeps R orthonormal -- is csrc/cloud_align_plane_core.h; this file holds the two kernels, the host twin's
// entry point and the C ABI.
//
//   plane_moments_kernel   one workgroup of 256 per pair, rigid_moments_kernel's form.  Every lane reads its pair's transform once.
//     Pass 1: the lane sums of 1 and y = T q over the used rows, the 4 folded through LDS together (segs::fold_sums); the centroid c in
//     every lane.  Pass 2: the 28 lane sums of a_j a_k, a_j r and r r, folded the same way.  The gathers t_xyz[index[i]] and
//     t_normals[index[i]] are scattered 24-byte reads of rows the search has just touched.  Lane 0 writes the pair's record of 32
//     doubles.  No atomics; no lane reads another's registers.
//   plane_solve_kernel     one lane per pair: the 6 x 6 factorisation, the substitutions, the quaternion update, the status and the
//     loop's counter.  A kernel of its own for rigid_solve_kernel's reason: its matrices would set the register count of the summing
//     kernel (Resources).
// Every table entry a lane indexes with is clamped first.
#include "mspa_common.h"
#include "segments_device.h"
#include "cloud_align_plane_core.h"

namespace mspa {
namespace calign {                                               // csrc/cloud_align.hip: the checks of the host tables of a fit
int64_t checked_pairs(const std::string &who, const int64_t *q_offsets, int64_t Sq, int64_t St, const int64_t *pairs, int64_t P,
                      const int64_t *out_offsets, int64_t &Nq);
bool fit_knobs_ok(const std::string &who, int64_t Nt, int64_t iteration);
}  // namespace calign

namespace cplane {

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

__global__ void __launch_bounds__(segs::kLanes) plane_moments_kernel(Tables t, const double *__restrict__ t_xyz, const double *__restrict__ t_normals,
                                                                     int64_t Nt, const int64_t *__restrict__ index,
                                                                     const double *__restrict__ init, double *__restrict__ moments) {
    __shared__ double partial[kSecond][segs::kLanes];
    const int64_t p = blockIdx.x;
    const int32_t j = threadIdx.x;
    const int64_t a = clamp_to(t.out_offsets[p], 0, t.M), n = clamp_to(t.out_offsets[p + 1] - a, 0, t.M - a);
    const int64_t qs = clamp_to(pair_side(t.pairs, p, 0), 0, t.Sq - 1);
    const int64_t first_row = clamp_to(t.q_offsets[qs], 0, t.Nq);
    double T[12];
    for (int k = 0; k < 12; ++k) T[k] = init[12 * p + k];
    auto row = [&](int64_t i, double y[3], double r[3], double nn[3]) {
        return used_row(t.q_xyz, clamp_to(first_row + i, 0, t.Nq - 1), t_xyz, t_normals, calign::clamped_index(index[a + i], Nt), T, y, r, nn);
    };
    double sum[kSecond], first[kFirst], c[3];
    for (int k = 0; k < kFirst; ++k) sum[k] = 0.0;
    for (int64_t i = j; i < n; i += segs::kLanes) {
        double y[3] = {0.0, 0.0, 0.0}, r[3] = {0.0, 0.0, 0.0}, nn[3] = {0.0, 0.0, 0.0}, term[kFirst];
        first_terms(row(i, y, r, nn), y, term);
        for (int k = 0; k < kFirst; ++k) sum[k] = sum[k] + term[k];
    }
    for (int k = 0; k < kFirst; ++k) partial[k][j] = sum[k];
    segs::fold_sums<kFirst>(partial, j, first);
    centroid(first, c);
    for (int k = 0; k < kSecond; ++k) sum[k] = 0.0;
    for (int64_t i = j; i < n; i += segs::kLanes) {
        double y[3] = {0.0, 0.0, 0.0}, r[3] = {0.0, 0.0, 0.0}, nn[3] = {0.0, 0.0, 0.0}, term[kSecond];
        second_terms(row(i, y, r, nn), y, r, nn, c, term);
        for (int k = 0; k < kSecond; ++k) sum[k] = sum[k] + term[k];
    }
    for (int k = 0; k < kSecond; ++k) partial[k][j] = sum[k];
    segs::fold_sums<kSecond>(partial, j, sum);
    if (j == 0) {
        double *m = moments + kMoments * p;
        m[0] = first[0];
        for (int ax = 0; ax < 3; ++ax) m[1 + ax] = c[ax];
        for (int k = 0; k < kSecond; ++k) m[4 + k] = sum[k];
    }
}

__global__ void __launch_bounds__(kBlock) plane_solve_kernel(const double *__restrict__ moments, const double *__restrict__ init, int64_t P,
                                                             int64_t iteration, double *__restrict__ transform, int64_t *__restrict__ used,
                                                             int32_t *__restrict__ status, double *__restrict__ rmse,
                                                             int64_t *__restrict__ converged) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= P) return;
    double m[kMoments], T0[12], T[12];
    for (int k = 0; k < kMoments; ++k) m[k] = moments[kMoments * p + k];
    for (int k = 0; k < 12; ++k) T0[k] = init[12 * p + k];      // all of init is read before anything is written: the two may be one buffer
    const int32_t st = solve(m, T0, T);
    for (int k = 0; k < 12; ++k) transform[12 * p + k] = T[k];
    used[p] = (int64_t)m[0];
    status[p] = st;
    if (rmse) rmse[p] = m[0] > 0.0 ? sqrt(m[31] / m[0]) : segs::no_value();
    if (converged) converged[p] = calign::converged_now(converged[p], iteration, T0, T);
}

}  // namespace cplane
}  // namespace mspa

using namespace mspa;

extern "C" int mspa_cloud_align_plane_fit_device(const double *q_xyz_dev, const int64_t *q_offsets_host, int64_t Sq, const int64_t *q_offsets_dev,
                                                 const double *t_xyz_dev, const double *t_normals_dev, int64_t Nt, int64_t St,
                                                 const int64_t *pairs_host, const int64_t *pairs_dev, int64_t P, const int64_t *out_offsets_host,
                                                 const int64_t *out_offsets_dev, const int64_t *index_dev, const double *init_dev,
                                                 int64_t iteration, double *moments_dev, double *transform_dev, int64_t *used_dev,
                                                 int32_t *status_dev, double *rmse_dev, int64_t *converged_dev, void *stream) {
    const std::string who = "mspa_cloud_align_plane_fit_device";
    int64_t Nq;
    const int64_t M = calign::checked_pairs(who, q_offsets_host, Sq, St, pairs_host, P, out_offsets_host, Nq);
    if (M < 0 || !calign::fit_knobs_ok(who, Nt, iteration)) return MSPA_EINVAL;
    if (P == 0) return MSPA_OK;
    if (!q_offsets_dev || !out_offsets_dev || !init_dev || !moments_dev || !transform_dev || !used_dev || !status_dev || (pairs_host && !pairs_dev) ||
        (M > 0 && (!q_xyz_dev || !index_dev)) || (Nt > 0 && (!t_xyz_dev || !t_normals_dev)))
        return fail(MSPA_EINVAL, who + ": null pointer");
    if (moments_dev == init_dev || moments_dev == transform_dev) return fail(MSPA_EINVAL, who + ": moments_dev must be a buffer of its own");
    const void *eight[] = {q_xyz_dev, q_offsets_dev, t_xyz_dev, t_normals_dev, pairs_dev, out_offsets_dev, index_dev, init_dev, moments_dev, transform_dev,
                           used_dev, rmse_dev, converged_dev};
    for (const void *ptr : eight)
        if (segs::misaligned(ptr, 8)) return fail(MSPA_EINVAL, who + ": a buffer is not aligned to its element");
    if (segs::misaligned(status_dev, 4)) return fail(MSPA_EINVAL, who + ": a buffer is not aligned to its element");
    const cplane::Tables t{q_xyz_dev, q_offsets_dev, pairs_dev, out_offsets_dev, Nq, Sq, P, M};
    hipLaunchKernelGGL(cplane::plane_moments_kernel, dim3((unsigned)P), dim3(segs::kLanes), 0, (hipStream_t)stream, t, t_xyz_dev, t_normals_dev, Nt,
                       index_dev, init_dev, moments_dev);
    hipLaunchKernelGGL(cplane::plane_solve_kernel, dim3((unsigned)((P + cplane::kBlock - 1) / cplane::kBlock)), dim3(cplane::kBlock), 0,
                       (hipStream_t)stream, (const double *)moments_dev, init_dev, P, iteration, transform_dev, used_dev, status_dev, rmse_dev,
                       converged_dev);
    return check_hip(hipGetLastError(), who.c_str());
}

extern "C" int mspa_cloud_align_plane_fit_host(const double *q_xyz_host, const int64_t *q_offsets_host, int64_t Sq, const double *t_xyz_host,
                                               const double *t_normals_host, int64_t Nt, int64_t St, const int64_t *pairs_host, int64_t P,
                                               const int64_t *out_offsets_host, const int64_t *index_host, const double *init_host,
                                               int64_t iteration, double *transform_host, int64_t *used_host, int32_t *status_host,
                                               double *rmse_host, int64_t *converged_host) {
    const std::string who = "mspa_cloud_align_plane_fit_host";
    int64_t Nq;
    const int64_t M = calign::checked_pairs(who, q_offsets_host, Sq, St, pairs_host, P, out_offsets_host, Nq);
    if (M < 0 || !calign::fit_knobs_ok(who, Nt, iteration)) return MSPA_EINVAL;
    if (P == 0) return MSPA_OK;
    if (!init_host || !transform_host || !used_host || !status_host || (M > 0 && (!q_xyz_host || !index_host)) ||
        (Nt > 0 && (!t_xyz_host || !t_normals_host)))
        return fail(MSPA_EINVAL, who + ": null pointer");
    cplane::fit_all(q_xyz_host, q_offsets_host, t_xyz_host, t_normals_host, Nt, pairs_host, P, out_offsets_host, index_host, init_host, iteration,
                    transform_host, used_host, status_host, rmse_host, converged_host);
    return MSPA_OK;
}
