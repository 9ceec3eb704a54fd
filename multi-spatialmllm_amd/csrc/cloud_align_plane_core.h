// ONE LINEARISED POINT-TO-PLANE STEP PER PAIR OF TWO RAGGED BATCHES (what point-to-plane ICP adds to the search of cloud_distance_core.h
// and the normals of cloud_normals_core.h), stated once for the kernels of cloud_align_plane.hip and their host twin
// (mspa_cloud_align_plane_fit_host), on top of cloud_align_core.h.  A plain C++ build of the headers is the reference the device must
// agree with bit for bit.  Every step is one float64 + - * / or sqrt, nothing is fused (-ffp-contract=off), no
// libm function is called.
//
// Rows.  The batches, the pair table, out_offsets, index and the 12 doubles of a transform are cloud_align_core.h's.  With T the
// transform the pair comes in with (init), output row i has y_i = calign::transform_row(T, q_i), its match p_i = t_xyz[index_i] and
// that row's normal n_i = t_normals[index_i].  A row is USED when section 0.29 uses it (clamped index >= 0, a finite query row) and
// n_i is finite (a target row whose normal is NaN -- FEW or DEGENERATE in cloud_normals_core.h -- constrains nothing).
//
// Sums, two passes, both in segs::ordered_sum's order (256 lane sums folded by halving strides), 0.0 as every term of an unused row.
//   1. used = the sum of 1.0 and sum y [3]; c = sum y / used, one division each (0.0 where nothing is used).
//   2. With d = y - c, a = [d x n, n] (a_0 = d_1 n_2 - d_2 n_1, a_1 = d_2 n_0 - d_0 n_2, a_2 = d_0 n_1 - d_1 n_0, a_3..5 = n) and
//      r = ((y_0 - p_0) * n_0 + (y_1 - p_1) * n_1) + (y_2 - p_2) * n_2: the 21 products a_j a_k (j <= k, row by row), the 6 products
//      a_j r and r * r.  Taking moments about c keeps the two blocks of the matrix at the scale of the cloud, not of its offset.
//
// The step solves (A^T A) x = -(A^T r), x = (alpha, beta, gamma, s_0, s_1, s_2): the motion y -> y + w x (y - c) + s with w = (alpha,
// beta, gamma), whose residual is r + a . x to first order.  The 6 x 6 is factored as L D L^T in a fixed order (column by column, the
// sums over k ascending) and solved by the two substitutions.  Status: kFew where used < 6; else kDegenerate where a pivot D_j is NOT
// above kGap * (the largest diagonal entry of A^T A), kGap = 2^-26, or is not finite -- a flat target (every n equal) leaves the two
// slides and the spin about n without any constraint, its matrix has rank 3, and it must say so, not return a NaN; else kOk.  A pair
// that is not kOk KEEPS THE TRANSFORM IT CAME IN WITH.
//
// The update, and why R stays orthonormal.  R of the state is never multiplied by anything.  The incoming R is turned into a
// quaternion by Shepperd's method (the largest of trace, R_00, R_11, R_22 picks the branch: one sqrt, three divisions), normalised;
// it is multiplied from the left by the step's quaternion (1, alpha / 2, beta / 2, gamma / 2) (Hamilton's product, written out); the
// product is divided by its norm sqrt(((w * w + x * x) + y * y) + z * z), negated when its first non-zero component is negative, and
// R' is cloud_align_core.h's written-out expression of that quaternion.  So every R this header writes is that expression of a
// quaternion that was normalised in the line before: section 0.29's derivation applies word for word and max |R'^T R' - I| <=
// calign::kOrthoBound after ANY number of steps -- an error in the incoming R, or in Shepperd's branch, moves the rotation, not its
// orthonormality; nothing drifts.  A quaternion whose norm is not finite and positive (an init that is no rotation at all) is
// kDegenerate.  The translation: with Rs the same expression of the normalised step quaternion, t' = ((Rs (t - c)) + c) + s, each
// row ((Rs_a0 * e_0 + Rs_a1 * e_1) + Rs_a2 * e_2) with e = t - c.
//   * A step that is EXACTLY zero (all six x_j == 0.0) leaves the 12 doubles untouched, bit for bit.
//   * A cloud against itself with its own normals, from the identity: y_i = ((1 * x + 0 * y) + 0 * z) + 0 = q_i exactly, the nearest
//     row of q_i has q_i's coordinates (the lowest of coincident rows), so y - p = 0, every r_i is +-0.0, the six sums a_j r are 0.0,
//     the right-hand side is -0.0 or 0.0, both substitutions and the divisions by D_j keep zeros zero, the step is exactly zero and
//     the state is untouched: the identity, exactly, with converged_at = 0.
//   * EQUAL T GIVES EQUAL BITS: the step reads the original rows, index, the normals and T.  Equal T gives equal y, an equal search,
//     equal sums and an equal step, so `converged_at` (cloud_align_core.h's: the first iteration whose 12 doubles equal those it came
//     in with) keeps sync_every's guarantee.  A linearised step need not ever reach that fixed point; `iterations` is then the stop.
#pragma once
#include "cloud_align_core.h"

namespace mspa {
namespace cplane {

using calign::kDegenerate;
using calign::kFew;
using calign::kGap;
using calign::kOk;

constexpr int kFirst = 4, kSecond = 28, kMoments = 32;           // a pair's record: used, c [3], A^T A [21], A^T r [6], r r
constexpr int32_t kMinRows = 6;

// A row of a pair under T: is it used, and with which y, p and n.  They are read only where the answer is true.
MSPA_HD bool used_row(const double *__restrict__ q_xyz, int64_t row, const double *__restrict__ t_xyz, const double *__restrict__ t_normals,
                      int64_t at, const double *__restrict__ T, double y[3], double p[3], double n[3]) {
    if (at < 0) return false;
    double q[3];
    for (int ax = 0; ax < 3; ++ax) q[ax] = q_xyz[3 * row + ax];
    if (!cdist::finite3(q)) return false;
    for (int ax = 0; ax < 3; ++ax) n[ax] = t_normals[3 * at + ax];
    if (!cdist::finite3(n)) return false;
    for (int ax = 0; ax < 3; ++ax) p[ax] = t_xyz[3 * at + ax];
    calign::transform_row(T, q, y);
    return true;
}

MSPA_HD void first_terms(bool used, const double y[3], double term[kFirst]) {
    term[0] = used ? 1.0 : 0.0;
    for (int ax = 0; ax < 3; ++ax) term[1 + ax] = used ? y[ax] : 0.0;
}

MSPA_HD void centroid(const double first[kFirst], double c[3]) {
    for (int ax = 0; ax < 3; ++ax) c[ax] = first[0] > 0.0 ? first[1 + ax] / first[0] : 0.0;
}

MSPA_HD void second_terms(bool used, const double y[3], const double p[3], const double n[3], const double c[3], double term[kSecond]) {
    if (!used) {
        for (int k = 0; k < kSecond; ++k) term[k] = 0.0;
        return;
    }
    const double d[3] = {y[0] - c[0], y[1] - c[1], y[2] - c[2]};
    const double a[6] = {d[1] * n[2] - d[2] * n[1], d[2] * n[0] - d[0] * n[2], d[0] * n[1] - d[1] * n[0], n[0], n[1], n[2]};
    const double r = ((y[0] - p[0]) * n[0] + (y[1] - p[1]) * n[1]) + (y[2] - p[2]) * n[2];
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) term[k++] = a[i] * a[j];
    for (int i = 0; i < 6; ++i) term[21 + i] = a[i] * r;
    term[27] = r * r;
}

MSPA_HD void rotation_of(double w, double x, double y, double z, double R[9]) {      // cloud_align_core.h's expression
    const double ww = w * w, xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    R[0] = ((ww + xx) - yy) - zz;
    R[1] = 2.0 * (xy - wz);
    R[2] = 2.0 * (xz + wy);
    R[3] = 2.0 * (xy + wz);
    R[4] = ((ww - xx) + yy) - zz;
    R[5] = 2.0 * (yz - wx);
    R[6] = 2.0 * (xz - wy);
    R[7] = 2.0 * (yz + wx);
    R[8] = ((ww - xx) - yy) + zz;
}

// q / |q|; false where the norm is not finite and positive.
MSPA_HD bool normalise(double q[4]) {
    const double norm = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    if (!(norm > 0.0) || !(norm < INFINITY)) return false;
    for (int k = 0; k < 4; ++k) q[k] = q[k] / norm;
    return true;
}

// Shepperd: the quaternion (w, x, y, z) of a row-major R, not normalised.
MSPA_HD void quaternion_of(const double *__restrict__ R, double q[4]) {
    const double tr = (R[0] + R[4]) + R[8];
    if (tr >= R[0] && tr >= R[4] && tr >= R[8]) {
        const double s = 2.0 * sqrt(tr + 1.0);
        q[0] = s / 4.0, q[1] = (R[7] - R[5]) / s, q[2] = (R[2] - R[6]) / s, q[3] = (R[3] - R[1]) / s;
    } else if (R[0] >= R[4] && R[0] >= R[8]) {
        const double s = 2.0 * sqrt(((1.0 + R[0]) - R[4]) - R[8]);
        q[0] = (R[7] - R[5]) / s, q[1] = s / 4.0, q[2] = (R[1] + R[3]) / s, q[3] = (R[2] + R[6]) / s;
    } else if (R[4] >= R[8]) {
        const double s = 2.0 * sqrt(((1.0 + R[4]) - R[0]) - R[8]);
        q[0] = (R[2] - R[6]) / s, q[1] = (R[1] + R[3]) / s, q[2] = s / 4.0, q[3] = (R[5] + R[7]) / s;
    } else {
        const double s = 2.0 * sqrt(((1.0 + R[8]) - R[0]) - R[4]);
        q[0] = (R[3] - R[1]) / s, q[1] = (R[2] + R[6]) / s, q[2] = (R[5] + R[7]) / s, q[3] = s / 4.0;
    }
}

// A pair's record m = (used, c [3], A^T A [21], A^T r [6], r r) and the transform it came in with -> the transform it leaves with
// and its status.
MSPA_HD int32_t solve(const double *__restrict__ m, const double *__restrict__ init, double *__restrict__ T) {
    for (int k = 0; k < 12; ++k) T[k] = init[k];
    if (m[0] < (double)kMinRows) return kFew;
    double A[6][6], L[6][6], D[6], x[6];
    int k = 4;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) A[i][j] = A[j][i] = m[k++];
    double top = A[0][0];
    for (int i = 1; i < 6; ++i) top = A[i][i] > top ? A[i][i] : top;
    if (!(top < INFINITY)) return kDegenerate;
    for (int j = 0; j < 6; ++j) {
        double dj = A[j][j];
        for (int e = 0; e < j; ++e) dj = dj - (L[j][e] * L[j][e]) * D[e];
        if (!(dj > kGap * top) || !(dj < INFINITY)) return kDegenerate;
        D[j] = dj;
        for (int i = j + 1; i < 6; ++i) {
            double v = A[i][j];
            for (int e = 0; e < j; ++e) v = v - (L[i][e] * L[j][e]) * D[e];
            L[i][j] = v / dj;
        }
    }
    for (int i = 0; i < 6; ++i) {                                // L z = -A^T r
        double v = -m[25 + i];
        for (int e = 0; e < i; ++e) v = v - L[i][e] * x[e];
        x[i] = v;
    }
    for (int i = 0; i < 6; ++i) x[i] = x[i] / D[i];
    for (int i = 5; i >= 0; --i) {                               // L^T x = z / D
        double v = x[i];
        for (int e = i + 1; e < 6; ++e) v = v - L[e][i] * x[e];
        x[i] = v;
    }
    bool zero = true, finite = true;
    for (int i = 0; i < 6; ++i) {
        zero = zero && x[i] == 0.0;
        finite = finite && fabs(x[i]) < INFINITY;
    }
    if (!finite) return kDegenerate;
    if (zero) return kOk;                                        // the state is untouched
    double q0[4], dq[4] = {1.0, x[0] / 2.0, x[1] / 2.0, x[2] / 2.0}, q[4], R[9], Rs[9];
    quaternion_of(init, q0);
    if (!normalise(q0)) return kDegenerate;
    q[0] = ((dq[0] * q0[0] - dq[1] * q0[1]) - dq[2] * q0[2]) - dq[3] * q0[3];
    q[1] = ((dq[0] * q0[1] + dq[1] * q0[0]) + dq[2] * q0[3]) - dq[3] * q0[2];
    q[2] = ((dq[0] * q0[2] - dq[1] * q0[3]) + dq[2] * q0[0]) + dq[3] * q0[1];
    q[3] = ((dq[0] * q0[3] + dq[1] * q0[2]) - dq[2] * q0[1]) + dq[3] * q0[0];
    if (!normalise(q) || !normalise(dq)) return kDegenerate;
    const double lead = q[0] != 0.0 ? q[0] : q[1] != 0.0 ? q[1] : q[2] != 0.0 ? q[2] : q[3];
    if (lead < 0.0) q[0] = -q[0], q[1] = -q[1], q[2] = -q[2], q[3] = -q[3];
    rotation_of(q[0], q[1], q[2], q[3], R);
    rotation_of(dq[0], dq[1], dq[2], dq[3], Rs);
    const double *c = m + 1;
    const double e[3] = {init[9] - c[0], init[10] - c[1], init[11] - c[2]};
    for (int i = 0; i < 9; ++i) T[i] = R[i];
    for (int a = 0; a < 3; ++a) T[9 + a] = ((((Rs[3 * a] * e[0] + Rs[3 * a + 1] * e[1]) + Rs[3 * a + 2] * e[2])) + c[a]) + x[3 + a];
    return kOk;
}

// ---- the host twin ------------------------------------------------------------------------------------------------------------

// The record of pair p on the CPU under its transform T: kFirst, then kSecond sums, every row's terms evaluated once per pass.
inline void moments_of(const double *q_xyz, const int64_t *q_offsets, const double *t_xyz, const double *t_normals, int64_t Nt, const int64_t *pairs,
                       const int64_t *out_offsets, const int64_t *index, const double *T, int64_t p, double m[kMoments]) {
    const int64_t a = out_offsets[p], n = out_offsets[p + 1] - a;
    double first[kFirst], c[3];
    auto row = [&](int64_t i, double y[3], double t[3], double nn[3]) {
        return used_row(q_xyz, calign::query_row(q_offsets, pairs, out_offsets, p, a + i), t_xyz, t_normals, calign::clamped_index(index[a + i], Nt), T, y,
                        t, nn);
    };
    calign::ordered_sums<kFirst>(n, [&](int64_t i, double term[kFirst]) {
        double y[3] = {0.0, 0.0, 0.0}, t[3] = {0.0, 0.0, 0.0}, nn[3] = {0.0, 0.0, 0.0};
        first_terms(row(i, y, t, nn), y, term);
    }, first);
    centroid(first, c);
    m[0] = first[0];
    for (int ax = 0; ax < 3; ++ax) m[1 + ax] = c[ax];
    calign::ordered_sums<kSecond>(n, [&](int64_t i, double term[kSecond]) {
        double y[3] = {0.0, 0.0, 0.0}, t[3] = {0.0, 0.0, 0.0}, nn[3] = {0.0, 0.0, 0.0};
        second_terms(row(i, y, t, nn), y, t, nn, c, term);
    }, m + 4);
}

// The step of P pairs on the CPU.  rmse [P] (sqrt(r r / used), NaN where nothing is used) and converged [P] may be null.
inline void fit_all(const double *q_xyz, const int64_t *q_offsets, const double *t_xyz, const double *t_normals, int64_t Nt, const int64_t *pairs,
                    int64_t P, const int64_t *out_offsets, const int64_t *index, const double *init, int64_t iteration, double *transform,
                    int64_t *used, int32_t *status, double *rmse, int64_t *converged) {
    for (int64_t p = 0; p < P; ++p) {
        double m[kMoments], T0[12], T[12];
        for (int k = 0; k < 12; ++k) T0[k] = init[12 * p + k];
        moments_of(q_xyz, q_offsets, t_xyz, t_normals, Nt, pairs, out_offsets, index, T0, p, m);
        status[p] = solve(m, T0, T);
        used[p] = (int64_t)m[0];
        if (rmse) rmse[p] = m[0] > 0.0 ? sqrt(m[31] / m[0]) : segs::no_value();
        if (converged) converged[p] = calign::converged_now(converged[p], iteration, T0, T);
        for (int k = 0; k < 12; ++k) transform[12 * p + k] = T[k];
    }
}

}  // namespace cplane
}  // namespace mspa
