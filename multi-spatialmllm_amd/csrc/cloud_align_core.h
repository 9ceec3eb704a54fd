// RIGID ALIGNMENT OF THE CLOUDS OF TWO RAGGED BATCHES (the fit of matched rows, Kabsch / Horn, and what point-to-point ICP is made of),
// stated once for the kernels of cloud_align.hip and their host twins (mspa_cloud_align_transform_host, mspa_cloud_align_fit_host), on
// top of cloud_distance_core.h.  A plain C++ build of the headers is the reference the device must agree with bit for bit (DESIGN.md
// section 0.29).  Every step is one float64 + - * / or sqrt, nothing is fused (-ffp-contract=off), no libm function is called.
//
// Correspondences.  The batches, the pair table and out_offsets are cloud_distance_core.h's.  Output row i of pair p belongs to query
// row q = q_offsets[pairs[p][0]] + (i - out_offsets[p]) of q_xyz and carries index[i], a row of t_xyz [Nt, 3] or -1 (what nearest()
// reported for it, or any table a caller has: index = the row itself is the fit of known correspondences).  index[i] is clamped into
// [-1, Nt) before it addresses anything: a corrupt table gives a wrong fit, never an access outside a buffer.  A row is USED when its
// clamped index is >= 0 and its query row is finite; the target row it names is p.
//
// A transform is 12 doubles: R row-major (9), then t (3).  Of a row: y_a = ((R_a0 * x + R_a1 * y) + R_a2 * z) + t_a.  A non-finite row
// stays what IEEE makes of it.
//
// Moments, two passes, both in segs::ordered_sum's order (256 lane sums folded by halving strides) with 0.0 as every term of a row
// that is not used.
//   1. used = the sum of 1.0 (exact below 2^53), sum q [3], sum p [3]; the centroids qc = sum q / used, pc = sum p / used, one
//      division each (0.0 where nothing is used).
//   2. S_ab = the sum of (q_a - qc_a) * (p_b - pc_b): one subtraction each, then one product.  Centring first: a cloud 10^6 m from the
//      origin loses nothing to its offset beyond the one rounding of each difference.
//
// The solver is Horn's closed form.  N is the symmetric 4 x 4 matrix
//      [ (Sxx + Syy) + Szz     Syz - Szy              Szx - Sxz              Sxy - Syx          ]
//      [                       (Sxx - Syy) - Szz      Sxy + Syx              Szx + Sxz          ]
//      [                                              (Syy - Sxx) - Szz      Syz + Szy          ]
//      [                                                                     (Szz - Sxx) - Syy  ]
// whose eigenvector of the largest eigenvalue is the unit quaternion (w, x, y, z) of the rotation that maximises sum (R q') . p'.  N is
// diagonalised by cyclic Jacobi rotations: kSweeps sweeps, each over the pivots (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) in that order.  A
// pivot a_pq that is exactly 0.0 is skipped, the only data-dependent branch.  Otherwise
//      theta = (a_qq - a_pp) / (2 * a_pq);  t = sign(theta) / (|theta| + sqrt(theta * theta + 1))  (sign(0) = +1);
//      c = 1 / sqrt(t * t + 1);  s = t * c;
//      a_pp -= t * a_pq;  a_qq += t * a_pq;  a_pq = a_qp = 0;
//      for the other two k: (a_kp, a_kq) <- (c * a_kp - s * a_kq, s * a_kp + c * a_kq), mirrored;
//      for every k: (v_kp, v_kq) <- (c * v_kp - s * v_kq, s * v_kp + c * v_kq),  V from the identity.
// A theta whose square overflows gives t = 0, c = 1, s = 0: no NaN arises from finite S.  kSweeps = 12: the cyclic-by-rows method
// converges quadratically once the off-diagonal norm is below the eigenvalue gaps (Wilkinson 1962, van Kempen 1966), and a 4 x 4
// matrix reaches that after three or four sweeps; a double eigenvalue (which the status below turns away where it matters) only
// slows the rotation inside its own eigenspace.  Twelve leaves a margin of several sweeps and costs one lane 72 rotations a pair, 20
// microseconds for 1 792 pairs; the check of the constant is the accuracy against a 60-digit oracle that
// tests/test_cloud_align_cpu.py asserts on every class of input, rotations by 1e-9 rad and by pi among them.
// The eigenvalues are the diagonal.  The quaternion is the column of the largest one, the lowest column among equal ones, divided by
// its norm sqrt(((w * w + x * x) + y * y) + z * z) and negated when its first non-zero component is negative.  Then
//      R = [ ((ww + xx) - yy) - zz    2 * (xy - wz)            2 * (xz + wy)          ]
//          [ 2 * (xy + wz)            ((ww - xx) + yy) - zz    2 * (yz - wx)          ]
//          [ 2 * (xz - wy)            2 * (yz + wx)            ((ww - xx) - yy) + zz  ]      (ww = w * w, xy = x * y, ...)
// and t_a = pc_a - ((R_a0 * qc_x + R_a1 * qc_y) + R_a2 * qc_z).  No determinant is fixed up: this R is |q|^2 times a proper rotation
// for ANY non-zero q.
//   * A cloud fitted to itself: S is symmetric, the three pivots of row 0 are exactly 0.0 and stay so (c * 0 - s * 0), the largest
//     eigenvalue is a_00 = the trace, the quaternion (1, 0, 0, 0), R = I and t = pc - qc = 0, exactly.
//   * EQUAL CORRESPONDENCES GIVE EQUAL BITS: the fit reads the original query rows and index, never an earlier transform.  An ICP loop
//     that fits the original rows each time therefore reaches a true fixed point, and composes no products that drift from
//     orthonormality.
//
// The bound on orthonormality (kOrthoBound).  Let u = 2^-53.  The norm's square is 4 products and 3 sums of non-negative terms:
// relative error <= 4u; its root <= 2u + u; each quotient one more u: the stored q_i = v_i / |v| * (1 + e_i) with |e_i| <= 4u, so
// |q|^2 = 1 + d with |d| <= 8u.  The exact R of that q is (1 + d) times a rotation: R^T R - I = ((1 + d)^2 - 1) I, at most 16u.  Each
// entry of R is evaluated with an absolute error of at most 4u (a diagonal entry: four products and three sums of terms that add up
// to |q|^2; another entry: 2 * (two products, one sum), |xy| + |wz| <= |q|^2 / 2).  An entry of R^T E + E^T R is at most 2 * 4u * the
// 1-norm of a column of R, <= 2 * 4u * sqrt(3).  In all max |R^T R - I| <= 16u + 13.9u + O(u^2) < 32u = kOrthoBound, for every
// transform the solver writes.
//
// Status of a pair: kFew where used < 3; else kDegenerate where, with l1 >= l2 >= l3 >= l4 the eigenvalues, NOT (l1 - l2 > kGap *
// (l1 - l4)) or l1 - l4 is not finite -- kGap = 2^-26: below that gap the rotation about the best axis is not determined to half the
// digits; collinear rows (l1 = l2) and coincident rows (N = 0) fall here, and so does an S that overflowed; else kOk.  A pair that is
// not kOk KEEPS THE TRANSFORM IT CAME IN WITH (init), and its eigenvalues are still reported.
//
// converged_at (the loop's counter, in and out): where it is -1 and the 12 doubles written equal the 12 of init bit for bit, it
// becomes `iteration`.  A pair that kept its init is at a fixed point by that rule.
#pragma once
#include "cloud_distance_core.h"

namespace mspa {
namespace calign {

constexpr int32_t kSweeps = 12;
constexpr int32_t kGapExponent = -26;
constexpr double kGap = 1.0 / (double)((int64_t)1 << 26);
constexpr double kOrthoBound = 32.0 / 9007199254740992.0;        // 32 * 2^-53
constexpr int32_t kOk = 0, kFew = 1, kDegenerate = 2;
constexpr int kFirst = 7, kSecond = 9, kMoments = 16;            // the sums of the two passes; a pair's record: used, qc, pc, S

MSPA_HD int64_t clamped_index(int64_t index, int64_t Nt) { return cdist::clamp_to(index, -1, Nt - 1); }   // Nt >= 0

// A row of a pair: is it used, and with which target row.  q and p are read only where the answer is true.
MSPA_HD bool used_row(const double *__restrict__ q_xyz, int64_t row, const double *__restrict__ t_xyz, int64_t at, double q[3], double p[3]) {
    if (at < 0) return false;
    for (int ax = 0; ax < 3; ++ax) q[ax] = q_xyz[3 * row + ax];
    if (!cdist::finite3(q)) return false;
    for (int ax = 0; ax < 3; ++ax) p[ax] = t_xyz[3 * at + ax];
    return true;
}

MSPA_HD void first_terms(bool used, const double q[3], const double p[3], double term[kFirst]) {
    term[0] = used ? 1.0 : 0.0;
    for (int ax = 0; ax < 3; ++ax) {
        term[1 + ax] = used ? q[ax] : 0.0;
        term[4 + ax] = used ? p[ax] : 0.0;
    }
}

MSPA_HD void second_terms(bool used, const double q[3], const double p[3], const double qc[3], const double pc[3], double term[kSecond]) {
    for (int a = 0; a < 3; ++a) {
        const double da = used ? q[a] - qc[a] : 0.0;
        for (int b = 0; b < 3; ++b) {
            const double db = used ? p[b] - pc[b] : 0.0;
            term[3 * a + b] = used ? da * db : 0.0;
        }
    }
}

MSPA_HD void centroids(const double first[kFirst], double qc[3], double pc[3]) {
    for (int ax = 0; ax < 3; ++ax) {
        qc[ax] = first[0] > 0.0 ? first[1 + ax] / first[0] : 0.0;
        pc[ax] = first[0] > 0.0 ? first[4 + ax] / first[0] : 0.0;
    }
}

MSPA_HD void transform_row(const double *__restrict__ T, const double q[3], double y[3]) {
    for (int a = 0; a < 3; ++a) y[a] = ((T[3 * a] * q[0] + T[3 * a + 1] * q[1]) + T[3 * a + 2] * q[2]) + T[9 + a];
}

MSPA_HD bool same_bits(double a, double b) {
    uint64_t x, y;
    __builtin_memcpy(&x, &a, 8);
    __builtin_memcpy(&y, &b, 8);
    return x == y;
}

// One Jacobi rotation of the symmetric a and of v at the pivot (p, q), p < q.
MSPA_HD void rotate(double a[4][4], double v[4][4], int p, int q) {
    const double apq = a[p][q];
    if (apq == 0.0) return;
    const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
    const double root = sqrt(theta * theta + 1.0);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + root);
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    a[p][p] = a[p][p] - t * apq;
    a[q][q] = a[q][q] + t * apq;
    a[p][q] = a[q][p] = 0.0;
    for (int k = 0; k < 4; ++k) {
        if (k != p && k != q) {
            const double akp = a[k][p], akq = a[k][q];
            a[k][p] = a[p][k] = c * akp - s * akq;
            a[k][q] = a[q][k] = s * akp + c * akq;
        }
        const double vkp = v[k][p], vkq = v[k][q];
        v[k][p] = c * vkp - s * vkq;
        v[k][q] = s * vkp + c * vkq;
    }
}

// A pair's record m = (used, qc [3], pc [3], S [9]) and the transform it came in with -> the transform it leaves with, its status
// and, where wanted, its four eigenvalues in descending order.
MSPA_HD int32_t solve(const double *__restrict__ m, const double *__restrict__ init, double *__restrict__ T, double *__restrict__ eigen) {
    const double *S = m + 7;
    const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
    double a[4][4], v[4][4];
    a[0][0] = (Sxx + Syy) + Szz;
    a[1][1] = (Sxx - Syy) - Szz;
    a[2][2] = (Syy - Sxx) - Szz;
    a[3][3] = (Szz - Sxx) - Syy;
    a[0][1] = a[1][0] = Syz - Szy;
    a[0][2] = a[2][0] = Szx - Sxz;
    a[0][3] = a[3][0] = Sxy - Syx;
    a[1][2] = a[2][1] = Sxy + Syx;
    a[1][3] = a[3][1] = Szx + Sxz;
    a[2][3] = a[3][2] = Syz + Szy;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) v[i][j] = i == j ? 1.0 : 0.0;
    for (int32_t sweep = 0; sweep < kSweeps; ++sweep) {
        rotate(a, v, 0, 1);
        rotate(a, v, 0, 2);
        rotate(a, v, 0, 3);
        rotate(a, v, 1, 2);
        rotate(a, v, 1, 3);
        rotate(a, v, 2, 3);
    }
    int best = 0;
    for (int k = 1; k < 4; ++k)
        if (a[k][k] > a[best][best]) best = k;
    double second = -INFINITY, low = a[best][best];
    for (int k = 0; k < 4; ++k) {
        if (k != best && a[k][k] > second) second = a[k][k];
        if (a[k][k] < low) low = a[k][k];
    }
    if (eigen) {                                                 // descending: four values, a sorting network
        double e[4] = {a[0][0], a[1][1], a[2][2], a[3][3]};
        auto down = [&](int i, int j) {
            if (e[j] > e[i]) {
                const double x = e[i];
                e[i] = e[j];
                e[j] = x;
            }
        };
        down(0, 1), down(2, 3), down(0, 2), down(1, 3), down(1, 2);
        for (int k = 0; k < 4; ++k) eigen[k] = e[k];
    }
    const double l1 = a[best][best], spread = l1 - low;
    int32_t status = kOk;
    if (m[0] < 3.0)
        status = kFew;
    else if (!(spread < INFINITY) || !(l1 - second > kGap * spread))
        status = kDegenerate;
    if (status != kOk) {
        for (int k = 0; k < 12; ++k) T[k] = init[k];
        return status;
    }
    double w = v[0][best], x = v[1][best], y = v[2][best], z = v[3][best];
    const double norm = sqrt(((w * w + x * x) + y * y) + z * z);
    w = w / norm, x = x / norm, y = y / norm, z = z / norm;
    const double lead = w != 0.0 ? w : x != 0.0 ? x : y != 0.0 ? y : z;
    if (lead < 0.0) w = -w, x = -x, y = -y, z = -z;
    const double ww = w * w, xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    double R[9];
    R[0] = ((ww + xx) - yy) - zz;
    R[1] = 2.0 * (xy - wz);
    R[2] = 2.0 * (xz + wy);
    R[3] = 2.0 * (xy + wz);
    R[4] = ((ww - xx) + yy) - zz;
    R[5] = 2.0 * (yz - wx);
    R[6] = 2.0 * (xz - wy);
    R[7] = 2.0 * (yz + wx);
    R[8] = ((ww - xx) - yy) + zz;
    const double *qc = m + 1, *pc = m + 4;
    for (int k = 0; k < 9; ++k) T[k] = R[k];
    for (int r = 0; r < 3; ++r) T[9 + r] = pc[r] - ((R[3 * r] * qc[0] + R[3 * r + 1] * qc[1]) + R[3 * r + 2] * qc[2]);
    return status;
}

// What the loop's counter becomes.
MSPA_HD int64_t converged_now(int64_t before, int64_t iteration, const double *__restrict__ init, const double *__restrict__ T) {
    if (before != -1) return before;
    bool same = true;
    for (int k = 0; k < 12; ++k) same = same && same_bits(init[k], T[k]);
    return same ? iteration : -1;
}

// ---- the host twins -------------------------------------------------------------------------------------------------------------

// The query row of output row i of pair p.
inline int64_t query_row(const int64_t *q_offsets, const int64_t *pairs, const int64_t *out_offsets, int64_t p, int64_t i) {
    return q_offsets[cdist::pair_side(pairs, p, 0)] + (i - out_offsets[p]);
}

// out [M, 3] of tables that pair_rows accepted.
inline void transform_all(const double *q_xyz, const int64_t *q_offsets, const int64_t *pairs, int64_t P, const int64_t *out_offsets,
                          const double *transform, double *out) {
    for (int64_t p = 0; p < P; ++p)
        for (int64_t i = out_offsets[p]; i < out_offsets[p + 1]; ++i) {
            const int64_t row = query_row(q_offsets, pairs, out_offsets, p, i);
            const double q[3] = {q_xyz[3 * row], q_xyz[3 * row + 1], q_xyz[3 * row + 2]};
            transform_row(transform + 12 * p, q, out + 3 * i);
        }
}

// K sums at once on one thread, each in segs::ordered_sum's order: lane j's partial of sum k starts from 0.0 and adds term k of rows j,
// j + kLanes, ... in ascending order; the partials fold by strides kLanes / 2, ..., 1.  terms(i, term) fills the K terms of row i, once.
template <int K, typename Terms>
inline void ordered_sums(int64_t n, Terms terms, double total[K]) {
    double partial[K][segs::kLanes];
    for (int32_t j = 0; j < segs::kLanes; ++j) {
        for (int k = 0; k < K; ++k) partial[k][j] = 0.0;
        for (int64_t i = j; i < n; i += segs::kLanes) {
            double term[K];
            terms(i, term);
            for (int k = 0; k < K; ++k) partial[k][j] += term[k];
        }
    }
    for (int32_t t = segs::kLanes / 2; t >= 1; t >>= 1)
        for (int32_t j = 0; j < t; ++j)
            for (int k = 0; k < K; ++k) partial[k][j] += partial[k][j + t];
    for (int k = 0; k < K; ++k) total[k] = partial[k][0];
}

// The record of pair p on the CPU: kFirst, then kSecond sums, every row's terms evaluated once per pass.
inline void moments_of(const double *q_xyz, const int64_t *q_offsets, const double *t_xyz, int64_t Nt, const int64_t *pairs,
                       const int64_t *out_offsets, const int64_t *index, int64_t p, double m[kMoments]) {
    const int64_t a = out_offsets[p], n = out_offsets[p + 1] - a;
    double first[kFirst], qc[3], pc[3];
    auto row = [&](int64_t i, double q[3], double t[3]) {
        return used_row(q_xyz, query_row(q_offsets, pairs, out_offsets, p, a + i), t_xyz, clamped_index(index[a + i], Nt), q, t);
    };
    ordered_sums<kFirst>(n, [&](int64_t i, double term[kFirst]) {
        double q[3] = {0.0, 0.0, 0.0}, t[3] = {0.0, 0.0, 0.0};
        first_terms(row(i, q, t), q, t, term);
    }, first);
    centroids(first, qc, pc);
    m[0] = first[0];
    for (int ax = 0; ax < 3; ++ax) m[1 + ax] = qc[ax], m[4 + ax] = pc[ax];
    ordered_sums<kSecond>(n, [&](int64_t i, double term[kSecond]) {
        double q[3] = {0.0, 0.0, 0.0}, t[3] = {0.0, 0.0, 0.0};
        second_terms(row(i, q, t), q, t, qc, pc, term);
    }, m + 7);
}

// The fit of P pairs on the CPU.  eigen [P, 4] and converged [P] may be null.
inline void fit_all(const double *q_xyz, const int64_t *q_offsets, const double *t_xyz, int64_t Nt, const int64_t *pairs, int64_t P,
                    const int64_t *out_offsets, const int64_t *index, const double *init, int64_t iteration, double *transform, int64_t *used,
                    int32_t *status, double *eigen, int64_t *converged) {
    for (int64_t p = 0; p < P; ++p) {
        double m[kMoments], T[12];
        moments_of(q_xyz, q_offsets, t_xyz, Nt, pairs, out_offsets, index, p, m);
        status[p] = solve(m, init + 12 * p, T, eigen ? eigen + 4 * p : nullptr);
        used[p] = (int64_t)m[0];
        if (converged) converged[p] = converged_now(converged[p], iteration, init + 12 * p, T);
        for (int k = 0; k < 12; ++k) transform[12 * p + k] = T[k];
    }
}

}  // namespace calign
}  // namespace mspa
