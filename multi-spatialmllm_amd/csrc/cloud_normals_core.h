// THE K NEAREST ROWS AND THE NORMAL OF EVERY ROW OF A RAGGED BATCH OF CLOUDS, stated once for the kernel of cloud_normals.hip and its host
// twin (mspa_cloud_normals_host), on top of cloud_distance_core.h, cloud_segments_core.h and knn_grid_core.h.  A plain C++ build of the
// headers is the reference the device must agree with bit for bit.  Every step is one float64 + - * / or sqrt,
// nothing is fused (-ffp-contract=off), no libm function is called.
//
// 1. NEIGHBOURS.  The neighbours of row i of a segment of n rows are the min(k, n) rows of the SAME segment with the smallest
// (d2, original row), in lexicographic order, 1 <= k <= knn::kMaxK.  d2 = (dx * dx + dy * dy) + dz * dz with d = p - q: knn::walk's own
// dist2.  The row itself is among them at d2 = 0 (Open3D's KNN search counts the query point too).  With a max_distance (finite, > 0;
// cap2 = cdist::cap2_of, one rounded product; +inf: no cap) only rows with d2 <= cap2 count: Open3D's hybrid search.  A d2 that is not
// below +inf (an overflowed square of coordinates beyond 1e154) counts nowhere.  `used` is the number of neighbours found.
//
// The walk (neighbours()) is a third function beside knn::walk and cdist::nearest: the same shells over the segment's grid, the same
// outside_bound and kShrink, with an ascending list of (d2, sorted slot) in place of walk's list of d2 and nearest's single best.  An
// entry goes in front of the entries with a larger d2 and, among entries of EQUAL d2, in front of those with a larger original row;
// the original row of a slot is read through the segment's `order`, clamped by segs::row_in_segment, and only where two d2 are equal.
// With the list full a candidate above the k-th d2, or equal to it with a row that is not lower than the k-th's, is dropped.  After
// the shell of radius r, b = outside_bound of the visited block; the walk ends when b is +inf (the block is the whole grid) or when
// b > 0 && min(kth, cap2) <= b * b * kShrink, kth = the list's k-th d2, +inf while the list is not full.
//   * Why the k-th element may decide.  cloud_distance_core.h's argument is about a point p, a face F_i and ANY finite query: the
//     evaluated d2 of every point in an unvisited cell is above b * b * kShrink, STRICTLY (the exact distance is at least b * (1 - 2u),
//     its evaluated square within 4u, and kShrink = 1 - 2^-40 is far below both).  There it makes "the minimum and the lowest row among
//     its ties" final.  Here the stop compares kth, and an equal d2 in an unvisited cell WOULD change the set (its row may be lower
//     than the k-th's).  The strict bound rules that out as it did there: kth <= b * b * kShrink < every unvisited d2 means no
//     unvisited point has d2 < kth, and none has d2 == kth.  So every row that belongs to the k smallest (d2, row) has been visited;
//     the list holds the k smallest (d2, row) of the visited rows whatever the order they came in (an insertion keeps the list sorted by
//     the full key, and a row is dropped only when k visited rows precede it); the set, and its order, are final.  The order of the
//     rows inside a cell, which a stable sort inherits from the input, decides nothing.
//   * The cap: cap2 <= b * b * kShrink means every unvisited point has d2 > cap2 and counts nowhere.
// Every table entry used as an index is clamped first (a cell into the segment's slots of `starts`, a start into [0, n], an order
// entry into the segment, a list slot into [0, n) before the moments read it): a corrupt table gives wrong neighbours, never an
// access outside a buffer.  The input contract is knn_mean_distance_segments': finite xyz, checked where the grid is built.
//
// 2. MOMENTS, over the neighbours in ascending (d2, row) order, summed sequentially from 0.0.  First the centroid: three sums, one
// division by `used` each.  Then the six centred products (p - c)_a * (p - c)_b, a <= b: one subtraction per coordinate, one product,
// one addition.  They are NOT divided by `used`: the normal and the curvature are ratios.  Because of the centring, a cloud 10^6 m from
// the origin loses nothing to its offset beyond the one rounding of each difference.
//
// 3. EIGENVECTORS.  Cyclic Jacobi on the symmetric 3 x 3, kSweeps sweeps over the pivots (0,1), (0,2), (1,2) in that order, V from the
// identity.  The rotation is calign::rotate's, formula for formula (cloud_align_core.h; a 3 x 3 copy, rotate3, so that file's kernels
// keep their text):
//      theta = (a_qq - a_pp) / (2 * a_pq);  t = sign(theta) / (|theta| + sqrt(theta * theta + 1))  (sign(0) = +1);
//      c = 1 / sqrt(t * t + 1);  s = t * c;   a_pp -= t * a_pq;  a_qq += t * a_pq;  a_pq = a_qp = 0;
//      the third k: (a_kp, a_kq) <- (c * a_kp - s * a_kq, s * a_kp + c * a_kq), mirrored; every k: the same for (v_kp, v_kq).
// A pivot that is exactly 0.0 is skipped, the only data-dependent branch.  A theta whose square overflows gives t = 0, c = 1, s = 0.
// kSweeps = 8.  The argument is section 0.29's, one size down: the cyclic-by-rows method converges quadratically once the off-diagonal
// norm is below the eigenvalue gaps (Wilkinson 1962; van Kempen 1966 for multiple eigenvalues), and before that every rotation takes
// 2 * a_pq^2 off the off-diagonal square sum, which therefore never grows (Forsythe and Henrici 1960 for the convergence).  A
// 3 x 3 matrix reaches the quadratic phase in two or three sweeps; from an off-diagonal norm of 2^-10 of the spread, three more
// sweeps square it to below 2^-80, under one rounding of the entries.  A gap near the status limit 2^-26 only slows the rotation
// inside the nearly double eigenspace, whose mix the status turns away where it matters.  That is a sketch, not a bound: no bound
// on the sweeps of the pre-quadratic phase is derived here, and THE CONSTANT IS EMPIRICAL WITH A MARGIN.  Measured with these
// formulas in float64: over every row of the test batch (3 959 neighbourhoods: slabs, lattices with exact zeros, a sphere, a plane
// 10^6 m away, extents of 1 cm and 100 m) the off-diagonal norm falls to 2^-53 of the largest diagonal entry after at most 4
// sweeps (1: 695 rows, 2: 261, 3: 2 421, 4: 582); over 20 000 random matrices whose two smallest, or two middle, eigenvalues
// lie 2^-20 to 2^-30 of the spread apart -- around the status limit -- after at most 3 (the worst: 1.7e-7, 3.8e-15, 8.5e-52).
// Eight is twice the worst seen and costs one lane 24 rotations a row.  The standing check of the constant is the accuracy against
// a 60-digit oracle that tests/test_cloud_normals_cpu.py asserts on every class of input.
// The eigenvalues are the diagonal; l0 <= l1 <= l2 their ascending order.  The normal is the column of the smallest one, the LOWEST
// column among equal ones, divided by its norm sqrt((x * x + y * y) + z * z).
//
// 4. SIGN.  Without a viewpoint the first non-zero component is positive: section 0.29's quaternion convention.  With a viewpoint v
// of the segment (viewpoints [S, 3]; a row with a non-finite component, NaN by convention, means "none"), the canonical normal is
// negated when ((v_x - p_x) * n_x + (v_y - p_y) * n_y) + (v_z - p_z) * n_z < 0, p the row itself; a dot of exactly 0 keeps the
// canonical sign.
//
// 5. PER-ROW OUTPUTS.  normal [3]; curvature = l0 / ((l0 + l1) + l2), the surface variation (Pauly 2002), 0.0 where the denominator is
// 0.0; used; status: kOk; kFew where used < 3; else kDegenerate where NOT (l1 - l0 > kGap * (l2 - l0)) or l2 - l0 is not finite,
// kGap = 2^-26 -- collinear (l1 = l0 = 0), coincident (all 0) and isotropic neighbourhoods fall here, and below that gap the normal is
// not determined to half the digits.  A row that is not kOk has a NaN normal and a NaN curvature (segs::no_value()).
//
// 6. EXACT IDENTITIES.
//   * A neighbourhood in a plane z = const whose `used`-fold sequential sum of z is exact (any z that is an integer below 2^46, as
//     the tests' lattice at z = 3) has the normal (0, 0, 1) and the curvature 0.0 exactly, without a viewpoint.  The centroid's z is
//     then z itself (the exact sum divided by used rounds to the representable quotient), every (p - c)_z is 0.0, the products xz, yz
//     and zz are +-0.0 and their sums from 0.0 are +0.0.  The pivots (0,2) and (1,2) are exactly 0.0 and are skipped; the pivot (0,1)
//     makes a_20 = c * 0 - s * 0 and a_21 = s * 0 + c * 0, still zero, and touches the columns 0 and 1 of V alone, whose third row
//     stays zero the same way.  So column 2 of V stays (0, 0, 1) and a_22 stays 0.0 through every rotation.  Where the status is kOk the
//     other two eigenvalues exceed 0.0 (l1 - l0 > 0 with l0 <= 0 would need a negative eigenvalue of a 2 x 2 block whose larger one is
//     2^26 times its size: the rotation's rounding is 2^-52 of it), so column 2 is the one of the smallest: the normal is
//     (0, 0, 1) / sqrt((0 + 0) + 1) = (0, 0, 1), its first non-zero component positive, and the curvature 0.0 / (positive) = 0.0.
//   * The same input gives the same bits on every run, and in any order of the rows inside a cell (1. above): the list is a function
//     of the set of (d2, row), and everything after it reads the list alone.
//   * Renumbering the rows of a segment moves the outputs with the rows wherever no two d2 of a neighbourhood's candidates are equal
//     (the row breaks ties, so a tie may be broken the other way after a renumbering).
//
// The unit norm (kUnitBound).  Let u = 2^-53.  The norm's square is 3 products and 2 sums of non-negative terms: relative error
// <= 3u; its root <= 1.5u + u; each quotient one more u: the stored n_i = v_i / |v| * (1 + e_i) with |e_i| <= 3.5u + O(u^2), so
// | |n|^2 - 1 | <= 7u + O(u^2) < 8u = kUnitBound, for every normal written; a negation is exact.
#pragma once
#include "cloud_distance_core.h"

namespace mspa {
namespace cnorm {

using knn::Grid;

constexpr int32_t kSweeps = 8;
constexpr int32_t kGapExponent = -26;
constexpr double kGap = 1.0 / (double)((int64_t)1 << 26);
constexpr double kUnitBound = 8.0 / 9007199254740992.0;          // 8 * 2^-53
constexpr int32_t kOk = 0, kFew = 1, kDegenerate = 2;

// ---- the walk -----------------------------------------------------------------------------------------------------------------

// The min(k, n) nearest of a segment's n >= 1 sorted points to a finite q, ascending by (d2, original row) in list.d2(j) / list.slot(j),
// j < count: pts and order at the segment's first slot, starts at its first entry with n_slots >= 1 entries behind it, [a, a + n) the
// segment's rows among the N of the batch, 1 <= k.  List is anything with `double &d2(int)` and `int32_t &slot(int)` for j < k.
// Returns the number of distances evaluated.
template <typename List>
MSPA_HD int64_t neighbours(const Grid &g, const double *__restrict__ pts, const int32_t *__restrict__ starts, int64_t n_slots,
                           const int64_t *__restrict__ order, int64_t N, int64_t a, int64_t n, const double q[3], int32_t k, double cap2,
                           List list, int32_t &count) {
    int32_t m = 0;
    double kth = INFINITY;                                       // the list's k-th d2 once it is full
    int64_t evals = 0;
    const int32_t c[3] = {knn::axis_cell(g, 0, q[0]), knn::axis_cell(g, 1, q[1]), knn::axis_cell(g, 2, q[2])};
    auto row_of = [&](int32_t slot) { return segs::row_in_segment(order[slot], N, a, a + n); };
    auto take = [&](double d2, int32_t i) {
        if (!(d2 <= cap2) || !(d2 < INFINITY) || d2 > kth) return;
        int64_t mine = -1;
        if (m == k && d2 == kth) {
            mine = row_of(i);
            if (mine >= row_of(list.slot(k - 1))) return;
        }
        int32_t j = m < k ? m : k - 1;
        for (; j > 0; --j) {
            const double before = list.d2(j - 1);
            if (before < d2) break;
            if (before == d2) {
                if (mine < 0) mine = row_of(i);
                if (row_of(list.slot(j - 1)) < mine) break;
            }
            list.d2(j) = before;
            list.slot(j) = list.slot(j - 1);
        }
        list.d2(j) = d2;
        list.slot(j) = i;
        if (m < k) ++m;
        if (m == k) kth = list.d2(k - 1);
    };
    auto dist2 = [&](int32_t i) {
        const double dx = pts[3 * (int64_t)i] - q[0], dy = pts[3 * (int64_t)i + 1] - q[1], dz = pts[3 * (int64_t)i + 2] - q[2];
        return (dx * dx + dy * dy) + dz * dz;
    };
    auto start_of = [&](int32_t cell) { return (int32_t)cdist::clamp_to(starts[cdist::clamp_to(cell, 0, n_slots - 1)], 0, n); };
    auto scan = [&](int32_t row_cell, int32_t x0, int32_t x1) {              // the cells x0 .. x1 of one row: one run of points
        const int32_t begin = start_of(row_cell + x0), end = start_of(row_cell + x1 + 1);
        int32_t i = begin;
        for (; i + 4 <= end; i += 4) {                                        // four points' loads in flight before the list is touched
            const double d0 = dist2(i), d1 = dist2(i + 1), d2 = dist2(i + 2), d3 = dist2(i + 3);
            take(d0, i);
            take(d1, i + 1);
            take(d2, i + 2);
            take(d3, i + 3);
        }
        for (; i < end; ++i) take(dist2(i), i);
        if (end > begin) evals += end - begin;
    };
    for (int32_t r = 0;; ++r) {
        int32_t lo[3], hi[3];
        for (int ax = 0; ax < 3; ++ax) {
            lo[ax] = c[ax] - r > 0 ? c[ax] - r : 0;
            hi[ax] = c[ax] + r < g.dim[ax] - 1 ? c[ax] + r : g.dim[ax] - 1;
        }
        for (int32_t z = lo[2]; z <= hi[2]; ++z) {
            const bool z_in = z > c[2] - r && z < c[2] + r;                   // inside the block visited so far, along z
            for (int32_t y = lo[1]; y <= hi[1]; ++y) {
                const int32_t row_cell = (z * g.dim[1] + y) * g.dim[0];
                if (!(z_in && y > c[1] - r && y < c[1] + r)) {
                    scan(row_cell, lo[0], hi[0]);
                } else {                                                      // only the two ends of the row are new
                    if (c[0] - r >= 0) scan(row_cell, c[0] - r, c[0] - r);
                    if (c[0] + r <= g.dim[0] - 1) scan(row_cell, c[0] + r, c[0] + r);
                }
            }
        }
        const double b = knn::outside_bound(g, q, lo, hi);
        if (b == INFINITY) break;                                             // the block is the whole grid
        if (b > 0.0 && (kth < cap2 ? kth : cap2) <= b * b * knn::kShrink) break;
    }
    count = m;
    return evals;
}

// ---- the fit of one neighbourhood ---------------------------------------------------------------------------------------------

// One Jacobi rotation of the symmetric a and of v at the pivot (p, q), p < q: calign::rotate on 3 x 3.
MSPA_HD void rotate3(double a[3][3], double v[3][3], int p, int q) {
    const double apq = a[p][q];
    if (apq == 0.0) return;
    const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
    const double root = sqrt(theta * theta + 1.0);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + root);
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    a[p][p] = a[p][p] - t * apq;
    a[q][q] = a[q][q] + t * apq;
    a[p][q] = a[q][p] = 0.0;
    for (int k = 0; k < 3; ++k) {
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

struct Fit {
    double normal[3], curvature;
    int32_t status;
};

// The centroid and the six centred sums (xx, xy, xz, yy, yz, zz) of the list's `count` >= 1 neighbours among the segment's n sorted points.
template <typename List>
MSPA_HD void moments(const double *__restrict__ pts, int64_t n, List list, int32_t count, double c[3], double m[6]) {
    double sum[3] = {0.0, 0.0, 0.0};
    for (int32_t j = 0; j < count; ++j) {
        const int64_t at = cdist::clamp_to(list.slot(j), 0, n - 1);
        for (int ax = 0; ax < 3; ++ax) sum[ax] = sum[ax] + pts[3 * at + ax];
    }
    for (int ax = 0; ax < 3; ++ax) c[ax] = sum[ax] / (double)count;
    for (int e = 0; e < 6; ++e) m[e] = 0.0;
    for (int32_t j = 0; j < count; ++j) {
        const int64_t at = cdist::clamp_to(list.slot(j), 0, n - 1);
        const double dx = pts[3 * at] - c[0], dy = pts[3 * at + 1] - c[1], dz = pts[3 * at + 2] - c[2];
        m[0] = m[0] + dx * dx;
        m[1] = m[1] + dx * dy;
        m[2] = m[2] + dx * dz;
        m[3] = m[3] + dy * dy;
        m[4] = m[4] + dy * dz;
        m[5] = m[5] + dz * dz;
    }
}

// The six sums, the neighbour count, the row p itself and its segment's viewpoint (null or a non-finite row: none) -> the row's fit.
MSPA_HD void solve(const double m[6], int32_t count, const double p[3], const double *__restrict__ view, Fit &f) {
    double a[3][3], v[3][3];
    a[0][0] = m[0], a[0][1] = a[1][0] = m[1], a[0][2] = a[2][0] = m[2];
    a[1][1] = m[3], a[1][2] = a[2][1] = m[4], a[2][2] = m[5];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) v[i][j] = i == j ? 1.0 : 0.0;
    for (int32_t sweep = 0; sweep < kSweeps; ++sweep) {
        rotate3(a, v, 0, 1);
        rotate3(a, v, 0, 2);
        rotate3(a, v, 1, 2);
    }
    int low = 0;
    for (int k = 1; k < 3; ++k)
        if (a[k][k] < a[low][low]) low = k;
    const double e1 = a[(low + 1) % 3][(low + 1) % 3], e2 = a[(low + 2) % 3][(low + 2) % 3];
    const double l0 = a[low][low], l1 = e1 < e2 ? e1 : e2, l2 = e1 < e2 ? e2 : e1;
    const double spread = l2 - l0;
    f.status = kOk;
    if (count < 3)
        f.status = kFew;
    else if (!(spread < INFINITY) || !(l1 - l0 > kGap * spread))
        f.status = kDegenerate;
    if (f.status != kOk) {
        f.normal[0] = f.normal[1] = f.normal[2] = f.curvature = segs::no_value();
        return;
    }
    double x = v[0][low], y = v[1][low], z = v[2][low];
    const double norm = sqrt((x * x + y * y) + z * z);
    x = x / norm, y = y / norm, z = z / norm;
    const double lead = x != 0.0 ? x : y != 0.0 ? y : z;
    if (lead < 0.0) x = -x, y = -y, z = -z;
    if (view) {
        const double w[3] = {view[0], view[1], view[2]};
        if (cdist::finite3(w)) {
            const double dot = ((w[0] - p[0]) * x + (w[1] - p[1]) * y) + (w[2] - p[2]) * z;
            if (dot < 0.0) x = -x, y = -y, z = -z;
        }
    }
    f.normal[0] = x, f.normal[1] = y, f.normal[2] = z;
    const double den = (l0 + l1) + l2;
    f.curvature = den == 0.0 ? 0.0 : l0 / den;
}

// What the neighbour table reports for entry j of a row with `count` neighbours.
MSPA_HD double reported_distance(double d2, int32_t j, int32_t count) { return j < count ? sqrt(d2) : INFINITY; }

// ---- the host twin ------------------------------------------------------------------------------------------------------------

struct HostPairs {
    double *d;
    int32_t *s;
    double &d2(int32_t j) const { return d[j]; }
    int32_t &slot(int32_t j) const { return s[j]; }
};

// The whole op on the CPU, in the device's form (cdist::build_index with k as the grids' neighbour count, then one walk and one fit per
// sorted slot).  Any of the two output groups may be absent: normal [N, 3], curvature [N] and status [N] (null together), nbr_index
// [N, k] and nbr_distance [N, k] (null together); used [N] always.  viewpoints [S, 3] or null.  Finite coordinates, a batch that
// batch_rows accepts, 1 <= k <= kMaxK, cap2 from cap2_of.  False: no grid for a segment.
inline bool normals_all(const double *xyz, const int64_t *offsets, int64_t S, int32_t k, double cap2, const double *viewpoints, double *normal,
                        double *curvature, int32_t *used, uint8_t *status, int64_t *nbr_index, double *nbr_distance) {
    cdist::HostIndex ix;
    if (!cdist::build_index(xyz, offsets, S, k, ix)) return false;
    const int64_t N = offsets[S], slots = segs::starts_slots(ix.cell_base.data(), S);
    double d2[knn::kMaxK];
    int32_t slot[knn::kMaxK];
    const HostPairs list{d2, slot};
    for (int64_t i = 0; i < N; ++i) {
        const int64_t s = segs::segment_of(offsets, S, i);
        const int64_t a = offsets[s], n = offsets[s + 1] - a, sb = segs::starts_base(ix.cell_base.data(), s);
        const int32_t kk = (int32_t)(k < n ? k : n);
        const double *pts = ix.pts.data() + 3 * a;
        const double q[3] = {ix.pts[(size_t)(3 * i)], ix.pts[(size_t)(3 * i + 1)], ix.pts[(size_t)(3 * i + 2)]};
        int32_t count = 0;
        neighbours(ix.grids[(size_t)s], pts, ix.starts.data() + sb, slots - sb, ix.order.data() + a, N, a, n, q, kk, cap2, list, count);
        const int64_t o = segs::row_in_segment(ix.order[(size_t)i], N, a, a + n);
        used[o] = count;
        if (nbr_index)
            for (int32_t j = 0; j < k; ++j) {
                nbr_index[o * k + j] = j < count ? segs::row_in_segment(ix.order[(size_t)(a + cdist::clamp_to(slot[j], 0, n - 1))], N, a, a + n) : -1;
                nbr_distance[o * k + j] = reported_distance(j < count ? d2[j] : 0.0, j, count);
            }
        if (normal) {
            Fit f;
            double c[3], m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (count > 0) moments(pts, n, list, count, c, m);
            solve(m, count, q, viewpoints ? viewpoints + 3 * s : nullptr, f);
            for (int ax = 0; ax < 3; ++ax) normal[3 * o + ax] = f.normal[ax];
            curvature[o] = f.curvature;
            status[o] = (uint8_t)f.status;
        }
    }
    return true;
}

}  // namespace cnorm
}  // namespace mspa
