// NEAREST-POINT DISTANCES BETWEEN THE CLOUDS OF TWO RAGGED BATCHES, stated once for the kernels of cloud_distance.hip and their host
// twins (mspa_cloud_distance_host, mspa_cloud_distance_fit_host), on top of knn_grid_core.h and cloud_segments_core.h.  A plain C++
// build of the three headers is the reference the device must agree with bit for bit.
//
// Batches and pairs.  The targets are t_xyz [Nt, 3] float64 with t_offsets [St + 1], the queries q_xyz [Nq, 3] float64 with q_offsets
// [Sq + 1]: two batches of cloud_segments_core.h.  pairs [P, 2] int64: pair p searches the rows of query segment pairs[p][0] in target
// segment pairs[p][1]; a segment of either side may stand in any number of pairs.  The output rows lie back to back by pair:
// out_offsets[p + 1] - out_offsets[p] = the rows of query segment pairs[p][0], a function of the host tables alone.  Without a pair
// table Sq == St and pair s is (s, s).  At most 2^30 output rows and 2^24 pairs.
//
// The distance.  d2(q, p) = (dx * dx + dy * dy) + dz * dz with d = p - q: knn::walk's own dist2, nothing fused (-ffp-contract=off).
// A query row reports sqrt(min over the target segment of d2) and the row OF t_xyz (global, int64) that attains the minimum, the
// LOWEST such row among equal d2.  The minimum of a set does not depend on the order of evaluation, so the device, the host twin
// and a brute force over all rows give the same bits.  An empty target segment gives +inf and -1.  A query row with a non-finite
// coordinate gives NaN and -1 and walks nothing.  Target coordinates are finite (checked where the grid is built).
//
// The cap.  With a max_distance (finite, > 0), cap2 = max_distance * max_distance, one rounded product; a row whose minimum d2 > cap2
// reports +inf and -1, every other row exactly what it reports without a cap.  No cap is cap2 = +inf.
//
// The grid of a target segment is make_grids of that segment's order-statistics box, unchanged, with kGridK as its neighbour count.
// The count only sizes the cells: results do not depend on it, the time does.
//
// The walk (nearest).  The same shells over the segment's grid as knn::walk, with one best d2, its sorted slot and that slot's
// original row instead of a list.  On d2 < best, or on d2 == best, the slot's original row is read from the target's order; an equal
// d2 replaces the best only with a lower row.  After the shell of radius r, b = outside_bound of the visited block; the walk ends
// when b is +inf (the block is the whole grid) or when b > 0 && min(best, cap2) <= b * b * kShrink.
//   * knn_grid_core.h's argument is about a point p and a face F_i alone: every point of a cell below i lies below F_i + eps, every
//     point of a cell from i up lies above F_i - eps.  It never uses that the query is one of the points.  The query enters only
//     through its own cell c (axis_cell clamps a query outside the box into the border cell of its side, so no block ever has an
//     unvisited neighbour on that side and outside_bound takes no face there) and through q - F_i, rounded once.  A query whose
//     cell is off by rounding sees a b that is zero or negative for one shell, and `b > 0` keeps the walk going.  So for ANY finite q
//     the evaluated d2 of every point in an unvisited cell is above b * b * kShrink, strictly: the exact distance is at least
//     b * (1 - 2u), its evaluated square within 4u, and kShrink = 1 - 2^-40 is far below both.
//   * best <= b * b * kShrink therefore means no unvisited point reaches best, neither below it nor equal to it: the minimum AND
//     the lowest row among its ties are final.
//   * The cap: cap2 <= b * b * kShrink means every unvisited point has d2 > cap2, so a row with d2 <= cap2 has been visited.  If the
//     walk ends by the cap with best > cap2, the true minimum is above cap2 too and the row reports +inf; if best <= cap2, then best
//     <= b * b * kShrink as well, which is the end without a cap.
// A far query without a cap walks the whole grid: its b stays below its best until the block is everything.
//
// Every table entry the walk indexes with is clamped first (starts into [0, n], the order entry into the segment by
// row_in_segment): a corrupt table gives wrong distances, never an access outside a buffer.
//
// The summary of a pair over its n output rows d: rows = n; finite = the rows with d < inf; within = the rows with d <= tau (tau
// finite, >= 0; NaN counts nowhere); sum and sum_sq = the sums of d and of d * d over the finite rows, in segs::ordered_sum's order
// (256 lane sums folded by halving strides) with 0.0 as the term of a non-finite row; max = the largest finite d, -inf where none is.
#pragma once
#include "cloud_segments_core.h"

namespace mspa {
namespace cdist {

using knn::Grid;

constexpr int32_t kGridK = 1;                                    // measured: profiles/cloud_distance_device.md
constexpr int64_t kMaxRows = (int64_t)1 << 30;
constexpr int64_t kMaxPairs = (int64_t)1 << 24;

MSPA_HD int64_t clamp_to(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }   // lo <= hi

MSPA_HD bool finite3(const double q[3]) { return fabs(q[0]) < INFINITY && fabs(q[1]) < INFINITY && fabs(q[2]) < INFINITY; }

// cap2 of a max_distance.  The entry points spell "no cap" as max_distance = +inf, whose cap2 is +inf by the same product.
MSPA_HD double cap2_of(double max_distance) { return max_distance * max_distance; }
inline bool cap_ok(double max_distance) { return max_distance > 0.0; }                          // finite and > 0, or +inf: no cap
inline bool tau_ok(double tau) { return tau >= 0.0 && tau < INFINITY; }

// ---- the pairs ----------------------------------------------------------------------------------------------------------------

MSPA_HD int64_t pair_side(const int64_t *__restrict__ pairs, int64_t p, int side) { return pairs ? pairs[2 * p + side] : p; }

// out_offsets [P + 1] of a pair table (pairs null: the identity, P == Sq == St) and the rows in all, or -1 for a pair outside
// [0, Sq) x [0, St), more than kMaxPairs pairs or more than kMaxRows rows.
inline int64_t pair_rows(const int64_t *q_offsets, int64_t Sq, int64_t St, const int64_t *pairs, int64_t P, int64_t *out_offsets) {
    if (P < 0 || P > kMaxPairs || (!pairs && (P != Sq || P != St))) return -1;
    int64_t run = 0;
    if (out_offsets) out_offsets[0] = 0;
    for (int64_t p = 0; p < P; ++p) {
        const int64_t qs = pair_side(pairs, p, 0), ts = pair_side(pairs, p, 1);
        if (qs < 0 || qs >= Sq || ts < 0 || ts >= St) return -1;
        run += q_offsets[qs + 1] - q_offsets[qs];
        if (run > kMaxRows) return -1;
        if (out_offsets) out_offsets[p + 1] = run;
    }
    return run;
}

// ---- the walk -----------------------------------------------------------------------------------------------------------------

struct Found {
    double d2;                                                   // the smallest squared distance, +inf where no point was met
    int64_t row;                                                 // the lowest row of t_xyz that attains it, -1 where none
    int32_t slot;                                                // its sorted slot in the segment
};

// The nearest of a target segment's n >= 1 sorted points to a finite q: pts and order at the segment's first slot, starts at its
// first entry with n_slots >= 1 entries behind it, [a, a + n) the segment's rows among the N of the batch.  Returns the number of
// distances evaluated.
MSPA_HD int64_t nearest(const Grid &g, const double *__restrict__ pts, const int32_t *__restrict__ starts, int64_t n_slots,
                        const int64_t *__restrict__ order, int64_t N, int64_t a, int64_t n, const double q[3], double cap2, Found &f) {
    double best = INFINITY;
    int64_t row = -1;
    int32_t at = 0;
    int64_t evals = 0;
    const int32_t c[3] = {knn::axis_cell(g, 0, q[0]), knn::axis_cell(g, 1, q[1]), knn::axis_cell(g, 2, q[2])};
    auto take = [&](double d2, int32_t i) {
        if (d2 <= best) {
            const int64_t o = segs::row_in_segment(order[i], N, a, a + n);
            if (d2 < best || o < row) {
                best = d2;
                row = o;
                at = i;
            }
        }
    };
    auto dist2 = [&](int32_t i) {
        const double dx = pts[3 * (int64_t)i] - q[0], dy = pts[3 * (int64_t)i + 1] - q[1], dz = pts[3 * (int64_t)i + 2] - q[2];
        return (dx * dx + dy * dy) + dz * dz;
    };
    auto start_of = [&](int32_t cell) { return (int32_t)clamp_to(starts[clamp_to(cell, 0, n_slots - 1)], 0, n); };
    auto scan = [&](int32_t row_cell, int32_t x0, int32_t x1) {              // the cells x0 .. x1 of one row: one run of points
        const int32_t begin = start_of(row_cell + x0), end = start_of(row_cell + x1 + 1);
        int32_t i = begin;
        for (; i + 4 <= end; i += 4) {                                        // four points' loads in flight before the best is touched
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
        if (b > 0.0 && (best < cap2 ? best : cap2) <= b * b * knn::kShrink) break;
    }
    f.d2 = best;
    f.row = row;
    f.slot = at;
    return evals;
}

// What a row reports from what its walk found.
MSPA_HD double reported_distance(const Found &f, double cap2) { return f.row >= 0 && f.d2 <= cap2 ? sqrt(f.d2) : INFINITY; }
MSPA_HD int64_t reported_index(const Found &f, double cap2) { return f.row >= 0 && f.d2 <= cap2 ? f.row : -1; }

// One output row, whole: the query q against target segment [a, a + n) of N rows.  Everything a caller indexed the tables with is
// clamped already.  Returns the evaluations.
MSPA_HD int64_t nearest_row(const Grid &g, const double *__restrict__ pts, const int32_t *__restrict__ starts, int64_t n_slots,
                            const int64_t *__restrict__ order, int64_t N, int64_t a, int64_t n, const double q[3], double cap2,
                            double &distance, int64_t &index) {
    if (!finite3(q)) {
        distance = segs::no_value();
        index = -1;
        return 0;
    }
    Found f{INFINITY, -1, 0};
    const int64_t evals = n > 0 ? nearest(g, pts + 3 * a, starts, n_slots, order + a, N, a, n, q, cap2, f) : 0;
    distance = reported_distance(f, cap2);
    index = reported_index(f, cap2);
    return evals;
}

// ---- the summary ----------------------------------------------------------------------------------------------------------------

MSPA_HD double finite_term(double d) { return d < INFINITY ? d : 0.0; }
MSPA_HD double square_term(double d) { return d < INFINITY ? d * d : 0.0; }

// ---- the host twins -------------------------------------------------------------------------------------------------------------

// The search structure of a target batch in the device's form: boxes from each segment's order statistics, the grids, ONE stable
// sort of the global keys, the gather, the starts.
struct HostIndex {
    std::vector<Grid> grids;
    std::vector<int64_t> cell_base, order;
    std::vector<double> pts;
    std::vector<int32_t> starts;
};

// False: no grid for a segment.  Finite coordinates and a batch that batch_rows accepts.
inline bool build_index(const double *xyz, const int64_t *offsets, int64_t S, int32_t k, HostIndex &ix) {
    const int64_t N = offsets[S];
    std::vector<double> lo((size_t)S * 3 + 3, 0.0), hi((size_t)S * 3 + 3, 0.0), col;
    for (int64_t s = 0; s < S; ++s) {
        const int64_t a = offsets[s], n = offsets[s + 1] - a, r = n / 100;
        if (n == 0) continue;
        col.resize((size_t)n);
        for (int ax = 0; ax < 3; ++ax) {
            for (int64_t i = 0; i < n; ++i) col[(size_t)i] = xyz[3 * (a + i) + ax];
            std::nth_element(col.begin(), col.begin() + r, col.end());
            lo[(size_t)(3 * s + ax)] = col[(size_t)r];
            std::nth_element(col.begin(), col.begin() + (n - 1 - r), col.end());
            hi[(size_t)(3 * s + ax)] = col[(size_t)(n - 1 - r)];
        }
    }
    ix.grids.assign((size_t)S + 1, Grid{});
    if (!segs::make_grids(lo.data(), hi.data(), offsets, S, k, ix.grids.data())) return false;
    ix.cell_base.assign((size_t)S + 1, 0);
    segs::cell_tables(offsets, S, k, ix.cell_base.data());
    std::vector<int64_t> keys((size_t)N), sorted_keys((size_t)N);
    ix.order.resize((size_t)N);
    for (int64_t i = 0; i < N; ++i) {
        const int64_t s = segs::segment_of(offsets, S, i);
        keys[(size_t)i] = segs::key_of(ix.grids[(size_t)s], ix.cell_base[(size_t)s], xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
    }
    std::iota(ix.order.begin(), ix.order.end(), (int64_t)0);
    std::stable_sort(ix.order.begin(), ix.order.end(), [&](int64_t x, int64_t y) { return keys[(size_t)x] < keys[(size_t)y]; });
    ix.pts.resize((size_t)N * 3);
    for (int64_t i = 0; i < N; ++i) {                            // the gather: the key comes from the point that was copied
        const int64_t s = segs::segment_of(offsets, S, i);
        const int64_t o = segs::row_in_segment(ix.order[(size_t)i], N, offsets[s], offsets[s + 1]);
        for (int ax = 0; ax < 3; ++ax) ix.pts[(size_t)(3 * i + ax)] = xyz[3 * o + ax];
        sorted_keys[(size_t)i] = segs::key_of(ix.grids[(size_t)s], ix.cell_base[(size_t)s], ix.pts[(size_t)(3 * i)], ix.pts[(size_t)(3 * i + 1)],
                                              ix.pts[(size_t)(3 * i + 2)]);
    }
    ix.starts.assign((size_t)segs::starts_slots(ix.cell_base.data(), S) + 1, 0);
    for (int64_t s = 0; s < S; ++s) {
        const int64_t a = offsets[s], b = offsets[s + 1];
        if (a == b) continue;
        for (int32_t c = 0; c <= ix.grids[(size_t)s].cells; ++c)
            ix.starts[(size_t)(segs::starts_base(ix.cell_base.data(), s) + c)] =
                (int32_t)(segs::first_at_or_above(sorted_keys.data(), a, b, ix.cell_base[(size_t)s] + c) - a);
    }
    return true;
}

// The whole search on the CPU: distance [M], index [M] (when wanted) and evals [M] (when wanted) for the M = out_offsets[P] output
// rows.  pairs may be null (the identity).  Tables that pair_rows accepted, finite targets, cap2 from cap2_of.  False: no grid.
inline bool nearest_segments_all(const double *t_xyz, const int64_t *t_offsets, int64_t St, const double *q_xyz, const int64_t *q_offsets,
                                 const int64_t *pairs, int64_t P, const int64_t *out_offsets, int32_t k, double cap2, double *distance,
                                 int64_t *index, int32_t *evals) {
    HostIndex ix;
    if (!build_index(t_xyz, t_offsets, St, k, ix)) return false;
    const int64_t Nt = t_offsets[St], slots = segs::starts_slots(ix.cell_base.data(), St);
    for (int64_t p = 0; p < P; ++p) {
        const int64_t qs = pair_side(pairs, p, 0), ts = pair_side(pairs, p, 1);
        const int64_t a = t_offsets[ts], n = t_offsets[ts + 1] - a, sb = segs::starts_base(ix.cell_base.data(), ts);
        for (int64_t i = out_offsets[p]; i < out_offsets[p + 1]; ++i) {
            const int64_t row = q_offsets[qs] + (i - out_offsets[p]);
            const double q[3] = {q_xyz[3 * row], q_xyz[3 * row + 1], q_xyz[3 * row + 2]};
            double d;
            int64_t at;
            const int64_t e = nearest_row(ix.grids[(size_t)ts], ix.pts.data(), ix.starts.data() + sb, slots - sb, ix.order.data(), Nt, a, n, q,
                                          cap2, d, at);
            distance[i] = d;
            if (index) index[i] = at;
            if (evals) evals[i] = (int32_t)e;
        }
    }
    return true;
}

// The summaries of P pairs on the CPU.
inline void fit_segments_all(const double *distance, const int64_t *out_offsets, int64_t P, double tau, int64_t *rows, int64_t *finite,
                             int64_t *within, double *sum, double *sum_sq, double *max) {
    for (int64_t p = 0; p < P; ++p) {
        const double *d = distance + out_offsets[p];
        const int64_t n = out_offsets[p + 1] - out_offsets[p];
        int64_t nf = 0, nw = 0;
        double m = -INFINITY;
        for (int64_t i = 0; i < n; ++i) {
            if (d[i] < INFINITY) {
                ++nf;
                m = d[i] > m ? d[i] : m;
            }
            if (d[i] <= tau) ++nw;
        }
        rows[p] = n;
        finite[p] = nf;
        within[p] = nw;
        sum[p] = segs::ordered_sum(n, [&](int64_t i) { return finite_term(d[i]); });
        sum_sq[p] = segs::ordered_sum(n, [&](int64_t i) { return square_term(d[i]); });
        max[p] = m;
    }
}

}  // namespace cdist
}  // namespace mspa
