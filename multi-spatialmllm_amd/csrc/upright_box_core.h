// The upright (gravity-aligned) minimal box of every cloud of a ragged batch, stated once for the kernels of upright_segments.hip and
// their host twin (mspa_upright_segments_host).  A plain C++ build of this header is the reference the device must agree with bit
// for bit.  The box is the z extent of the cloud times the minimum-area rectangle around the convex hull
// of its (x, y) footprint.
//
// The batch is cloud_segments_core.h's, with more columns: rows [N, C >= 3] float64, xyz in front, offsets [S + 1].
//
// THE RULE, per segment of n >= 0 rows.  Every floating-point step is one rounded float64 operation in the order written here (the
// library is built with -ffp-contract=off); the only fused operations are the fma calls of two_prod, on both sides.
//   * refusals   a non-finite x, y or z raises kNonFinite; a non-zero |x| or |y| outside [2^-200, 2^200] raises kOutOfWindow
//                (refusal_of).  A raised bit refuses the whole call.
//   * height     z_lo = min z, z_hi = max z.
//   * hull       the strict convex hull of the segment's distinct (x, y) pairs: counter-clockwise from the lexicographically
//                smallest vertex (x, then y); a collinear boundary point is no vertex; a vertex is reported as the lowest input row
//                that holds its coordinates.  h = 0 for n = 0, 1 for one distinct point, 2 for collinear points (their two
//                lexicographic ends), else >= 3.  orient(a, b, c) is the sign of the EXACT real determinant
//                (bx - ax)(cy - ay) - (by - ay)(cx - ax) of the three float64 points (first argument below), so the hull is the
//                mathematical one: no input order, and no filter in front of it that only removes non-vertices, changes it.
//                The form is Andrew's monotone chain (chain) over the rows sorted stably by (x, y): the lower chain ascending, the
//                upper chain descending, a point popped while orient(second, top, p) <= 0; hull = lower[:-1] + upper[:-1].
//   * rectangle  for every hull edge k: a = v_k, b = v_(k+1 mod h), d = b - a, and for every hull vertex j: q = v_j - a,
//                    t_j = q.x * d.x + q.y * d.y        c_j = q.y * d.x - q.x * d.y                                   (project)
//                    along_k = max t - min t            across_k = max c - min c
//                    m_k = (along_k * across_k) / (d.x * d.x + d.y * d.y)                                           (edge_measure)
//                the chosen edge k* is the lowest k with the smallest m_k (better_edge).  Minimum and maximum do not depend on
//                the order they are taken in, so no reduction order enters.
//   * box        [cx, cy, cz, length, width, height, ux, uy] (box_of): dd = d.d, L = sqrt(dd); length = along / L, width =
//                across / L; tm = (max t + min t) / 2, cm likewise; cx = a.x + (tm * d.x - cm * d.y) / dd, cy = a.y +
//                (tm * d.y + cm * d.x) / dd; cz = (z_hi + z_lo) / 2, height = z_hi - z_lo (calculate_aabb's z); (ux, uy) = d / L.
//                If width > length the two are swapped and the axis turns by 90 degrees, (-uy, ux).  Then the axis is negated
//                (exactly) unless ux > 0, or ux == 0 and uy > 0.  So length >= width and (ux, uy) is the direction of the length.
//                Division and square root are IEEE's; there is no trigonometric function in the rule.
//                h = 2: the generic path (edge 0, across 0, width 0).  h = 1: centre the point, sizes 0, axis (1, 0).  h = 0: eight NaN.
//
// THE WINDOW [2^-200, 2^200] on non-zero |x|, |y| keeps every product of the rule clear of overflow and underflow.  Write u = 2^-53.
//   (a) A non-zero coordinate is a multiple of 2^-252 (its last bit), so every difference of two coordinates is zero or a multiple
//       of 2^-252 at most 2^201 in size, rounded or not; a product of two differences is zero or at least 2^-504 and at most 2^402.
//   (b) The products that two_prod splits are coordinate times coordinate: in [2^-400, 2^400] or zero, and their rounding error is
//       a multiple of 2^-504, far above the smallest subnormal 2^-1074: fma(a, b, -p) is the exact error.  Sums of twelve such
//       terms stay below 2^404.  two_sum is exact whenever nothing overflows.
//   (c) The squared length of an edge is at least 2^-504 (the ends are distinct) and at most 2^403; t and c are at most 2^403, the
//       spans at most 2^404, the product of two spans at most 2^808.
//   (d) The vertex b itself has t = d.d, computed by the same operations as the divisor, and a has t = 0: along_k >= dd.  across_k
//       is zero or at least 2^-504.  So along * across is zero or at least 2^-1008 > DBL_MIN, and the quotient is at least across
//       (1 - 2u): every operation of m_k works on normal numbers (or exact zeros), and the standard model fl(x op y) = (x op y)
//       (1 + e), |e| <= u, holds for each.  A window down to 2^-240 would let along * across fall to 2^-1168.
//
// FIRST FLOATING-POINT ARGUMENT: orient returns the sign of the exact determinant.
//   The filter computes l = fl(fl(bx - ax) * fl(cy - ay)), r likewise, det = fl(l - r).  By (a) nothing underflows, so each of l, r
//   carries a relative error below 3u + 4u^2 and the subtraction one more u of det: the computed det differs from the exact one by
//   no more than u |det| + (3u + 4u^2)(|l| + |r|).  Shewchuk (Adaptive Precision Floating-Point Arithmetic and Fast Robust
//   Geometric Predicates, 1997, ccwerrboundA) carries this through the rounding of the bound itself: |det| > (3 + 16u) u
//   (|l| + |r|), the right side evaluated in floating point, implies that det has the exact sign.  Where the
//   filter does not decide, orient_exact expands the determinant into its six products
//       bx cy - bx ay - ax cy - by cx + by ax + ay cx        (the two ax ay cancel)
//   each as an error-free pair (two_prod, exact by (b)), and adds the twelve terms one by one into a non-overlapping expansion
//   (Shewchuk's Grow-Expansion: a chain of two_sum, exact).  The terms of a non-overlapping expansion in ascending order of
//   magnitude are dominated by the last non-zero one, whose sign is the determinant's.
//
// SECOND FLOATING-POINT ARGUMENT: the forward error of m_k against its exact rational value (the area of the rectangle on edge k).
//   Write ell = |d| for the edge's length, R for the diagonal of the footprint's axis-aligned bounding box (every |q| <= R and
//   ell <= R), W_d and W_n for the hull's exact extents along and across d (both <= R), so the exact m_k = W_d W_n.
//   Each difference carries (1 + e); t_j is two products of two such differences and one sum: |t^ - t| <= g4 (|q.x d.x| + |q.y d.y|)
//   <= g4 R ell, g_n = n u / (1 - n u), and the same for c_j.  A span is a difference of two of them, rounded once:
//   |along^ - ell W_d| <= 2 g4 R ell + u (ell R + 2 g4 R ell) <= 10 u R ell, and the same for across.  HERE IS THE CANCELLATION: the
//   error of a span is of the order u R ell whatever the span itself is, so relative to the rectangle's side W it is u R / W -- for
//   an edge that is short against a wide hull (W_d >= ell only) up to u R / ell, the diameter over the edge's length.  In absolute
//   terms the division by dd = ell^2 (relative error g4) takes the ell away again:
//       |m^ - m| <= (10 u R (W_d + W_n) + 100 u^2 R^2)(1 + g6) + g6 W_d W_n <= 27 u R^2.
//   rect_bound(R^2) = 64 u R^2 is stated with room: every m^_k lies within half of it of the exact m_k, so (i) the exact m of the
//   chosen edge exceeds the exact minimum by at most rect_bound, and (ii) length * width -- three more roundings and a square root,
//   a relative 6 u of a value <= R^2 -- lies within rect_bound of the chosen edge's exact m.  The spans over L are the box's sizes:
//   each is within 12 u R of the exact extent, and the centre within 12 u R plus u times the centre's own magnitude.
//
// THE ITERATION CAP.  A chain over m sorted points pushes each point once and pops a point at most once: at most m pops.  The
// pops are counted against cap (m by the rule); exceeding it sets kCapReached and the chain stops.  No lane waits for another.
#pragma once
#include "cloud_segments_core.h"

#include <cfloat>

#ifndef MSPA_UNROLL
#ifdef __HIPCC__
#define MSPA_UNROLL _Pragma("unroll")
#else
#define MSPA_UNROLL
#endif
#endif

namespace mspa {
namespace upright {

enum : int32_t { kNonFinite = 1, kOutOfWindow = 2, kCapReached = 4 };       // bits of the flag word
constexpr double kU = 0x1p-53;
constexpr double kWindowLo = 0x1p-200, kWindowHi = 0x1p200;
constexpr double kOrientFilter = (3.0 + 16.0 * kU) * kU;
constexpr double kRectBound = 64.0 * kU;                         // rect_bound over R^2
constexpr int kBoxValues = 8;

using segs::batch_rows;
using segs::first_at_or_above;
using segs::segment_of;

MSPA_HD bool in_window(double v) {
    const double a = fabs(v);
    return a == 0.0 || (a >= kWindowLo && a <= kWindowHi);
}

MSPA_HD int32_t refusal_of(double x, double y, double z) {
    if (!(fabs(x) < INFINITY) || !(fabs(y) < INFINITY) || !(fabs(z) < INFINITY)) return kNonFinite;
    return in_window(x) && in_window(y) ? 0 : kOutOfWindow;
}

MSPA_HD double rect_bound(double diagonal_sq) { return kRectBound * diagonal_sq; }

// ---- the exact predicate ------------------------------------------------------------------------------------------------------

MSPA_HD void two_sum(double a, double b, double &s, double &e) {
    s = a + b;
    const double bv = s - a;
    const double av = s - bv;
    const double br = b - bv;
    const double ar = a - av;
    e = ar + br;
}

MSPA_HD void two_prod(double a, double b, double &p, double &e) {
    p = a * b;
    e = fma(a, b, -p);
}

// The sign of the exact determinant, by expansion.
MSPA_HD int orient_exact(double ax, double ay, double bx, double by, double cx, double cy) {
    double term[12], e[12];
    two_prod(bx, cy, term[0], term[1]);
    two_prod(-bx, ay, term[2], term[3]);
    two_prod(-ax, cy, term[4], term[5]);
    two_prod(-by, cx, term[6], term[7]);
    two_prod(by, ax, term[8], term[9]);
    two_prod(ay, cx, term[10], term[11]);
    MSPA_UNROLL
    for (int i = 0; i < 12; ++i) {
        double q = term[i];
        MSPA_UNROLL
        for (int j = 0; j < i; ++j) {
            double s, r;
            two_sum(q, e[j], s, r);
            e[j] = r;
            q = s;
        }
        e[i] = q;
    }
    int sign = 0;
    MSPA_UNROLL
    for (int j = 0; j < 12; ++j) sign = e[j] > 0.0 ? 1 : e[j] < 0.0 ? -1 : sign;  // the last non-zero term decides
    return sign;
}

// The filter alone: +1 / -1 where the floating determinant proves its sign, 0 where it does not.
MSPA_HD int orient_certain(double ax, double ay, double bx, double by, double cx, double cy) {
    const double abx = bx - ax, acy = cy - ay, aby = by - ay, acx = cx - ax;
    const double l = abx * acy, r = aby * acx;
    const double det = l - r;
    const double sum = fabs(l) + fabs(r);
    const double bound = kOrientFilter * sum;
    return det > bound ? 1 : -det > bound ? -1 : 0;
}

MSPA_HD int orient(double ax, double ay, double bx, double by, double cx, double cy) {
    const int certain = orient_certain(ax, ay, bx, by, cx, cy);
    return certain != 0 ? certain : orient_exact(ax, ay, bx, by, cx, cy);
}

// Whether p is PROVED strictly inside the triangle a b c (of either orientation) by the filter alone.  Such a point is an interior
// point of the hull of any set that holds a, b and c: never a vertex.
MSPA_HD bool proved_inside(double ax, double ay, double bx, double by, double cx, double cy, double px, double py) {
    const int o = orient_certain(ax, ay, bx, by, px, py);
    return o != 0 && orient_certain(bx, by, cx, cy, px, py) == o && orient_certain(cx, cy, ax, ay, px, py) == o;
}

// ---- the hull -------------------------------------------------------------------------------------------------------------------

// One chain of Andrew's scan over the slots [a, b) of pts [*, 2], sorted by (x, y) with equal points in ascending row order: the
// lower chain walks ascending, the upper chain descending.  stack [*] takes the chain's slots at [a, a + count); the count is
// returned.  Of equal points the slot of the lowest row stays (ascending: the first met; descending: the last met replaces the
// top).  More than cap pops set capped and end the walk.
MSPA_HD int64_t chain(const double *__restrict__ pts, int64_t a, int64_t b, bool upper, int32_t *__restrict__ stack, int64_t cap, bool &capped) {
    int64_t k = 0, pops = 0;
    double sx = 0.0, sy = 0.0, tx = 0.0, ty = 0.0;               // the second (k >= 2) and the top (k >= 1) of the stack, as coordinates
    for (int64_t n = 0; n < b - a; ++n) {
        const int64_t i = upper ? b - 1 - n : a + n;
        const double px = pts[2 * i], py = pts[2 * i + 1];
        if (k > 0 && tx == px && ty == py) {
            if (upper) stack[a + k - 1] = (int32_t)i;
            continue;
        }
        while (k >= 2) {
            if (orient(sx, sy, tx, ty, px, py) > 0) break;
            if (++pops > cap) {
                capped = true;
                return k;
            }
            --k;                                                 // the top goes: the second is the top, and the one below it is read back
            tx = sx;
            ty = sy;
            if (k >= 2) {
                const int64_t s = stack[a + k - 2];
                sx = pts[2 * s];
                sy = pts[2 * s + 1];
            }
        }
        stack[a + k++] = (int32_t)i;
        sx = tx;
        sy = ty;
        tx = px;
        ty = py;
    }
    return k;
}

// The vertices of a segment whose chains hold lower_count and upper_count slots (both 0 for an empty segment).
MSPA_HD int64_t hull_size(int64_t lower_count, int64_t upper_count) {
    return lower_count <= 0 ? 0 : lower_count == 1 || upper_count <= 1 ? 1 : lower_count + upper_count - 2;
}

// The slot of hull vertex k (0 <= k < hull_size) of the segment whose chains start at stack slot a.
MSPA_HD int64_t hull_slot(const int32_t *__restrict__ lower, const int32_t *__restrict__ upper, int64_t a, int64_t lower_count, int64_t k) {
    const int64_t in_lower = lower_count > 1 ? lower_count - 1 : 1;
    return k < in_lower ? lower[a + k] : upper[a + (k - in_lower)];
}

// ---- the rectangle --------------------------------------------------------------------------------------------------------------

struct Spans {
    double t_min, t_max, c_min, c_max;
};

MSPA_HD Spans no_spans() { return Spans{INFINITY, -INFINITY, INFINITY, -INFINITY}; }

MSPA_HD double length_sq(double dx, double dy) {
    const double xx = dx * dx, yy = dy * dy;
    return xx + yy;
}

MSPA_HD void project(double ax, double ay, double dx, double dy, double vx, double vy, Spans &sp) {
    const double qx = vx - ax, qy = vy - ay;
    const double xx = qx * dx, yy = qy * dy, yx = qy * dx, xy = qx * dy;
    const double t = xx + yy, c = yx - xy;
    sp.t_min = t < sp.t_min ? t : sp.t_min;
    sp.t_max = t > sp.t_max ? t : sp.t_max;
    sp.c_min = c < sp.c_min ? c : sp.c_min;
    sp.c_max = c > sp.c_max ? c : sp.c_max;
}

MSPA_HD double edge_measure(const Spans &sp, double dd) {
    const double along = sp.t_max - sp.t_min, across = sp.c_max - sp.c_min;
    const double area = along * across;
    return area / dd;
}

MSPA_HD bool better_edge(double m_a, int64_t k_a, double m_b, int64_t k_b) {                     // true: b beats a
    return k_b >= 0 && (k_a < 0 || m_b < m_a || (m_b == m_a && k_b < k_a));
}

MSPA_HD void box_of(double ax, double ay, double dx, double dy, const Spans &sp, double z_lo, double z_hi, double *__restrict__ box) {
    const double dd = length_sq(dx, dy), L = sqrt(dd);
    const double along = sp.t_max - sp.t_min, across = sp.c_max - sp.c_min;
    double length = along / L, width = across / L;
    const double t_sum = sp.t_max + sp.t_min, c_sum = sp.c_max + sp.c_min;
    const double tm = t_sum / 2.0, cm = c_sum / 2.0;
    const double tx = tm * dx, cy_ = cm * dy, ty = tm * dy, cx_ = cm * dx;
    const double px = tx - cy_, py = ty + cx_;
    const double ox = px / dd, oy = py / dd;
    double ux = dx / L, uy = dy / L;
    if (width > length) {
        const double w = width, x = ux;
        width = length;
        length = w;
        ux = -uy;
        uy = x;
    }
    if (ux < 0.0 || (ux == 0.0 && uy < 0.0)) {
        ux = -ux;
        uy = -uy;
    }
    if (ux == 0.0) ux = 0.0;                                     // one zero, the positive one
    if (uy == 0.0) uy = 0.0;
    const double z_sum = z_hi + z_lo;
    box[0] = ax + ox;
    box[1] = ay + oy;
    box[2] = z_sum / 2.0;
    box[3] = length;
    box[4] = width;
    box[5] = z_hi - z_lo;
    box[6] = ux;
    box[7] = uy;
}

MSPA_HD void point_box(double x, double y, double z_lo, double z_hi, double *__restrict__ box) {
    const double z_sum = z_hi + z_lo;
    box[0] = x;
    box[1] = y;
    box[2] = z_sum / 2.0;
    box[3] = 0.0;
    box[4] = 0.0;
    box[5] = z_hi - z_lo;
    box[6] = 1.0;
    box[7] = 0.0;
}

MSPA_HD void no_box(double *__restrict__ box) {
    for (int e = 0; e < kBoxValues; ++e) box[e] = segs::no_value();
}

// ---- the host twin ------------------------------------------------------------------------------------------------------------

// The whole op on the CPU: per segment the refusals, the z extent, one stable sort by (x, y), the two chains, the hull and the
// all-edges rectangle.  hull_index takes the hull rows of all segments back to back (room for N), hull_offsets [S + 1] their
// offsets, edges [S] int32 the chosen edge (-1 for an empty segment), boxes [S, 8].  Returns the flag word: non-zero means a
// refusal.  pop_cap < 0 means the rule's cap; a lower cap is for the test of the cap itself.
inline int32_t upright_all(const double *rows, int64_t C, const int64_t *offsets, int64_t S, int64_t *hull_index, int64_t *hull_offsets,
                           int32_t *edges, double *boxes, int64_t pop_cap = -1) {
    int32_t flags = 0;
    std::vector<int64_t> order;
    std::vector<double> pts, hull;
    std::vector<int32_t> lower, upper;
    hull_offsets[0] = 0;
    for (int64_t s = 0; s < S; ++s) {
        const int64_t a = offsets[s], n = offsets[s + 1] - a;
        double z_lo = INFINITY, z_hi = -INFINITY;
        int32_t refused = 0;
        for (int64_t i = a; i < a + n; ++i) {
            const double z = rows[i * C + 2];
            refused |= refusal_of(rows[i * C], rows[i * C + 1], z);
            z_lo = z < z_lo ? z : z_lo;
            z_hi = z > z_hi ? z : z_hi;
        }
        flags |= refused;
        hull_offsets[s + 1] = hull_offsets[s];
        edges[s] = -1;
        no_box(boxes + s * kBoxValues);
        if (n == 0 || refused) continue;
        order.resize((size_t)n);
        std::iota(order.begin(), order.end(), a);
        std::stable_sort(order.begin(), order.end(), [&](int64_t p, int64_t q) {
            return rows[p * C] < rows[q * C] || (rows[p * C] == rows[q * C] && rows[p * C + 1] < rows[q * C + 1]);
        });
        pts.resize((size_t)n * 2);
        for (int64_t i = 0; i < n; ++i) {
            pts[(size_t)(2 * i)] = rows[order[(size_t)i] * C];
            pts[(size_t)(2 * i + 1)] = rows[order[(size_t)i] * C + 1];
        }
        lower.assign((size_t)n, 0);
        upper.assign((size_t)n, 0);
        bool capped = false;
        const int64_t cap = pop_cap < 0 ? n : pop_cap;
        const int64_t lc = chain(pts.data(), 0, n, false, lower.data(), cap, capped);
        const int64_t uc = chain(pts.data(), 0, n, true, upper.data(), cap, capped);
        if (capped) {
            flags |= kCapReached;
            continue;
        }
        const int64_t h = hull_size(lc, uc);
        hull.resize((size_t)h * 2);
        int64_t *out = hull_index + hull_offsets[s];
        for (int64_t k = 0; k < h; ++k) {
            const int64_t slot = hull_slot(lower.data(), upper.data(), 0, lc, k);
            out[k] = order[(size_t)slot];
            hull[(size_t)(2 * k)] = pts[(size_t)(2 * slot)];
            hull[(size_t)(2 * k + 1)] = pts[(size_t)(2 * slot + 1)];
        }
        hull_offsets[s + 1] = hull_offsets[s] + h;
        edges[s] = 0;
        if (h == 1) {
            point_box(hull[0], hull[1], z_lo, z_hi, boxes + s * kBoxValues);
            continue;
        }
        double best = 0.0;
        int64_t best_k = -1;
        Spans best_spans = no_spans();
        for (int64_t k = 0; k < h; ++k) {
            const int64_t k1 = k + 1 < h ? k + 1 : 0;
            const double ax = hull[(size_t)(2 * k)], ay = hull[(size_t)(2 * k + 1)];
            const double dx = hull[(size_t)(2 * k1)] - ax, dy = hull[(size_t)(2 * k1 + 1)] - ay;
            Spans sp = no_spans();
            for (int64_t j = 0; j < h; ++j) project(ax, ay, dx, dy, hull[(size_t)(2 * j)], hull[(size_t)(2 * j + 1)], sp);
            const double m = edge_measure(sp, length_sq(dx, dy));
            if (better_edge(best, best_k, m, k)) {
                best = m;
                best_k = k;
                best_spans = sp;
            }
        }
        const int64_t k1 = best_k + 1 < h ? best_k + 1 : 0;
        const double ax = hull[(size_t)(2 * best_k)], ay = hull[(size_t)(2 * best_k + 1)];
        edges[s] = (int32_t)best_k;
        box_of(ax, ay, hull[(size_t)(2 * k1)] - ax, hull[(size_t)(2 * k1 + 1)] - ay, best_spans, z_lo, z_hi, boxes + s * kBoxValues);
    }
    return flags;
}

}  // namespace upright
}  // namespace mspa
