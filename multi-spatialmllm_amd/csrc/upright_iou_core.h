// The intersection over union of two UPRIGHT boxes [cx, cy, cz, length, width, height, ux, uy] (upright_box_core.h's box), stated once
// for the kernel of upright_iou.hip and its host twin (mspa_upright_iou_host).  A plain C++ build of this header is the reference
// the device must agree with bit for bit.  One pair of boxes, 8 float64 each, gives one float64 IoU and, for
// who asks, the footprint intersection area and the z overlap.
//
// THE RULE, per pair (a, b).  Every floating-point step is one rounded float64 operation in the order written here (the library is
// built with -ffp-contract=off); there is no fused operation in the rule and no function beyond + - * /.
//   * values      every value is read as v + 0.0, so a negative zero enters as the positive one.
//   * a box       its footprint is the rectangle with corners c +- (length / 2) u +- (width / 2) n, n = (-uy, ux): upright_corners'
//                 definition, (ux, uy) as given, not re-normalised.  Its volume is (length * width) * height, iou_3d's order.
//   * refusals    a box is refused (refused) where a value is not finite, a size is negative, |s2 - 1| > 2^-20 for s2 = ux * ux +
//                 uy * uy (the axes upright_box_core.h emits have |s2 - 1| <= 4u; an axis of norm 1.01 has 2e-2), or a non-zero
//                 |cx|, |cy|, |cz|, length, width or height lies outside [2^-200, 2^200] (THE WINDOW below).  A pair with a refused
//                 box gives NaN in every output.  Nothing is raised and no flag is kept.
//   * identical   where the eight values of a equal those of b: area = length * width, dz = height, and the IoU is exactly 1.0 if
//                 the volume is positive, else NaN (the 0 / 0 of calculate_iou_3d).
//   * order       the WINDOW w is the box with the larger length * width (rounded); on a tie the box with the larger value at the
//                 first of the eight places where they differ (a_is_window).  The other box is the SUBJECT s.  Only the pair's own
//                 values decide, so iou(a, b) and iou(b, a) run the same operations on the same numbers.
//   * z           top = c.z + height / 2, bottom = c.z - height / 2 per box; dz = min(top_w, top_s) - max(bottom_w, bottom_s)
//                 (iou_3d's operations), then dz = min(dz, height_w, height_s): the real overlap never exceeds either height, but
//                 the rounded one can (a centre of 10^6 and a height of 10^-12), and without the clamp the IoU could exceed 1.
//   * corners     d = (s.cx - w.cx, s.cy - w.cy) first, so that a scene far from the origin pays one subtraction.  With hl =
//                 s.length / 2, hw = s.width / 2: e = (hl * s.ux, hl * s.uy), f = (-(hw * s.uy), hw * s.ux), m = d - e, p = d + e,
//                 and the corners q0 = m - f, q1 = p - f, q2 = p + f, q3 = m + f (counter-clockwise, upright_corners' order).
//   * frame       each corner into the window's frame: x = q.x * w.ux + q.y * w.uy, y = q.y * w.ux - q.x * w.uy.  This map scales
//                 lengths by |u_w| and areas by |u_w|^2, and the window is |x| <= hx, |y| <= hy there with s2 = w.ux * w.ux +
//                 w.uy * w.uy, hx = (w.length / 2) * s2, hy = (w.width / 2) * s2.  (Clipping against length / 2 itself would be
//                 wrong by the relative |s2 - 1|, up to 2^-20: far above the bound below.)
//   * clipping    Sutherland-Hodgman against the four sides in the order x <= hx, x >= -hx, y <= hy, y >= -hy (clip_side).  A
//                 vertex is inside where the comparison holds (closed).  Per stage, for i = 0 .. n - 1 with p = v_i, q = v_(i+1 mod n):
//                 p is kept if inside; then, if exactly one of p, q is inside, the crossing vertex follows: its clipped coordinate
//                 is the bound itself, and the other one is p.o + t * (q.o - p.o), t = (bound - p.c) / (q.c - p.c) (c the
//                 clipped coordinate, o the other one; p is the start of the edge as walked, whichever end is inside; 0 <= t <= 1
//                 because rounding is monotone).  A convex polygon gains at most one vertex per stage: 4 -> at most 8.  A ninth
//                 vertex is dropped (a guard for the storage; it takes three nearly collinear vertices that rounding has bent
//                 across a side, which no input is known to produce).
//   * area        0 for fewer than three vertices; else with g_i = v_i - v_0 the sum over i = 1 .. n - 2, in this order from 0.0,
//                 of (g_i.x * g_(i+1).y) - (g_i.y * g_(i+1).x); area = (sum / 2) / s2; then max(area, 0), then min with
//                 min(a.length * a.width, b.length * b.width).
//   * IoU         inter = dz > 0 ? area * dz : 0; IoU = inter / ((v_w + v_s) - inter).  0 / 0 (both volumes zero) is NaN, as in
//                 calculate_iou_3d.  Otherwise 0 <= IoU <= 1: area <= either length * width and dz <= either height, so by the
//                 monotonicity of rounding inter <= v_w and inter <= v_s, v_w + v_s >= 2 inter and the divisor is >= inter.
//   The second output is (area, dz): the clamped area, and the dz after its clamp (zero or negative where the boxes do not overlap
//   in z).
//
// THE WINDOW [2^-200, 2^200] on the non-zero centres and sizes (|ux|, |uy| <= 1 + 2^-21 by the axis test).  A corner coordinate is at
// most 2^203, a product of two at most 2^406, the sum times dz at most 2^612, a volume at most 2^600: nothing overflows.  A product of
// two sizes is zero or at least 2^-400, a volume zero or at least 2^-600: normal.  What can underflow is a product with a tiny
// ux or uy, or a difference of rotated coordinates that cancel; the model used below is fl(x op y) = (x op y)(1 + e) + h, |e| <= u =
// 2^-53, |h| <= 2^-1075 (h = 0 for + and -).  The scale R below is zero (then every corner is the origin and the area is exactly
// 0) or at least 2^-200; the h terms, each times a factor of at most 2^204, stay below 2^-800 and vanish in u R^2 >= 2^-453.
//
// THE FORWARD ERROR BOUND, against the exact rational value for the same sixteen doubles (area_bound, iou_bound; pair_bounds).
//   Scale: R = |d.x| + |d.y| + w.length + w.width + s.length + s.width.  dev_k = |s2_k - 1| + 4u for box k (s2 as computed: its own
//   error is 2u).
//   (1) The corners.  d carries u |d| per coordinate (one subtraction of the inputs: relative to the DIFFERENCE, not to |c|; the
//       u |c| of the issue text is an upper estimate of it).  e and f carry one rounding, the two sums two more: each coordinate
//       of a corner is within 4u (|d| + hl + hw) <= 4u R of its exact value.  The rotation multiplies by |w.ux| + |w.uy| <= 1.5
//       and adds two products and a sum of magnitudes <= 1.5 R: within 6u R + 3u (1.5 R) <= 11u R per coordinate, 16u R in the plane.
//   (2) The window.  hx and hy carry s2's 2u and one product: within 3u R.
//   (3) Clipping.  A stage computes the exact clip of its input polygon with each crossing vertex moved ALONG the side by the
//       error of one interpolation: t within 3u, the product and the sum: at most 6u times the edge's extent <= 6u (2R).  Over
//       four stages a vertex moves by at most 16u R + 4 * 12u R = 64u R, and the sides by 3u R.  The area of a polygon cut by a
//       half-plane is the integral of its winding number there, so moving vertices changes it by at most the area they sweep:
//       displacement times perimeter.  The perimeter is at most the subject's in the frame (a convex part of it), <= 2 R (1 + 2^-20); the
//       window's sides sweep at most 3u R times the same.  Together (64 + 3) u R * 2R * 1.01 <= 136 u R^2.
//   (4) The shoelace.  Each g carries u, each term three roundings of products bounded by the squared diameter <= R^2: 4u R^2 per
//       term, six terms, and six additions of a sum <= 2 R^2: (24 + 12) / 2 = 18u R^2; the division by s2 (exact s2 within 2u) 3u R^2.
//   (5) In the frame everything is the true geometry scaled by |u_w|^2, which the division by s2 takes out, up to (4).  The clamp at
//       min(length * width) is below the true area of the smaller footprint, length width |u|^2, by at most dev of that box.
//   area_bound = 512 u R^2 + (dev_a + dev_b) min(a.length * a.width, b.length * b.width): 136 + 21 = 157, stated with room.
//   For the IoU, with z_err = 4u (|a.cz| + |b.cz| + a.height + b.height) (two sums, one difference), dzp = max(dz, 0):
//       inter_err = area_bound (dzp + z_err) + 2 min_area z_err + 2u inter
//       vol_err   = (dev_a + 4u) v_a + (dev_b + 4u) v_b          (the exact volume is length width (ux^2 + uy^2) height)
//   and for x / y with y >= x: |x^ / y^ - x / y| <= (|dx| + |dy|) / y.  The divisor's error is inter_err + vol_err:
//       iou_bound = 2 (2 inter_err + vol_err) / divisor + 8u
//   with the computed divisor; the factor 2 covers the divisor's own error while that is below half of it, and above that the bound
//   exceeds 1, the distance of any two IoUs.  A refused pair has both bounds NaN and a divisor of 0 an IoU bound of NaN; an identical
//   pair has the area bound (dev_a + dev_b) length * width (the rule reports length * width itself) and the IoU bound 0.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#ifndef MSPA_HD
#ifdef __HIPCC__
#define MSPA_HD __host__ __device__ __forceinline__
#else
#define MSPA_HD inline
#endif
#endif

namespace mspa {
namespace uiou {

constexpr double kU = 0x1p-53;
constexpr double kAxisTol = 0x1p-20;
constexpr double kWindowLo = 0x1p-200, kWindowHi = 0x1p200;
constexpr double kAreaBound = 512.0 * kU;                        // area_bound over R^2
constexpr int kBoxValues = 8;
constexpr int kMaxVertices = 8;
enum : int32_t { kPairs = 0, kMatrix = 1 };                      // the two launch shapes
constexpr int64_t kMaxOutputs = (int64_t)1 << 31;

MSPA_HD double no_value() { return __builtin_nan(""); }

MSPA_HD bool in_window(double v) { return v == 0.0 || (fabs(v) >= kWindowLo && fabs(v) <= kWindowHi); }

MSPA_HD double axis_sq(double ux, double uy) {
    const double xx = ux * ux, yy = uy * uy;
    return xx + yy;
}

MSPA_HD void load_box(const double *__restrict__ src, double box[kBoxValues]) {
    for (int e = 0; e < kBoxValues; ++e) box[e] = src[e] + 0.0;
}

MSPA_HD bool refused(const double box[kBoxValues]) {
    bool bad = false;
    for (int e = 0; e < kBoxValues; ++e) bad = bad || !(fabs(box[e]) < INFINITY);
    for (int e = 0; e < 6; ++e) bad = bad || !in_window(box[e]);
    for (int e = 3; e < 6; ++e) bad = bad || box[e] < 0.0;
    const double dev = axis_sq(box[6], box[7]) - 1.0;
    return bad || !(fabs(dev) <= kAxisTol);
}

MSPA_HD bool identical(const double a[kBoxValues], const double b[kBoxValues]) {
    bool same = true;
    for (int e = 0; e < kBoxValues; ++e) same = same && a[e] == b[e];
    return same;
}

// Whether a is the clip window of the pair (a, b); for identical boxes either answer is the same pair.
MSPA_HD bool a_is_window(const double a[kBoxValues], const double b[kBoxValues]) {
    const double fa = a[3] * a[4], fb = b[3] * b[4];
    if (fa != fb) return fa > fb;
    bool decided = false, first = true;
    for (int e = 0; e < kBoxValues; ++e) {
        if (!decided && a[e] != b[e]) {
            decided = true;
            first = a[e] > b[e];
        }
    }
    return first;
}

// One stage of the clipping: the polygon of n vertices whose clipped coordinate is in_c and whose other coordinate is in_o (vertex
// i at [i * stride]) against c <= bound (upper) or c >= bound (not upper) -> out_c / out_o, the new count returned.
MSPA_HD int clip_side(const double *in_c, const double *in_o, int n, double bound, bool upper, double *out_c, double *out_o, int stride) {
    int m = 0;
    for (int i = 0; i < n; ++i) {
        const int j = i + 1 < n ? i + 1 : 0;
        const double pc = in_c[i * stride], po = in_o[i * stride], qc = in_c[j * stride], qo = in_o[j * stride];
        const bool p_in = upper ? pc <= bound : pc >= bound, q_in = upper ? qc <= bound : qc >= bound;
        if (p_in && m < kMaxVertices) {
            out_c[m * stride] = pc;
            out_o[m * stride] = po;
            ++m;
        }
        if (p_in != q_in && m < kMaxVertices) {
            const double num = bound - pc, den = qc - pc;
            const double t = num / den;
            const double span = qo - po;
            const double step = t * span;
            out_c[m * stride] = bound;
            out_o[m * stride] = po + step;
            ++m;
        }
    }
    return m;
}

struct Result {                                                  // what one pair gives; every member NaN for a refused pair
    double iou, area, dz, inter, divisor, v_a, v_b;
};

// The rule.  x0, y0, x1, y1: room for kMaxVertices doubles each at the given stride (two polygons, used in turn).
MSPA_HD Result pair_iou(const double *__restrict__ a_src, const double *__restrict__ b_src, double *x0, double *y0, double *x1, double *y1, int stride) {
    double a[kBoxValues], b[kBoxValues];
    load_box(a_src, a);
    load_box(b_src, b);
    Result r;
    r.iou = r.area = r.dz = r.inter = r.divisor = r.v_a = r.v_b = no_value();
    if (refused(a) || refused(b)) return r;
    const double fa = a[3] * a[4], fb = b[3] * b[4];
    r.v_a = fa * a[5];
    r.v_b = fb * b[5];
    if (identical(a, b)) {
        r.area = fa;
        r.dz = a[5];
        r.inter = r.v_a;
        r.divisor = r.v_a;
        r.iou = r.v_a > 0.0 ? 1.0 : no_value();
        return r;
    }
    const bool first = a_is_window(a, b);
    double w[kBoxValues], s[kBoxValues];
    for (int e = 0; e < kBoxValues; ++e) {
        w[e] = first ? a[e] : b[e];
        s[e] = first ? b[e] : a[e];
    }
    // z
    const double half_w = w[5] / 2.0, half_s = s[5] / 2.0;
    const double top_w = w[2] + half_w, top_s = s[2] + half_s, bottom_w = w[2] - half_w, bottom_s = s[2] - half_s;
    const double top = top_w < top_s ? top_w : top_s, bottom = bottom_w > bottom_s ? bottom_w : bottom_s;
    double dz = top - bottom;
    dz = dz < w[5] ? dz : w[5];
    dz = dz < s[5] ? dz : s[5];
    // the subject's corners about the window's centre, in the window's frame
    const double dx = s[0] - w[0], dy = s[1] - w[1];
    const double hl = s[3] / 2.0, hw = s[4] / 2.0;
    const double ex = hl * s[6], ey = hl * s[7];
    const double wy = hw * s[7];
    const double fx = -wy, fy = hw * s[6];
    const double mx = dx - ex, my = dy - ey, px = dx + ex, py = dy + ey;
    const double qx[4] = {mx - fx, px - fx, px + fx, mx + fx}, qy[4] = {my - fy, py - fy, py + fy, my + fy};
    for (int k = 0; k < 4; ++k) {
        const double xx = qx[k] * w[6], yy = qy[k] * w[7], yx = qy[k] * w[6], xy = qx[k] * w[7];
        x0[k * stride] = xx + yy;
        y0[k * stride] = yx - xy;
    }
    const double s2 = axis_sq(w[6], w[7]);
    const double half_l = w[3] / 2.0, half_b = w[4] / 2.0;
    const double hx = half_l * s2, hy = half_b * s2;
    int n = clip_side(x0, y0, 4, hx, true, x1, y1, stride);
    n = clip_side(x1, y1, n, -hx, false, x0, y0, stride);
    n = clip_side(y0, x0, n, hy, true, y1, x1, stride);
    n = clip_side(y1, x1, n, -hy, false, y0, x0, stride);
    double sum = 0.0;
    if (n >= 3) {
        const double ox = x0[0], oy = y0[0];
        double gx = x0[stride] - ox, gy = y0[stride] - oy;
        for (int i = 2; i < n; ++i) {
            const double nx = x0[i * stride] - ox, ny = y0[i * stride] - oy;
            const double l = gx * ny, m = gy * nx;
            const double term = l - m;
            sum = sum + term;
            gx = nx;
            gy = ny;
        }
    }
    const double half = sum / 2.0;
    double area = half / s2;
    area = area > 0.0 ? area : 0.0;
    const double least = fa < fb ? fa : fb;
    area = area < least ? area : least;
    const double v_w = first ? r.v_a : r.v_b, v_s = first ? r.v_b : r.v_a;
    const double volume = area * dz;
    const double inter = dz > 0.0 ? volume : 0.0;
    const double both = v_w + v_s;
    r.area = area;
    r.dz = dz;
    r.inter = inter;
    r.divisor = both - inter;
    r.iou = inter / r.divisor;
    return r;
}

// The element of a and of b that output i reads.  Pairs are G = P matrices of 1 x 1; a_one / b_one: that side is a single box.
MSPA_HD void operands_of(int64_t i, int64_t A, int64_t B, bool a_one, bool b_one, int64_t &ia, int64_t &ib) {
    const int64_t cells = A * B;
    const int64_t g = i / cells, cell = i - g * cells;
    const int64_t row = cell / B;
    ia = a_one ? 0 : g * A + row;
    ib = b_one ? 0 : g * B + (cell - row * B);
}

// The launch shape of a call: outputs >= 0 and what operands_of takes, or outputs < 0 for counts that do not fit the mode.
struct Shape {
    int64_t outputs, A, B;
    bool a_one, b_one;
};

inline Shape shape_of(int64_t Pa, int64_t Pb, int64_t G, int64_t A, int64_t B, int32_t mode) {
    Shape sh{-1, 1, 1, false, false};
    if (Pa < 0 || Pb < 0 || G < 0 || A < 0 || B < 0) return sh;
    if (mode == kPairs) {
        if (G != 0 || A != 0 || B != 0) return sh;
        if (Pa != Pb && Pa != 1 && Pb != 1) return sh;
        sh.outputs = Pa == 1 ? Pb : Pb == 1 ? Pa : Pa;
        sh.a_one = Pa == 1 && Pb != 1;
        sh.b_one = Pb == 1 && Pa != 1;
        return sh.outputs > kMaxOutputs ? Shape{-1, 1, 1, false, false} : sh;
    }
    if (mode != kMatrix) return sh;
    if (G > kMaxOutputs || A > kMaxOutputs || B > kMaxOutputs) return sh;
    const __int128 rows_a = (__int128)G * A, rows_b = (__int128)G * B, cells = rows_a * B;
    if (rows_a != Pa || rows_b != Pb || cells > kMaxOutputs) return sh;
    sh.outputs = (int64_t)cells;
    sh.A = A;
    sh.B = B;
    return sh;
}

// ---- the host twin ------------------------------------------------------------------------------------------------------------

inline void iou_all(const double *a, const double *b, const Shape &sh, double *out, double *parts) {
    double x0[kMaxVertices], y0[kMaxVertices], x1[kMaxVertices], y1[kMaxVertices];
    for (int64_t i = 0; i < sh.outputs; ++i) {
        int64_t ia, ib;
        operands_of(i, sh.A, sh.B, sh.a_one, sh.b_one, ia, ib);
        const Result r = pair_iou(a + ia * kBoxValues, b + ib * kBoxValues, x0, y0, x1, y1, 1);
        out[i] = r.iou;
        if (parts) {
            parts[2 * i] = r.area;
            parts[2 * i + 1] = r.dz;
        }
    }
}

// The two bounds of one pair (the derivation is at the top of this file).
inline void pair_bounds(const double *a_src, const double *b_src, double &area_bound, double &iou_bound) {
    double x0[kMaxVertices], y0[kMaxVertices], x1[kMaxVertices], y1[kMaxVertices], a[kBoxValues], b[kBoxValues];
    const Result r = pair_iou(a_src, b_src, x0, y0, x1, y1, 1);
    load_box(a_src, a);
    load_box(b_src, b);
    area_bound = iou_bound = no_value();
    if (refused(a) || refused(b)) return;
    const double dev_a = fabs(axis_sq(a[6], a[7]) - 1.0) + 4.0 * kU, dev_b = fabs(axis_sq(b[6], b[7]) - 1.0) + 4.0 * kU;
    const double fa = a[3] * a[4], fb = b[3] * b[4], least = fa < fb ? fa : fb;
    if (identical(a, b)) {                                       // length * width against length width |u|^2; the IoU is exact
        area_bound = (dev_a + dev_b) * least;
        iou_bound = r.v_a > 0.0 ? 0.0 : no_value();
        return;
    }
    const double R = fabs(b[0] - a[0]) + fabs(b[1] - a[1]) + a[3] + a[4] + b[3] + b[4];
    area_bound = kAreaBound * R * R + (dev_a + dev_b) * least;
    if (!(r.divisor > 0.0)) return;
    const double z_err = 4.0 * kU * (fabs(a[2]) + fabs(b[2]) + a[5] + b[5]);
    const double dzp = r.dz > 0.0 ? r.dz : 0.0;
    const double inter_err = area_bound * (dzp + z_err) + 2.0 * least * z_err + 2.0 * kU * r.inter;
    const double vol_err = (dev_a + 4.0 * kU) * r.v_a + (dev_b + 4.0 * kU) * r.v_b;
    iou_bound = 2.0 * (2.0 * inter_err + vol_err) / r.divisor + 8.0 * kU;
}

}  // namespace uiou
}  // namespace mspa
