// Image resampling: the arithmetic shared by the device kernels of resize.hip and the host table builder.  Everything that
// decides an output value is an MSPA_HD function here, so that a plain C++ build of this header can be checked against Pillow
// on a CPU.  The arithmetic restates Pillow's `Image.resize((W, H), resample)` of an 8-bit RGB image for the BILINEAR and
// BICUBIC filters (no box, no reducing_gap):
//   * per axis, scale = in / out, filterscale = max(scale, 1), support = filter support (1 / 2) * filterscale,
//     ksize = 2 * ceil(support) + 1;
//   * per output index xx, center = (xx + 0.5) * scale, the taps [xmin, xmin + xmax) = [(int)(center - support + 0.5),
//     (int)(center + support + 0.5)) clipped to the axis, weights filter((x + xmin - center + 0.5) * (1 / filterscale)) summed
//     in index order and divided by that sum when it is not zero -- all in float64, one rounding per written operation (build
//     the host side with -ffp-contract=off);
//   * the weights in fixed point with 22 fractional bits, rounded half away from zero;
//   * a value is clamp((2^21 + sum(value * k)) >> 22, 0, 255) in a 32-bit accumulator; the horizontal pass runs first, over the
//     source rows the vertical pass reads only, and is rounded to 8 bits before the vertical pass; a pass whose size does not
//     change is skipped.
//
// The accumulator.  Pillow's own accumulator is a C `int`, so 32 bits are the definition, not an economy.  It cannot wrap for
// the tables built here: |2^21 + sum(v * k)| <= 2^21 + 255 * sum|k|, and coeffs() refuses (returns -1) a table with a row whose
// sum|k| exceeds kMaxAbsSum = (2^31 - 1 - 2^21) / 255.  For bilinear every weight is >= 0 and a row sums to 2^22 up to one unit
// per tap.  For bicubic (Keys, a = -0.5) the negative lobes hold 1/12 of the kernel's mass, an interior row has
// sum|k| <= 1.25 * 2^22 (the four taps at phase 1/2), and a row cut by the border is renormalised by a sum of at least the
// central lobe's share.  The largest row over every in <= 96 and every out with 1/8 <= out / in <= 8 has sum|k| = 1.269 * 2^22
// (tests/test_resize_cpu.py::test_accumulator_bound walks that range), against the 2.007 * 2^22 that fits.
#pragma once
#include <stdint.h>
#include <stddef.h>

#ifndef MSPA_HD
#ifdef __HIPCC__
#define MSPA_HD __host__ __device__ __forceinline__
#else
#define MSPA_HD inline
#endif
#endif
#ifndef MSPA_UNROLL
#ifdef __HIPCC__
#define MSPA_UNROLL _Pragma("unroll")
#else
#define MSPA_UNROLL
#endif
#endif

namespace mspa {
namespace resize {

enum : int32_t { kBilinear = 2, kBicubic = 3 };       // Pillow's Image.Resampling numbers

constexpr int kPrecisionBits = 22;                    // 32 - 8 - 2, Pillow's PRECISION_BITS
constexpr int32_t kHalf = 1 << (kPrecisionBits - 1);
constexpr int64_t kMaxAbsSum = (2147483647ll - kHalf) / 255;
constexpr int kMaxFactor = 8;                         // per-axis enlargement / reduction the device path takes

MSPA_HD bool valid_filter(int32_t f) { return f == kBilinear || f == kBicubic; }

MSPA_HD double filter_support(int32_t f) { return f == kBicubic ? 2.0 : 1.0; }

MSPA_HD double filter_weight(int32_t f, double x) {
    if (x < 0.0) x = -x;
    if (f == kBicubic) {
        const double a = -0.5;
        if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
        if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
        return 0.0;
    }
    return x < 1.0 ? 1.0 - x : 0.0;
}

// One axis of `in` samples resampled to `out`.
struct Axis {
    double scale, filterscale, support;
    int32_t in, out, filter, ksize;
};

MSPA_HD Axis axis(int32_t in, int32_t out, int32_t filter) {
    Axis a;
    a.in = in;
    a.out = out;
    a.filter = filter;
    a.scale = a.filterscale = (double)in / (double)out;
    if (a.filterscale < 1.0) a.filterscale = 1.0;
    a.support = filter_support(filter) * a.filterscale;
    int32_t c = (int32_t)a.support;                    // ceil of a positive value
    if ((double)c < a.support) ++c;
    a.ksize = c * 2 + 1;
    return a;
}

// The device path's range: both factors within 1/8 .. 8 (sizes up to 65535, so the products stay inside int32).
MSPA_HD bool in_range(int32_t in, int32_t out) {
    return in >= 1 && out >= 1 && in <= 65535 && out <= 65535 && in <= kMaxFactor * out && out <= kMaxFactor * in;
}

// Taps of output index xx: [xmin, xmin + xmax) inside [0, in).
MSPA_HD void taps(const Axis &a, int32_t xx, int32_t &xmin, int32_t &xmax) {
    const double center = (xx + 0.5) * a.scale;
    xmin = (int32_t)(center - a.support + 0.5);
    if (xmin < 0) xmin = 0;
    xmax = (int32_t)(center + a.support + 0.5);
    if (xmax > a.in) xmax = a.in;
    xmax -= xmin;
}

// Row xx of the fixed-point table: k[0 .. ksize), zero past xmax.  `w` is ksize doubles of scratch.  Returns sum|k|.
MSPA_HD int64_t coeff_row(const Axis &a, int32_t xx, int32_t &xmin, int32_t &xmax, double *w, int32_t *k) {
    taps(a, xx, xmin, xmax);
    const double center = (xx + 0.5) * a.scale;
    const double ss = 1.0 / a.filterscale;
    double ww = 0.0;
    for (int32_t x = 0; x < xmax; ++x) {
        w[x] = filter_weight(a.filter, (x + xmin - center + 0.5) * ss);
        ww += w[x];
    }
    int64_t sum = 0;
    for (int32_t x = 0; x < a.ksize; ++x) {
        double v = 0.0;
        if (x < xmax) v = ww != 0.0 ? w[x] / ww : w[x];
        k[x] = v < 0 ? (int32_t)(-0.5 + v * (double)(1 << kPrecisionBits)) : (int32_t)(0.5 + v * (double)(1 << kPrecisionBits));
        sum += k[x] < 0 ? -(int64_t)k[x] : (int64_t)k[x];
    }
    return sum;
}

// The whole table of one axis: bounds [2 * out] = (xmin, xmax) pairs, coeffs [out * ksize] (may be null: bounds only).
// `w` is ksize doubles, `krow` ksize int32 of scratch.  Returns the largest sum|k| of a row, or -1 when one exceeds kMaxAbsSum.
MSPA_HD int64_t coeffs(const Axis &a, int32_t *bounds, int32_t *coef, double *w, int32_t *krow) {
    int64_t worst = 0;
    for (int32_t xx = 0; xx < a.out; ++xx) {
        int32_t xmin, xmax;
        const int64_t s = coeff_row(a, xx, xmin, xmax, w, coef ? coef + (int64_t)xx * a.ksize : krow);
        if (s > worst) worst = s;
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
    return worst > kMaxAbsSum ? -1 : worst;
}

MSPA_HD uint8_t clip8(int32_t acc) {
    const int32_t v = acc >> kPrecisionBits;
    return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// Source rows the vertical pass reads: [first, first + rows).
MSPA_HD void rows_read(const Axis &ay, int32_t &first, int32_t &rows) {
    int32_t lo, n, hi, m;
    taps(ay, 0, lo, n);
    taps(ay, ay.out - 1, hi, m);
    first = lo;
    rows = hi + m - lo;
}

// Source samples a run of `count` consecutive outputs can touch at most (the LDS window of a tile), never more than `in`.
MSPA_HD int32_t window_cap(const Axis &a, int32_t count) {
    const double span = (count - 1) * a.scale + 2.0 * a.support + 1.0;
    const int32_t cap = (int32_t)span + 1;
    return cap < a.in ? cap : a.in;
}

}  // namespace resize
}  // namespace mspa

#ifndef __HIPCC__
#include <vector>
namespace mspa {
namespace resize {

// The whole resize on the host (tests): src [h, w, 3] -> dst [H, W, 3], both contiguous.  `vertical_first` runs the passes in
// the other order (a diagnostic; Pillow's order is horizontal first).  Returns false for a table coeffs() refuses.
inline bool resize_host(const uint8_t *src, int32_t h, int32_t w, uint8_t *dst, int32_t H, int32_t W, int32_t filter,
                        bool vertical_first = false) {
    const Axis ax = axis(w, W, filter), ay = axis(h, H, filter);
    std::vector<int32_t> bx(2 * (size_t)W), by(2 * (size_t)H), kx((size_t)W * ax.ksize), ky((size_t)H * ay.ksize);
    std::vector<double> scratch((size_t)(ax.ksize > ay.ksize ? ax.ksize : ay.ksize));
    if (coeffs(ax, bx.data(), kx.data(), scratch.data(), nullptr) < 0 || coeffs(ay, by.data(), ky.data(), scratch.data(), nullptr) < 0)
        return false;
    auto horizontal = [&](const uint8_t *s, int32_t rows, uint8_t *d) {          // [rows, w, 3] -> [rows, W, 3]
        for (int32_t y = 0; y < rows; ++y)
            for (int32_t x = 0; x < W; ++x)
                for (int c = 0; c < 3; ++c) {
                    int32_t acc = kHalf;
                    for (int32_t j = 0; j < bx[2 * x + 1]; ++j)
                        acc += s[((size_t)y * w + bx[2 * x] + j) * 3 + c] * kx[(size_t)x * ax.ksize + j];
                    d[((size_t)y * W + x) * 3 + c] = clip8(acc);
                }
    };
    auto vertical = [&](const uint8_t *s, int32_t first, int32_t wd, uint8_t *d) {   // rows from `first` of [.., wd, 3] -> [H, wd, 3]
        for (int32_t y = 0; y < H; ++y)
            for (size_t b = 0; b < (size_t)wd * 3; ++b) {
                int32_t acc = kHalf;
                for (int32_t j = 0; j < by[2 * y + 1]; ++j)
                    acc += s[(size_t)(by[2 * y] - first + j) * wd * 3 + b] * ky[(size_t)y * ay.ksize + j];
                d[(size_t)y * wd * 3 + b] = clip8(acc);
            }
    };
    const bool need_h = w != W, need_v = h != H;
    if (!need_h && !need_v) {
        for (size_t i = 0; i < (size_t)h * w * 3; ++i) dst[i] = src[i];
    } else if (!need_v) {
        horizontal(src, h, dst);
    } else if (!need_h) {
        vertical(src, 0, w, dst);
    } else if (vertical_first) {
        std::vector<uint8_t> tmp((size_t)H * w * 3);
        vertical(src, 0, w, tmp.data());
        horizontal(tmp.data(), H, dst);
    } else {
        int32_t first, rows;
        rows_read(ay, first, rows);
        std::vector<uint8_t> tmp((size_t)rows * W * 3);
        horizontal(src + (size_t)first * w * 3, rows, tmp.data());
        vertical(tmp.data(), first, W, dst);
    }
    return true;
}

}  // namespace resize
}  // namespace mspa
#endif
