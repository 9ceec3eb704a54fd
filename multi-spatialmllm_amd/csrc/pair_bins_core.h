// The overlap-bin rule of the pair table's sampler (mspa/sampling.py: sample_dataframe), stated once for the device kernel of
// pair_table.hip and the host reference.  A plain C++ build of this header is the reference the device must equal.
//
//   edges = np.arange(overlap_min, overlap_max + interval, interval) as float64, ascending, n_edges >= 2.
//   * a row is in the ZERO part iff x == 0 (-0.0 counts: the frame's `overlap == 0` mask);
//   * otherwise code = #{e in edges : e < x} (pd.cut: edges.searchsorted(x, side="left")) and code = 1 where x == edges[0]
//     (include_lowest=True);
//   * the row belongs to bin code - 1 iff x is not NaN and 1 <= code <= n_edges - 1; otherwise it is DROPPED (dropna).
//   A class is one byte: the bin number (at most kMaxBins bins), kZero or kDropped.
#pragma once
#include <stdint.h>

#ifndef MSPA_HD
#ifdef __HIPCC__
#define MSPA_HD __host__ __device__ __forceinline__
#else
#define MSPA_HD inline
#endif
#endif

namespace mspa {
namespace pair_bins {

constexpr int32_t kMaxBins = 250;
constexpr int32_t kClasses = 256;        // entries of a count table: one per byte value
constexpr uint8_t kZero = 254;
constexpr uint8_t kDropped = 255;

// How many of edges[0, n) lie below x (x is not NaN; edges ascend).
MSPA_HD int32_t edges_below(const double *edges, int32_t n, double x) {
    int32_t lo = 0, hi = n;                                     // edges[lo - 1] < x <= edges[hi]
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (edges[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

MSPA_HD uint8_t classify(double x, const double *edges, int32_t n_edges) {
    if (x == 0.0) return kZero;
    if (x != x) return kDropped;
    int32_t code = edges_below(edges, n_edges, x);
    if (x == edges[0]) code = 1;
    return (code >= 1 && code <= n_edges - 1) ? (uint8_t)(code - 1) : kDropped;
}

// The reference of the whole pass: codes[i] and counts[c] (kClasses entries, zeroed here).
MSPA_HD void classify_all(const double *x, int64_t n, const double *edges, int32_t n_edges, uint8_t *codes, int64_t *counts) {
    for (int32_t c = 0; c < kClasses; ++c) counts[c] = 0;
    for (int64_t i = 0; i < n; ++i) {
        codes[i] = classify(x[i], edges, n_edges);
        ++counts[codes[i]];
    }
}

}  // namespace pair_bins
}  // namespace mspa
