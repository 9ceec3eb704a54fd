// VOXEL-GRID DOWN-SAMPLING of a ragged batch of clouds, stated once for the kernels of voxel_segments.hip and their host twin
// (mspa_voxel_segments_host).  A plain C++ build of this header is the reference the device must agree with bit for bit
// (DESIGN.md section 0.24).  The rule restates Open3D's voxel_down_sample from its documentation and source as the maintainers
// recall them; Open3D is not a dependency and the rule is NOT CHECKED AGAINST Open3D.
//
// The batch is cloud_segments_core.h's, with more columns.  rows [N, C >= 3] float64 (xyz first, then whatever the caller carries:
// colour, ...) plus offsets [S + 1] int64, ascending, offsets[0] = 0, offsets[S] = N <= 2^30, S <= 2^24: segment s is the rows
// offsets[s] .. offsets[s + 1]; empty segments are allowed anywhere and give no output rows.
//
// The rule, per segment of n >= 1 rows with finite xyz and voxel_size > 0, every step one float64 operation (the library is built
// with -ffp-contract=off, and nothing is rewritten as a multiplication by a reciprocal):
//   * grid origin   min_bound[a] = lo[a] - voxel_size * 0.5, lo the segment's own per-axis minimum             (min_bound)
//   * voxel index   idx[a] = (int64) floor((p[a] - min_bound[a]) / voxel_size): one subtraction, one IEEE division, one floor;
//                   >= 0 by construction (min_bound <= lo <= p and rounding is monotone)                        (axis_index)
//   * range         every idx[a] < 2^21 (Open3D refuses at INT_MAX per axis; this project at 2^21), so that
//                   key = idx[0] << 42 | idx[1] << 21 | idx[2] fits 63 bits and orders voxels lexicographically by (ix, iy, iz).
//                   A row that is non-finite or out of range raises a flag (kNonFinite, kOutOfRange) and gets a clamped index,
//                   so nothing downstream indexes outside a buffer                                               (row_key)
//   * output        one row per occupied voxel: every one of the C columns is the mean of that column over the voxel's rows, and a
//                   count.  Segments stay in segment order; inside a segment voxels come in ascending key order (Open3D's order
//                   is its hash map's and unspecified: this one is the project's own).
//
// THE ORDER OF A VOXEL'S SUM is a function of its run length m alone.  Its terms t_0 .. t_{m-1} are its rows in ascending input
// row index (a STABLE sort of the keys puts them so).
//   m <= kSequential = 64:  ((0.0 + t_0) + t_1) + ...                                                            (sequential_sum)
//   m >  64:                lane j of kLanes = 64 adds t_j, t_{j + 64}, ... ascending from 0.0 (lane_sum), then the 64 partials
//                           fold by strides 32, 16, ..., 1: partial[j] += partial[j + stride] for j < stride     (strided_sum)
//   mean = sum / (double) m.  There is no product, so nothing can be fused.
// The routing by m is part of the rule: the device runs the first form on one lane per voxel and the second on one wave per voxel.
#pragma once
#include "cloud_segments_core.h"

namespace mspa {
namespace voxel {

constexpr int32_t kAxisBits = 21;
constexpr int64_t kAxisLimit = (int64_t)1 << kAxisBits;           // every per-axis index is below it
constexpr int32_t kSequential = 64;                              // the longest run summed sequentially
constexpr int32_t kLanes = 64;                                   // lanes of the strided order
enum : int32_t { kNonFinite = 1, kOutOfRange = 2 };              // bits of the flag word

// ---- the batch ----------------------------------------------------------------------------------------------------------------

// The batch is cloud_segments_core.h's, with its checks and its clamps: batch_rows (N, or -1 for offsets that are no batch),
// segment_of (the segment of a row; empty segments in front of it are passed over -- used for the extents tiles as well, with
// tile_base as the table), row_in_segment (a caller's order entry clamped into [0, N) and then into the slot's own segment),
// first_at_or_above, and the extents pass's tiles (kExtentTile, tiles_of, tile_table).
using segs::batch_rows;
using segs::first_at_or_above;
using segs::kExtentTile;
using segs::row_in_segment;
using segs::segment_of;
using segs::tile_table;
using segs::tiles_of;

// ---- the grid -----------------------------------------------------------------------------------------------------------------

MSPA_HD bool size_ok(double voxel_size) { return voxel_size > 0.0 && voxel_size < INFINITY; }

MSPA_HD double min_bound(double lo, double voxel_size) {
    const double half = voxel_size * 0.5;
    return lo - half;
}

// The index of coordinate p on an axis whose segment minimum is lo.  Never outside [0, kAxisLimit): a coordinate that is not
// finite raises kNonFinite and sits at 0; a quotient at or above the limit raises kOutOfRange and sits at the limit - 1; one below
// zero or NaN (a lo that is not this segment's minimum, or not finite) raises kOutOfRange and sits at 0.
MSPA_HD int64_t axis_index(double p, double lo, double voxel_size, int32_t &flags) {
    if (!(fabs(p) < INFINITY)) {
        flags |= kNonFinite;
        return 0;
    }
    const double from = p - min_bound(lo, voxel_size);
    const double cells = from / voxel_size;
    const double idx = floor(cells);
    if (!(idx >= 0.0)) {
        flags |= kOutOfRange;
        return 0;
    }
    if (!(idx < (double)kAxisLimit)) {
        flags |= kOutOfRange;
        return kAxisLimit - 1;
    }
    return (int64_t)idx;
}

MSPA_HD int64_t key_of(int64_t ix, int64_t iy, int64_t iz) { return ix << (2 * kAxisBits) | iy << kAxisBits | iz; }

MSPA_HD int64_t row_key(const double *__restrict__ p, const double *__restrict__ lo, double voxel_size, int32_t &flags) {
    const int64_t ix = axis_index(p[0], lo[0], voxel_size, flags);
    const int64_t iy = axis_index(p[1], lo[1], voxel_size, flags);
    const int64_t iz = axis_index(p[2], lo[2], voxel_size, flags);
    return key_of(ix, iy, iz);
}

// ---- the sums -----------------------------------------------------------------------------------------------------------------

MSPA_HD bool is_long(int64_t m) { return m > kSequential; }

template <typename Term>
MSPA_HD double sequential_sum(int64_t m, Term term) {
    double sum = 0.0;
    for (int64_t i = 0; i < m; ++i) sum += term(i);
    return sum;
}

// What lane j of kLanes adds up: term(j), term(j + kLanes), ... below m, ascending, from 0.0.
template <typename Term>
MSPA_HD double lane_sum(int32_t j, int64_t m, Term term) {
    double p = 0.0;
    for (int64_t i = j; i < m; i += kLanes) p += term(i);
    return p;
}

// The strided order on one thread: the kLanes lane sums, folded by strides kLanes / 2, ..., 1.
template <typename Term>
inline double strided_sum(int64_t m, Term term) {
    double partial[kLanes];
    for (int32_t j = 0; j < kLanes; ++j) partial[j] = lane_sum(j, m, term);
    for (int32_t t = kLanes / 2; t >= 1; t >>= 1)
        for (int32_t j = 0; j < t; ++j) partial[j] += partial[j + t];
    return partial[0];
}

template <typename Term>
inline double run_sum(int64_t m, Term term) { return is_long(m) ? strided_sum(m, term) : sequential_sum(m, term); }

MSPA_HD double mean_of(double sum, int64_t m) { return sum / (double)m; }

// ---- the host twin ------------------------------------------------------------------------------------------------------------

// The whole op on the CPU in the device's form: extents per segment, keys, ONE stable sort by (segment, key), run heads, means.
// out_rows [N, C] and out_counts [N] are sized for the worst case and hold M = out_offsets[S] rows; out_offsets [S + 1].  Returns
// the flag word: non-zero means a refusal, and the outputs then hold the clamped keys' result.  A batch that batch_rows accepts,
// C >= 3, size_ok(voxel_size).
inline int32_t down_sample_all(const double *rows, int64_t C, const int64_t *offsets, int64_t S, double voxel_size, double *out_rows,
                               int64_t *out_offsets, int32_t *out_counts) {
    const int64_t N = offsets[S];
    int32_t flags = 0;
    std::vector<int64_t> keys((size_t)N), order((size_t)N);
    int64_t M = 0;
    out_offsets[0] = 0;
    for (int64_t s = 0; s < S; ++s) {
        const int64_t a = offsets[s], b = offsets[s + 1];
        if (a < b) {
            double lo[3] = {INFINITY, INFINITY, INFINITY};
            for (int64_t i = a; i < b; ++i)
                for (int ax = 0; ax < 3; ++ax) lo[ax] = rows[i * C + ax] < lo[ax] ? rows[i * C + ax] : lo[ax];
            for (int64_t i = a; i < b; ++i) keys[(size_t)i] = row_key(rows + i * C, lo, voxel_size, flags);
            std::iota(order.begin() + a, order.begin() + b, a);
            std::stable_sort(order.begin() + a, order.begin() + b, [&](int64_t x, int64_t y) { return keys[(size_t)x] < keys[(size_t)y]; });
            for (int64_t start = a; start < b;) {
                int64_t end = start + 1;
                while (end < b && keys[(size_t)order[(size_t)end]] == keys[(size_t)order[(size_t)start]]) ++end;
                const int64_t m = end - start;
                for (int64_t c = 0; c < C; ++c)
                    out_rows[M * C + c] = mean_of(run_sum(m, [&](int64_t i) { return rows[order[(size_t)(start + i)] * C + c]; }), m);
                out_counts[M++] = (int32_t)m;
                start = end;
            }
        }
        out_offsets[s + 1] = M;
    }
    return flags;
}

}  // namespace voxel
}  // namespace mspa
