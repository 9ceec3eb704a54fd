// A RAGGED BATCH of clouds through the k-nearest search of knn_grid_core.h and the statistical-outlier rule, stated once for the
// kernels of cloud_segments.hip and their host twins (mspa_knn_segments_mean_distance_host, mspa_outlier_segments_host).  A plain
// C++ build of this header and knn_grid_core.h is the reference the device must agree with bit for bit.
//
// The batch.  xyz [N, 3] float64 plus offsets [S + 1] int64, ascending, offsets[0] = 0, offsets[S] = N: segment s is the rows
// offsets[s] .. offsets[s + 1], n_s of them; empty segments are allowed anywhere.
//
// The search.  Per segment it is exactly knn_grid_core.h's: the box is the per-axis order statistics of rank n_s / 100 and
// n_s - 1 - n_s / 100 OF THAT SEGMENT, make_grid(lo, hi, n_s, k, g) runs on the host, unchanged, and walk / mean_root are called
// with the segment's own pts base, its own starts base (segment-local int32 indices) and min(k, n_s).  (The single-cloud kernel
// passes k itself to walk; for k > n_s both visit the whole grid, evaluate n_s distances and leave the same n_s entries.)  The grid
// of a segment is the grid the single-cloud op builds for it, so avg and the evaluation count per point equal the single-cloud
// op's bit for bit.  What is new is the bookkeeping that lets ONE sort order the whole batch:
//   * cell_base[s] = the exclusive prefix of max_cells(n_s, k) over the non-empty segments (cell_tables) -- a function of the
//     offsets and k alone, so the host has it without a read-back;
//   * the key of a row is cell_base[s] + cell_of(grid_s, x, y, z): monotone in s, so a stable sort of the keys orders the rows by
//     segment and, inside a segment, by cell, and every row stays inside its segment's range of slots;
//   * starts of segment s begin at slot cell_base[s] + s of one table (one slot more than its cells, also for an empty segment).
//
// The statistics.  For a segment of n rows, P its rows with avg > 0:
//     mean = (sum over P of avg) / n;   sd = sqrt((sum over P of (avg - mean)^2) / (n - 1));   thr = mean + std_ratio * sd;
//     row i stays iff 0 < avg[i] < thr.
// n = 0 has no mean and n < 2 no sd (0 / 0): mean, sd and thr are then the one quiet NaN of no_value(), and nothing stays.  No
// product is fused with a sum anywhere (the library is built with -ffp-contract=off).
//
// THE ORDER OF THE TWO SUMS is a function of n alone, and is this: the term of row i is term(i) (0.0 for a row outside P).  Lane j
// of kLanes = 256 starts from 0.0 and adds term(j), term(j + 256), term(j + 512), ... in ascending order (lane_sum).  Then the 256
// partials fold by strides 128, 64, ..., 1: at stride t, partial[j] += partial[j + t] for every j < t (ordered_sum).  The host twin
// and the statistics kernel implement that order literally -- the kernel with one thread per lane and partial[] in LDS.  It is NOT
// torch.sum's order: the single-cloud op (handler/ops.py) sums with torch.sum, whose order is torch's own, so its mean, sd and
// threshold may differ from these in the last bits, and a row whose avg lies within those bits of the threshold may fall on the
// other side.  The tests assert that no row of their batches does before they compare kept sets.
#pragma once
#include "knn_grid_core.h"

namespace mspa {
namespace segs {

constexpr int32_t kLanes = 256;
constexpr int64_t kMaxSegments = (int64_t)1 << 24;

MSPA_HD double no_value() { return __builtin_nan(""); }

// ---- the batch --------------------------------------------------------------------------------------------------------------

// N where offsets [S + 1] describes a batch (offsets[0] = 0, ascending, N <= 2^30, 0 <= S <= 2^24), else -1.
inline int64_t batch_rows(const int64_t *offsets, int64_t S) {
    if (S < 0 || S > kMaxSegments || !offsets || offsets[0] != 0) return -1;
    for (int64_t s = 0; s < S; ++s)
        if (offsets[s + 1] < offsets[s]) return -1;
    return offsets[S] <= knn::kMaxPoints ? offsets[S] : -1;
}

// The segment of row i, 0 <= i < offsets[S]: the LAST s with offsets[s] <= i (empty segments in front of it are passed over).
MSPA_HD int64_t segment_of(const int64_t *__restrict__ offsets, int64_t S, int64_t i) {
    int64_t lo = 0, hi = S;                                      // invariant: offsets[lo] <= i < offsets[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (offsets[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The extents pass cuts every segment into tiles of kExtentTile rows: tile_base [S + 1] is the exclusive prefix of the tiles.
constexpr int64_t kExtentTile = 4096;                            // rows one workgroup of the extents pass takes
MSPA_HD int64_t tiles_of(int64_t n) { return (n + kExtentTile - 1) / kExtentTile; }
inline void tile_table(const int64_t *offsets, int64_t S, int64_t *tile_base) {
    tile_base[0] = 0;
    for (int64_t s = 0; s < S; ++s) tile_base[s + 1] = tile_base[s] + tiles_of(offsets[s + 1] - offsets[s]);
}

// cell_base [S + 1]: the exclusive prefix of max_cells(n_s, k) over the non-empty segments.
inline void cell_tables(const int64_t *offsets, int64_t S, int32_t k, int64_t *cell_base) {
    cell_base[0] = 0;
    for (int64_t s = 0; s < S; ++s) {
        const int64_t n = offsets[s + 1] - offsets[s];
        cell_base[s + 1] = cell_base[s] + (n > 0 ? knn::max_cells(n, k) : 0);
    }
}

// The first slot of segment s in the table of starts, and the slots of the whole table.
MSPA_HD int64_t starts_base(const int64_t *__restrict__ cell_base, int64_t s) { return cell_base[s] + s; }
inline int64_t starts_slots(const int64_t *cell_base, int64_t S) { return cell_base[S] + S; }

// The grid records of a batch from its segments' boxes lo / hi [S, 3] (an empty segment's box is not read: its record is zeros).
// False where make_grid has no grid for a box.
inline bool make_grids(const double *lo, const double *hi, const int64_t *offsets, int64_t S, int32_t k, knn::Grid *grids) {
    for (int64_t s = 0; s < S; ++s) {
        const int64_t n = offsets[s + 1] - offsets[s];
        memset(&grids[s], 0, sizeof(knn::Grid));
        if (n == 0) continue;
        for (int a = 0; a < 3; ++a)
            if (!(fabs(lo[3 * s + a]) < INFINITY) || !(fabs(hi[3 * s + a]) < INFINITY) || !(lo[3 * s + a] <= hi[3 * s + a])) return false;
        knn::make_grid(lo + 3 * s, hi + 3 * s, n, k, grids[s]);
        if (!knn::grid_ok(grids[s], n, k)) return false;
    }
    return true;
}

// Records that make_grids could have written for these offsets and this k.
inline bool grids_ok(const knn::Grid *grids, const int64_t *offsets, int64_t S, int32_t k) {
    for (int64_t s = 0; s < S; ++s) {
        const int64_t n = offsets[s + 1] - offsets[s];
        if (n > 0 && !knn::grid_ok(grids[s], n, k)) return false;
    }
    return true;
}

MSPA_HD int64_t key_of(const knn::Grid &g, int64_t base, double x, double y, double z) { return base + knn::cell_of(g, x, y, z); }

// A caller's order entry as a row of the slot's own segment [a, b), a < b: first into [0, N), then into the segment.
MSPA_HD int64_t row_in_segment(int64_t o, int64_t N, int64_t a, int64_t b) {
    o = o < 0 ? 0 : o >= N ? N - 1 : o;
    return o < a ? a : o >= b ? b - 1 : o;
}

// The first slot in [a, b) whose key is at least `key` (b where none is), for keys ascending over [a, b).
MSPA_HD int64_t first_at_or_above(const int64_t *__restrict__ keys, int64_t a, int64_t b, int64_t key) {
    while (a < b) {
        const int64_t mid = (a + b) >> 1;
        if (keys[mid] < key) a = mid + 1;
        else b = mid;
    }
    return a;
}

// ---- the statistics ---------------------------------------------------------------------------------------------------------

MSPA_HD double positive_term(double avg) { return avg > 0.0 ? avg : 0.0; }

MSPA_HD double deviation_term(double avg, double mean) {
    if (!(avg > 0.0)) return 0.0;
    const double d = avg - mean;
    return d * d;
}

// What lane j of kLanes adds up: term(j), term(j + kLanes), ... below n, ascending, from 0.0.
template <typename Term>
MSPA_HD double lane_sum(int32_t j, int64_t n, Term term) {
    double p = 0.0;
    for (int64_t i = j; i < n; i += kLanes) p += term(i);
    return p;
}

// The stated order on one thread: the kLanes lane sums, folded by strides kLanes / 2, ..., 1.
template <typename Term>
inline double ordered_sum(int64_t n, Term term) {
    double partial[kLanes];
    for (int32_t j = 0; j < kLanes; ++j) partial[j] = lane_sum(j, n, term);
    for (int32_t t = kLanes / 2; t >= 1; t >>= 1)
        for (int32_t j = 0; j < t; ++j) partial[j] += partial[j + t];
    return partial[0];
}

MSPA_HD double mean_of(double sum, int64_t n) { return n > 0 ? sum / (double)n : no_value(); }
MSPA_HD double sd_of(double squares, int64_t n) { return n > 1 ? sqrt(squares / (double)(n - 1)) : no_value(); }
MSPA_HD double threshold_of(double mean, double sd, double std_ratio, int64_t n) {
    if (n < 2) return no_value();
    const double scaled = std_ratio * sd;
    return mean + scaled;
}
MSPA_HD bool stays(double avg, double thr) { return avg > 0.0 && avg < thr; }

// ---- the host twins -----------------------------------------------------------------------------------------------------------

// The whole search of a batch on the CPU, in the device's form: boxes from each segment's order statistics, one table of grids,
// ONE stable sort of the global keys, the gather, the starts per segment, the walk per sorted slot.  mean [N] (and evals [N], when
// wanted) in the input's order.  False: no grid for a segment.  Finite coordinates, a batch that batch_rows accepts, 1 <= k <= kMaxK.
inline bool mean_distance_segments_all(const double *xyz_host, const int64_t *offsets, int64_t S, int32_t k, double *mean_host,
                                       int32_t *evals_host) {
    const int64_t N = offsets[S];
    std::vector<double> lo((size_t)S * 3, 0.0), hi((size_t)S * 3, 0.0), col;
    for (int64_t s = 0; s < S; ++s) {
        const int64_t a = offsets[s], n = offsets[s + 1] - a, r = n / 100;
        if (n == 0) continue;
        col.resize((size_t)n);
        for (int ax = 0; ax < 3; ++ax) {
            for (int64_t i = 0; i < n; ++i) col[(size_t)i] = xyz_host[3 * (a + i) + ax];
            std::nth_element(col.begin(), col.begin() + r, col.end());
            lo[(size_t)(3 * s + ax)] = col[(size_t)r];
            std::nth_element(col.begin(), col.begin() + (n - 1 - r), col.end());
            hi[(size_t)(3 * s + ax)] = col[(size_t)(n - 1 - r)];
        }
    }
    std::vector<knn::Grid> grids((size_t)S + 1);
    if (!make_grids(lo.data(), hi.data(), offsets, S, k, grids.data())) return false;
    std::vector<int64_t> cell_base((size_t)S + 1);
    cell_tables(offsets, S, k, cell_base.data());
    std::vector<int64_t> keys((size_t)N), order((size_t)N), sorted_keys((size_t)N);
    for (int64_t i = 0; i < N; ++i) {
        const int64_t s = segment_of(offsets, S, i);
        keys[(size_t)i] = key_of(grids[(size_t)s], cell_base[(size_t)s], xyz_host[3 * i], xyz_host[3 * i + 1], xyz_host[3 * i + 2]);
    }
    std::iota(order.begin(), order.end(), (int64_t)0);
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return keys[(size_t)a] < keys[(size_t)b]; });
    std::vector<double> pts((size_t)N * 3);
    for (int64_t i = 0; i < N; ++i) {                            // the gather: the key comes from the point that was copied
        const int64_t s = segment_of(offsets, S, i);
        const int64_t o = row_in_segment(order[(size_t)i], N, offsets[s], offsets[s + 1]);
        for (int ax = 0; ax < 3; ++ax) pts[(size_t)(3 * i + ax)] = xyz_host[3 * o + ax];
        sorted_keys[(size_t)i] = key_of(grids[(size_t)s], cell_base[(size_t)s], pts[(size_t)(3 * i)], pts[(size_t)(3 * i + 1)], pts[(size_t)(3 * i + 2)]);
    }
    std::vector<int32_t> starts((size_t)starts_slots(cell_base.data(), S), 0);
    for (int64_t s = 0; s < S; ++s) {
        const int64_t a = offsets[s], b = offsets[s + 1];
        if (a == b) continue;
        for (int32_t c = 0; c <= grids[(size_t)s].cells; ++c)
            starts[(size_t)(starts_base(cell_base.data(), s) + c)] =
                (int32_t)(first_at_or_above(sorted_keys.data(), a, b, cell_base[(size_t)s] + c) - a);
    }
    double best[knn::kMaxK];
    for (int64_t i = 0; i < N; ++i) {
        const int64_t s = segment_of(offsets, S, i);
        const int64_t a = offsets[s], n = offsets[s + 1] - a;
        const int32_t kk = (int32_t)(k < n ? k : n);
        const double q[3] = {pts[(size_t)(3 * i)], pts[(size_t)(3 * i + 1)], pts[(size_t)(3 * i + 2)]};
        const int64_t e = knn::walk(grids[(size_t)s], pts.data() + 3 * a, starts.data() + starts_base(cell_base.data(), s), q, kk,
                                    knn::HostList{best});
        const int64_t o = row_in_segment(order[(size_t)i], N, a, a + n);
        mean_host[o] = knn::mean_root(knn::HostList{best}, kk);
        if (evals_host) evals_host[o] = (int32_t)e;
    }
    return true;
}

// The rule of a batch on the CPU: keep [N] (1 / 0) and, per segment, kept, mean, sd, thr and lo / hi [S, 3] of the kept rows
// (+inf / -inf where none stays).
inline void outlier_segments_all(const double *avg, const double *xyz, const int64_t *offsets, int64_t S, double std_ratio, uint8_t *keep,
                                 int64_t *kept, double *mean, double *sd, double *thr, double *lo, double *hi) {
    for (int64_t s = 0; s < S; ++s) {
        const double *v = avg + offsets[s];
        const int64_t n = offsets[s + 1] - offsets[s];
        const double m = mean_of(ordered_sum(n, [&](int64_t i) { return positive_term(v[i]); }), n);
        const double d = sd_of(ordered_sum(n, [&](int64_t i) { return deviation_term(v[i], m); }), n);
        const double t = threshold_of(m, d, std_ratio, n);
        int64_t count = 0;
        double l[3] = {INFINITY, INFINITY, INFINITY}, h[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int64_t i = 0; i < n; ++i) {
            const bool in = stays(v[i], t);
            keep[offsets[s] + i] = in ? 1 : 0;
            if (!in) continue;
            ++count;
            for (int a = 0; a < 3; ++a) {
                const double x = xyz[3 * (offsets[s] + i) + a];
                l[a] = x < l[a] ? x : l[a];
                h[a] = x > h[a] ? x : h[a];
            }
        }
        kept[s] = count;
        mean[s] = m;
        sd[s] = d;
        thr[s] = t;
        for (int a = 0; a < 3; ++a) {
            lo[3 * s + a] = l[a];
            hi[3 * s + a] = h[a];
        }
    }
}

}  // namespace segs
}  // namespace mspa
