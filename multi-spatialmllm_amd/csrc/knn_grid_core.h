// The uniform grid behind the exact k-nearest-neighbour search of cloud_ops.hip, stated once for the device kernel and the host
// twin (mspa_knn_mean_distance_host): the cell of a point, the lower bound on everything outside a visited block of cells, and
// the walk itself.  A plain C++ build of this header is the reference the device must agree with.
//
//   * The grid's box [lo, hi] comes from per-axis ORDER STATISTICS of the cloud, not its min / max: a few points very far
//     away do not decide the cell size.  A point outside the box is clamped into the border cell of its side, so a border cell
//     is unbounded outwards and never has an unvisited neighbour on that side.
//   * Points are ordered by cell id (x fastest); starts[c] is the first sorted point of cell c, starts[cells] = n.
//   * A query visits the cells [c - r, c + r] (clipped to the grid) for r = 0, 1, 2, ...: at each r the shell that r adds.  Its k
//     smallest squared distances sit in an ascending list.  After a shell, `outside_bound` is a lower bound on the distance to
//     every point in a cell not yet visited; the walk ends once the k-th best squared distance is no larger than its square.
//
// The floating-point argument (u = 2^-53).  cell = trunc(t), t = fl(fl(p - org) * inv), inv = fl(1 / size), clamped to
// [0, dim - 1]; the face below cell i is F_i = fl(org + fl(i * size)).  For 1 <= i <= dim - 1:
//   cell(p) <  i  =>  t < i  =>  fl(p - org) * inv < i (rounding is monotone and i is representable)
//                 =>  p - org < i * size * (1 + 2u) / (1 - u)  =>  p < org + i * size + 4u * ext,
//   cell(p) >= i  =>  t >= i =>  fl(p - org) * inv >= i * (1 - u)  =>  p > org + i * size - 4u * ext,
// and |F_i - (org + i * size)| <= u * ext + 2u * (|org| + ext), with or without a fused multiply-add.  So every point of a
// cell below i lies below F_i + eps and every point of a cell from i up lies above F_i - eps for any
// eps >= u * (7 * ext + 2 * |org|); make_grid takes eps = 2^-48 * (|lo| + |hi| + ext), 32 times that and still some 2^-38 of a
// cell.  The subtraction q - F_i and the square each round once more, and a squared distance is three products and two sums
// (relative error < 4u): the walk compares against b * b * (1 - 2^-40), which absorbs all of them.  Too small a bound costs
// cells; too large a one would drop a neighbour.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#ifndef MSPA_HD
#ifdef __HIPCC__
#define MSPA_HD __host__ __device__ __forceinline__
#else
#define MSPA_HD inline
#endif
#endif

namespace mspa {
namespace knn {

constexpr int32_t kMaxK = 64;
constexpr int32_t kMaxAxisCells = 1024;
constexpr int64_t kMaxPoints = (int64_t)1 << 30;
constexpr double kCellFill = 0.4;                  // points per cell aimed at, as a fraction of k: a 3 x 3 x 3 block then holds
                                                   // the k nearest of a uniform cloud within one cell size of the query
constexpr double kShrink = 1.0 - 0x1p-40;

struct Grid {
    double org[3], size[3], inv[3], eps[3];
    int32_t dim[3];
    int32_t cells;
};

// The most cells make_grid can give n points with k neighbours: per axis ceil(ext / s) <= 2 * ext / s, and the live axes'
// ext / s multiply to n / max(1, kCellFill * k).
MSPA_HD int64_t max_cells(int64_t n, int32_t k) {
    const double fill = kCellFill * k > 1.0 ? kCellFill * k : 1.0;
    return (int64_t)(8.0 * ((double)n / fill + 1.0)) + 8;
}

// The grid over the box [lo, hi] (finite, lo <= hi per axis) for n points and k neighbours.  An axis without extent, or
// thinner than a cell of the others, is one cell deep: a plane gets a 2-D grid and a line a 1-D one.
inline void make_grid(const double lo[3], const double hi[3], int64_t n, int32_t k, Grid &g) {
    double ext[3];
    bool live[3];
    for (int a = 0; a < 3; ++a) {
        ext[a] = hi[a] - lo[a];
        live[a] = ext[a] > 0.0 && ext[a] < INFINITY;
    }
    const double fill = kCellFill * k > 1.0 ? kCellFill * k : 1.0;
    const double want = (double)n / fill > 1.0 ? (double)n / fill : 1.0;
    double s = 1.0;
    for (int pass = 0; pass < 3; ++pass) {
        int d = 0;
        double vol = 1.0;
        for (int a = 0; a < 3; ++a)
            if (live[a]) {
                ++d;
                vol *= ext[a];
            }
        if (d == 0) break;
        s = pow(vol / want, 1.0 / d);
        bool dropped = false;
        for (int a = 0; a < 3; ++a)
            if (live[a] && !(ext[a] >= s)) {
                live[a] = false;
                dropped = true;
            }
        if (!dropped) break;
    }
    int64_t cells = 1;
    for (int a = 0; a < 3; ++a) {
        double cnt = live[a] && s > 0.0 ? ceil(ext[a] / s) : 1.0;
        if (!(cnt >= 1.0)) cnt = 1.0;
        if (cnt > kMaxAxisCells) cnt = kMaxAxisCells;
        g.dim[a] = (int32_t)cnt;
        g.org[a] = lo[a];
        g.size[a] = g.dim[a] > 1 ? ext[a] / g.dim[a] : 1.0;
        if (!(g.size[a] > 0.0)) {                    // an extent so small that a cell of it underflows: one cell
            g.dim[a] = 1;
            g.size[a] = 1.0;
        }
        g.inv[a] = 1.0 / g.size[a];
        g.eps[a] = 0x1p-48 * (fabs(lo[a]) + fabs(hi[a]) + ext[a]);
        cells *= g.dim[a];
    }
    g.cells = (int32_t)cells;                        // <= max_cells(n, k): every live axis has ext >= s (grid_ok checks it again)
}

// A grid that make_grid could have written: what the entry points check before a kernel trusts it.
inline bool grid_ok(const Grid &g, int64_t n, int32_t k) {
    int64_t cells = 1;
    for (int a = 0; a < 3; ++a) {
        if (g.dim[a] < 1 || g.dim[a] > kMaxAxisCells) return false;
        if (!(g.size[a] > 0.0) || !(g.size[a] < INFINITY) || !(g.inv[a] > 0.0) || !(g.inv[a] < INFINITY)) return false;
        if (!(g.eps[a] >= 0.0) || !(g.eps[a] < INFINITY) || !(fabs(g.org[a]) < INFINITY)) return false;
        cells *= g.dim[a];
    }
    return cells == g.cells && cells <= max_cells(n, k);
}

MSPA_HD int32_t axis_cell(const Grid &g, int a, double x) {
    const double t = (x - g.org[a]) * g.inv[a];
    if (!(t >= 1.0)) return 0;                       // below the box, the first cell, or NaN
    if (t >= (double)g.dim[a]) return g.dim[a] - 1;
    return (int32_t)t;
}

MSPA_HD int32_t cell_of(const Grid &g, double x, double y, double z) {
    return (axis_cell(g, 2, z) * g.dim[1] + axis_cell(g, 1, y)) * g.dim[0] + axis_cell(g, 0, x);
}

MSPA_HD double face(const Grid &g, int a, int32_t i) { return g.org[a] + (double)i * g.size[a]; }

// A lower bound on the distance from q to any point whose cell is outside [lo, hi] (per axis, inside the grid): the nearest of
// the faces behind which unvisited cells remain.  +inf when the block is the whole grid; may be <= 0 for a query outside the box.
MSPA_HD double outside_bound(const Grid &g, const double q[3], const int32_t lo[3], const int32_t hi[3]) {
    double b = INFINITY;
    for (int a = 0; a < 3; ++a) {
        if (lo[a] > 0) {
            const double d = (q[a] - face(g, a, lo[a])) - g.eps[a];
            b = d < b ? d : b;
        }
        if (hi[a] < g.dim[a] - 1) {
            const double d = (face(g, a, hi[a] + 1) - q[a]) - g.eps[a];
            b = d < b ? d : b;
        }
    }
    return b;
}

// The k smallest squared distances from q to the sorted points, ascending in best[0 .. k) (+inf where the cloud has fewer
// than k points).  Best is anything with `double &operator[](int)`.  Returns the number of distances evaluated.
template <typename Best>
MSPA_HD int64_t walk(const Grid &g, const double *__restrict__ pts, const int32_t *__restrict__ starts, const double q[3], int32_t k,
                     Best best) {
    for (int32_t j = 0; j < k; ++j) best[j] = INFINITY;
    double kth = INFINITY;
    int64_t evals = 0;
    const int32_t c[3] = {axis_cell(g, 0, q[0]), axis_cell(g, 1, q[1]), axis_cell(g, 2, q[2])};
    auto take = [&](double d2) {
        if (d2 < kth) {
            int32_t j = k - 1;
            for (; j > 0 && best[j - 1] > d2; --j) best[j] = best[j - 1];
            best[j] = d2;
            kth = best[k - 1];
        }
    };
    auto dist2 = [&](int32_t i) {
        const double dx = pts[3 * (int64_t)i] - q[0], dy = pts[3 * (int64_t)i + 1] - q[1], dz = pts[3 * (int64_t)i + 2] - q[2];
        return (dx * dx + dy * dy) + dz * dz;
    };
    auto scan = [&](int32_t row, int32_t x0, int32_t x1) {                    // the cells x0 .. x1 of one row: one run of points
        const int32_t begin = starts[row + x0], end = starts[row + x1 + 1];
        int32_t i = begin;
        for (; i + 4 <= end; i += 4) {                                        // four points' loads in flight before the list is touched
            const double d0 = dist2(i), d1 = dist2(i + 1), d2 = dist2(i + 2), d3 = dist2(i + 3);
            take(d0);
            take(d1);
            take(d2);
            take(d3);
        }
        for (; i < end; ++i) take(dist2(i));
        if (end > begin) evals += end - begin;
    };
    for (int32_t r = 0;; ++r) {
        int32_t lo[3], hi[3];
        for (int a = 0; a < 3; ++a) {
            lo[a] = c[a] - r > 0 ? c[a] - r : 0;
            hi[a] = c[a] + r < g.dim[a] - 1 ? c[a] + r : g.dim[a] - 1;
        }
        for (int32_t z = lo[2]; z <= hi[2]; ++z) {
            const bool z_in = z > c[2] - r && z < c[2] + r;                   // inside the block visited so far, along z
            for (int32_t y = lo[1]; y <= hi[1]; ++y) {
                const int32_t row = (z * g.dim[1] + y) * g.dim[0];
                if (!(z_in && y > c[1] - r && y < c[1] + r)) {
                    scan(row, lo[0], hi[0]);
                } else {                                                      // only the two ends of the row are new
                    if (c[0] - r >= 0) scan(row, c[0] - r, c[0] - r);
                    if (c[0] + r <= g.dim[0] - 1) scan(row, c[0] + r, c[0] + r);
                }
            }
        }
        const double b = outside_bound(g, q, lo, hi);
        if (b == INFINITY) break;                                             // the block is the whole grid
        if (b > 0.0 && kth <= b * b * kShrink) break;
    }
    return evals;
}

// The mean of the roots of best[0 .. count), summed in ascending order.
template <typename Best>
MSPA_HD double mean_root(Best best, int32_t count) {
    double sum = 0.0;
    for (int32_t j = 0; j < count; ++j) sum += sqrt(best[j]);
    return sum / (double)count;
}

struct HostList {
    double *base;
    double &operator[](int32_t j) const { return base[j]; }
};

// The whole search on the CPU for n >= 1 finite points: box from the order statistics of rank n / 100 and n - 1 - n / 100 per axis,
// a stable order by cell, the walk per point.  mean[i] (and evals[i], when wanted) in the input's order.  False: no grid.
inline bool mean_distance_all(const double *xyz_host, int64_t n, int32_t k, double *mean_host, int32_t *evals_host) {
    double lo[3], hi[3];
    const int64_t r = n / 100;
    std::vector<double> col((size_t)n);
    for (int a = 0; a < 3; ++a) {
        for (int64_t i = 0; i < n; ++i) col[(size_t)i] = xyz_host[3 * i + a];
        std::nth_element(col.begin(), col.begin() + r, col.end());
        lo[a] = col[(size_t)r];
        std::nth_element(col.begin(), col.begin() + (n - 1 - r), col.end());
        hi[a] = col[(size_t)(n - 1 - r)];
    }
    Grid g;
    memset(&g, 0, sizeof(g));
    make_grid(lo, hi, n, k, g);
    if (!grid_ok(g, n, k)) return false;
    std::vector<int32_t> cells((size_t)n), order((size_t)n), starts((size_t)g.cells + 1, 0);
    for (int64_t i = 0; i < n; ++i) cells[(size_t)i] = cell_of(g, xyz_host[3 * i], xyz_host[3 * i + 1], xyz_host[3 * i + 2]);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return cells[(size_t)a] < cells[(size_t)b]; });
    std::vector<double> pts((size_t)n * 3);
    for (int64_t i = 0; i < n; ++i) {
        const int32_t o = order[(size_t)i];
        for (int a = 0; a < 3; ++a) pts[(size_t)(3 * i + a)] = xyz_host[3 * (int64_t)o + a];
        ++starts[(size_t)cells[(size_t)o] + 1];
    }
    for (int32_t c = 0; c < g.cells; ++c) starts[(size_t)c + 1] += starts[(size_t)c];
    double best[kMaxK];
    for (int64_t i = 0; i < n; ++i) {
        const double q[3] = {pts[(size_t)(3 * i)], pts[(size_t)(3 * i + 1)], pts[(size_t)(3 * i + 2)]};
        const int64_t e = walk(g, pts.data(), starts.data(), q, k, HostList{best});
        mean_host[order[(size_t)i]] = mean_root(HostList{best}, (int32_t)(k < n ? k : n));
        if (evals_host) evals_host[order[(size_t)i]] = (int32_t)e;
    }
    return true;
}

}  // namespace knn
}  // namespace mspa
