// DBSCAN of a ragged batch of clouds, stated once for the kernels of dbscan_segments.hip and their host twin
// (mspa_dbscan_segments_host).  A plain C++ build of this header is the reference the device must agree with value for value
// (DESIGN.md section 0.25).  The labels are scikit-learn's: sklearn.cluster.DBSCAN(eps, min_samples = min_points,
// algorithm = "kd_tree").fit(X).labels_ per segment (tests/test_dbscan_segments_cpu.py holds the twin to it).
//
// The batch is cloud_segments_core.h's, with more columns: rows [N, C >= 3] float64, xyz in front, offsets [S + 1].
//
// THE RULE, per segment of n >= 0 rows with finite xyz, eps_ok(eps) and min_points >= 1, every step one float64 operation (the
// library is built with -ffp-contract=off):
//   * near(i, j)  <=>  (dx * dx + dy * dy) + dz * dz <= eps * eps, dx = x_i - x_j and so on: the sum in that order, the
//                 comparison <=; i is near itself                                                                       (near)
//   * core(i)     <=>  |{j : near(i, j)}| >= min_points: the point itself counts, and so does every duplicate           (is_core)   
//   * clusters    the connected components of the core points under near, numbered 0, 1, ... in ascending order of the lowest input
//                 row index among their core points (the component's REPRESENTATIVE)
//   * border      a non-core point takes the lowest cluster number among the core points near it, -1 (noise) where there is none
//   * labels      int32 in input row order: a function of the rows and the two parameters alone
//   * largest     the cluster with the most rows, core and border together; a tie goes to the lowest number; a segment that is all
//                 noise keeps nothing                                                                                   (largest_of)
//
// FIRST FLOATING-POINT ARGUMENT: a near pair lies in cells whose indices differ by at most 1 per axis.
// The cells are voxel_grid_core.h's at side h = cell_side(eps) = fl(eps * kCellFactor), kCellFactor = 1 + 2^-20: per axis
// q(p) = fl(fl(p - mb) / h), idx = floor(q), with ONE mb per segment and axis, and idx < 2^21 for every row (a row beyond raises
// kOutOfRange, and the call is refused).  Write u = 2^-53.
//   (a) near(i, j) gives fl(dx * dx) <= fl(eps * eps), because every term of the sum is >= 0 and rounding is monotone.  eps_ok
//       asks for eps * eps >= DBL_MIN (and finite), so the right side carries a relative error of at most u and the left side one of
//       at most u (or, where it is subnormal, an absolute error below 2^-1075 <= u * eps^2): dx^2 <= eps^2 (1 + u)^2 / (1 - u), hence
//       |dx| <= eps (1 + 2u).  dx itself is fl(x_i - x_j), so |x_i - x_j| <= |dx| / (1 - u) <= eps (1 + 4u).
//   (b) fl(p - mb) is the exact difference times (1 + e), |e| <= u, and the division adds another such factor; both quotients
//       are below 2^21 + 1, so each computed q differs from the exact (p - mb) / h by at most 2^22 * 2u = 2^-30.
//   (c) The exact quotients differ by |x_i - x_j| / h <= eps (1 + 4u) / (eps (1 + 2^-20) (1 - u)) < 1 - 2^-21.
//   So |q_i - q_j| < 1 - 2^-21 + 2^-29 < 1, and two reals less than 1 apart have floors at most 1 apart.  With h = eps alone (c)
//   would only give <= 1 + 4u, and a pair at exactly eps -- every neighbour of a lattice k / 8 at eps = 0.125 -- may sit two cells
//   apart.  The walk (walk_near) therefore visits the 27 cells around a point's own and misses no near pair; a point in those
//   cells that is not near is rejected by near itself, so the factor costs work, never a label.
//
// SECOND FLOATING-POINT ARGUMENT: near is symmetric, and the labels do not depend on the order in which pairs are met.
//   x_j - x_i is the exact negation of x_i - x_j in IEEE arithmetic, its square is the same number, and the three squares are added
//   in the same order for (i, j) and (j, i): near(i, j) = near(j, i) bit for bit, so it is enough that ONE end of a pair links it
//   (link_point links towards earlier slots only).  The components are a set function of the near relation.  hook() always puts
//   the larger root under the smaller one, so a tree's root is its lowest row: after any interleaving of the hooks the root of a
//   component is its lowest core row, the representative.  Cluster numbers ascend with the representatives' rows, so the lowest
//   cluster number among a border point's near core points is the number of the lowest ROOT among them: border_root takes a minimum
//   of integers, which no order changes.
//
// THE ITERATION CAPS.  parent[r] <= r always (a hook writes a smaller root into a root; path halving replaces a parent by an
// ancestor), and parent values of a segment stay inside the segment.  A find from row r of a segment of n rows therefore reads a
// strictly descending path: at most n - 1 steps.  A hook that loses its compare-and-swap lost it because its larger root got a
// parent from somebody else; the roots it finds next are both below the larger root it held, so the larger root of the pair
// strictly descends: at most n - 1 retries.  Both loops are capped at n (cap_of): reaching the cap means the parent array is not
// one these rules wrote, the lane sets kCapReached and stops.  No lane waits for another: every step either succeeds or observes
// somebody else's success.
#pragma once
#include "voxel_grid_core.h"

#include <cfloat>

namespace mspa {
namespace dbscan {

constexpr double kCellFactor = 1.0 + 1.0 / 1048576.0;            // 1 + 2^-20: the cell side over eps
enum : int32_t { kNonFinite = voxel::kNonFinite, kOutOfRange = voxel::kOutOfRange, kCapReached = 4 };       // bits of the flag word
constexpr int64_t kAxisMask = voxel::kAxisLimit - 1;

using segs::batch_rows;
using segs::first_at_or_above;
using segs::row_in_segment;
using segs::segment_of;

// eps > 0, finite, and its square a normal number (the first argument's (a)).
MSPA_HD bool eps_ok(double eps) {
    const double sq = eps * eps;
    return eps > 0.0 && eps < INFINITY && sq >= DBL_MIN && sq < INFINITY;
}

MSPA_HD double cell_side(double eps) { return eps * kCellFactor; }

MSPA_HD bool near(const double *__restrict__ p, const double *__restrict__ q, double eps_sq) {
    const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const double xy = xx + yy;
    return xy + zz <= eps_sq;
}

// Every slot j of the segment's sorted range [a, b) whose cell is one of the 27 around slot i's and whose point is near slot i's,
// in ascending (cell key, slot) order per (x, y) column of cells; i itself included.  pts [*, 3] and keys [*] are in sorted order
// (keys ascending over [a, b)).  visit(j) returns true to stop the walk.  The three cells iz - 1 .. iz + 1 of a column are one
// run of keys, so a column costs one binary search.
template <typename Visit>
MSPA_HD void walk_near(const double *__restrict__ pts, const int64_t *__restrict__ keys, int64_t a, int64_t b, int64_t i, double eps_sq,
                       Visit visit) {
    const int64_t key = keys[i];
    const int64_t ix = (key >> (2 * voxel::kAxisBits)) & kAxisMask, iy = (key >> voxel::kAxisBits) & kAxisMask, iz = key & kAxisMask;
    const double p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    const int64_t z0 = iz > 0 ? iz - 1 : 0, z1 = iz < kAxisMask ? iz + 1 : kAxisMask;
    for (int64_t x = ix > 0 ? ix - 1 : 0; x <= ix + 1 && x <= kAxisMask; ++x) {
        for (int64_t y = iy > 0 ? iy - 1 : 0; y <= iy + 1 && y <= kAxisMask; ++y) {
            const int64_t last = voxel::key_of(x, y, z1);
            for (int64_t j = first_at_or_above(keys, a, b, voxel::key_of(x, y, z0)); j < b && keys[j] <= last; ++j)
                if (near(p, pts + 3 * j, eps_sq) && visit(j)) return;
        }
    }
}

// Whether slot i has min_points near points; the count stops there.
MSPA_HD bool is_core(const double *__restrict__ pts, const int64_t *__restrict__ keys, int64_t a, int64_t b, int64_t i, double eps_sq,
                     int64_t min_points) {
    int64_t count = 0;
    walk_near(pts, keys, a, b, i, eps_sq, [&](int64_t) { return ++count >= min_points; });
    return count >= min_points;
}

// ---- union-find over the core rows ------------------------------------------------------------------------------------------
// parent [N] int32, indexed by input row: -1 for a row that is not core, else a core row of the same component and <= the row.
// Mem is how parent is read and written: PlainMemory on the host, agent-scope atomics on the device.

struct PlainMemory {
    int32_t *parent;
    int32_t load(int32_t i) const { return parent[i]; }
    void lower(int32_t i, int32_t v) const { parent[i] = v < parent[i] ? v : parent[i]; }
    int32_t compare_and_swap(int32_t i, int32_t expected, int32_t desired) const {
        const int32_t old = parent[i];
        if (old == expected) parent[i] = desired;
        return old;
    }
};

MSPA_HD int64_t cap_of(int64_t n) { return n; }

// The root of core row r, with path halving on the way; cap steps at the most, else capped is set and the row reached returned.
template <typename Mem>
MSPA_HD int32_t find_root(const Mem &mem, int32_t r, int64_t cap, bool &capped) {
    int64_t steps = 0;
    for (;;) {
        const int32_t p = mem.load(r);
        if (p == r || p < 0) return r;
        const int32_t g = mem.load(p);
        if (g == p || g < 0) return p;
        if (++steps > cap) {
            capped = true;
            return r;
        }
        mem.lower(r, g);                                         // min(parent, an ancestor below it): the path only gets shorter
        r = g;
    }
}

// The same without a store (the flattening pass reads while nothing writes).
template <typename Mem>
MSPA_HD int32_t read_root(const Mem &mem, int32_t r, int64_t cap, bool &capped) {
    int64_t steps = 0;
    for (;;) {
        const int32_t p = mem.load(r);
        if (p == r || p < 0) return r;
        if (++steps > cap) {
            capped = true;
            return r;
        }
        r = p;
    }
}

// Core rows x and y are of one component: the larger root goes under the smaller.
template <typename Mem>
MSPA_HD void hook(const Mem &mem, int32_t x, int32_t y, int64_t cap, bool &capped) {
    for (int64_t tries = 0;; ++tries) {
        x = find_root(mem, x, cap, capped);
        y = find_root(mem, y, cap, capped);
        if (x == y || capped) return;
        if (x < y) {
            const int32_t t = x;
            x = y;
            y = t;
        }
        const int32_t old = mem.compare_and_swap(x, x, y);       // x > y: x is hooked only while it is still a root
        if (old == x) return;
        if (old < 0 || tries >= cap) {                           // (old < 0: a row that is not core -- not a parent array of these rules)
            capped = true;
            return;
        }
        x = old;                                                 // somebody else's hook: go on from the parent it gave
    }
}

// Slot i, core, with every near core slot in front of it (near is symmetric: the pair's later slot links it).  row [*] int32 the
// input row of a sorted slot, core [*] the slots' core flags.
template <typename Mem>
MSPA_HD void link_point(const Mem &mem, const double *__restrict__ pts, const int64_t *__restrict__ keys, const int32_t *__restrict__ row,
                        const uint8_t *__restrict__ core, int64_t a, int64_t b, int64_t i, double eps_sq, int64_t cap, bool &capped) {
    walk_near(pts, keys, a, b, i, eps_sq, [&](int64_t j) {
        if (j < i && core[j]) hook(mem, row[i], row[j], cap, capped);
        return capped;
    });
}

// The lowest root among the core slots near slot i, -1 where there is none.  root [N] by input row.
MSPA_HD int32_t border_root(const double *__restrict__ pts, const int64_t *__restrict__ keys, const int32_t *__restrict__ row,
                            const uint8_t *__restrict__ core, const int32_t *__restrict__ root, int64_t a, int64_t b, int64_t i,
                            double eps_sq) {
    int32_t best = -1;
    walk_near(pts, keys, a, b, i, eps_sq, [&](int64_t j) {
        if (core[j]) {
            const int32_t r = root[row[j]];
            best = best < 0 || r < best ? r : best;
        }
        return false;
    });
    return best;
}

// The largest of count clusters of sizes size[0 .. count): its number (-1 for none) -- the most rows, a tie to the lowest number.
MSPA_HD bool better_of(int32_t size_a, int32_t id_a, int32_t size_b, int32_t id_b) {             // true: b beats a
    return id_b >= 0 && (id_a < 0 || size_b > size_a || (size_b == size_a && id_b < id_a));
}
inline int32_t largest_of(const int32_t *size, int64_t count) {
    int32_t best = -1;
    for (int64_t c = 0; c < count; ++c)
        if (better_of(best < 0 ? 0 : size[best], best, size[c], (int32_t)c)) best = (int32_t)c;
    return best;
}

// ---- the host twin ------------------------------------------------------------------------------------------------------------

// The whole op on the CPU in the device's form: per segment the voxel keys at cell_side(eps), one stable sort, the gather, the core
// flags, the links, the roots, the representatives' ranks, the labels, the sizes and the largest cluster.  labels [N] int32,
// clusters [S] int32, keep [N] uint8 and kept [S] int32 (both may be null).  Returns the flag word: non-zero means a refusal.
// find_cap < 0 means cap_of(n); a lower cap is for the test of the cap itself.
inline int32_t dbscan_all(const double *rows, int64_t C, const int64_t *offsets, int64_t S, double eps, int64_t min_points, int32_t *labels,
                          int32_t *clusters, uint8_t *keep, int32_t *kept, int64_t find_cap = -1) {
    const int64_t N = offsets[S];
    const double h = cell_side(eps), eps_sq = eps * eps;
    int32_t flags = 0;
    std::vector<int64_t> raw((size_t)N), order((size_t)N), keys((size_t)N);
    std::vector<double> pts((size_t)N * 3);
    std::vector<int32_t> row((size_t)N), parent((size_t)N), root((size_t)N), size;
    std::vector<uint8_t> core((size_t)N);
    const PlainMemory mem{parent.data()};
    for (int64_t s = 0; s < S; ++s) {
        const int64_t a = offsets[s], b = offsets[s + 1];
        clusters[s] = 0;
        if (kept) kept[s] = 0;
        if (a == b) continue;
        double lo[3] = {INFINITY, INFINITY, INFINITY};
        for (int64_t i = a; i < b; ++i)
            for (int ax = 0; ax < 3; ++ax) lo[ax] = rows[i * C + ax] < lo[ax] ? rows[i * C + ax] : lo[ax];
        for (int64_t i = a; i < b; ++i) raw[(size_t)i] = voxel::row_key(rows + i * C, lo, h, flags);
        std::iota(order.begin() + a, order.begin() + b, a);
        std::stable_sort(order.begin() + a, order.begin() + b, [&](int64_t x, int64_t y) { return raw[(size_t)x] < raw[(size_t)y]; });
        for (int64_t i = a; i < b; ++i) {
            const int64_t o = order[(size_t)i];
            for (int ax = 0; ax < 3; ++ax) pts[(size_t)(3 * i + ax)] = rows[o * C + ax];
            keys[(size_t)i] = raw[(size_t)o];
            row[(size_t)i] = (int32_t)o;
        }
        for (int64_t i = a; i < b; ++i) {
            core[(size_t)i] = is_core(pts.data(), keys.data(), a, b, i, eps_sq, min_points) ? 1 : 0;
            parent[(size_t)row[(size_t)i]] = core[(size_t)i] ? row[(size_t)i] : -1;
        }
        const int64_t cap = find_cap < 0 ? cap_of(b - a) : find_cap;
        bool capped = false;
        for (int64_t i = a; i < b && !capped; ++i)
            if (core[(size_t)i]) link_point(mem, pts.data(), keys.data(), row.data(), core.data(), a, b, i, eps_sq, cap, capped);
        for (int64_t r = a; r < b; ++r) root[(size_t)r] = parent[(size_t)r] < 0 ? -1 : read_root(mem, (int32_t)r, cap, capped);
        if (capped) flags |= kCapReached;
        std::vector<int32_t> reps;                               // the representatives, ascending: cluster c is reps[c]
        for (int64_t r = a; r < b; ++r)
            if (root[(size_t)r] == r) reps.push_back((int32_t)r);
        clusters[s] = (int32_t)reps.size();
        size.assign(reps.size(), 0);
        for (int64_t i = a; i < b; ++i) {
            const int32_t o = row[(size_t)i];
            const int32_t r = core[(size_t)i] ? root[(size_t)o]
                                              : border_root(pts.data(), keys.data(), row.data(), core.data(), root.data(), a, b, i, eps_sq);
            const int64_t c = r < 0 ? -1 : std::lower_bound(reps.begin(), reps.end(), r) - reps.begin();
            labels[o] = (int32_t)(c >= 0 && c < (int64_t)reps.size() ? c : -1);
            if (labels[o] >= 0) ++size[(size_t)labels[o]];
        }
        if (keep) {
            const int32_t best = largest_of(size.data(), (int64_t)size.size());
            for (int64_t r = a; r < b; ++r) keep[r] = best >= 0 && labels[r] == best ? 1 : 0;
            if (kept) kept[s] = best >= 0 ? size[(size_t)best] : 0;
        }
    }
    return flags;
}

}  // namespace dbscan
}  // namespace mspa
