// Average linkage and fcluster of one distance matrix: the arithmetic and the tie rules shared by the device kernel of
// track_linkage.hip and a plain C++ build (tests/test_linkage_cpu.py compares that build with SciPy on a CPU).  It restates
// SciPy 1.15's  fcluster(linkage(squareform(loss, checks=False), 'average'), t, criterion='distance'):
//   * linkage is the nearest-neighbour chain.  The chain starts at the lowest live cluster; the nearest neighbour of the chain
//     top x is the lowest i with the smallest D[x, i], except that the entry below the top keeps its place unless some i is
//     STRICTLY closer; two mutual neighbours merge into the higher index, the lower one dies, and every live row is updated as
//     (nx * D[i, x] + ny * D[i, y]) / (nx + ny) in float64, one rounding per written operation (build with -ffp-contract=off);
//   * the merges are stable-sorted by height (a counting rank: row j precedes row i when d_j < d_i, or d_j == d_i and j < i)
//     and relabelled with a union-find: (min root, max root), new cluster id = n + row, column 3 = merged size;
//   * fcluster takes the per-node maximum height over the subtree (kept here as the flag "maximum <= t", which is all the walk
//     asks) and walks the tree from the root with a stack, left child first; leaves are numbered when their parent is left for
//     good, so cluster numbers follow the post-order of internal nodes.
// The code is written once, over a context `Ctx` that supplies the lane's place in the team (tid, nthr), a team barrier and a
// team-wide argmin.  The host context is a team of one.  Every branch that decides control flow depends on team-uniform values
// only, so all lanes take the same path and meet at the same barriers.
//
// Loop bound.  A scan either pushes or stops.  Over one matrix there are n - 1 stops, and pushes are at most 2 (n - 1) + n, so
// the scans stay below 4 n; reaching 4 n ends the block with kIterationCap instead of hanging on a wrong tie rule.
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

namespace mspa {
namespace linkage {

constexpr int kMaxPoints = 2048;                 // MSPA_LINKAGE_MAX_POINTS: 6 n int32 of team-shared memory = 48 KiB
enum : int32_t { kOk = 0, kNonFinite = 1, kIterationCap = 2 };
constexpr int kNoIndex = 0x7fffffff;

// Team-shared int32 words one matrix needs (LDS on the device): size, chain | union-find parent and size, later the walk's state.
MSPA_HD int64_t shared_words(int n) { return 6 * (int64_t)n; }

// Per-matrix scratch in ordinary memory: the working matrix, then the raw merges and their order.
struct Scratch {
    double *W;          // [n, n] working copy, kept symmetric
    double *rd;         // [n] merge heights in merge order
    int32_t *rx, *ry;   // [n] merged pair (x < y) in merge order
    int32_t *order;     // [n] order[rank] = merge index
};
MSPA_HD int64_t scratch_bytes(int n) {
    const int64_t b = (int64_t)n * n * 8 + (int64_t)n * 8 + 3 * (int64_t)n * 4;
    return (b + 15) & ~(int64_t)15;
}
MSPA_HD Scratch carve(void *base, int n) {
    Scratch s;
    s.W = (double *)base;
    s.rd = s.W + (int64_t)n * n;
    s.rx = (int32_t *)(s.rd + n);
    s.ry = s.rx + n;
    s.order = s.ry + n;
    return s;
}

template <class Ctx>
MSPA_HD void give_up(Ctx &c, int n, int32_t code, double *Z, int32_t *labels, int32_t *status) {
    for (int i = c.tid; i < 4 * (n - 1); i += c.nthr) Z[i] = 0.0;
    for (int i = c.tid; i < n; i += c.nthr) labels[i] = 0;
    if (c.tid == 0) *status = code;
}

// One matrix, n >= 2.  loss [n, n] is read only (strict upper triangle); scratch >= scratch_bytes(n), 8-byte aligned; shared
// >= shared_words(n); Z [n - 1, 4], labels [n], status [1] are written in full.
template <class Ctx>
MSPA_HD void block(Ctx &c, const double *loss, int n, double threshold, void *scratch, int32_t *shared, double *Z,
                   int32_t *labels, int32_t *status) {
    const Scratch s = carve(scratch, n);
    int32_t *size = shared, *chain = shared + n, *uf = shared + 2 * (int64_t)n;
    const double kInf = __builtin_inf();

    // working copy: symmetric from the upper triangle, zero diagonal; any non-finite entry ends the block
    bool bad = false;
    for (int i = 0; i < n; ++i) {
        double *row = s.W + (int64_t)i * n;
        for (int j = c.tid; j < n; j += c.nthr) {
            const double v = i == j ? 0.0 : (i < j ? loss[(int64_t)i * n + j] : loss[(int64_t)j * n + i]);
            bad |= !__builtin_isfinite(v);
            row[j] = v;
        }
    }
    for (int i = c.tid; i < n; i += c.nthr) size[i] = 1;
    if (c.any(bad)) {                                   // (barrier inside: W and size are visible to the team from here)
        give_up(c, n, kNonFinite, Z, labels, status);
        return;
    }

    // ---- nearest-neighbour chain ----------------------------------------------------------------------------------------
    int len = 0, scans = 0, lowest = 0;
    for (int k = 0; k < n - 1; ++k) {
        int x, below = -1;                              // chain top and the entry below it
        if (len == 0) {
            while (size[lowest] == 0) ++lowest;         // live indices only ever die, so the lowest one only moves up
            x = lowest;
            if (c.tid == 0) chain[0] = x;
            len = 1;
        } else {
            x = chain[len - 1];
            if (len >= 2) below = chain[len - 2];
        }
        double cur;
        int y;
        for (;;) {
            if (scans == 4 * n) {
                give_up(c, n, kIterationCap, Z, labels, status);
                return;
            }
            ++scans;
            const double *row = s.W + (int64_t)x * n;
            const double kept = len >= 2 ? row[below] : kInf;
            double bv = kInf;
            int bi = kNoIndex;
            for (int i = c.tid; i < n; i += c.nthr)
                if (size[i] > 0 && i != x) {
                    const double d = row[i];
                    if (d < bv) { bv = d; bi = i; }
                }
            c.argmin(bv, bi);
            if (bi >= n) {                              // no live neighbour: cannot happen for finite input
                give_up(c, n, kIterationCap, Z, labels, status);
                return;
            }
            if (len >= 2 && !(bv < kept)) { cur = kept; y = below; }
            else { cur = bv; y = bi; }
            if (len >= 2 && y == below) break;
            if (c.tid == 0) chain[len] = y;
            ++len;
            below = x;
            x = y;
        }
        len -= 2;
        if (x > y) { const int t = x; x = y; y = t; }
        const int nx = size[x], ny = size[y];
        c.sync();                                       // every lane has nx and ny before lane 0 overwrites them
        if (c.tid == 0) {
            size[x] = 0;
            size[y] = nx + ny;
            s.rx[k] = x;
            s.ry[k] = y;
            s.rd[k] = cur;
        }
        double *rowx = s.W + (int64_t)x * n, *rowy = s.W + (int64_t)y * n;
        const double dnx = (double)nx, dny = (double)ny, dn = (double)(nx + ny);
        for (int i = c.tid; i < n; i += c.nthr)
            if (i != x && i != y && size[i] > 0) {
                const double v = (dnx * rowx[i] + dny * rowy[i]) / dn;
                rowy[i] = v;
                s.W[(int64_t)i * n + y] = v;
            }
        c.sync();                                       // the updated row / column and sizes, before the next scan
    }

    // ---- stable sort by height, union-find relabelling ------------------------------------------------------------------
    const int m = n - 1;
    int32_t *left = size, *right = chain;               // both dead now: every lane is past the last barrier above
    int32_t *parent = uf, *usize = uf + 2 * (int64_t)n;
    for (int i = c.tid; i < m; i += c.nthr) {
        const double di = s.rd[i];
        int r = 0;
        for (int j = 0; j < m; ++j) {
            const double dj = s.rd[j];
            r += (dj < di || (dj == di && j < i)) ? 1 : 0;
        }
        s.order[r] = i;
        left[r] = s.rx[i];
        right[r] = s.ry[i];
    }
    for (int i = c.tid; i < 2 * n - 1; i += c.nthr) { parent[i] = i; usize[i] = 1; }
    c.sync();
    if (c.tid == 0) {
        for (int r = 0; r < m; ++r) {
            int root[2];
            for (int e = 0; e < 2; ++e) {
                int p = e ? right[r] : left[r], q = p;
                while (parent[q] != q) q = parent[q];
                while (parent[p] != q) { const int up = parent[p]; parent[p] = q; p = up; }
                root[e] = q;
            }
            left[r] = root[0] < root[1] ? root[0] : root[1];
            right[r] = root[0] < root[1] ? root[1] : root[0];
            parent[root[0]] = n + r;
            parent[root[1]] = n + r;
            usize[n + r] = usize[root[0]] + usize[root[1]];
        }
    }
    c.sync();

    // ---- Z, and the walk's state: stack, visited, "subtree maximum <= threshold" ---------------------------------------
    // The walk's three arrays sit in uf[0, 3 n): parent and the leaves' sizes, both dead; the merged sizes Z still needs are in
    // uf[3 n, 4 n).
    int32_t *stack = uf, *visited = uf + n, *under = uf + 2 * (int64_t)n;
    for (int r = c.tid; r < m; r += c.nthr) {
        const double d = s.rd[s.order[r]];
        Z[4 * (int64_t)r] = (double)left[r];
        Z[4 * (int64_t)r + 1] = (double)right[r];
        Z[4 * (int64_t)r + 2] = d;
        Z[4 * (int64_t)r + 3] = (double)usize[n + r];
        under[r] = d <= threshold ? 1 : 0;
        visited[r] = 0;
    }
    c.sync();
    if (c.tid == 0) {
        for (int r = 0; r < m; ++r) {                   // a child cluster n + j was made by an earlier row j < r
            const int l = left[r], rr = right[r];
            under[r] = under[r] & (l < n ? 1 : under[l - n]) & (rr < n ? 1 : under[rr - n]);
        }
        int k = 0, n_cluster = 0, leader = -1;
        stack[0] = 2 * n - 2;
        while (k >= 0) {
            const int root = stack[k] - n;
            const int l = left[root], rr = right[root];
            if (leader == -1 && under[root]) { leader = root; ++n_cluster; }
            if (l >= n && !visited[l - n]) { visited[l - n] = 1; stack[++k] = l; continue; }
            if (rr >= n && !visited[rr - n]) { visited[rr - n] = 1; stack[++k] = rr; continue; }
            if (l < n) { if (leader == -1) ++n_cluster; labels[l] = n_cluster; }
            if (rr < n) { if (leader == -1) ++n_cluster; labels[rr] = n_cluster; }
            if (leader == root) leader = -1;
            --k;
        }
        *status = kOk;
    }
}

}  // namespace linkage
}  // namespace mspa

#ifndef __HIPCC__
#include <vector>
namespace mspa {
namespace linkage {

struct HostCtx {                                        // a team of one
    int tid = 0, nthr = 1;
    void sync() {}
    void argmin(double &, int &) {}
    bool any(bool b) { return b; }
};

// One matrix on the host; returns the status.  n >= 2.
inline int32_t block_host(const double *loss, int n, double threshold, double *Z, int32_t *labels) {
    std::vector<double> scratch((size_t)(scratch_bytes(n) / 8));
    std::vector<int32_t> shared((size_t)shared_words(n));
    int32_t status = -1;
    HostCtx c;
    block(c, loss, n, threshold, scratch.data(), shared.data(), Z, labels, &status);
    return status;
}

}  // namespace linkage
}  // namespace mspa
#endif
