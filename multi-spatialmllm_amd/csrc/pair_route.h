// K3's launch decision as plain host arithmetic: which of pair_reproject.hip's kernels a call gets and how its grid is tiled.
//
// Plain C++17, no HIP: pair_reproject.hip includes it for the kernels' template arguments, their __launch_bounds__ and the
// one launch site, and tests/test_pair_route_cpu.py builds it with g++ and walks route() over shapes, output sets and flags
// without a GPU.  Everything that answers "fused or dense?", "which instantiation?", "how many tiles?" asks route(); the
// instantiations that exist are kKeys, and pair_reproject.hip generates its kernel table from that array, so a key that
// route() returns and a kernel that is compiled cannot drift apart (the CPU test checks that the two sets are equal).
#pragma once
#include <stdint.h>

#include "../../include/mspa.h"

namespace mspa {

constexpr int kWave = 64;

// Output sets.  A kernel instantiated with GENERIC = true tests every output pointer at run time
// (wave-uniform branches); the specialised instances know their set at compile time, which frees
// ~20 SGPRs of pointers and removes the dead stores' address arithmetic.
enum : uint32_t {
    O_VIS_BITS = 1u << 0, O_VIS_U8 = 1u << 1, O_VALID_U8 = 1u << 2, O_PIX = 1u << 3, O_XYZ32 = 1u << 4,
    O_RGBA = 1u << 5, O_XYZ64 = 1u << 6, O_UV64 = 1u << 7, O_DEPTH64 = 1u << 8, O_COUNTS = 1u << 9, O_CPIX = 1u << 10,
};
constexpr uint32_t kSetCorr = O_VIS_BITS | O_PIX | O_COUNTS;                         // correspondence
constexpr uint32_t kSetDense = O_VIS_U8 | O_PIX | O_XYZ32 | O_RGBA | O_COUNTS;       // coloured point cloud
constexpr uint32_t kSetDenseXyz = O_VIS_U8 | O_PIX | O_XYZ32 | O_COUNTS;              // point cloud without colour (rgb = 0)
constexpr uint32_t kSetMinimal = O_VIS_BITS | O_COUNTS;                              // overlap only
constexpr uint32_t kSetCompact = O_VIS_BITS | O_CPIX | O_COUNTS;                     // correspondences of the visible pixels only

constexpr int kThreads = 256;
constexpr int kIters = 16;                       // 4096 pixels per workgroup
constexpr int kStrip = kThreads * kIters;

constexpr int kTileRows = 16;                    // a wave owns a 64-column x 16-row tile
constexpr int kRowGroup = 4;                     // rows whose depth-2 gathers are in flight together

constexpr int kTightRows = 48;                         // tile height of the correspondence family (= MSPA_CORR_TILE_H)
// The dense sets carry a 3 KB transpose stage per wave: with 48-row tiles that is 36 KB of LDS per workgroup (four per CU),
// with 32-row tiles 28 KB (five): measured 1.22 -> 1.17 ms per 1 000 pairs (dense without colour words, tools/ab_k3.py)
constexpr int kTightRowsDense = 32;
// rows whose depth-2 gathers are in flight together: the sets without a transpose stage (minimal, compact) may take more
constexpr int tight_rg_of(uint32_t set) { return (set & (O_PIX | O_XYZ32 | O_RGBA | O_VIS_U8)) ? kRowGroup : 4; }
// Tile height of the SCALED form (no LDS tile: height costs no occupancy; one lane per tile row holds its visibility word, so
// 64 at most).  A tile's fixed work -- box scan, composition, culling test, ~400 VALU issues and their round trips -- is paid
// per tile whatever it goes on to do, and at ScanNet's shape about half the tiles are culled: the minimal set runs 10 % faster
// on 64-row tiles (1.298 vs 1.445 ms per 1 000 pairs), the correspondence set 7 % slower (1.821 vs 1.708: coarser culling
// writes more of its index table), tools/ab_scannet.py round 5.  The compacted set's tile is part of the API (48).
constexpr int kScaledRows = 48;
constexpr int kScaledRowsNoPix = 64;
// A wave of the SCALED form takes ONE tile.  Walking several vertically adjacent tiles per wave -- launch, the pair's matrices,
// the column's depth-grid offsets and the other per-stripe constants paid once for them, the culling still per tile -- was
// measured at ScanNet's shape (tools/ab_scannet.py, round 5, ms per 1 000 pairs at 1 / 2 / 3 / 4 tiles) and rejected:
// corr 1.745 / 2.102 / 2.125 / 2.256, minimal 1.349 / 2.021 / 2.055 / 1.996 -- bit-identical and 20-50 % SLOWER: what was live
// across the tile loop cost the row loop its registers (minimal: 42 VGPRs spilled to scratch in it).  For the compacted set
// it never worked at all: with its spills the SGPR quad of the inline-asm `idxen` store came back wrong (memory fault).
constexpr int tight_rows_of(uint32_t set, bool scaled = false) {
    return (set & (O_XYZ32 | O_RGBA | O_VIS_U8)) ? kTightRowsDense
           : (scaled && !(set & O_CPIX)) ? ((set & O_PIX) ? kScaledRows : kScaledRowsNoPix) : kTightRows;
}
// waves (= tiles) per workgroup, per output set (tools/ab_k3.py, one box, ms per 1 000 pairs at 1 / 2 / 4 / 8 waves): the sets
// without an index table like small workgroups -- a workgroup's LDS is released only when its slowest tile is done --
// minimal 0.325 / 0.309 / 0.319 / 0.351, compact 0.388 / 0.377 / 0.388 / 0.424; corr 0.525 / 0.505 / 0.503 / 0.558; the dense
// point set without colour a large one, dense_xyz 1.303 / 1.200 / 1.149 / 1.132 (with colour words 4 stay better than 8:
// 1.572 vs 1.587).
// The SCALED form (no LDS depth tile: a workgroup's size costs no occupancy) runs best at four for every set
// (tools/ab_scannet.py at ScanNet's shape, ms per 1 000 pairs at 1 / 2 / 4 / 8 waves: minimal 2.76 / 1.94 / 1.55-1.63 / 1.63,
// compact 3.03 / 2.18 / 1.93 / 2.01, corr 2.55 / - / 1.72-1.80 / 1.79).
constexpr int tight_bw_of(uint32_t set, bool scaled = false) {
    return scaled ? 4
           : (set & O_RGBA) ? 4
           : (set & (O_XYZ32 | O_VIS_U8)) ? 8
           : (set & O_PIX) ? 4 : 2;
}
// waves per SIMD the register allocator must leave room for (second argument of __launch_bounds__): the sets without an
// index table run best at six (80 VGPRs); round 4's guard-band bookkeeping had pushed `minimal` to 82 = five waves, +5 %
// (the SCALED correspondence set sat at 97 VGPRs = four waves: held at five; the whole-tile correspondence set is not held)
constexpr int tight_minwaves_of(uint32_t set, bool scaled) {
    return (set & (O_XYZ32 | O_RGBA | O_VIS_U8)) ? 1
           : (set & O_PIX) ? (scaled ? 5 : 1)
           : 6;
}

// image sizes every K3 entry point takes
constexpr bool size_ok(int32_t h, int32_t w) { return h >= 2 && w >= 2 && h <= 32767 && w <= 32767; }

// 64 x 48 tiles of the compacted correspondence output (include/mspa.h, mspa_corr_tiles)
constexpr int corr_stripes(int32_t W) { return (W + MSPA_CORR_TILE_W - 1) / MSPA_CORR_TILE_W; }
constexpr int corr_tiles(int32_t H, int32_t W) { return corr_stripes(W) * ((H + MSPA_CORR_TILE_H - 1) / MSPA_CORR_TILE_H); }

// whole-tile shapes the tight kernel takes (W % 64 == 0, H % 48 == 0, colour grid == depth grid, 32-bit byte offsets)
constexpr bool tight_shape(int32_t dh, int32_t dw, int32_t H, int32_t W, int rows = kTightRows) {
    return dh == H && dw == W && (W % 64 == 0) && (H % rows == 0) && ((uint64_t)H * (uint64_t)W * 4 < (1ull << 31));
}

// shapes the tight kernel takes in its SCALED form (rectangular tiles on a colour grid at least as fine as the depth grid):
// bitset rows in whole 16-bit pieces, whole 4-row groups, depth rows in whole 8-byte pieces, 32-bit byte offsets
constexpr bool rect_shape(int32_t dh, int32_t dw, int32_t H, int32_t W) {
    return !tight_shape(dh, dw, H, W) && dw <= W && dh <= H && (W % 16 == 0) && (H % 4 == 0) && (dw % 4 == 0) && (dh % 2 == 0) &&
           ((uint64_t)H * (uint64_t)W * 4 < (1ull << 31)) && ((uint64_t)dh * (uint64_t)dw * 2 < (1ull << 31));
}

// One instantiation.  A field a kernel is not templated on is false / 0 in its key: the exact kernel has `ident` only, the
// tight kernel `set`, `scaled` and `stream` only.  set == 0 is the GENERIC form, which tests its output pointers at run time.
enum KernelKind : uint8_t { kKernelExact, kKernelFast, kKernelTight };
struct Key {
    KernelKind kernel;
    uint32_t set;
    bool ident;          // colour grid == depth grid
    bool whole_tiles;    // fast kernel: W % 64 == 0 and H % kTileRows == 0, no edge predicates
    bool linear;         // fast kernel: 64 consecutive pixel indices per wave row (bitset on a width that is not a multiple of 64)
    bool scaled;         // tight kernel: rectangular tiles over a colour grid that differs from the depth grid
    bool stream;         // tight kernel: MSPA_PAIR_STREAM
};
constexpr bool operator==(const Key &a, const Key &b) {
    return a.kernel == b.kernel && a.set == b.set && a.ident == b.ident && a.whole_tiles == b.whole_tiles && a.linear == b.linear &&
           a.scaled == b.scaled && a.stream == b.stream;
}
constexpr Key exact_key(bool ident) { return {kKernelExact, 0u, ident, false, false, false, false}; }
constexpr Key fast_key(bool ident, bool whole_tiles, uint32_t set, bool linear = false) {
    return {kKernelFast, set, ident, whole_tiles, linear, false, false};
}
constexpr Key tight_key(uint32_t set, bool stream, bool scaled = false) { return {kKernelTight, set, false, false, false, scaled, stream}; }

// Every instantiation of the three kernels that exists: pair_reproject.hip compiles exactly these.
constexpr Key kKeys[] = {
    exact_key(true), exact_key(false),
    fast_key(true, true, kSetCorr), fast_key(true, true, kSetDense), fast_key(true, true, kSetMinimal), fast_key(true, true, 0u),
    fast_key(true, false, kSetCorr, true), fast_key(true, false, kSetMinimal, true), fast_key(true, false, 0u, true),
    fast_key(false, false, kSetCorr, true), fast_key(false, false, kSetMinimal, true), fast_key(false, false, 0u, true),
    fast_key(true, false, 0u), fast_key(false, false, 0u),
    tight_key(kSetCorr, false), tight_key(kSetCorr, true), tight_key(kSetDense, false), tight_key(kSetDense, true),
    tight_key(kSetDenseXyz, false), tight_key(kSetDenseXyz, true), tight_key(kSetMinimal, false), tight_key(kSetMinimal, true),
    tight_key(kSetCompact, false), tight_key(kSetCompact, true),
    tight_key(kSetCorr, false, true), tight_key(kSetCorr, true, true), tight_key(kSetMinimal, false, true),
    tight_key(kSetMinimal, true, true), tight_key(kSetCompact, false, true), tight_key(kSetCompact, true, true),
};
constexpr int kNumKeys = (int)(sizeof(kKeys) / sizeof(kKeys[0]));
static_assert(kNumKeys == 30, "2 exact, 12 fast, 16 tight (10 whole-tile, 6 rectangular)");

constexpr int key_index(const Key &k) {
    for (int i = 0; i < kNumKeys; ++i)
        if (kKeys[i] == k) return i;
    return -1;
}

enum RouteError { kRouteOk = 0, kRouteBadSize, kRouteTooLarge, kRouteBadFlag, kRouteNeedsTight };
constexpr const char *route_error_text(RouteError e) {
    return e == kRouteBadSize ? "mspa_pair_reproject: image size out of range [2, 32767]"
           : e == kRouteTooLarge ? "mspa_pair_reproject: H*W*W must be < 2^32"
           : e == kRouteBadFlag ? "mspa_pair_reproject: unknown flag"
           : e == kRouteNeedsTight ? "pair_reproject_impl: the fused compacted set needs the tight kernel and a tile-count table"
                                   : "";
}

struct Route {
    RouteError err;      // every such call fails with MSPA_EINVAL and route_error_text(err); the other fields hold when it is kRouteOk
    int family;          // MSPA_KERNEL_PAIR_*
    Key key;
    int rows;            // tile height (0: the exact kernel has no tiles)
    int waves, threads;  // per workgroup
    int n_stripes;       // 64-column stripes per row band
    int n_tiles;         // wave tiles per pair
    int groups;          // workgroups per pair: the exact kernel's 4096-pixel strips, the others' groups of `waves` wave tiles
};

// dh x dw depth grid under an H x W colour grid; `outputs` has the O_* bit of every output the call produces (O_CPIX: the
// compacted set, which only the tight kernel writes); `aligned`: every pointer meets the tight kernel's alignment (its
// LDS-DMA moves depth in 4-byte units and its 16-byte stores need aligned outputs); `flags`: MSPA_PAIR_*.
constexpr Route route(int32_t dh, int32_t dw, int32_t H, int32_t W, uint32_t outputs, bool aligned, uint32_t flags) {
    Route r = {};
    if (!size_ok(dh, dw) || !size_ok(H, W)) return r.err = kRouteBadSize, r;
    const uint64_t P = (uint64_t)H * (uint64_t)W;
    if (P * (uint64_t)W >= (1ull << 32)) return r.err = kRouteTooLarge, r;
    if (flags & ~(MSPA_PAIR_FAST | MSPA_PAIR_STREAM | MSPA_PAIR_WORD_STRIPES)) return r.err = kRouteBadFlag, r;
    const bool ident = (dh == H && dw == W);
    // float64 outputs are defined as the reference's own operation order: they force the exact kernel
    // ... and so does a depth grid LARGER than the colour grid (sx or sy > 1; no dataset has one): the guard band is built from
    // colour-grid quantities and its half-guard margin is only argued for sx, sy <= 1.
    const bool fast = (flags & MSPA_PAIR_FAST) && !(outputs & (O_XYZ64 | O_UV64 | O_DEPTH64)) && dw <= W && dh <= H;
    const uint32_t set = outputs;
    // bitset on a width that is not a multiple of 64: the LINEAR mapping, whose wave rows are whole words of the bitset (the
    // stripe mapping would need two atomicOr per wave-row there)
    const bool linear = fast && (set & O_VIS_BITS) && (W % 64 != 0);
    const bool tight = fast && aligned && tight_shape(dh, dw, H, W, tight_rows_of(set)) &&
                       (set == kSetCorr || set == kSetDense || set == kSetDenseXyz || set == kSetMinimal || set == kSetCompact);
    // The tight kernel's SCALED form (rectangular tiles) takes the correspondence / minimal / compacted sets on every
    // rect_shape, ScanNet's own (1296 x 968 colour over 640 x 480 depth) included: at four waves per workgroup it beat rounds
    // 2-3's word-stripe kernel for that shape (corr 1.72-1.80 vs 1.90-2.05, minimal 1.55-1.63 vs 1.64-1.69 ms per 1 000 pairs,
    // profiles/r04_ab_scannet.txt, r05_ab_scannet*.txt), which was removed; MSPA_PAIR_WORD_STRIPES, which selected it, is ignored
    const bool rect = fast && !tight && aligned && rect_shape(dh, dw, H, W) &&
                      (set == kSetCompact || set == kSetCorr || set == kSetMinimal);
    if ((set & O_CPIX) && !(tight || rect)) return r.err = kRouteNeedsTight, r;
    if (!fast) {
        r.family = MSPA_KERNEL_PAIR_EXACT;
        r.key = exact_key(ident);
        r.waves = kThreads / kWave;
        r.groups = (int)((P + kStrip - 1) / kStrip);
    } else {
        const bool stream = (flags & MSPA_PAIR_STREAM) != 0;
        const bool whole = ident && (W % 64 == 0) && (H % kTileRows == 0);   // the BASELINE shape: 640x480 colour == depth
        r.family = rect ? MSPA_KERNEL_PAIR_FAST_RECT
                   : tight ? MSPA_KERNEL_PAIR_FAST_TIGHT
                   : linear ? MSPA_KERNEL_PAIR_FAST_LINEAR : MSPA_KERNEL_PAIR_FAST;
        r.key = (rect || tight) ? tight_key(set, stream, rect)
                : whole ? fast_key(true, true, (set == kSetCorr || set == kSetDense || set == kSetMinimal) ? set : 0u)
                : linear ? fast_key(ident, false, (set == kSetCorr || set == kSetMinimal) ? set : 0u, true)
                         : fast_key(ident, false, 0u);
        r.rows = (rect || tight) ? tight_rows_of(set, rect) : kTileRows;
        r.waves = (rect || tight) ? tight_bw_of(set, rect) : kThreads / kWave;
        r.n_stripes = (W + 63) / 64;
        r.n_tiles = (linear && !rect) ? (int)((P + (uint64_t)kTileRows * 64 - 1) / ((uint64_t)kTileRows * 64))
                                      : r.n_stripes * ((H + r.rows - 1) / r.rows);
        r.groups = (r.n_tiles + r.waves - 1) / r.waves;
    }
    r.threads = r.waves * kWave;
    return r;
}

}  // namespace mspa
