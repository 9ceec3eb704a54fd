// The stable split of a frame's valid pixels by instance label: ONE statement of the rule and of the decomposition the kernels of
// csrc/instance_split.hip use, so that the CPU tests can check the stability argument without a GPU.
//
// The rule.  labels [F, P] uint8 (0 = nothing; object `target_id` is label `target_id + 1`), valid [F, P] uint8.  Pixel p of frame
// f is SELECTED when label != 0 and valid != 0.  Segment (f, v) holds the selected pixels of frame f with label v in ascending
// pixel index -- `np.flatnonzero((labels[f] == v) & valid[f])`, the order `np.where(mask)` gives the reference's
// project_mask_to_3d -- and the segments follow each other in (frame, label) order.
//
// The decomposition.  A frame is cut into tiles of kTile consecutive pixels; a tile is walked in kTile / kBlock rounds of kBlock
// consecutive pixels, a round by kBlock / 64 waves of 64 consecutive pixels.  The row of a selected pixel is
//     offsets[f * 256 + v]                       the segment's start (exclusive prefix of the counts)
//   + tile_base[f][tile][v]                      selected pixels of (f, v) in EARLIER tiles (exclusive scan of the tile histograms)
//   + selected pixels of (f, v) in earlier rounds of this tile and in earlier waves of this round
//   + rank(mask, lane)                           those in lower lanes of its own wave: popcount(ballot & lanes below)
// Every term counts pixels with a SMALLER index and the same (f, v), and together they count all of them once: the row is the
// pixel's rank in its segment whatever order tiles, rounds' waves or lanes are executed in.  No term depends on an arrival order.
#pragma once
#include <stdint.h>

#include <limits>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MSPA_SPLIT_HD __host__ __device__ __forceinline__
#else
#define MSPA_SPLIT_HD inline
#endif

namespace mspa {
namespace split {

constexpr int kLabels = 256;
constexpr int kBlock = 256;                      // pixels of a round: the workgroup's threads
constexpr int kWaves = kBlock / 64;
constexpr int kTile = 4096;                      // pixels of a tile
constexpr int kRounds = kTile / kBlock;

MSPA_SPLIT_HD int64_t tiles(int64_t P) { return (P + kTile - 1) / kTile; }
MSPA_SPLIT_HD bool selected(uint8_t label, uint8_t valid) { return label != 0 && valid != 0; }
// rank of `lane` among the set bits of a wave's ballot
MSPA_SPLIT_HD int rank_below(uint64_t mask, int lane) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(mask & ((1ull << lane) - 1ull));
#else
    return __builtin_popcountll(mask & ((1ull << lane) - 1ull));
#endif
}
// int32 words of the workspace: the tile histograms, turned into tile bases by the first call
MSPA_SPLIT_HD int64_t workspace_words(int64_t F, int64_t P) { return F * tiles(P) * kLabels; }

// ---- the host restatement of the kernels' decomposition ------------------------------------------------------------------------
// pass 1: tile histograms -> counts [F, 256] and tile bases (in place in `work`, workspace_words(F, P) int32)
inline void count_host(const uint8_t *labels, const uint8_t *valid, int64_t F, int64_t P, int32_t *counts, int32_t *work) {
    const int64_t T = tiles(P);
    for (int64_t i = 0; i < F * T * kLabels; ++i) work[i] = 0;
    for (int64_t f = 0; f < F; ++f)
        for (int64_t p = 0; p < P; ++p)
            if (selected(labels[f * P + p], valid[f * P + p])) ++work[(f * T + p / kTile) * kLabels + labels[f * P + p]];
    for (int64_t f = 0; f < F; ++f)
        for (int v = 0; v < kLabels; ++v) {
            int32_t run = 0;
            for (int64_t t = 0; t < T; ++t) {
                int32_t &slot = work[(f * T + t) * kLabels + v];
                const int32_t n = slot;
                slot = run;
                run += n;
            }
            counts[f * kLabels + v] = run;
        }
}

// pass 2: the scatter, wave by wave with ballots as masks.  `reversed` walks the tiles from the last to the first and, inside a
// round, ranks the waves' pixels in the order 3, 2, 1, 0: an execution order the device is free to take -- the output must not change.
// rgb (or null) is [F, P, 3]; lo / hi [F, 256, 3] are written for every segment (+inf / -inf where it is empty).
inline void scatter_host(const uint8_t *labels, const uint8_t *valid, const double *xyz, const uint8_t *rgb, int64_t F, int64_t P,
                         const int64_t *offsets, const int32_t *work, double *out_xyz, uint8_t *out_rgb, int32_t *out_pixel,
                         double *out_lo, double *out_hi, bool reversed) {
    const int64_t T = tiles(P);
    const double inf = std::numeric_limits<double>::infinity();
    for (int64_t i = 0; i < F * kLabels * 3; ++i) { out_lo[i] = inf; out_hi[i] = -inf; }
    for (int64_t f = 0; f < F; ++f) {
        for (int64_t tt = 0; tt < T; ++tt) {
            const int64_t t = reversed ? T - 1 - tt : tt;
            int64_t run[kLabels];
            for (int v = 0; v < kLabels; ++v) run[v] = offsets[f * kLabels + v] + work[(f * T + t) * kLabels + v];
            for (int r = 0; r < kRounds; ++r) {
                int32_t wcnt[kWaves][kLabels] = {};
                int64_t dest[kBlock];
                for (int ww = 0; ww < kWaves; ++ww) {
                    const int w = reversed ? kWaves - 1 - ww : ww;
                    const int64_t p0 = t * kTile + (int64_t)r * kBlock + w * 64;
                    uint64_t todo = 0;
                    for (int l = 0; l < 64; ++l)
                        if (p0 + l < P && selected(labels[f * P + p0 + l], valid[f * P + p0 + l])) todo |= 1ull << l;
                    while (todo) {
                        const int v = labels[f * P + p0 + __builtin_ctzll(todo)];
                        uint64_t m = 0;
                        for (int l = 0; l < 64; ++l)
                            if ((todo >> l & 1) && labels[f * P + p0 + l] == v) m |= 1ull << l;
                        for (int l = 0; l < 64; ++l)
                            if (m >> l & 1) dest[w * 64 + l] = rank_below(m, l);
                        wcnt[w][v] = __builtin_popcountll(m);
                        todo &= ~m;
                    }
                }
                for (int w = 0; w < kWaves; ++w)
                    for (int l = 0; l < 64; ++l) {
                        const int64_t p = t * kTile + (int64_t)r * kBlock + w * 64 + l;
                        if (p >= P || !selected(labels[f * P + p], valid[f * P + p])) continue;
                        const int v = labels[f * P + p];
                        int64_t row = run[v] + dest[w * 64 + l];
                        for (int e = 0; e < w; ++e) row += wcnt[e][v];
                        for (int k = 0; k < 3; ++k) {
                            const double c = xyz[(f * P + p) * 3 + k];
                            out_xyz[row * 3 + k] = c;
                            if (out_rgb) out_rgb[row * 3 + k] = rgb[(f * P + p) * 3 + k];
                            double &lo = out_lo[(f * kLabels + v) * 3 + k], &hi = out_hi[(f * kLabels + v) * 3 + k];
                            lo = c < lo ? c : lo;
                            hi = c > hi ? c : hi;
                        }
                        out_pixel[row] = (int32_t)p;
                    }
                for (int v = 0; v < kLabels; ++v)
                    for (int w = 0; w < kWaves; ++w) run[v] += wcnt[w][v];
            }
        }
    }
}

}  // namespace split
}  // namespace mspa
