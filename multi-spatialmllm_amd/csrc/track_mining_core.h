// The frame-pair rule of the object-movement head's pair mining (OM_C:465-567; mspa/heads.py: object_movement_mine_pairs),
// stated once for the kernels of track_mining.hip and any host check.  A plain C++ build of this header is the reference.
//
//   For a point, `frames` is the ascending list of the frames it is visible in (V of them) and the pairs are (i, j), i < j, in
//   row-major order.
//   * d = sqrt((dx*dx + dy*dy) + dz*dz) of position[j] - position[i]: K5c's expression, no contraction (-ffp-contract=off);
//   * a pair is DROPPED when (double)frames[i] > d + future_frame_windows (upstream's test as written, OM_C:505-507);
//   * otherwise it is STATIC when d < object_not_moving_threshold and MOVING if not (a NaN distance is moving);
//   * a moving pair's bin is min(#{e in edges[0..10] : e <= d} - 1, 9): np.digitize, then min(.., 9).  The 11 edges come from the
//     host (np.histogram_bin_edges of the point's smallest and largest moving distance);
//   * the moving pairs are ordered by (key, payload): key = the bit pattern of d (monotone for finite d >= 0), payload =
//     (i << 16) | j, which ascends in row-major order -- upstream's stable sort by d.
#pragma once
#include <stdint.h>
#include <string.h>

#ifndef MSPA_HD
#ifdef __HIPCC__
#define MSPA_HD __host__ __device__ __forceinline__
#else
#define MSPA_HD inline
#endif
#endif

namespace mspa {
namespace track_mining {

constexpr int32_t kBins = 10;
constexpr int32_t kEdges = kBins + 1;
constexpr int32_t kStatic = kBins;           // the class of a pick: a bin 0..9, or the static pairs
constexpr int32_t kClasses = kBins + 1;
constexpr int32_t kMaxFrames = 65535;        // i and j share a 32-bit payload
enum { kDropped = 0, kIsStatic = 1, kIsMoving = 2 };
// one point's record of the statistics pass (int64 each)
enum { kStatV = 0, kStatStatic, kStatMoving, kStatMinBits, kStatMaxBits, kStatFlags, kStatWords };
constexpr int64_t kFlagNonFinite = 1;        // a moving distance that is NaN or inf: upstream's histogram_bin_edges raises
constexpr int64_t kFlagBadPoint = 2;         // the point index lies outside the track

MSPA_HD double pair_distance(const double *a, const double *b) {
    const double dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
    return __builtin_sqrt((dx * dx + dy * dy) + dz * dz);
}

MSPA_HD int32_t classify(double d, int32_t frame_i, double threshold, double window) {
    if ((double)frame_i > d + window) return kDropped;
    return d < threshold ? kIsStatic : kIsMoving;
}

MSPA_HD int32_t bin_of(double d, const double *edges) {
    int32_t n = 0;
    for (int32_t e = 0; e < kEdges; ++e) n += edges[e] <= d ? 1 : 0;
    return n - 1 < kBins - 1 ? n - 1 : kBins - 1;
}

MSPA_HD uint64_t key_of(double d) {
    uint64_t k;
    memcpy(&k, &d, 8);
    return k;
}

MSPA_HD bool key_finite(uint64_t k) { return (k & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }

MSPA_HD uint32_t payload_of(int32_t i, int32_t j) { return ((uint32_t)i << 16) | (uint32_t)j; }

MSPA_HD int64_t pair_count(int32_t V) { return V < 2 ? 0 : (int64_t)V * (V - 1) / 2; }

// (i, j) -> the pair n >= 0 places later in row-major order; false once that is past the last pair (i, j are then meaningless).
MSPA_HD bool advance(int32_t &i, int32_t &j, int32_t V, int64_t n) {
    while (i < V - 1) {
        const int64_t left = V - j;              // pairs (i, j) .. (i, V - 1)
        if (n < left) {
            j += (int32_t)n;
            return true;
        }
        n -= left;
        ++i;
        j = i + 1;
    }
    return false;
}

}  // namespace track_mining
}  // namespace mspa
