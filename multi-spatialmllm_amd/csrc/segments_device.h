// The device passes that any op over the RAGGED BATCH of cloud_segments_core.h uses (rows [N, C] on the device plus host offsets
// [S + 1]), each stated once for cloud_segments.hip, voxel_segments.hip and dbscan_segments.hip: the one check of the offsets, the
// flag compaction and the tiled extents pass.  An op brings its own predicate (a functor over a row or slot index) and its own
// workspace; what it launches from here has the same text for every op with the same predicate.
#pragma once
#include "mspa_common.h"
#include "cloud_segments_core.h"

namespace mspa {
namespace segs {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int kRounds = 8;
constexpr int64_t kFlagTile = (int64_t)kBlock * kRounds;         // slots one workgroup of the compaction takes

// ---- the batch on the host side of an entry point -----------------------------------------------------------------------------

// N of a batch an entry point takes, or -1 with the error text set, `who` in front.
inline int64_t checked_rows(const char *who, const int64_t *offsets_host, int64_t S) {
    const int64_t N = batch_rows(offsets_host, S);
    if (N < 0)
        fail(MSPA_EINVAL, std::string(who) + ": offsets must be [S + 1] with offsets[0] = 0, ascending, at most 2^30 rows and 2^24 segments");
    return N;
}

// The tiles of a batch's extents pass: tile_base[S] without the table.
inline int64_t extent_tiles(const int64_t *offsets, int64_t S) {
    int64_t T = 0;
    for (int64_t s = 0; s < S; ++s) T += tiles_of(offsets[s + 1] - offsets[s]);
    return T;
}

inline bool misaligned(const void *p, uintptr_t to) { return ((uintptr_t)p & (to - 1)) != 0; }

// ---- the fold of K sums through LDS -------------------------------------------------------------------------------------------

// partial [K][kLanes] in LDS, every thread j of a workgroup of kLanes has written its own K entries: segs::ordered_sum's fold of all K
// sums at once -- partial[k][j] += partial[k][j + stride] for every j < stride, strides kLanes / 2, ..., 1, one barrier a stride --
// with the K totals in every thread afterwards and partial[] free again.
template <int K>
__device__ __forceinline__ void fold_sums(double (*partial)[kLanes], int32_t j, double total[K]) {
    __syncthreads();
    for (int32_t s = kLanes / 2; s >= 1; s >>= 1) {
        if (j < s)
            for (int k = 0; k < K; ++k) partial[k][j] = partial[k][j] + partial[k][j + s];
        __syncthreads();
    }
    for (int k = 0; k < K; ++k) total[k] = partial[k][0];
    __syncthreads();
}

// ---- the flag compaction ------------------------------------------------------------------------------------------------------

// The indices i in [0, n) with flag(i), in ascending order: per tile of kFlagTile slots a count (wave ballots), one workgroup's
// exclusive scan over the tiles, then every flagged slot's position = tile base + rounds before + waves before + its rank below in
// the wave's ballot.  No atomic hands out a position.
template <typename Flag>
__global__ void __launch_bounds__(kBlock) flag_count_kernel(Flag flag, int64_t n, int32_t *__restrict__ tile_counts) {
    __shared__ int32_t wcnt[kWaves];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    int32_t count = 0;
    for (int r = 0; r < kRounds; ++r) {
        const int64_t i = (int64_t)blockIdx.x * kFlagTile + (int64_t)r * kBlock + tid;
        count += __popcll(__ballot(i < n && flag(i)));
    }
    if (lane == 0) wcnt[w] = count;
    __syncthreads();
    if (tid == 0) {
        int32_t all = 0;
#pragma unroll
        for (int e = 0; e < kWaves; ++e) all += wcnt[e];
        tile_counts[blockIdx.x] = all;
    }
}

// One workgroup: tile_counts [T] -> their exclusive prefix, in place; the total to *total and, where list is given, list[total] = end.
// The template parameter means nothing.  It is there for the linkage of a kernel defined in a header: a plain __global__ function
// would be emitted, and its host stub defined, in every file that includes this one, whether the file compacts anything or not.
template <typename = void>
__global__ void __launch_bounds__(kBlock) tile_scan_kernel(int32_t *__restrict__ tile_counts, int64_t T, int64_t *__restrict__ total,
                                                           int64_t *__restrict__ list, int64_t end) {
    __shared__ int64_t chunk_sum[kBlock];
    const int tid = (int)threadIdx.x;
    const int64_t per = (T + kBlock - 1) / kBlock;
    const int64_t a = tid * per < T ? tid * per : T, b = a + per < T ? a + per : T;
    int64_t sum = 0;
    for (int64_t t = a; t < b; ++t) sum += tile_counts[t];
    chunk_sum[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        int64_t run = 0;
        for (int e = 0; e < kBlock; ++e) {
            const int64_t c = chunk_sum[e];
            chunk_sum[e] = run;
            run += c;
        }
        *total = run;
        if (list) list[run] = end;
    }
    __syncthreads();
    int64_t run = chunk_sum[tid];
    for (int64_t t = a; t < b; ++t) {
        const int32_t c = tile_counts[t];
        tile_counts[t] = (int32_t)run;
        run += c;
    }
}

template <typename Flag>
__global__ void __launch_bounds__(kBlock) flag_place_kernel(Flag flag, int64_t n, const int32_t *__restrict__ tile_base, int64_t *__restrict__ list) {
    __shared__ int32_t wcnt[kWaves];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    int64_t run = tile_base[blockIdx.x];
    for (int r = 0; r < kRounds; ++r) {
        const int64_t i = (int64_t)blockIdx.x * kFlagTile + (int64_t)r * kBlock + tid;
        const bool set = i < n && flag(i);
        const uint64_t m = __ballot(set);
        if (lane == 0) wcnt[w] = __popcll(m);
        __syncthreads();
        int32_t before = 0, all = 0;
#pragma unroll
        for (int e = 0; e < kWaves; ++e) {
            before += e < w ? wcnt[e] : 0;
            all += wcnt[e];
        }
        if (set) list[run + before + __popcll(m & (((uint64_t)1 << lane) - 1))] = i;
        run += all;
        __syncthreads();
    }
}

// list [total] <- the flagged indices below n, *total their number; with_end also list[total] = n.  tile_counts holds one int32 per
// tile of kFlagTile slots.  Three launches.
template <typename Flag>
void compact(Flag flag, int64_t n, int32_t *tile_counts, int64_t *total, int64_t *list, bool with_end, hipStream_t st) {
    const int64_t T = (n + kFlagTile - 1) / kFlagTile;
    hipLaunchKernelGGL(flag_count_kernel<Flag>, dim3((unsigned)T), dim3(kBlock), 0, st, flag, n, tile_counts);
    hipLaunchKernelGGL(tile_scan_kernel<>, dim3(1), dim3(kBlock), 0, st, tile_counts, T, total, with_end ? list : (int64_t *)nullptr, n);
    hipLaunchKernelGGL(flag_place_kernel<Flag>, dim3((unsigned)T), dim3(kBlock), 0, st, flag, n, (const int32_t *)tile_counts, list);
}

// ---- the tiled extents pass ---------------------------------------------------------------------------------------------------

struct TakeAll {                                                 // every row counts
    __device__ __forceinline__ bool operator()(int64_t) const { return true; }
};

// One workgroup per tile of kExtentTile rows of ONE segment (tile_base: the host's prefix of the segments' tiles), so a segment of
// 1.5 M rows is 367 workgroups, not one.  part [T, 3 * kEnds]: per tile the minimum of the taken rows' x, y, z and, with kEnds = 2,
// the minimum of their negations behind it (so one fold serves both ends); +inf where the tile has no taken row.
template <int kEnds, typename Take>
__global__ void __launch_bounds__(kBlock) extent_tiles_kernel(const double *__restrict__ rows, int64_t C, const int64_t *__restrict__ offsets,
                                                              const int64_t *__restrict__ tile_base, int64_t S, double *__restrict__ part,
                                                              Take take) {
    constexpr int kOut = 3 * kEnds;
    __shared__ double mins[kWaves][kOut];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t t = blockIdx.x;
    const int64_t s = segment_of(tile_base, S, t);
    const int64_t a = offsets[s] + (t - tile_base[s]) * kExtentTile;
    const int64_t end = offsets[s + 1], b = a + kExtentTile < end ? a + kExtentTile : end;
    double m[kOut];
#pragma unroll
    for (int e = 0; e < kOut; ++e) m[e] = INFINITY;
    for (int64_t i = a + tid; i < b; i += kBlock) {
        if (!take(i)) continue;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const double x = rows[i * C + ax];
            m[ax] = x < m[ax] ? x : m[ax];
            if constexpr (kEnds == 2) m[3 + ax] = -x < m[3 + ax] ? -x : m[3 + ax];
        }
    }
#pragma unroll
    for (int e = 0; e < kOut; ++e) {
        const double v = wave_min(m[e]);
        if (lane == 0) mins[w][e] = v;
    }
    __syncthreads();
    if (tid < kOut) {
        double v = mins[0][tid];
#pragma unroll
        for (int e = 1; e < kWaves; ++e) v = mins[e][tid] < v ? mins[e][tid] : v;
        part[t * kOut + tid] = v;
    }
}

// One wave per segment: the minimum over its tiles (min is order-independent) -> lo [S, 3] and, with kEnds = 2, the negated second
// half -> hi [S, 3] (hi is not read with kEnds = 1); +inf / -inf for a segment without a taken row.
template <int kEnds>
__global__ void __launch_bounds__(kWave) extent_fold_kernel(const double *__restrict__ part, const int64_t *__restrict__ tile_base,
                                                            double *__restrict__ lo, double *__restrict__ hi) {
    constexpr int kOut = 3 * kEnds;
    const int lane = (int)threadIdx.x;
    const int64_t s = blockIdx.x;
    const int64_t a = tile_base[s], b = tile_base[s + 1];
    double m[kOut];
#pragma unroll
    for (int e = 0; e < kOut; ++e) m[e] = INFINITY;
    for (int64_t t = a + lane; t < b; t += kWave) {
#pragma unroll
        for (int e = 0; e < kOut; ++e) m[e] = part[t * kOut + e] < m[e] ? part[t * kOut + e] : m[e];
    }
#pragma unroll
    for (int e = 0; e < kOut; ++e) {
        const double v = wave_min(m[e]);
        if (lane == e) (e < 3 ? lo : hi)[s * 3 + e % 3] = e < 3 ? v : -v;
    }
}

}  // namespace segs
}  // namespace mspa
