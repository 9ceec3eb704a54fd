// Frame-pair mining of the object-movement head (OM_C:465-567) ON the MI355X: the rule is csrc/track_mining_core.h, the draws
// stay on the host (mspa/heads.py: plan_track_draws), and what crosses the bus is counts one way and picked frame pairs the other.
//
//   statistics   a workgroup per point: its visible frames and its positions there, compacted in frame order (ballot ranks, wave
//                totals through LDS), then a walk over its V (V - 1) / 2 pairs, 256 at a step: the static and the moving count,
//                the smallest and the largest moving distance as bit patterns, a non-finite flag.  Distances are recomputed
//                wherever they are needed, never stored.
//   bin counts   the same walk once the host has turned (min, max) into 11 edges: ten counts per point, by wave ballots.
//   order        a workgroup per SELECTED point: its moving pairs compacted in row-major order to (key, payload), then sorted.
//   sort         one workgroup per segment, LSD radix of 8 bits a pass over the two halves of the (key, payload) buffers.  A wave
//                owns a contiguous sixteenth of the segment and walks it in order, so every pass is stable; the lanes of a step
//                that share a digit find each other with 8 ballots.  One OR-reduction up front tells which digits vary over the
//                segment: the others are skipped (the exponent bytes of distances of one point, usually), and so are the payload's
//                when the caller says the input ascends in it already (the compaction's order).
//   resolve      a wave per pick: a bin pick is the payload at (bin start + rank) of the sorted segment, a static pick a walk
//                over the point's pairs that counts static ones up to the rank.
// Every count is an integer sum over ballots, every min / max an integer one: nothing depends on the order of execution.  No
// atomics on global memory; every store is checked against the extent of the buffer it goes to.
#include "mspa_common.h"
#include "track_mining_core.h"

namespace mspa {
namespace track_mining {

constexpr int kBlock = 256, kWaves = kBlock / 64;
constexpr int kSortBlock = 1024, kSortWaves = kSortBlock / 64;
constexpr int kDigits = 12;                  // 4 payload bytes, then 8 key bytes: least significant first

template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
    for (int m = 32; m; m >>= 1) v = op(v, __shfl_xor(v, m, 64));
    return v;
}

__device__ __forceinline__ int32_t clamp_frames(int64_t v, int32_t T) { return v < 0 ? 0 : v > T ? T : (int32_t)v; }

__global__ __launch_bounds__(kBlock) void stats_kernel(const double *__restrict__ world, const uint8_t *__restrict__ visibility, int32_t T,
                                                       int32_t P, const int32_t *__restrict__ points, double threshold, double window,
                                                       int32_t *frames_out, double *pos_out, int64_t *__restrict__ stats) {
    __shared__ int32_t s_wave[kWaves];
    __shared__ unsigned long long s_red[kWaves][5];
    const int32_t row = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint64_t below = (1ull << lane) - 1;
    const int32_t p = points[row];
    const bool bad = p < 0 || p >= P;
    int32_t *frames = frames_out + (int64_t)row * T;
    double *pos = pos_out + (int64_t)row * T * 3;
    int32_t V = 0;
    for (int32_t t0 = 0; t0 < T && !bad; t0 += kBlock) {         // block-uniform
        const int32_t t = t0 + tid;
        const bool on = t < T && visibility[(int64_t)t * P + p] != 0;
        const uint64_t b = __ballot(on);
        if (lane == 0) s_wave[wave] = __popcll(b);
        __syncthreads();
        int32_t base = V, total = 0;
#pragma unroll
        for (int32_t w = 0; w < kWaves; ++w) {
            const int32_t c = s_wave[w];
            base += w < wave ? c : 0;
            total += c;
        }
        if (on) {
            const int32_t at = base + __popcll(b & below);       // < T: one slot per visible frame
            const double *src = world + ((int64_t)t * P + p) * 3;
            frames[at] = t;
            pos[3 * at] = src[0];
            pos[3 * at + 1] = src[1];
            pos[3 * at + 2] = src[2];
        }
        V += total;
        __syncthreads();
    }
    __syncthreads();                                             // the lists are read back by every lane
    unsigned long long n_static = 0, n_moving = 0, kmin = ~0ull, kmax = 0, flags = bad ? kFlagBadPoint : 0;
    int32_t i = 0, j = 1;
    bool valid = advance(i, j, V, tid);
    while (valid) {
        const double d = pair_distance(pos + 3 * i, pos + 3 * j);
        const int32_t c = classify(d, frames[i], threshold, window);
        n_static += c == kIsStatic;
        if (c == kIsMoving) {
            const uint64_t k = key_of(d);
            ++n_moving;
            if (!key_finite(k)) flags |= kFlagNonFinite;
            kmin = k < kmin ? k : kmin;
            kmax = k > kmax ? k : kmax;
        }
        valid = advance(i, j, V, kBlock);
    }
    typedef unsigned long long u64;
    n_static = wave_reduce(n_static, [](u64 a, u64 b) { return a + b; });
    n_moving = wave_reduce(n_moving, [](u64 a, u64 b) { return a + b; });
    kmin = wave_reduce(kmin, [](u64 a, u64 b) { return a < b ? a : b; });
    kmax = wave_reduce(kmax, [](u64 a, u64 b) { return a > b ? a : b; });
    flags = wave_reduce(flags, [](u64 a, u64 b) { return a | b; });
    if (lane == 0) {
        s_red[wave][0] = n_static;
        s_red[wave][1] = n_moving;
        s_red[wave][2] = kmin;
        s_red[wave][3] = kmax;
        s_red[wave][4] = flags;
    }
    __syncthreads();
    if (tid == 0) {
        for (int32_t w = 1; w < kWaves; ++w) {
            n_static += s_red[w][0];
            n_moving += s_red[w][1];
            kmin = s_red[w][2] < kmin ? s_red[w][2] : kmin;
            kmax = s_red[w][3] > kmax ? s_red[w][3] : kmax;
            flags |= s_red[w][4];
        }
        int64_t *o = stats + (int64_t)row * kStatWords;
        o[kStatV] = V;
        o[kStatStatic] = (int64_t)n_static;
        o[kStatMoving] = (int64_t)n_moving;
        o[kStatMinBits] = (int64_t)kmin;
        o[kStatMaxBits] = (int64_t)kmax;
        o[kStatFlags] = (int64_t)flags;
    }
}

__global__ __launch_bounds__(kBlock) void bin_counts_kernel(const int32_t *__restrict__ frames_all, const double *__restrict__ pos_all,
                                                            const int64_t *__restrict__ stats, int32_t T, const double *__restrict__ edges,
                                                            double threshold, double window, int32_t *__restrict__ out) {
    __shared__ double s_edges[kEdges];
    __shared__ int32_t s_count[kWaves][kBins];
    const int32_t row = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid < kEdges) s_edges[tid] = edges[(int64_t)row * kEdges + tid];
    __syncthreads();
    const int32_t V = clamp_frames(stats[(int64_t)row * kStatWords + kStatV], T);
    const int32_t *__restrict__ frames = frames_all + (int64_t)row * T;
    const double *__restrict__ pos = pos_all + (int64_t)row * T * 3;
    const int64_t steps = (pair_count(V) + kBlock - 1) / kBlock;
    int32_t count[kBins] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int32_t i = 0, j = 1;
    bool valid = advance(i, j, V, tid);
    for (int64_t s = 0; s < steps; ++s) {                        // block-uniform: the ballots see whole waves
        int32_t bin = -1;
        if (valid) {
            const double d = pair_distance(pos + 3 * i, pos + 3 * j);
            if (classify(d, frames[i], threshold, window) == kIsMoving) bin = bin_of(d, s_edges);
        }
#pragma unroll
        for (int32_t b = 0; b < kBins; ++b) count[b] += __popcll(__ballot(bin == b));
        valid = valid && advance(i, j, V, kBlock);
    }
    if (lane == 0) {
#pragma unroll
        for (int32_t b = 0; b < kBins; ++b) s_count[wave][b] = count[b];
    }
    __syncthreads();
    if (tid < kBins) {
        int32_t c = 0;
        for (int32_t w = 0; w < kWaves; ++w) c += s_count[w][tid];
        out[(int64_t)row * kBins + tid] = c;
    }
}

// Sorts (ka, pa)[0, n) by (key, payload) in place; (kb, pb) is the other half of the ping-pong.  Called by a whole workgroup of
// kSortBlock lanes with block-uniform arguments.
__device__ __forceinline__ void segment_sort(uint64_t *ka, uint32_t *pa, uint64_t *kb, uint32_t *pb, int32_t n, bool payload_ordered) {
    __shared__ int32_t s_next[kSortWaves][256];
    __shared__ int32_t s_wave_total[4];
    __shared__ unsigned long long s_key_bits;
    __shared__ uint32_t s_payload_bits;
    if (n < 2) return;
    const int32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint64_t below = (1ull << lane) - 1;
    if (tid == 0) {
        s_key_bits = 0;
        s_payload_bits = 0;
    }
    __syncthreads();
    {   // which bits differ anywhere in the segment: a permutation does not change that
        const uint64_t k0 = ka[0];
        const uint32_t p0 = pa[0];
        unsigned long long kbits = 0;
        uint32_t pbits = 0;
        for (int32_t at = tid; at < n; at += kSortBlock) {
            kbits |= ka[at] ^ k0;
            pbits |= pa[at] ^ p0;
        }
        kbits = wave_reduce(kbits, [](unsigned long long a, unsigned long long b) { return a | b; });
        pbits = wave_reduce(pbits, [](uint32_t a, uint32_t b) { return a | b; });
        if (lane == 0) {
            atomicOr(&s_key_bits, kbits);
            atomicOr(&s_payload_bits, pbits);
        }
    }
    __syncthreads();
    const uint64_t key_bits = s_key_bits;
    const uint32_t payload_bits = payload_ordered ? 0u : s_payload_bits;
    const int32_t per = (int32_t)((((int64_t)n + kSortBlock - 1) / kSortBlock) * 64);      // a wave's share: whole steps
    const int64_t begin64 = (int64_t)wave * per;
    const int32_t begin = begin64 < n ? (int32_t)begin64 : n, end = begin64 + per < n ? (int32_t)(begin64 + per) : n;
    int32_t *next = s_next[wave];
    uint64_t *ksrc = ka, *kdst = kb;
    uint32_t *psrc = pa, *pdst = pb;
    for (int32_t pass = 0; pass < kDigits; ++pass) {
        const bool of_key = pass >= 4;
        const int32_t shift = 8 * (of_key ? pass - 4 : pass);
        if ((((of_key ? key_bits : (uint64_t)payload_bits) >> shift) & 0xff) == 0) continue;     // constant over the segment
        for (int32_t d = lane; d < 256; d += 64) next[d] = 0;
        wave_lds_fence();
        for (int32_t at = begin; at < end; at += 64) {
            const int32_t e = at + lane;
            if (e < end) atomicAdd(&next[(int32_t)(((of_key ? ksrc[e] : (uint64_t)psrc[e]) >> shift) & 0xff)], 1);
        }
        __syncthreads();
        int32_t mine = 0, incl = 0;
        if (tid < 256) {                                         // digit tid: the waves' counts become their starts inside the digit
            for (int32_t w = 0; w < kSortWaves; ++w) {
                const int32_t c = s_next[w][tid];
                s_next[w][tid] = mine;
                mine += c;
            }
            incl = mine;
#pragma unroll
            for (int32_t m = 1; m < 64; m <<= 1) {
                const int32_t up = __shfl_up(incl, m, 64);
                incl += lane >= m ? up : 0;
            }
            if (lane == 63) s_wave_total[wave] = incl;
        }
        __syncthreads();
        if (tid < 256) {
            int32_t start = incl - mine;
            for (int32_t w = 0; w < wave; ++w) start += s_wave_total[w];
            for (int32_t w = 0; w < kSortWaves; ++w) s_next[w][tid] += start;
        }
        __syncthreads();
        for (int32_t at = begin; at < end; at += 64) {           // wave-uniform
            const int32_t e = at + lane;
            const bool on = e < end;
            const uint64_t k = on ? ksrc[e] : 0;
            const uint32_t p = on ? psrc[e] : 0;
            const int32_t d = (int32_t)(((of_key ? k : (uint64_t)p) >> shift) & 0xff);
            uint64_t equals = __ballot(on);
#pragma unroll
            for (int32_t bit = 0; bit < 8; ++bit) {
                const bool set = (d >> bit) & 1;
                const uint64_t b = __ballot(on && set);
                equals &= set ? b : ~b;
            }
            const int32_t rank = __popcll(equals & below);
            const int32_t dest = on ? next[d] + rank : -1;
            wave_lds_fence();
            if (on && rank == 0) next[d] = dest + __popcll(equals);
            wave_lds_fence();
            if (dest >= 0 && dest < n) {
                kdst[dest] = k;
                pdst[dest] = p;
            }
        }
        __syncthreads();
        uint64_t *kt = ksrc;
        ksrc = kdst;
        kdst = kt;
        uint32_t *pt = psrc;
        psrc = pdst;
        pdst = pt;
    }
    if (ksrc != ka) {
        for (int32_t at = tid; at < n; at += kSortBlock) {
            ka[at] = ksrc[at];
            pa[at] = psrc[at];
        }
    }
}

struct Segment {
    int64_t begin, n;
    bool ok;
};

__device__ __forceinline__ Segment segment_of(const int64_t *__restrict__ seg_offsets, int64_t s, int64_t total) {
    const int64_t a = seg_offsets[s], b = seg_offsets[s + 1];
    Segment g;
    g.ok = a >= 0 && b >= a && b <= total && b - a <= 0x7fffffffLL;
    g.begin = a;
    g.n = g.ok ? b - a : 0;
    return g;
}

__global__ __launch_bounds__(kSortBlock) void sort_kernel(uint64_t *keys, uint32_t *payload, const int64_t *__restrict__ seg_offsets,
                                                          int64_t total, int32_t payload_ordered) {
    const Segment g = segment_of(seg_offsets, blockIdx.x, total);
    if (!g.ok) return;                                           // block-uniform
    segment_sort(keys + g.begin, payload + g.begin, keys + total + g.begin, payload + total + g.begin, (int32_t)g.n, payload_ordered != 0);
}

__global__ __launch_bounds__(kSortBlock) void order_kernel(const int32_t *__restrict__ frames_all, const double *__restrict__ pos_all,
                                                           const int64_t *__restrict__ stats, int32_t T, int32_t n_points,
                                                           const int32_t *__restrict__ rows, const int64_t *__restrict__ seg_offsets,
                                                           int64_t total, double threshold, double window, uint64_t *keys,
                                                           uint32_t *payload) {
    __shared__ int32_t s_wave[kSortWaves];
    const int32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint64_t below = (1ull << lane) - 1;
    const int32_t row = rows[blockIdx.x];
    const Segment g = segment_of(seg_offsets, blockIdx.x, total);
    if (!g.ok || row < 0 || row >= n_points) return;             // block-uniform
    uint64_t *ka = keys + g.begin;
    uint32_t *pa = payload + g.begin;
    const int32_t V = clamp_frames(stats[(int64_t)row * kStatWords + kStatV], T);
    const int32_t *__restrict__ frames = frames_all + (int64_t)row * T;
    const double *__restrict__ pos = pos_all + (int64_t)row * T * 3;
    const int64_t steps = (pair_count(V) + kSortBlock - 1) / kSortBlock;
    int64_t filled = 0;
    int32_t i = 0, j = 1;
    bool valid = advance(i, j, V, tid);
    for (int64_t s = 0; s < steps; ++s) {                        // block-uniform
        double d = 0.0;
        bool moving = false;
        if (valid) {
            d = pair_distance(pos + 3 * i, pos + 3 * j);
            moving = classify(d, frames[i], threshold, window) == kIsMoving;
        }
        const uint64_t b = __ballot(moving);
        if (lane == 0) s_wave[wave] = __popcll(b);
        __syncthreads();
        int64_t at = filled;
        int32_t step_total = 0;
#pragma unroll
        for (int32_t w = 0; w < kSortWaves; ++w) {
            const int32_t c = s_wave[w];
            at += w < wave ? c : 0;
            step_total += c;
        }
        at += __popcll(b & below);
        if (moving && at < g.n) {
            ka[at] = key_of(d);
            pa[at] = payload_of(i, j);
        }
        filled += step_total;
        valid = valid && advance(i, j, V, kSortBlock);
        __syncthreads();
    }
    for (int64_t at = filled + tid; at < g.n; at += kSortBlock) {   // a segment longer than the point's moving pairs: a defined tail
        ka[at] = ~0ull;
        pa[at] = ~0u;
    }
    __syncthreads();
    segment_sort(ka, pa, keys + total + g.begin, payload + total + g.begin, (int32_t)g.n, true);
}

__global__ __launch_bounds__(64) void resolve_kernel(const int32_t *__restrict__ frames_all, const double *__restrict__ pos_all,
                                                     const int64_t *__restrict__ stats, const int32_t *__restrict__ bin_counts, int32_t T,
                                                     int32_t n_points, const int32_t *__restrict__ rows,
                                                     const int64_t *__restrict__ seg_offsets, int32_t n_selected,
                                                     const uint32_t *__restrict__ payload, int64_t total, const int32_t *__restrict__ picks,
                                                     double threshold, double window, int32_t *__restrict__ out) {
    const int64_t k = blockIdx.x;
    const int32_t lane = threadIdx.x;
    const uint64_t below = (1ull << lane) - 1;
    const int32_t sel = picks[3 * k], cls = picks[3 * k + 1], rank = picks[3 * k + 2];
    bool found = false;
    if (sel >= 0 && sel < n_selected && cls >= 0 && cls < kClasses && rank >= 0) {          // wave-uniform throughout
        const int32_t row = rows[sel];
        if (row >= 0 && row < n_points) {
            const int32_t V = clamp_frames(stats[(int64_t)row * kStatWords + kStatV], T);
            const int32_t *__restrict__ frames = frames_all + (int64_t)row * T;
            if (cls < kBins) {
                const Segment g = segment_of(seg_offsets, sel, total);
                int64_t at = rank;
                for (int32_t b = 0; b < cls; ++b) at += bin_counts[(int64_t)row * kBins + b];
                if (g.ok && rank < bin_counts[(int64_t)row * kBins + cls] && at < g.n) {
                    const uint32_t pl = payload[g.begin + at];
                    const int32_t i = (int32_t)(pl >> 16), j = (int32_t)(pl & 0xffff);
                    if (i < j && j < V) {
                        found = true;
                        if (lane == 0) {
                            out[2 * k] = frames[i];
                            out[2 * k + 1] = frames[j];
                        }
                    }
                }
            } else {
                const double *__restrict__ pos = pos_all + (int64_t)row * T * 3;
                const int64_t steps = (pair_count(V) + 63) / 64;
                int64_t seen = 0;
                int32_t i = 0, j = 1;
                bool valid = advance(i, j, V, lane);
                for (int64_t s = 0; s < steps && !found; ++s) {
                    const bool is_static = valid && classify(pair_distance(pos + 3 * i, pos + 3 * j), frames[i], threshold, window) == kIsStatic;
                    const uint64_t b = __ballot(is_static);
                    const int32_t c = __popcll(b);
                    if (rank < seen + c) {
                        found = true;
                        if (is_static && __popcll(b & below) == rank - seen) {
                            out[2 * k] = frames[i];
                            out[2 * k + 1] = frames[j];
                        }
                    }
                    seen += c;
                    valid = valid && advance(i, j, V, 64);
                }
            }
        }
    }
    if (!found && lane == 0) out[2 * k] = out[2 * k + 1] = -1;
}

}  // namespace track_mining
}  // namespace mspa

using namespace mspa;


static bool bad_extents(int32_t T, int32_t n_points) { return T < 0 || T > track_mining::kMaxFrames || n_points < 0; }

extern "C" int mspa_track_pair_stats(const double *world, const uint8_t *visibility, int32_t T, int32_t P, const int32_t *points,
                                     int32_t n_points, double object_not_moving_threshold, double future_frame_windows,
                                     int32_t *out_frames, double *out_positions, int64_t *out_stats, mspa_stream_t stream) {
    if (bad_extents(T, n_points) || P < 0) return fail(MSPA_EINVAL, "mspa_track_pair_stats: 0 <= T <= 65535, 0 <= P, 0 <= n_points");
    if (n_points == 0) return MSPA_OK;
    if (!points || !out_stats || (T > 0 && (!out_frames || !out_positions)) || (T > 0 && P > 0 && (!world || !visibility)))
        return fail(MSPA_EINVAL, "mspa_track_pair_stats: null pointer");
    hipLaunchKernelGGL(track_mining::stats_kernel, dim3((unsigned)n_points), dim3(track_mining::kBlock), 0, (hipStream_t)stream, world, visibility, T, P, points,
                       object_not_moving_threshold, future_frame_windows, out_frames, out_positions, out_stats);
    return check_hip(hipGetLastError(), "mspa_track_pair_stats");
}

extern "C" int mspa_track_pair_bin_counts(const int32_t *frames, const double *positions, const int64_t *stats, int32_t T, int32_t n_points,
                                          const double *edges, double object_not_moving_threshold, double future_frame_windows,
                                          int32_t *out_bin_counts, mspa_stream_t stream) {
    if (bad_extents(T, n_points)) return fail(MSPA_EINVAL, "mspa_track_pair_bin_counts: 0 <= T <= 65535, 0 <= n_points");
    if (n_points == 0) return MSPA_OK;
    if (!stats || !edges || !out_bin_counts || (T > 0 && (!frames || !positions))) return fail(MSPA_EINVAL, "mspa_track_pair_bin_counts: null pointer");
    hipLaunchKernelGGL(track_mining::bin_counts_kernel, dim3((unsigned)n_points), dim3(track_mining::kBlock), 0, (hipStream_t)stream, frames, positions, stats, T, edges,
                       object_not_moving_threshold, future_frame_windows, out_bin_counts);
    return check_hip(hipGetLastError(), "mspa_track_pair_bin_counts");
}

extern "C" int mspa_track_pair_sort(uint64_t *keys, uint32_t *payload, const int64_t *seg_offsets, int64_t n_segments, int64_t n_total,
                                    int32_t payload_ordered, mspa_stream_t stream) {
    if (n_segments < 0 || n_segments > 0x7fffffffLL || n_total < 0) return fail(MSPA_EINVAL, "mspa_track_pair_sort: 0 <= n_segments < 2^31, 0 <= n_total");
    if (n_segments == 0 || n_total == 0) return MSPA_OK;
    if (!keys || !payload || !seg_offsets) return fail(MSPA_EINVAL, "mspa_track_pair_sort: null pointer");
    hipLaunchKernelGGL(track_mining::sort_kernel, dim3((unsigned)n_segments), dim3(track_mining::kSortBlock), 0, (hipStream_t)stream, keys, payload, seg_offsets, n_total,
                       payload_ordered);
    return check_hip(hipGetLastError(), "mspa_track_pair_sort");
}

extern "C" int mspa_track_pair_order(const int32_t *frames, const double *positions, const int64_t *stats, int32_t T, int32_t n_points,
                                     const int32_t *rows, const int64_t *seg_offsets, int32_t n_selected, int64_t n_total,
                                     double object_not_moving_threshold, double future_frame_windows, uint64_t *keys, uint32_t *payload,
                                     mspa_stream_t stream) {
    if (bad_extents(T, n_points) || n_selected < 0 || n_total < 0)
        return fail(MSPA_EINVAL, "mspa_track_pair_order: 0 <= T <= 65535, 0 <= n_points, 0 <= n_selected, 0 <= n_total");
    if (n_selected == 0 || n_total == 0) return MSPA_OK;
    if (!frames || !positions || !stats || !rows || !seg_offsets || !keys || !payload) return fail(MSPA_EINVAL, "mspa_track_pair_order: null pointer");
    hipLaunchKernelGGL(track_mining::order_kernel, dim3((unsigned)n_selected), dim3(track_mining::kSortBlock), 0, (hipStream_t)stream, frames, positions, stats, T, n_points,
                       rows, seg_offsets, n_total, object_not_moving_threshold, future_frame_windows, keys, payload);
    return check_hip(hipGetLastError(), "mspa_track_pair_order");
}

extern "C" int mspa_track_pair_resolve(const int32_t *frames, const double *positions, const int64_t *stats, const int32_t *bin_counts, int32_t T,
                                       int32_t n_points, const int32_t *rows, const int64_t *seg_offsets, int32_t n_selected,
                                       const uint32_t *payload, int64_t n_total, const int32_t *picks_host, const int32_t *class_counts_host,
                                       const int32_t *picks, int64_t n_picks, double object_not_moving_threshold, double future_frame_windows,
                                       int32_t *out_frame_pairs, mspa_stream_t stream) {
    if (bad_extents(T, n_points) || n_selected < 0 || n_total < 0 || n_picks < 0 || n_picks > 0x7fffffffLL)
        return fail(MSPA_EINVAL, "mspa_track_pair_resolve: 0 <= T <= 65535, 0 <= n_points, 0 <= n_selected, 0 <= n_total, 0 <= n_picks < 2^31");
    if (n_picks == 0) return MSPA_OK;
    if (!picks_host || !class_counts_host) return fail(MSPA_EINVAL, "mspa_track_pair_resolve: null pointer");
    for (int64_t k = 0; k < n_picks; ++k) {
        const int32_t sel = picks_host[3 * k], cls = picks_host[3 * k + 1], rank = picks_host[3 * k + 2];
        if (sel < 0 || sel >= n_selected || cls < 0 || cls >= track_mining::kClasses)
            return fail(MSPA_EINVAL, "mspa_track_pair_resolve: pick " + std::to_string(k) + " names no selected point or no class");
        if (rank < 0 || rank >= class_counts_host[(int64_t)sel * track_mining::kClasses + cls])
            return fail(MSPA_EINVAL, "mspa_track_pair_resolve: pick " + std::to_string(k) + ": rank " + std::to_string(rank) + " of a class of " +
                                         std::to_string(class_counts_host[(int64_t)sel * track_mining::kClasses + cls]));
    }
    if (!frames || !positions || !stats || !bin_counts || !rows || !seg_offsets || !picks || !out_frame_pairs || (n_total > 0 && !payload))
        return fail(MSPA_EINVAL, "mspa_track_pair_resolve: null pointer");
    hipLaunchKernelGGL(track_mining::resolve_kernel, dim3((unsigned)n_picks), dim3(64), 0, (hipStream_t)stream, frames, positions, stats, bin_counts, T, n_points,
                       rows, seg_offsets, n_selected, payload, n_total, picks, object_not_moving_threshold, future_frame_windows, out_frame_pairs);
    return check_hip(hipGetLastError(), "mspa_track_pair_resolve");
}
