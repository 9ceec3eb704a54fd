// The pair table (`*_camera_info_D5.parquet`: 3 id strings and 4 doubles per frame pair) sampled ON the MI355X: its DOUBLE
// column chunks go from decompressed pages (csrc/snappy_decode.hip) to float64 columns, `overlap` to one class byte per row
// (csrc/pair_bins_core.h) and the classes to per-class lists of ascending file rows -- what mspa/pairtable.py draws from.
//
//   hybrid runs    one lane per RLE / bit-packed stream (csrc/rle_hybrid_core.h: definition levels of bit width 1, dictionary
//                  indices) walks the run headers, one step per run, and writes a run table: where each run's values go in
//                  the expanded output, where its bytes lie, how they are coded.  Called twice: to count, then to write.
//   hybrid expand  one lane per VALUE: a search for its run in the run table, then rle_hybrid's own value readers.
//   double layout  one lane per page: a v1 page's u32 level length, a dictionary-coded page's bit-width byte -> where the
//                  levels and the values lie.
//   double column  one lane per ROW: its page by a search in the pages' first rows, NaN for a null, else value k of the page
//                  (k = the row's rank among the non-nulls) -- 8 PLAIN bytes, or the dictionary entry its index names.
//   bin codes      a wave per tile of kTile rows, 64 consecutive rows a step (coalesced): the class byte, and the tile's count
//                  per class in an LDS table of the wave's own.  The count of a step is taken class by class with wave ballots:
//                  the first lane left names a class, the ballot of its equals is counted, those lanes leave.
//   partition      the same walk over the codes with the table preloaded with the tile's class OFFSETS (exclusive scan over
//                  tiles, class major: the caller's plumbing): a lane's place is the table entry plus the ballot bits below it,
//                  so every class list ascends in file order.
// Both row streams are bandwidth-bound (8 + 1 and 1 + 4 bytes per row; the class loop costs a few wave instructions per
// distinct class of a step).  No atomics; every load and store is checked against the buffer it goes to.
#include "mspa_common.h"
#include "snappy_core.h"
#include "rle_hybrid_core.h"
#include "pair_bins_core.h"

namespace mspa {
namespace pair_table {

constexpr int kTile = 2048;              // rows one wave takes: 32 steps of 64
constexpr int kWaves = 4;                // tiles a workgroup takes
constexpr int kBlock = 64 * kWaves;
constexpr int32_t kRunPacked = 1;        // run_info: bit 0 bit-packed, bit 1 a hole (a declined stream's rest), bits 8.. the bit width
constexpr int32_t kRunHole = 2;
constexpr int32_t kPageBounds = 1;       // layout: the tables do not describe the page, or a length runs past it
constexpr int32_t kPageValues = 5;       // column: a level, an index or a value the page does not hold
constexpr int32_t kLevelsInline = 1;     // page flags: v1, u32 length + RLE levels open the payload
constexpr int32_t kDictCoded = 2;        //             one byte of bit width + hybrid indices instead of PLAIN values
constexpr int32_t kLevelsGiven = 4;      //             v2: the caller says where the level bytes lie
enum { kLevOff = 0, kLevLen, kValOff, kValLen, kBitWidth, kLayoutRows };

__global__ __launch_bounds__(64) void hybrid_runs_kernel(const uint8_t *__restrict__ src, int64_t src_bytes, const int64_t *__restrict__ s_off,
                                                         const int64_t *__restrict__ s_len, const int64_t *__restrict__ s_bw,
                                                         const int64_t *__restrict__ s_values, const int64_t *__restrict__ out_begin,
                                                         const int64_t *__restrict__ run_begin, int64_t n_streams, int64_t n_runs,
                                                         int64_t *__restrict__ run_count, int32_t *__restrict__ status,
                                                         int32_t *__restrict__ const_value, int64_t *__restrict__ run_first,
                                                         int64_t *__restrict__ run_pos, int32_t *__restrict__ run_info) {
    const int64_t s = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (s >= n_streams) return;
    const int64_t off = s_off[s], len = s_len[s], bw = s_bw[s], nv = s_values[s], first0 = out_begin[s];
    int rc = 0;
    if (nv < 0 || off < 0 || len < 0 || off > src_bytes - len) rc = rle_hybrid::kErrRows;
    else if (bw < 0 || bw > 32) rc = rle_hybrid::kErrBitWidth;
    int64_t slot = 0, slot_end = 0;
    if (run_begin) {
        slot = run_begin[s];
        slot_end = run_begin[s + 1];
        if (slot < 0 || slot_end < slot || slot_end > n_runs) slot = slot_end = 0;          // a damaged table: nothing is written
    }
    const uint8_t *__restrict__ q = src + (rc ? 0 : off);
    int64_t covered = 0, p = 0, k = 0;
    int32_t cv = -1;
    while (!rc && covered < nv) {
        if (p >= len) {
            rc = rle_hybrid::kErrShort;
            break;
        }
        rle_hybrid::Run r;
        rc = rle_hybrid::parse_run(q, p, len, (int32_t)bw, r);
        if (rc) break;
        const int64_t count = r.count < nv - covered ? r.count : nv - covered;
        if (slot + k < slot_end) {
            run_first[slot + k] = first0 + covered;
            run_pos[slot + k] = off + p + r.head;
            run_info[slot + k] = (r.packed ? kRunPacked : 0) | ((int32_t)bw << 8);
        }
        if (k == 0 && !r.packed && count == nv) cv = rle_hybrid::rle_value(q + p + r.head, (int32_t)bw);
        ++k;
        covered += count;
        p += r.head + r.bytes;
    }
    if (rc && nv > 0) {                                          // what a declined stream did not give: one hole to its end
        if (slot + k < slot_end) {
            run_first[slot + k] = first0 + covered;
            run_pos[slot + k] = 0;
            run_info[slot + k] = kRunHole;
        }
        ++k;
        cv = -1;
    }
    run_count[s] = k;
    status[s] = rc;
    const_value[s] = cv;
}

__global__ __launch_bounds__(256) void hybrid_expand_kernel(const uint8_t *__restrict__ src, int64_t src_bytes,
                                                            const int64_t *__restrict__ run_first, const int64_t *__restrict__ run_pos,
                                                            const int32_t *__restrict__ run_info, int64_t n_runs, int64_t total,
                                                            int32_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    int32_t v = -1;
    if (run_first[0] <= i) {
        const int64_t r = last_at_or_below(run_first, n_runs, i);
        const int64_t k = i - run_first[r], pos = run_pos[r];
        const int32_t info = run_info[r], bw = info >> 8;
        if (!(info & kRunHole) && bw >= 0 && bw <= 32 && pos >= 0 && pos <= src_bytes) {
            if (info & kRunPacked) {
                const int64_t bit = k * bw;
                if ((bit >> 3) + ((int32_t)(bit & 7) + bw + 7) / 8 <= src_bytes - pos) v = rle_hybrid::packed_value(src + pos, k, bw);
            } else if ((bw + 7) / 8 <= src_bytes - pos) {
                v = rle_hybrid::rle_value(src + pos, bw);
            }
        }
    }
    out[i] = v;
}

__global__ __launch_bounds__(64) void double_layout_kernel(const uint8_t *__restrict__ pages, int64_t pages_bytes,
                                                           const int64_t *__restrict__ page_off, const int64_t *__restrict__ page_size,
                                                           const int32_t *__restrict__ page_flags, int64_t n_pages,
                                                           int64_t *__restrict__ layout, int32_t *__restrict__ page_status) {
    const int64_t pg = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (pg >= n_pages) return;
    const int64_t off = page_off[pg], size = page_size[pg];
    const int32_t flags = page_flags[pg];
    int64_t lev_off = 0, lev_len = 0, val_off = 0, val_len = 0, bw = 0, pos = 0;
    bool bad = off < 0 || size < 0 || off > pages_bytes - size;
    if (!bad && (flags & kLevelsGiven)) {
        lev_off = layout[kLevOff * n_pages + pg];
        lev_len = layout[kLevLen * n_pages + pg];
        bad = lev_off < 0 || lev_len < 0 || lev_off > pages_bytes - lev_len;
    } else if (!bad && (flags & kLevelsInline)) {
        bad = size < 4;
        if (!bad) {
            lev_len = snappy::load32(pages + off);
            lev_off = off + 4;
            pos = 4 + lev_len;
            bad = lev_len > size - 4;
        }
    }
    if (!bad && (flags & kDictCoded)) {
        bad = pos >= size;
        if (!bad) bw = pages[off + pos++];
    }
    if (!bad) {
        val_off = off + pos;
        val_len = size - pos;
    } else {
        lev_off = lev_len = bw = 0;
    }
    layout[kLevOff * n_pages + pg] = lev_off;
    layout[kLevLen * n_pages + pg] = lev_len;
    layout[kValOff * n_pages + pg] = val_off;
    layout[kValLen * n_pages + pg] = val_len;
    layout[kBitWidth * n_pages + pg] = bw;
    page_status[pg] = bad ? kPageBounds : 0;
}

// 8 bytes at base[at, at + 8), any alignment (the caller has checked 0 <= at <= bytes - 8): two aligned words where both lie
// inside the buffer, bytes otherwise.
__device__ __forceinline__ uint64_t load64(const uint8_t *__restrict__ base, int64_t at, int64_t bytes) {
    const uintptr_t a = (uintptr_t)(base + at), lo_at = a & ~(uintptr_t)7;
    const uint32_t shift = (uint32_t)(a & 7) * 8;
    if (shift == 0) return *(const uint64_t *)a;
    if (lo_at >= (uintptr_t)base && lo_at + 16 <= (uintptr_t)base + (uintptr_t)bytes) {
        const uint64_t lo = *(const uint64_t *)lo_at, hi = *(const uint64_t *)(lo_at + 8);
        return (lo >> shift) | (hi << (64 - shift));
    }
    uint64_t v = 0;
    for (int32_t b = 0; b < 8; ++b) v |= (uint64_t)base[at + b] << (8 * b);
    return v;
}

__global__ __launch_bounds__(256) void double_column_kernel(const uint8_t *__restrict__ pages, int64_t pages_bytes,
                                                            const int64_t *__restrict__ layout, const int64_t *__restrict__ page_values,
                                                            const int32_t *__restrict__ page_flags, const int64_t *__restrict__ page_first,
                                                            int64_t n_pages, const int32_t *__restrict__ levels,
                                                            const int64_t *__restrict__ level_rank, const int64_t *__restrict__ lev_begin,
                                                            int64_t n_levels, const int32_t *__restrict__ indices,
                                                            const int64_t *__restrict__ idx_begin, int64_t n_indices,
                                                            const int64_t *__restrict__ dict_off, const int64_t *__restrict__ dict_count,
                                                            uint64_t *__restrict__ out, int64_t n_out, int32_t *__restrict__ value_status) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_out) return;
    constexpr uint64_t kNaN = 0x7ff8000000000000ull;             // np.nan, what a null reads as
    if (page_first[0] > i) {
        out[i] = kNaN;
        value_status[0] = kPageValues;
        return;
    }
    const int64_t pg = last_at_or_below(page_first, n_pages, i);
    const int64_t r = i - page_first[pg], nv = page_values[pg];
    const int32_t flags = page_flags[pg];
    uint64_t v = kNaN;
    bool bad = r >= nv, null = false;
    int64_t k = r;
    if (!bad && levels && (flags & (kLevelsInline | kLevelsGiven))) {
        const int64_t l0 = lev_begin[pg];
        bad = l0 < 0 || l0 > n_levels - nv;
        if (!bad) {
            const int32_t level = levels[l0 + r];
            bad = level != 0 && level != 1;
            null = level == 0;
            k = level_rank[l0 + r] - level_rank[l0];             // the exclusive running sum: the non-nulls in front of this row
            bad = bad || k < 0 || k > r;
        }
    }
    if (!bad && !null) {
        if (flags & kDictCoded) {
            const int64_t x0 = idx_begin[pg], d0 = dict_off[pg], dn = dict_count[pg];
            bad = !indices || x0 < 0 || x0 > n_indices - nv || d0 < 0 || dn < 0 || dn > (pages_bytes - d0) / 8 || d0 > pages_bytes;
            if (!bad) {
                const int64_t idx = indices[x0 + k];
                bad = idx < 0 || idx >= dn;
                if (!bad) v = load64(pages, d0 + 8 * idx, pages_bytes);
            }
        } else {
            const int64_t v0 = layout[kValOff * n_pages + pg], vn = layout[kValLen * n_pages + pg];
            bad = v0 < 0 || vn < 0 || v0 > pages_bytes - vn || k > (vn - 8) / 8 || vn < 8;
            if (!bad) v = load64(pages, v0 + 8 * k, pages_bytes);
        }
    }
    out[i] = bad ? kNaN : v;
    if (bad) value_status[pg] = kPageValues;                     // a constant: lanes that race write the same thing
}

// One step of a tile walk: the lanes of `valid` leave class by class.  `visit(class, equals)` runs once per distinct class
// with the ballot of the lanes that hold it -- in every lane, with wave-uniform arguments.
template <typename Visit>
__device__ __forceinline__ void by_class(bool valid, int32_t code, Visit visit) {
    uint64_t remaining = __ballot(valid);
    while (remaining) {
        const int32_t leader = __builtin_ctzll(remaining);
        const int32_t c = __builtin_amdgcn_readlane(code, leader);
        const uint64_t equals = __ballot(valid && code == c);
        visit(c, equals, leader);
        remaining &= ~equals;
    }
}

__global__ __launch_bounds__(kBlock) void bin_codes_kernel(const double *__restrict__ x, int64_t n, const double *__restrict__ edges,
                                                           int32_t n_edges, uint8_t *__restrict__ codes,
                                                           int32_t *__restrict__ tile_counts, int64_t n_tiles) {
    __shared__ double s_edges[pair_bins::kMaxBins + 1];
    __shared__ int32_t s_count[kWaves][pair_bins::kClasses];
    for (int32_t k = threadIdx.x; k < n_edges; k += kBlock) s_edges[k] = edges[k];
    for (int32_t k = threadIdx.x; k < kWaves * pair_bins::kClasses; k += kBlock) (&s_count[0][0])[k] = 0;
    __syncthreads();
    const int32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * kWaves + wave;
    if (tile >= n_tiles) return;                                 // wave-uniform; no barrier below
    int32_t *__restrict__ count = s_count[wave];
    for (int64_t at = tile * kTile; at < (tile + 1) * kTile && at < n; at += 64) {
        const int64_t i = at + lane;
        const bool valid = i < n;
        const int32_t code = valid ? pair_bins::classify(x[i], s_edges, n_edges) : pair_bins::kDropped;
        if (valid) codes[i] = (uint8_t)code;
        by_class(valid, code, [&](int32_t c, uint64_t equals, int32_t leader) {
            if (lane == leader) count[c] += __popcll(equals);
        });
        wave_lds_fence();
    }
    for (int32_t k = lane; k < pair_bins::kClasses; k += 64) tile_counts[tile * pair_bins::kClasses + k] = count[k];
}

__global__ __launch_bounds__(kBlock) void partition_kernel(const uint8_t *__restrict__ codes, int64_t n,
                                                           const int32_t *__restrict__ tile_offsets, int64_t n_tiles,
                                                           int32_t *__restrict__ order) {
    __shared__ int32_t s_next[kWaves][pair_bins::kClasses];
    const int32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * kWaves + wave;
    if (tile >= n_tiles) return;                                 // wave-uniform; no barrier in this kernel
    int32_t *__restrict__ next = s_next[wave];
    for (int32_t k = lane; k < pair_bins::kClasses; k += 64) next[k] = tile_offsets[tile * pair_bins::kClasses + k];
    wave_lds_fence();
    const uint64_t below = (1ull << lane) - 1;
    for (int64_t at = tile * kTile; at < (tile + 1) * kTile && at < n; at += 64) {
        const int64_t i = at + lane;
        const bool valid = i < n;
        const int32_t code = valid ? (int32_t)codes[i] : 0;
        int64_t dest = -1;
        by_class(valid, code, [&](int32_t c, uint64_t equals, int32_t leader) {
            if (valid && code == c) dest = (int64_t)next[c] + __popcll(equals & below);
            if (lane == leader) next[c] += __popcll(equals);
        });
        wave_lds_fence();
        if (dest >= 0 && dest < n) order[dest] = (int32_t)i;     // offsets that are no exclusive scan of the counts write nothing outside
    }
}

}  // namespace pair_table
}  // namespace mspa

using namespace mspa;

extern "C" int32_t mspa_pair_tile_rows(void) { return pair_table::kTile; }

extern "C" int mspa_pair_bin_codes_host(const double *x, int64_t n, const double *edges, int32_t n_edges, uint8_t *out_codes,
                                        int64_t *out_counts) {
    if (n < 0 || n_edges < 2 || n_edges > pair_bins::kMaxBins + 1) return fail(MSPA_EINVAL, "mspa_pair_bin_codes_host: 0 <= n, 2 <= n_edges <= 251");
    if (!edges || !out_counts || (n > 0 && (!x || !out_codes))) return fail(MSPA_EINVAL, "mspa_pair_bin_codes_host: null pointer");
    for (int32_t k = 1; k < n_edges; ++k)
        if (!(edges[k - 1] < edges[k])) return fail(MSPA_EINVAL, "mspa_pair_bin_codes_host: edges ascend strictly");
    pair_bins::classify_all(x, n, edges, n_edges, out_codes, out_counts);
    return MSPA_OK;
}

extern "C" int mspa_pair_bin_codes_device(const double *x_dev, int64_t n, const double *edges_dev, int32_t n_edges, uint8_t *out_codes_dev,
                                          int32_t *out_tile_counts_dev, int64_t n_tiles, void *stream) {
    if (n < 0 || n > 0x7fffffffLL || n_edges < 2 || n_edges > pair_bins::kMaxBins + 1 || n_tiles != (n + pair_table::kTile - 1) / pair_table::kTile)
        return fail(MSPA_EINVAL, "mspa_pair_bin_codes_device: 0 <= n < 2^31, 2 <= n_edges <= 251, n_tiles = ceil(n / mspa_pair_tile_rows())");
    if (n == 0) return MSPA_OK;
    if (!x_dev || !edges_dev || !out_codes_dev || !out_tile_counts_dev) return fail(MSPA_EINVAL, "mspa_pair_bin_codes_device: null pointer");
    hipLaunchKernelGGL(pair_table::bin_codes_kernel, dim3((unsigned)((n_tiles + pair_table::kWaves - 1) / pair_table::kWaves)),
                       dim3(pair_table::kBlock), 0, (hipStream_t)stream, x_dev, n, edges_dev, n_edges, out_codes_dev, out_tile_counts_dev, n_tiles);
    return check_hip(hipGetLastError(), "mspa_pair_bin_codes_device");
}

extern "C" int mspa_pair_partition_device(const uint8_t *codes_dev, int64_t n, const int32_t *tile_offsets_dev, int64_t n_tiles,
                                          int32_t *out_order_dev, void *stream) {
    if (n < 0 || n > 0x7fffffffLL || n_tiles != (n + pair_table::kTile - 1) / pair_table::kTile)
        return fail(MSPA_EINVAL, "mspa_pair_partition_device: 0 <= n < 2^31, n_tiles = ceil(n / mspa_pair_tile_rows())");
    if (n == 0) return MSPA_OK;
    if (!codes_dev || !tile_offsets_dev || !out_order_dev) return fail(MSPA_EINVAL, "mspa_pair_partition_device: null pointer");
    hipLaunchKernelGGL(pair_table::partition_kernel, dim3((unsigned)((n_tiles + pair_table::kWaves - 1) / pair_table::kWaves)),
                       dim3(pair_table::kBlock), 0, (hipStream_t)stream, codes_dev, n, tile_offsets_dev, n_tiles, out_order_dev);
    return check_hip(hipGetLastError(), "mspa_pair_partition_device");
}

extern "C" int mspa_rle_hybrid_runs_device(const uint8_t *src_dev, int64_t src_bytes, const int64_t *stream_offsets_dev,
                                           const int64_t *stream_bytes_dev, const int64_t *stream_bit_width_dev,
                                           const int64_t *stream_values_dev, const int64_t *out_begin_dev, const int64_t *run_begin_dev,
                                           int64_t n_streams, int64_t n_runs, int64_t *run_count_dev, int32_t *status_dev,
                                           int32_t *const_value_dev, int64_t *run_first_dev, int64_t *run_pos_dev, int32_t *run_info_dev,
                                           void *stream) {
    if (src_bytes < 0 || n_streams < 0 || n_runs < 0 || n_streams > (int64_t)0x7fffffff * 64)
        return fail(MSPA_EINVAL, "mspa_rle_hybrid_runs_device: bad size");
    if (n_streams == 0) return MSPA_OK;
    if (!stream_offsets_dev || !stream_bytes_dev || !stream_bit_width_dev || !stream_values_dev || !out_begin_dev || !run_count_dev ||
        !status_dev || !const_value_dev || (src_bytes > 0 && !src_dev) ||
        (run_begin_dev && n_runs > 0 && (!run_first_dev || !run_pos_dev || !run_info_dev)))
        return fail(MSPA_EINVAL, "mspa_rle_hybrid_runs_device: null pointer");
    hipLaunchKernelGGL(pair_table::hybrid_runs_kernel, dim3((unsigned)((n_streams + 63) / 64)), dim3(64), 0, (hipStream_t)stream, src_dev, src_bytes,
                       stream_offsets_dev, stream_bytes_dev, stream_bit_width_dev, stream_values_dev, out_begin_dev,
                       n_runs > 0 ? run_begin_dev : nullptr, n_streams, n_runs, run_count_dev, status_dev, const_value_dev, run_first_dev,
                       run_pos_dev, run_info_dev);
    return check_hip(hipGetLastError(), "mspa_rle_hybrid_runs_device");
}

extern "C" int mspa_rle_hybrid_expand_device(const uint8_t *src_dev, int64_t src_bytes, const int64_t *run_first_dev,
                                             const int64_t *run_pos_dev, const int32_t *run_info_dev, int64_t n_runs, int32_t *out_dev,
                                             int64_t n_values, void *stream) {
    if (src_bytes < 0 || n_runs < 0 || n_values < 0 || n_values > (int64_t)0x7fffffff * 256)
        return fail(MSPA_EINVAL, "mspa_rle_hybrid_expand_device: bad size");
    if (n_values == 0) return MSPA_OK;
    if (n_runs == 0) return fail(MSPA_EINVAL, "mspa_rle_hybrid_expand_device: values without runs");
    if (!run_first_dev || !run_pos_dev || !run_info_dev || !out_dev || (src_bytes > 0 && !src_dev))
        return fail(MSPA_EINVAL, "mspa_rle_hybrid_expand_device: null pointer");
    hipLaunchKernelGGL(pair_table::hybrid_expand_kernel, dim3((unsigned)((n_values + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src_dev,
                       src_bytes, run_first_dev, run_pos_dev, run_info_dev, n_runs, n_values, out_dev);
    return check_hip(hipGetLastError(), "mspa_rle_hybrid_expand_device");
}

extern "C" int mspa_parquet_double_layout_device(const uint8_t *pages_dev, int64_t pages_bytes, const int64_t *page_offsets_dev,
                                                 const int64_t *page_bytes_dev, const int32_t *page_flags_dev, int64_t n_pages,
                                                 int64_t *layout_dev, int32_t *page_status_dev, void *stream) {
    if (pages_bytes < 0 || n_pages < 0 || n_pages > (int64_t)0x7fffffff * 64) return fail(MSPA_EINVAL, "mspa_parquet_double_layout_device: bad size");
    if (n_pages == 0) return MSPA_OK;
    if (!page_offsets_dev || !page_bytes_dev || !page_flags_dev || !layout_dev || !page_status_dev || (pages_bytes > 0 && !pages_dev))
        return fail(MSPA_EINVAL, "mspa_parquet_double_layout_device: null pointer");
    hipLaunchKernelGGL(pair_table::double_layout_kernel, dim3((unsigned)((n_pages + 63) / 64)), dim3(64), 0, (hipStream_t)stream, pages_dev,
                       pages_bytes, page_offsets_dev, page_bytes_dev, page_flags_dev, n_pages, layout_dev, page_status_dev);
    return check_hip(hipGetLastError(), "mspa_parquet_double_layout_device");
}

extern "C" int mspa_parquet_double_column_device(const uint8_t *pages_dev, int64_t pages_bytes, const int64_t *layout_dev,
                                                 const int64_t *page_values_dev, const int32_t *page_flags_dev,
                                                 const int64_t *page_first_dev, int64_t n_pages, const int32_t *levels_dev,
                                                 const int64_t *level_rank_dev, const int64_t *level_begin_dev, int64_t n_levels,
                                                 const int32_t *indices_dev, const int64_t *index_begin_dev, int64_t n_indices,
                                                 const int64_t *dict_offsets_dev, const int64_t *dict_count_dev, double *out_dev,
                                                 int64_t n_out, int32_t *value_status_dev, void *stream) {
    if (pages_bytes < 0 || n_pages < 0 || n_out < 0 || n_levels < 0 || n_indices < 0 || n_out > (int64_t)0x7fffffff * 256)
        return fail(MSPA_EINVAL, "mspa_parquet_double_column_device: bad size");
    if (n_out == 0) return MSPA_OK;
    if (n_pages == 0) return fail(MSPA_EINVAL, "mspa_parquet_double_column_device: rows without pages");
    if (!layout_dev || !page_values_dev || !page_flags_dev || !page_first_dev || !index_begin_dev || !dict_offsets_dev || !dict_count_dev ||
        !out_dev || !value_status_dev || (pages_bytes > 0 && !pages_dev) || (levels_dev && (!level_rank_dev || !level_begin_dev)))
        return fail(MSPA_EINVAL, "mspa_parquet_double_column_device: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int rc = check_hip(hipMemsetAsync(value_status_dev, 0, (size_t)n_pages * 4, st), "mspa_parquet_double_column_device: clearing the status");
    if (rc) return rc;
    hipLaunchKernelGGL(pair_table::double_column_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, st, pages_dev, pages_bytes, layout_dev,
                       page_values_dev, page_flags_dev, page_first_dev, n_pages, levels_dev, level_rank_dev, level_begin_dev, n_levels,
                       indices_dev, index_begin_dev, n_indices, dict_offsets_dev, dict_count_dev, (uint64_t *)out_dev, n_out, value_status_dev);
    return check_hip(hipGetLastError(), "mspa_parquet_double_column_device");
}
