// The visibility index's rows read back ON the MI355X: decompressed `values` pages (csrc/snappy_decode.hip) -> the image_to_points
// rows' bitsets, without the text ever leaving the device.  Between gather and lists->bits stands K11's list parser (scene_prep.hip);
// the page layout (PLAIN BYTE_ARRAY behind RLE definition levels) is csrc/snappy_core.h's, as csrc/parquet_pages.hip writes it.
//
//   spans        one lane per needed page walks the PLAIN u32 length chain from the page's first value to its last needed row: a
//                dependent-load chain as long as the values in front of that row.  In this project's files a scene's
//                image_to_points rows open the chunk (a few values per ~1 MiB page); a row group that mixes scenes may put
//                ~20 k short point_to_images rows of the scene before in front of them -- 20 k dependent L2 loads, a few
//                milliseconds for that one lane (not measured on such a file).
//   dict spans   one lane per needed dictionary-coded page walks the RLE / bit-packed runs of indices (csrc/rle_hybrid_core.h) to
//                its last needed row and looks the rows up in the span table `spans` wrote for the dictionary page's entries.
//   brackets     one lane per row: '[' and ']' behind / in front of JSON white space.
//   gather       the texts between the brackets back to back (what K11's list parser takes), one byte per lane.
//   lists->bits  one lane per parsed value.  A list ascends, so the values of one 64-bit word are neighbours in the value array:
//                the lane whose predecessor lies in another word (or that opens the row) ORs the run and stores the word with a
//                plain store into the zeroed row.  A value below its predecessor or outside [0, n_points) declines the row
//                (plain stores of a constant: lanes that race write the same thing); a duplicate is harmless.
//   pick         one lane per sample (row, position): element `position` of the row's parsed list, for the readers that use a
//                row as a LIST (len, list[j]: duplicates count, order is the text's) -- they stop in front of lists->bits.
// No atomics; every load and store is checked against the buffer it goes to.
#include "mspa_common.h"
#include "snappy_core.h"
#include "rle_hybrid_core.h"

namespace mspa {
namespace index_rows {

constexpr int32_t kPageBounds = 1;       // a length runs past the page, or the tables do not describe it
constexpr int32_t kPageLevels = 2;       // the definition levels are not one run of ones
constexpr int32_t kPageRuns = 3;         // dictionary-coded pages: the index runs are malformed (rle_hybrid's code beside it)
constexpr int32_t kPageIndex = 4;        // dictionary-coded pages: an index >= the dictionary's entry count
constexpr int32_t kRowBrackets = 1;      // a row's text is not [ ... ]
constexpr int32_t kRowOrder = 32;        // lists->bits: a value below its predecessor     (K11's parser owns bits 2 .. 16)
constexpr int32_t kRowRange = 64;        // lists->bits: a value outside [0, n_points)
constexpr int32_t kPickRow = 1;          // pick: the sample's row lies outside [0, n_rows)
constexpr int32_t kPickPosition = 2;     // pick: its position lies outside the row's list
constexpr int32_t kPickRange = 4;        // pick: the element lies outside [0, n_points)
constexpr int32_t kPickOffsets = 8;      // pick: the row's offsets descend or leave [0, n_values]
constexpr int kPickBlock = 256;

__device__ __forceinline__ bool json_space(uint8_t c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }

__global__ __launch_bounds__(64) void plain_spans_kernel(const uint8_t *__restrict__ pages, int64_t pages_bytes,
                                                         const int64_t *__restrict__ page_off, const int64_t *__restrict__ page_size,
                                                         const int64_t *__restrict__ page_values, int64_t n_pages, int32_t has_levels,
                                                         const int64_t *__restrict__ row_begin, const int64_t *__restrict__ row_index,
                                                         int64_t n_rows, int64_t *__restrict__ out_start, int64_t *__restrict__ out_len,
                                                         int32_t *__restrict__ page_status) {
    const int64_t pg = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (pg >= n_pages) return;
    const int64_t off = page_off[pg], size = page_size[pg], nv = page_values[pg];
    int64_t r0 = row_begin[pg], r1 = row_begin[pg + 1];
    int32_t bad = 0;
    if (r0 < 0 || r1 < r0 || r1 > n_rows) {
        page_status[pg] = kPageBounds;
        return;
    }
    if (off < 0 || size < 0 || off > pages_bytes - size || nv < 0) bad = kPageBounds;
    const uint8_t *__restrict__ q = pages + off;
    int64_t pos = 0;
    if (!bad && has_levels) {
        const int32_t head = snappy::page_head_len(nv);
        if (head > size) bad = kPageBounds;
        for (int32_t r = 0; !bad && r < head; ++r)
            if (q[r] != snappy::page_head_byte(nv, r)) bad = kPageLevels;
        pos = head;
    }
    int64_t v = 0, r = r0;
    for (; !bad && r < r1; ++r) {
        const int64_t target = row_index[r];
        if (target < v || target >= nv) {
            bad = kPageBounds;
            break;
        }
        for (;; ++v) {
            if (pos > size - 4) {
                bad = kPageBounds;
                break;
            }
            const int64_t len = snappy::load32(q + pos);
            if (len > size - pos - 4) {
                bad = kPageBounds;
                break;
            }
            if (v == target) {
                out_start[r] = off + pos + 4;
                out_len[r] = len;
            }
            pos += 4 + len;
            if (v == target) break;
        }
        if (bad) break;
        ++v;
    }
    for (; bad && r < r1; ++r) {                                 // the rows this page did not give
        out_start[r] = 0;
        out_len[r] = 0;
    }
    page_status[pg] = bad;
}

// One lane per needed dictionary-coded page (RLE_DICTIONARY / PLAIN_DICTIONARY): [levels,] one byte of bit width, then the
// indices as an RLE / bit-packed hybrid stream (csrc/rle_hybrid_core.h).  The lane takes the needed rows' indices through
// rle_hybrid::take -- a chain of one step per run in front of the last needed row -- and looks each one up in the page's
// dictionary: entries [dict_begin[pg], + dict_count[pg]) of the span table (dict_start / dict_len) that plain_spans_kernel wrote
// for the dictionary pages' PLAIN entries.  A page that declines gives its rows index -1 and an empty span.
__global__ __launch_bounds__(64) void dict_spans_kernel(const uint8_t *__restrict__ pages, int64_t pages_bytes,
                                                        const int64_t *__restrict__ page_off, const int64_t *__restrict__ page_size,
                                                        const int64_t *__restrict__ page_values, int64_t n_pages, int32_t has_levels,
                                                        const int64_t *__restrict__ row_begin, const int64_t *__restrict__ row_index,
                                                        int64_t n_rows, const int64_t *__restrict__ dict_begin,
                                                        const int64_t *__restrict__ dict_count, const int64_t *__restrict__ dict_start,
                                                        const int64_t *__restrict__ dict_len, int64_t n_dict, int32_t *out_index,
                                                        int64_t *__restrict__ out_start, int64_t *__restrict__ out_len,
                                                        int32_t *__restrict__ page_status, int32_t *__restrict__ page_code) {
    const int64_t pg = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (pg >= n_pages) return;
    const int64_t off = page_off[pg], size = page_size[pg], nv = page_values[pg], d0 = dict_begin[pg], dn = dict_count[pg];
    const int64_t r0 = row_begin[pg], r1 = row_begin[pg + 1];
    int32_t bad = 0, code = 0;
    if (r0 < 0 || r1 < r0 || r1 > n_rows) {
        page_status[pg] = kPageBounds;
        page_code[pg] = 0;
        return;
    }
    if (off < 0 || size < 0 || off > pages_bytes - size || nv < 0 || d0 < 0 || dn < 0 || d0 > n_dict - dn) bad = kPageBounds;
    const uint8_t *__restrict__ q = pages + off;
    int64_t pos = 0;
    if (!bad && has_levels) {
        const int32_t head = snappy::page_head_len(nv);
        if (head > size) bad = kPageBounds;
        for (int32_t r = 0; !bad && r < head; ++r)
            if (q[r] != snappy::page_head_byte(nv, r)) bad = kPageLevels;
        pos = head;
    }
    if (!bad && pos >= size) bad = kPageBounds;                  // no room for the bit width
    if (!bad) {
        const int rc = rle_hybrid::take(q + pos + 1, size - pos - 1, (int32_t)q[pos], nv, row_index + r0, r1 - r0, out_index + r0);
        if (rc == rle_hybrid::kErrRows) {
            bad = kPageBounds;
        } else if (rc != 0) {
            bad = kPageRuns;
            code = rc;
        }
    }
    for (int64_t r = r0; !bad && r < r1; ++r) {
        const int64_t k = (int64_t)(uint32_t)out_index[r];       // this lane's own stores
        if (k >= dn) {
            bad = kPageIndex;
            break;
        }
        out_start[r] = dict_start[d0 + k];
        out_len[r] = dict_len[d0 + k];
    }
    for (int64_t r = r0; bad && r < r1; ++r) {                   // the rows this page did not give
        out_index[r] = -1;
        out_start[r] = 0;
        out_len[r] = 0;
    }
    page_status[pg] = bad;
    page_code[pg] = code;
}

__global__ __launch_bounds__(64) void row_brackets_kernel(const uint8_t *__restrict__ pages, int64_t pages_bytes,
                                                          const int64_t *__restrict__ start, const int64_t *__restrict__ len, int64_t n_rows,
                                                          int64_t *__restrict__ inner_start, int64_t *__restrict__ inner_len,
                                                          int32_t *__restrict__ row_status) {
    const int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (r >= n_rows) return;
    int64_t a = start[r], z = a + len[r];
    bool ok = a >= 0 && len[r] >= 2 && len[r] <= pages_bytes && a <= pages_bytes - len[r];
    if (ok) {
        while (a < z && json_space(pages[a])) ++a;
        while (z > a && json_space(pages[z - 1])) --z;
        ok = z - a >= 2 && pages[a] == '[' && pages[z - 1] == ']';
    }
    inner_start[r] = ok ? a + 1 : 0;
    inner_len[r] = ok ? z - a - 2 : 0;
    row_status[r] = ok ? 0 : kRowBrackets;
}

__global__ __launch_bounds__(256) void row_gather_kernel(const uint8_t *__restrict__ pages, int64_t pages_bytes,
                                                         const int64_t *__restrict__ inner_start, const int64_t *__restrict__ prefix,
                                                         int64_t n_rows, int64_t total, uint8_t *__restrict__ text) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t lo = last_at_or_below(prefix, n_rows, i);      // the row this byte is of (empty rows in front of it share its prefix)
    const int64_t from = inner_start[lo] + (i - prefix[lo]);
    text[i] = (from >= 0 && from < pages_bytes) ? pages[from] : (uint8_t)0;      // a 0 byte is no list: the parser declines the row
}

__global__ __launch_bounds__(256) void lists_to_bits_kernel(const int32_t *__restrict__ values, int64_t n_values,
                                                            const int64_t *__restrict__ offsets, int64_t n_rows, int64_t n_points,
                                                            uint64_t *__restrict__ bits, int64_t n_words, int32_t *__restrict__ row_status) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_values) return;
    const int64_t lo = last_at_or_below(offsets, n_rows, i);     // the row this value is of (empty rows in front of it share its offset)
    const int64_t first = offsets[lo];
    int64_t end = offsets[lo + 1];
    if (end > n_values) end = n_values;
    if (i < first || i >= end) return;                           // offsets that do not hold this value: no row's
    const int64_t v = values[i], prev = (i > first && i > 0) ? (int64_t)values[i - 1] : -1;
    if (v < prev) row_status[lo] = kRowOrder;
    if (v < 0 || v >= n_points) {
        row_status[lo] = kRowRange;
        return;
    }
    if (prev >= 0 && (prev >> 6) == (v >> 6)) return;            // the lane in front owns this word
    uint64_t w = 0;
    for (int64_t j = i; j < end; ++j) {
        const int64_t u = values[j];
        if (u < 0 || (u >> 6) != (v >> 6)) break;
        w |= 1ull << (u & 63);
    }
    bits[lo * n_words + (v >> 6)] = w;                           // v < n_points <= 64 n_words
}

// One lane per sample (row, position): the row's list read as a list -- element `position` of it, duplicates and order as the
// text has them.  A sample that names no element, or an element that is no vertex of the scene, gives -1 and says why.
__global__ __launch_bounds__(kPickBlock) void list_pick_kernel(const int32_t *__restrict__ values, int64_t n_values,
                                                               const int64_t *__restrict__ offsets, int64_t n_rows,
                                                               const int64_t *__restrict__ samples, int64_t n_samples, int64_t n_points,
                                                               int32_t *__restrict__ out_vertex, int32_t *__restrict__ out_status) {
    const int64_t s = (int64_t)blockIdx.x * kPickBlock + threadIdx.x;
    if (s >= n_samples) return;
    const int64_t row = samples[2 * s], position = samples[2 * s + 1];
    int32_t vertex = -1, status = 0;
    if (row < 0 || row >= n_rows) {
        status = kPickRow;
    } else {
        const int64_t first = offsets[row], end = offsets[row + 1];
        if (first < 0 || end < first || end > n_values) {
            status = kPickOffsets;
        } else if (position < 0 || position >= end - first) {
            status = kPickPosition;
        } else {
            const int32_t v = values[first + position];          // 0 <= first + position < end <= n_values
            if (v < 0 || v >= n_points)
                status = kPickRange;
            else
                vertex = v;
        }
    }
    out_vertex[s] = vertex;
    out_status[s] = status;
}

}  // namespace index_rows
}  // namespace mspa

using namespace mspa;

extern "C" int mspa_parquet_plain_spans_device(const uint8_t *pages_dev, int64_t pages_bytes, const int64_t *page_offsets_dev,
                                               const int64_t *page_bytes_dev, const int64_t *page_values_dev, int64_t n_pages,
                                               int32_t has_levels, const int64_t *row_begin_dev, const int64_t *row_index_dev, int64_t n_rows,
                                               int64_t *out_start_dev, int64_t *out_len_dev, int32_t *page_status_dev, void *stream) {
    if (pages_bytes < 0 || n_pages < 0 || n_rows < 0 || n_pages > (int64_t)0x7fffffff * 64 || (has_levels != 0 && has_levels != 1))
        return fail(MSPA_EINVAL, "mspa_parquet_plain_spans_device: bad size");
    if (n_pages == 0) return n_rows == 0 ? MSPA_OK : fail(MSPA_EINVAL, "mspa_parquet_plain_spans_device: rows without pages");
    if (!page_offsets_dev || !page_bytes_dev || !page_values_dev || !row_begin_dev || !page_status_dev || (pages_bytes > 0 && !pages_dev) ||
        (n_rows > 0 && (!row_index_dev || !out_start_dev || !out_len_dev)))
        return fail(MSPA_EINVAL, "mspa_parquet_plain_spans_device: null pointer");
    hipLaunchKernelGGL(index_rows::plain_spans_kernel, dim3((unsigned)((n_pages + 63) / 64)), dim3(64), 0, (hipStream_t)stream, pages_dev, pages_bytes,
                       page_offsets_dev, page_bytes_dev, page_values_dev, n_pages, has_levels, row_begin_dev, row_index_dev, n_rows, out_start_dev,
                       out_len_dev, page_status_dev);
    return check_hip(hipGetLastError(), "mspa_parquet_plain_spans_device");
}

extern "C" int mspa_rle_hybrid_take_host(const uint8_t *src, int64_t src_len, int32_t bit_width, int64_t n_values, const int64_t *rows,
                                         int64_t n_rows, int32_t *out) {
    if (src_len < 0 || src_len > 0x7fffffffLL || n_values < 0 || n_rows < 0)
        return fail(MSPA_EINVAL, "mspa_rle_hybrid_take_host: 0 <= src_len < 2^31, 0 <= n_values, n_rows");
    if ((src_len > 0 && !src) || (n_rows > 0 && (!rows || !out))) return fail(MSPA_EINVAL, "mspa_rle_hybrid_take_host: null pointer");
    const int rc = rle_hybrid::take(src, src_len, bit_width, n_values, rows, n_rows, out);
    return rc == rle_hybrid::kErrRows ? fail(MSPA_EINVAL, "mspa_rle_hybrid_take_host: rows ascend and are < n_values") : rc;
}

extern "C" int mspa_parquet_dict_spans_device(const uint8_t *pages_dev, int64_t pages_bytes, const int64_t *page_offsets_dev,
                                              const int64_t *page_bytes_dev, const int64_t *page_values_dev, int64_t n_pages,
                                              int32_t has_levels, const int64_t *row_begin_dev, const int64_t *row_index_dev, int64_t n_rows,
                                              const int64_t *dict_begin_dev, const int64_t *dict_count_dev, const int64_t *dict_start_dev,
                                              const int64_t *dict_len_dev, int64_t n_dict, int32_t *out_index_dev, int64_t *out_start_dev,
                                              int64_t *out_len_dev, int32_t *page_status_dev, int32_t *page_code_dev, void *stream) {
    if (pages_bytes < 0 || n_pages < 0 || n_rows < 0 || n_dict < 0 || n_pages > (int64_t)0x7fffffff * 64 || (has_levels != 0 && has_levels != 1))
        return fail(MSPA_EINVAL, "mspa_parquet_dict_spans_device: bad size");
    if (n_pages == 0) return n_rows == 0 ? MSPA_OK : fail(MSPA_EINVAL, "mspa_parquet_dict_spans_device: rows without pages");
    if (!page_offsets_dev || !page_bytes_dev || !page_values_dev || !row_begin_dev || !dict_begin_dev || !dict_count_dev || !page_status_dev ||
        !page_code_dev || (pages_bytes > 0 && !pages_dev) || (n_dict > 0 && (!dict_start_dev || !dict_len_dev)) ||
        (n_rows > 0 && (!row_index_dev || !out_index_dev || !out_start_dev || !out_len_dev)))
        return fail(MSPA_EINVAL, "mspa_parquet_dict_spans_device: null pointer");
    hipLaunchKernelGGL(index_rows::dict_spans_kernel, dim3((unsigned)((n_pages + 63) / 64)), dim3(64), 0, (hipStream_t)stream, pages_dev, pages_bytes,
                       page_offsets_dev, page_bytes_dev, page_values_dev, n_pages, has_levels, row_begin_dev, row_index_dev, n_rows, dict_begin_dev,
                       dict_count_dev, dict_start_dev, dict_len_dev, n_dict, out_index_dev, out_start_dev, out_len_dev, page_status_dev,
                       page_code_dev);
    return check_hip(hipGetLastError(), "mspa_parquet_dict_spans_device");
}

extern "C" int mspa_index_rows_brackets_device(const uint8_t *pages_dev, int64_t pages_bytes, const int64_t *start_dev, const int64_t *len_dev,
                                               int64_t n_rows, int64_t *out_inner_start_dev, int64_t *out_inner_len_dev, int32_t *row_status_dev,
                                               void *stream) {
    if (pages_bytes < 0 || n_rows < 0 || n_rows > (int64_t)0x7fffffff * 64) return fail(MSPA_EINVAL, "mspa_index_rows_brackets_device: bad size");
    if (n_rows == 0) return MSPA_OK;
    if (!start_dev || !len_dev || !out_inner_start_dev || !out_inner_len_dev || !row_status_dev || (pages_bytes > 0 && !pages_dev))
        return fail(MSPA_EINVAL, "mspa_index_rows_brackets_device: null pointer");
    hipLaunchKernelGGL(index_rows::row_brackets_kernel, dim3((unsigned)((n_rows + 63) / 64)), dim3(64), 0, (hipStream_t)stream, pages_dev, pages_bytes,
                       start_dev, len_dev, n_rows, out_inner_start_dev, out_inner_len_dev, row_status_dev);
    return check_hip(hipGetLastError(), "mspa_index_rows_brackets_device");
}

extern "C" int mspa_index_rows_gather_device(const uint8_t *pages_dev, int64_t pages_bytes, const int64_t *inner_start_dev,
                                             const int64_t *inner_prefix_dev, int64_t n_rows, uint8_t *out_text_dev, int64_t text_bytes,
                                             void *stream) {
    if (pages_bytes < 0 || n_rows < 0 || text_bytes < 0 || text_bytes > 0x7fffffffLL)
        return fail(MSPA_EINVAL, "mspa_index_rows_gather_device: bad size (less than 2 GiB of text a call)");
    if (text_bytes == 0) return MSPA_OK;
    if (n_rows == 0) return fail(MSPA_EINVAL, "mspa_index_rows_gather_device: text without rows");
    if (!pages_dev || !inner_start_dev || !inner_prefix_dev || !out_text_dev) return fail(MSPA_EINVAL, "mspa_index_rows_gather_device: null pointer");
    hipLaunchKernelGGL(index_rows::row_gather_kernel, dim3((unsigned)((text_bytes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pages_dev,
                       pages_bytes, inner_start_dev, inner_prefix_dev, n_rows, text_bytes, out_text_dev);
    return check_hip(hipGetLastError(), "mspa_index_rows_gather_device");
}

extern "C" int mspa_index_lists_to_bits_device(const int32_t *values_dev, int64_t n_values, const int64_t *offsets_dev, int64_t n_rows,
                                               int64_t n_points, uint64_t *out_bits_dev, int64_t n_words, int32_t *row_status_dev, void *stream) {
    if (n_values < 0 || n_rows < 0 || n_points < 0 || n_words < 0 || n_values > (int64_t)0x7fffffff * 256 || n_points > 64 * n_words ||
        (n_words > 0 && n_rows > ((int64_t)1 << 40) / n_words))
        return fail(MSPA_EINVAL, "mspa_index_lists_to_bits_device: bad size (n_points <= 64 n_words)");
    if (n_rows == 0) return n_values == 0 ? MSPA_OK : fail(MSPA_EINVAL, "mspa_index_lists_to_bits_device: values without rows");
    if (!offsets_dev || !row_status_dev || (n_values > 0 && !values_dev) || (n_words > 0 && !out_bits_dev))
        return fail(MSPA_EINVAL, "mspa_index_lists_to_bits_device: null pointer");
    hipStream_t st = (hipStream_t)stream;
    int rc = check_hip(hipMemsetAsync(row_status_dev, 0, (size_t)n_rows * 4, st), "mspa_index_lists_to_bits_device: clearing the status");
    if (rc == MSPA_OK && n_words > 0)
        rc = check_hip(hipMemsetAsync(out_bits_dev, 0, (size_t)n_rows * (size_t)n_words * 8, st), "mspa_index_lists_to_bits_device: clearing the rows");
    if (rc) return rc;
    if (n_values > 0)
        hipLaunchKernelGGL(index_rows::lists_to_bits_kernel, dim3((unsigned)((n_values + 255) / 256)), dim3(256), 0, st, values_dev, n_values, offsets_dev,
                           n_rows, n_points, out_bits_dev, n_words, row_status_dev);
    return check_hip(hipGetLastError(), "mspa_index_lists_to_bits_device");
}

extern "C" int mspa_index_lists_pick_device(const int32_t *values_dev, int64_t n_values, const int64_t *offsets_dev, int64_t n_rows,
                                            const int64_t *samples_dev, int64_t n_samples, int64_t n_points, int32_t *out_vertex_dev,
                                            int32_t *out_status_dev, void *stream) {
    if (n_values < 0 || n_rows < 0 || n_samples < 0 || n_points < 0 || n_points > 0x7fffffffLL ||
        n_samples > (int64_t)0x7fffffff * index_rows::kPickBlock)
        return fail(MSPA_EINVAL, "mspa_index_lists_pick_device: bad size (0 <= n_points < 2^31)");
    if (n_samples == 0) return MSPA_OK;
    if (!samples_dev || !out_vertex_dev || !out_status_dev || (n_rows > 0 && !offsets_dev) || (n_values > 0 && !values_dev))
        return fail(MSPA_EINVAL, "mspa_index_lists_pick_device: null pointer");
    hipLaunchKernelGGL(index_rows::list_pick_kernel, dim3((unsigned)((n_samples + index_rows::kPickBlock - 1) / index_rows::kPickBlock)),
                       dim3(index_rows::kPickBlock), 0, (hipStream_t)stream, values_dev, n_values, offsets_dev, n_rows, samples_dev, n_samples,
                       n_points, out_vertex_dev, out_status_dev);
    return check_hip(hipGetLastError(), "mspa_index_lists_pick_device");
}
