// Parquet's RLE / bit-packed hybrid -- the encoding of a dictionary-coded data page's indices (RLE_DICTIONARY, PLAIN_DICTIONARY):
// the arithmetic shared by the device kernel of index_rows.hip (dict_spans_kernel) and the host reference.  Everything that
// decides a value or a code is an MSPA_HD function here, so that a plain C++ build of this header is the reference the device
// must equal.
//
//   * The stream is runs until the input ends.  A run opens with a ULEB128 header h (1 .. 5 bytes):
//       - h & 1 == 0  an RLE run of h >> 1 values: ONE value follows, in ceil(bit_width / 8) bytes, little endian;
//       - h & 1 == 1  a bit-packed run of h >> 1 groups of 8 values: bit_width bytes per group, value k of the run in bits
//         [k * bit_width, (k + 1) * bit_width) of the run's bytes, least significant bit first.
//     The last group may carry up to 7 padding values beyond the page's value count.
//   * bit_width is 0 .. 32 (in a data page: the byte in front of the stream).  Width 0: every value is 0 and a run has no bytes
//     behind its header.
//   * take() reads the values of chosen rows only, walks run by run (a run is skipped by its header alone) and stops at the last
//     needed row: what lies behind it is never looked at.  Nothing is read outside [src, src + len).
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
namespace rle_hybrid {

// (Snappy's codes are -16 .. -22, csrc/snappy_core.h; -1 .. -3 are the library's own.)
constexpr int kErrRows = -1;          // == MSPA_EINVAL: the rows do not ascend, or one is >= n_values
constexpr int kErrBitWidth = -32;     // bit width outside 0 .. 32
constexpr int kErrHeader = -33;       // a run header of more than 5 bytes, or one that runs past the input
constexpr int kErrZeroRun = -34;      // a run of zero values
constexpr int kErrTruncated = -35;    // a run whose bytes pass the input's end
constexpr int kErrShort = -36;        // the runs end before a needed row

struct Run {
    int32_t head;       // header bytes
    bool packed;        // bit-packed groups; false: one repeated value
    int64_t count;      // values it stands for (a bit-packed run: 8 per group, padding included)
    int64_t bytes;      // bytes behind the header
};

// The run that opens at s[p] (p < n).  Returns 0 or a code.
MSPA_HD int parse_run(const uint8_t *s, int64_t p, int64_t n, int32_t bit_width, Run &r) {
    uint64_t h = 0;
    int32_t k = 0;
    for (;;) {
        if (k == 5 || p + k >= n) return kErrHeader;
        const uint32_t b = s[p + k];
        h |= (uint64_t)(b & 127u) << (7 * k);
        ++k;
        if (b < 128u) break;
    }
    const int64_t m = (int64_t)(h >> 1);                 // < 2^34
    r.head = k;
    r.packed = (h & 1u) != 0;
    r.count = r.packed ? m * 8 : m;
    r.bytes = r.packed ? m * bit_width : (bit_width + 7) / 8;
    if (m == 0) return kErrZeroRun;
    return r.bytes > n - p - k ? kErrTruncated : 0;
}

// The one value of an RLE run whose bytes open at q.
MSPA_HD int32_t rle_value(const uint8_t *q, int32_t bit_width) {
    uint32_t v = 0;
    for (int32_t i = 0; i < (bit_width + 7) / 8; ++i) v |= (uint32_t)q[i] << (8 * i);
    return (int32_t)v;
}

// Value k of a bit-packed run whose bytes open at q (k < the run's count: the bytes read are the run's own).
MSPA_HD int32_t packed_value(const uint8_t *q, int64_t k, int32_t bit_width) {
    if (bit_width == 0) return 0;
    const int64_t bit = k * bit_width;
    const int32_t shift = (int32_t)(bit & 7), nbytes = (shift + bit_width + 7) / 8;      // <= 5
    uint64_t v = 0;
    for (int32_t i = 0; i < nbytes; ++i) v |= (uint64_t)q[(bit >> 3) + i] << (8 * i);
    return (int32_t)(uint32_t)((v >> shift) & ((1ull << bit_width) - 1));
}

// The reference: out[i] = value rows[i] of the stream src[0, len) that holds n_values values (rows strictly ascending, each
// < n_values).  Returns 0, or a code; out[i] is written for the rows in front of the one that met it.
MSPA_HD int take(const uint8_t *src, int64_t len, int32_t bit_width, int64_t n_values, const int64_t *rows, int64_t n_rows, int32_t *out) {
    if (bit_width < 0 || bit_width > 32) return kErrBitWidth;
    int64_t p = 0, q = 0, v0 = 0, v1 = 0, last = -1;                     // the current run stands for values [v0, v1); its bytes open at q
    bool packed = false;
    for (int64_t i = 0; i < n_rows; ++i) {
        const int64_t t = rows[i];
        if (t <= last || t >= n_values) return kErrRows;
        last = t;
        while (t >= v1) {
            if (p >= len) return kErrShort;
            Run r;
            const int rc = parse_run(src, p, len, bit_width, r);
            if (rc != 0) return rc;
            q = p + r.head;
            packed = r.packed;
            v0 = v1;
            v1 = v0 + r.count;                                           // < 2^31 runs of < 2^37 values
            p = q + r.bytes;
        }
        out[i] = packed ? packed_value(src + q, t - v0, bit_width) : rle_value(src + q, bit_width);
    }
    return 0;
}

}  // namespace rle_hybrid
}  // namespace mspa
