// Snappy compression, Snappy decoding and parquet v1 data pages for the visibility index's `values` column: the arithmetic shared by the device
// kernels of parquet_pages.hip (K12, the writer), snappy_decode.hip and index_rows.hip (the way back) and the host reference.
// Everything that decides an output byte is an MSPA_HD function here, so that a plain C++ build of this header is the reference
// the device must equal byte for byte.
//
//   * The compressor is this file's own, deterministic algorithm (not Google's): a function of the input bytes only.
//       - a stream is varint(n), then the elements of the input's consecutive blocks of kBlock = 64 KiB bytes.  Blocks are
//         independent: no copy reaches before its block's start, so the concatenation is one valid Snappy stream and every
//         block's elements decode alone;
//       - candidates, per block: for every position p with p + 3 < n_block, H(p) = (load32le(p) * 0x1e35a7bd) >> (32 - kHashBits);
//         cand(p) is the largest q < p of the block with H(q) == H(p).  EVERY position is inserted, whether the parse visits it or
//         not, so the candidates do not depend on the parse (nor on how a wave walks the block in chunks of 64 positions).  A
//         candidate is valid when its 4 bytes equal those at p;
//       - the parse is greedy and serial: at cursor p, a valid cand(p) is extended to its full length (it stops at the block's
//         end; source and target may overlap), the pending literal bytes are flushed, the copy is emitted and p += len;
//         otherwise p += 1.  Trailing bytes are one literal;
//       - a literal of len <= 60 is its tag alone, len <= 256 takes one length byte, len <= 65 536 two (no literal is longer than
//         a block);
//       - a copy with 4 <= len <= 11 and offset < 2048 takes the 2-byte form; every other copy is 3-byte pieces of at most 64
//         bytes, 60 when a 64-byte piece would leave 1 to 3 bytes behind;
//       - kHashBits = 14: a table of 16 384 uint16 positions, 32 KiB of LDS per wave (0xFFFF = empty; the largest hashed position
//         of a block is 65 532), five waves to a CU.  On the index's PLAIN text (3.8 MB, 40 images x 20 000 vertices) the streams
//         were 1.049 / 1.023 / 0.992 x the size of Google's Snappy for 12 / 13 / 14 bits: a bucket keeps only its latest position,
//         and the point_to_images lists repeat from several KiB back, where a small table has long forgotten them;
//       - capacity(n) = 32 + n + n / 6 bounds a stream: a literal run of L bytes costs L + 1 (L <= 60), L + 2 (L <= 256) or L + 3
//         bytes and is followed by a copy (>= 4 bytes in <= 3) or the block's end, so a block of b bytes takes at most
//         b + b / 65 + 3.
//   * Pages (parquet format v1, one optional BYTE_ARRAY column without nulls):
//       - page_cuts: a page ends after the first value at which its PLAIN bytes (4 + len per value) reach page_bytes;
//       - a page's payload is u32le(L), L bytes of RLE definition levels -- varint(num_values << 1), then 0x01: one run of level 1
//         at bit width 1 -- and the PLAIN values (u32le(len), bytes).
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
namespace snappy {

constexpr int kHashBits = 14;
constexpr int kTable = 1 << kHashBits;
constexpr int64_t kBlock = 65536;
constexpr int kChunk = 64;                      // positions a wave hashes at once; the rule itself does not depend on it
constexpr uint32_t kEmpty = 0xFFFFu;
constexpr int64_t kMaxStream = 0x7fffffff;     // n of one stream (a varint of at most 5 bytes; int32 arithmetic inside a block)

MSPA_HD int64_t capacity(int64_t n) { return 32 + n + n / 6; }
constexpr int64_t kSlot = (32 + kBlock + kBlock / 6 + 63) / 64 * 64;   // a block's worst-case output, rounded up to 64

MSPA_HD int varint_len(uint64_t v) {
    int k = 1;
    while (v >= 128) {
        v >>= 7;
        ++k;
    }
    return k;
}

// Byte i (< varint_len(v)) of varint(v).
MSPA_HD uint32_t varint_byte(uint64_t v, int i) {
    const uint32_t b = (uint32_t)(v >> (7 * i)) & 127u;
    return (v >> (7 * i)) >= 128 ? b | 128u : b;
}

MSPA_HD int put_varint(uint8_t *dst, uint64_t v) {
    const int k = varint_len(v);
    for (int i = 0; i < k; ++i) dst[i] = (uint8_t)varint_byte(v, i);
    return k;
}

MSPA_HD uint32_t load32(const uint8_t *s) {
    return (uint32_t)s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 | (uint32_t)s[3] << 24;
}

MSPA_HD uint32_t hash(uint32_t v) { return (v * 0x1e35a7bdu) >> (32 - kHashBits); }

// A literal's tag and length bytes (1 <= len <= 65 536); returns their count.  The len bytes themselves follow.
MSPA_HD int put_literal_head(uint8_t *dst, int32_t len) {
    const uint32_t m = (uint32_t)len - 1;
    if (len <= 60) {
        dst[0] = (uint8_t)(m << 2);
        return 1;
    }
    if (len <= 256) {
        dst[0] = (uint8_t)(60u << 2);
        dst[1] = (uint8_t)m;
        return 2;
    }
    dst[0] = (uint8_t)(61u << 2);
    dst[1] = (uint8_t)(m & 255u);
    dst[2] = (uint8_t)(m >> 8);
    return 3;
}

// A copy of len >= 4 bytes from `offset` (1 .. 65 535) back; returns the bytes written.
MSPA_HD int32_t put_copy(uint8_t *dst, int32_t offset, int32_t len) {
    if (len <= 11 && offset < 2048) {
        dst[0] = (uint8_t)(1u | (uint32_t)(len - 4) << 2 | (uint32_t)(offset >> 8) << 5);
        dst[1] = (uint8_t)(offset & 255);
        return 2;
    }
    int32_t o = 0;
    while (len > 0) {
        int32_t piece = len < 64 ? len : 64;
        if (len > 64 && len - 64 < 4) piece = 60;
        dst[o] = (uint8_t)(2u | (uint32_t)(piece - 1) << 2);
        dst[o + 1] = (uint8_t)(offset & 255);
        dst[o + 2] = (uint8_t)(offset >> 8);
        o += 3;
        len -= piece;
    }
    return o;
}

// Length of the match of s[p ..] with s[q ..] (q < p), at most nb - p: the bytes of the block beyond p + 4 are compared one by
// one; the first four are known to be equal.
MSPA_HD int32_t match_len(const uint8_t *s, int32_t q, int32_t p, int32_t nb) {
    int32_t len = 4;
    while (p + len < nb && s[q + len] == s[p + len]) ++len;
    return len;
}

// ---------------------------------------------------------------------------------------------------------------- decoding
// The decoder reads ANY raw Snappy stream (Google's, pyarrow's, this file's): varint(n), then elements until the input ends.
//   tag & 3 == 0  literal: len - 1 = tag >> 2 when that is < 60, else the next (tag >> 2) - 59 bytes (1 .. 4), little endian;
//   tag & 3 == 1  copy-1:  len = 4 + (tag >> 2 & 7), offset = (tag >> 5) << 8 | next byte;
//   tag & 3 == 2  copy-2:  len = 1 + (tag >> 2), offset = next 2 bytes;       tag & 3 == 3  copy-4: the same with 4 offset bytes.
// A copy's source may overlap its target (offset < len): byte i of the copy is byte i mod offset of the `offset` bytes in front.
// The rules below are everything that decides a status; the host loop (decompress) and the device kernel both go through
// them in the same order, so the two decline the same streams with the same code.  Nothing is read outside [src, src + src_len)
// and nothing written outside [dst, dst + expected).
constexpr int kErrPreamble = -16;     // the preamble is not varint(expected) (or does not end inside the input)
constexpr int kErrTruncated = -17;    // an element (its tag, its length / offset bytes or a literal's bytes) runs past the input
constexpr int kErrOverrun = -18;      // an element would write beyond `expected` bytes
constexpr int kErrOffset = -19;       // a copy with offset 0, or one that reaches in front of the output's first byte
constexpr int kErrTrailing = -20;     // input left over after `expected` bytes were written
constexpr int kErrShort = -21;        // the input ended before `expected` bytes were written
// (-22, kNotBlockwise, is block_starts' alone: a valid stream that does not decode block by block -- see below)

struct Element {
    int32_t head;       // tag and length / offset bytes
    int64_t len;        // bytes it writes (>= 1)
    int64_t offset;     // 0 for a literal (whose len bytes follow the head)
    bool literal;
};

// `bytes`: the input's next (up to) 8 bytes, little endian, zero where the input has ended; `avail` >= 1: how many input bytes
// are left.  Returns 0, or kErrTruncated when the head itself is cut off.
MSPA_HD int parse_element(uint64_t bytes, int64_t avail, Element &e) {
    const uint32_t tag = (uint32_t)bytes & 255u, kind = tag & 3u, m = tag >> 2;
    const uint64_t rest = bytes >> 8;
    const int32_t lit_extra = m < 60u ? 0 : (int32_t)m - 59;
    const int32_t extra = kind == 0 ? lit_extra : kind == 1 ? 1 : kind == 2 ? 2 : 4;
    const uint64_t field = rest & (extra == 4 ? 0xFFFFFFFFull : (1ull << (8 * extra)) - 1);      // the length / offset bytes
    const int64_t lit_len = (lit_extra == 0 ? (int64_t)m : (int64_t)field) + 1;
    const int64_t copy_len = kind == 1 ? 4 + (int64_t)(m & 7u) : 1 + (int64_t)m;
    const int64_t copy_offset = kind == 1 ? (int64_t)((uint64_t)(tag >> 5) << 8 | field) : (int64_t)field;
    e.head = 1 + extra;
    e.len = kind == 0 ? lit_len : copy_len;
    e.offset = kind == 0 ? 0 : copy_offset;
    e.literal = kind == 0;
    return e.head > avail ? kErrTruncated : 0;
}

// A parsed element against the input left (`avail`, counted from its tag), the bytes written so far and the stream's size.
MSPA_HD int check_element(const Element &e, int64_t avail, int64_t written, int64_t expected) {
    if (e.literal) {
        if (e.len > avail - e.head) return kErrTruncated;
    } else if (e.offset == 0 || e.offset > written) {
        return kErrOffset;
    }
    return e.len > expected - written ? kErrOverrun : 0;
}

// The preamble: `bytes` / `avail` as for parse_element (avail may be 0).  Returns its length (1 .. 5), or kErrPreamble.
MSPA_HD int parse_preamble(uint64_t bytes, int64_t avail, int64_t expected) {
    uint64_t v = 0;
    for (int i = 0; i < 5 && i < avail; ++i) {
        const uint32_t b = (uint32_t)(bytes >> (8 * i)) & 255u;
        v |= (uint64_t)(b & 127u) << (7 * i);
        if (b < 128u) return v == (uint64_t)expected ? i + 1 : kErrPreamble;
    }
    return kErrPreamble;
}

// The next (up to) 8 bytes of s[p, n), zero beyond n.
MSPA_HD uint64_t load_le(const uint8_t *s, int64_t p, int64_t n) {
    uint64_t v = 0;
    for (int i = 0; i < 8 && p + i < n; ++i) v |= (uint64_t)s[p + i] << (8 * i);
    return v;
}

// The reference: src[0, src_len) -> dst[0, expected).  Returns `expected`, or one of the codes above.
MSPA_HD int64_t decompress(const uint8_t *src, int64_t src_len, uint8_t *dst, int64_t expected) {
    const int pre = parse_preamble(load_le(src, 0, src_len), src_len, expected);
    if (pre < 0) return pre;
    int64_t p = pre, o = 0;
    while (p < src_len) {
        if (o == expected) return kErrTrailing;
        Element e;
        int rc = parse_element(load_le(src, p, src_len), src_len - p, e);
        if (rc == 0) rc = check_element(e, src_len - p, o, expected);
        if (rc != 0) return rc;
        if (e.literal) {
            for (int64_t i = 0; i < e.len; ++i) dst[o + i] = src[p + e.head + i];
            p += e.head + e.len;
        } else {
            for (int64_t i = 0; i < e.len; ++i) dst[o + i] = dst[o + i - e.offset];
            p += e.head;
        }
        o += e.len;
    }
    return o < expected ? kErrShort : o;
}

// ------------------------------------------------------------------------------------------------------- decoding by blocks
// Both writers (this file's by definition, Google's -- pyarrow's -- by what its compressor does) cut the input into blocks of
// kBlock bytes that are compressed independently.  Such a stream is BLOCKWISE: every multiple of kBlock output bytes is an
// element start, no element straddles one, and no copy reaches in front of its block's first byte -- so each block's elements
// decode alone, into their own kBlock bytes.  What a stream does not record is where a block's elements begin in the
// compressed bytes; block_starts is the serial definition of that, decompress_block the decoder of one block.
constexpr int kNotBlockwise = -22;    // a stream the decoder takes, but that is not blockwise (block_starts only)

MSPA_HD int64_t block_count(int64_t expected) { return (expected + kBlock - 1) / kBlock; }

// starts[b] = the compressed position of the element that begins at output b * kBlock, for b < block_count(expected), and
// starts[block_count] = src_len (the last block's end); `cap`: entries of `starts`, nothing is written beyond them.  Returns the
// block count; the code decompress() declines the stream with (whatever else is the matter with it); or kNotBlockwise.
MSPA_HD int64_t block_starts(const uint8_t *src, int64_t src_len, int64_t expected, int64_t *starts, int64_t cap) {
    const int pre = parse_preamble(load_le(src, 0, src_len), src_len, expected);
    if (pre < 0) return pre;
    const int64_t blocks = block_count(expected);
    bool blockwise = true;
    int64_t p = pre, o = 0;
    while (p < src_len) {
        if (o == expected) return kErrTrailing;
        Element e;
        int rc = parse_element(load_le(src, p, src_len), src_len - p, e);
        if (rc == 0) rc = check_element(e, src_len - p, o, expected);
        if (rc != 0) return rc;
        const int64_t in_block = o % kBlock;
        if (in_block == 0 && o / kBlock < cap) starts[o / kBlock] = p;
        if (in_block + e.len > kBlock || (!e.literal && e.offset > in_block)) blockwise = false;
        p += e.head + (e.literal ? e.len : 0);
        o += e.len;
    }
    if (o < expected) return kErrShort;
    if (!blockwise) return kNotBlockwise;
    if (blocks < cap) starts[blocks] = src_len;
    return blocks;
}

// The elements in src[p0, p1) -> dst_block[0, nb): one block of a blockwise stream.  An offset is checked against the bytes
// written in THIS block.  Returns nb, or a code (the elements must fill exactly nb bytes from exactly [p0, p1)).
MSPA_HD int64_t decompress_block(const uint8_t *src, int64_t p0, int64_t p1, uint8_t *dst_block, int64_t nb) {
    int64_t p = p0, o = 0;
    while (p < p1) {
        if (o == nb) return kErrTrailing;
        Element e;
        int rc = parse_element(load_le(src, p, p1), p1 - p, e);
        if (rc == 0) rc = check_element(e, p1 - p, o, nb);
        if (rc != 0) return rc;
        if (e.literal) {
            for (int64_t i = 0; i < e.len; ++i) dst_block[o + i] = src[p + e.head + i];
            p += e.head + e.len;
        } else {
            for (int64_t i = 0; i < e.len; ++i) dst_block[o + i] = dst_block[o + i - e.offset];
            p += e.head;
        }
        o += e.len;
    }
    return o < nb ? kErrShort : o;
}

// ------------------------------------------------------------------------------------------------------------------ pages

// Bytes of the RLE definition levels of a page of nv values (all present).
MSPA_HD int32_t levels_len(int64_t nv) { return varint_len((uint64_t)nv << 1) + 1; }

// Bytes in front of a page's PLAIN values: u32le(L) and the levels.
MSPA_HD int32_t page_head_len(int64_t nv) { return 4 + levels_len(nv); }

// Byte r (< page_head_len(nv)) of a page's head.
MSPA_HD uint32_t page_head_byte(int64_t nv, int32_t r) {
    const int32_t L = levels_len(nv);
    if (r < 4) return ((uint32_t)L >> (8 * r)) & 255u;
    if (r < 4 + L - 1) return varint_byte((uint64_t)nv << 1, r - 4);
    return 1u;
}

// PLAIN bytes in front of value k of a page that starts with value v0 (arrow string offsets).
MSPA_HD int64_t plain_start(const int32_t *offsets, int64_t v0, int64_t k) {
    return 4 * (k - v0) + ((int64_t)offsets[k] - (int64_t)offsets[v0]);
}

// Payload bytes of the page of values [v0, v1).
MSPA_HD int64_t page_payload_len(const int32_t *offsets, int64_t v0, int64_t v1) {
    return page_head_len(v1 - v0) + plain_start(offsets, v0, v1);
}

// Byte r of the PLAIN values of a page starting at v0, r inside value k (plain_start(k) <= r < plain_start(k + 1)).
MSPA_HD uint32_t plain_byte(const int32_t *offsets, const uint8_t *data, int64_t v0, int64_t k, int64_t r) {
    const int64_t rr = r - plain_start(offsets, v0, k);
    if (rr < 4) return ((uint32_t)(offsets[k + 1] - offsets[k]) >> (8 * rr)) & 255u;
    return data[(int64_t)offsets[k] + rr - 4];
}

// The page-cut rule: cuts[0] = 0 < cuts[1] < ... < cuts[pages] = rows; returns the page count, or -1 when `cap` entries do
// not hold the cuts.  cuts may be null to count only.
MSPA_HD int64_t page_cuts(const int32_t *offsets, int64_t rows, int64_t page_bytes, int64_t *cuts, int64_t cap) {
    int64_t pages = 0, acc = 0;
    if (cuts) {
        if (cap < 1) return -1;
        cuts[0] = 0;
    }
    for (int64_t k = 0; k < rows; ++k) {
        acc += 4 + ((int64_t)offsets[k + 1] - (int64_t)offsets[k]);
        if (acc >= page_bytes || k + 1 == rows) {
            ++pages;
            if (cuts) {
                if (pages >= cap) return -1;
                cuts[pages] = k + 1;
            }
            acc = 0;
        }
    }
    return pages;
}

}  // namespace snappy
}  // namespace mspa

// ---------------------------------------------------------------------------------------------------------------- host reference
#include <vector>
namespace mspa {
namespace snappy {

// The elements of one block s[0, nb) (1 <= nb <= kBlock) into dst (>= kSlot bytes); returns their byte count.
inline int32_t compress_block_host(const uint8_t *s, int32_t nb, uint8_t *dst) {
    std::vector<int32_t> cand((size_t)nb, -1);
    std::vector<uint16_t> table((size_t)kTable, (uint16_t)kEmpty);
    for (int32_t p = 0; p + 3 < nb; ++p) {
        const uint32_t h = hash(load32(s + p));
        if (table[h] != kEmpty) cand[(size_t)p] = table[h];
        table[h] = (uint16_t)p;
    }
    int32_t o = 0, lit = 0, p = 0;
    auto flush = [&](int32_t end) {
        if (end > lit) {
            o += put_literal_head(dst + o, end - lit);
            for (int32_t i = lit; i < end; ++i) dst[o++] = s[i];
        }
    };
    while (p < nb) {
        const int32_t q = p + 3 < nb ? cand[(size_t)p] : -1;
        if (q >= 0 && load32(s + q) == load32(s + p)) {
            const int32_t len = match_len(s, q, p, nb);
            flush(p);
            o += put_copy(dst + o, p - q, len);
            p += len;
            lit = p;
        } else {
            ++p;
        }
    }
    flush(nb);
    return o;
}

// A whole stream; dst holds at least capacity(n) bytes.  Returns the stream's length.
inline int64_t compress_host(const uint8_t *src, int64_t n, uint8_t *dst) {
    int64_t o = put_varint(dst, (uint64_t)n);
    std::vector<uint8_t> slot((size_t)kSlot);
    for (int64_t b0 = 0; b0 < n; b0 += kBlock) {
        const int32_t nb = (int32_t)(n - b0 < kBlock ? n - b0 : kBlock);
        const int32_t m = compress_block_host(src + b0, nb, slot.data());
        for (int32_t i = 0; i < m; ++i) dst[o + i] = slot[(size_t)i];
        o += m;
    }
    return o;
}

// The payload of the page of values [v0, v1) into dst (page_payload_len bytes).
inline void page_payload_host(const int32_t *offsets, const uint8_t *data, int64_t v0, int64_t v1, uint8_t *dst) {
    const int32_t head = page_head_len(v1 - v0);
    for (int32_t r = 0; r < head; ++r) dst[r] = (uint8_t)page_head_byte(v1 - v0, r);
    int64_t o = head;
    for (int64_t k = v0; k < v1; ++k) {
        const int64_t end = plain_start(offsets, v0, k + 1);
        for (int64_t r = plain_start(offsets, v0, k); r < end; ++r) dst[o++] = (uint8_t)plain_byte(offsets, data, v0, k, r);
    }
}

}  // namespace snappy
}  // namespace mspa
