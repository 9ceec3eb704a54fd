// 16-bit greyscale PNG encode: the per-image arithmetic shared by the device kernels of png_encode.hip and the host reference.
// Everything that decides an output byte is an MSPA_HD function here, so that a plain C++ build of this header is the
// reference the device must equal byte for byte.
//
//   * Row filters are Pillow's (ZipEncode.c): samples big-endian, bpp 2, a zero row above the first; per row the first strict
//     minimum of sum(min(v, 256 - v)) over None, Up, Sub, Paeth, in that order (Average is never tried).  The filtered stream is
//     therefore what zlib.decompress gives for Pillow's IDAT.
//   * Deflate is this file's own, deterministic algorithm (not zlib's):
//       - the filtered stream of N = h * (1 + 2 w) bytes is cut into segments of kSeg bytes (the last one shorter); each segment
//         becomes one block of a single zlib stream, so back-references reach up to 32 KiB into earlier segments;
//       - match candidates for position p: the distances 1, 2, one row and two rows, then up to kChain links of p's hash
//         chain.  A link goes to the largest q < chunk_start(p) (chunks of kChunk positions) whose 4-byte hash equals p's; a
//         hash bucket keeps only its largest position, so the links do not depend on which segment computes them.  No
//         candidate lies more than 32 768 bytes back;
//       - per segment, a serial lazy parse: the longest candidate match at p (first candidate on a tie; length 3 only within
//         4 096 bytes), or a literal when the match at p + 1 is longer and the match at p is shorter than kLazy;
//       - per segment, length-limited Huffman codes (15 bits, 7 for the code-length code; Moffat-Katajainen lengths, then the
//         Kraft-sum repair, symbols ranked by (frequency, symbol)); a dynamic block, or a stored block when the dynamic one is
//         not shorter than the stored block's worst case (42 + 8 L bits);
//   * The container: signature, IHDR (depth 16, colour type 0, no interlace), IDAT chunks of at most kIdat zlib bytes each
//     (78 9C, the deflate stream, Adler-32), IEND.  Nothing else.
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
namespace pnge {

constexpr int32_t kMaxSide = 8192;      // h, w <= 8192: a filtered stream stays below 2^31 bytes
constexpr int64_t kSeg = 32768;         // filtered-stream bytes per deflate block
constexpr int64_t kWindow = 32768;      // deflate's window
constexpr int kHashBits = 14;
constexpr int kChunk = 64;              // positions whose hash lookups see one table state
constexpr int kChain = 16;              // hash-chain links a match search follows
constexpr int kLazy = 32;               // look one position ahead while the match is shorter than this
constexpr int kTooFar = 4096;           // a 3-byte match only within this distance
constexpr int64_t kIdat = 16384;        // zlib bytes per IDAT chunk (the last one shorter)
constexpr int64_t kHead = 33;           // signature + IHDR
constexpr int kLitSyms = 286, kDistSyms = 30, kClSyms = 19;

constexpr uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
constexpr uint16_t kLenBase[29] = {3,  4,  5,  6,  7,  8,  9,  10, 11,  13,  15,  17,  19,  23, 27,
                                   31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
constexpr uint8_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
constexpr uint16_t kDistBase[30] = {1,   2,   3,   4,   5,   7,    9,    13,   17,   25,   33,   49,   65,    97,    129,
                                    193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
constexpr uint8_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
constexpr uint32_t kAdlerMod = 65521;

MSPA_HD bool valid_size(int64_t h, int64_t w) { return h >= 1 && w >= 1 && h <= kMaxSide && w <= kMaxSide; }

struct Geom {
    int32_t h, w;
    int64_t row;       // 1 + 2 w filtered bytes a row
    int64_t n;         // filtered-stream bytes
    int64_t nseg;      // deflate blocks
    int64_t dcap;      // worst-case deflate bytes
    int64_t nchunk;    // worst-case IDAT chunks
    int64_t cap;       // worst-case file bytes
};

// Capacity: every block is at most 42 + 8 L bits (a dynamic block is kept only when shorter than that; a stored block is
// 3 header bits, <= 7 padding bits, LEN / NLEN and L bytes), so the deflate stream has at most N + ceil(42 nseg / 8) bytes; the
// zlib stream adds 6, the container 33 + 12 per IDAT chunk + 12.
MSPA_HD Geom geom(int32_t h, int32_t w) {
    Geom g;
    g.h = h;
    g.w = w;
    g.row = 1 + 2 * (int64_t)w;
    g.n = (int64_t)h * g.row;
    g.nseg = (g.n + kSeg - 1) / kSeg;
    g.dcap = g.n + (42 * g.nseg + 7) / 8;
    const int64_t zcap = g.dcap + 6;
    g.nchunk = (zcap + kIdat - 1) / kIdat;
    g.cap = kHead + 12 * g.nchunk + zcap + 12;
    return g;
}

// ---------------------------------------------------------------------------------------------------------------- filters

MSPA_HD uint32_t sample_byte(const int16_t *row, int64_t i) {
    const uint32_t s = (uint16_t)row[i >> 1];
    return (i & 1) ? (s & 255u) : (s >> 8);
}

MSPA_HD uint32_t paeth(int32_t a, int32_t b, int32_t c) {
    const int32_t p = a + b - c;
    const int32_t pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    if (pa <= pb && pa <= pc) return (uint32_t)a;
    return pb <= pc ? (uint32_t)b : (uint32_t)c;
}

// Filtered byte i (0 .. 2w-1) of a row under filter f (0 None, 1 Sub, 2 Up, 4 Paeth); prev == nullptr is the zero row.
MSPA_HD uint32_t filtered(const int16_t *cur, const int16_t *prev, int64_t i, int f) {
    const uint32_t x = sample_byte(cur, i);
    const uint32_t a = i >= 2 ? sample_byte(cur, i - 2) : 0;
    const uint32_t b = prev ? sample_byte(prev, i) : 0;
    const uint32_t c = (prev && i >= 2) ? sample_byte(prev, i - 2) : 0;
    uint32_t v = x;
    if (f == 1) v = x - a;
    else if (f == 2) v = x - b;
    else if (f == 4) v = x - paeth((int32_t)a, (int32_t)b, (int32_t)c);
    return v & 255u;
}

MSPA_HD uint32_t filter_cost(uint32_t v) { return v < 128 ? v : 256 - v; }

// Pillow's choice: the first strict minimum over None, Up, Sub, Paeth.
MSPA_HD int choose_filter(const int16_t *cur, const int16_t *prev, int32_t w) {
    uint64_t s0 = 0, s1 = 0, s2 = 0, s4 = 0;
    for (int64_t i = 0; i < 2 * (int64_t)w; ++i) {
        s0 += filter_cost(filtered(cur, prev, i, 0));
        s1 += filter_cost(filtered(cur, prev, i, 1));
        s2 += filter_cost(filtered(cur, prev, i, 2));
        s4 += filter_cost(filtered(cur, prev, i, 4));
    }
    int f = 0;
    uint64_t best = s0;
    if (s2 < best) { f = 2; best = s2; }
    if (s1 < best) { f = 1; best = s1; }
    if (s4 < best) f = 4;
    return f;
}

MSPA_HD void filter_row(const int16_t *cur, const int16_t *prev, int32_t w, uint8_t *out) {
    const int f = choose_filter(cur, prev, w);
    out[0] = (uint8_t)f;
    for (int64_t i = 0; i < 2 * (int64_t)w; ++i) out[1 + i] = (uint8_t)filtered(cur, prev, i, f);
}

// ---------------------------------------------------------------------------------------------------------------- matches

MSPA_HD uint32_t hash4(const uint8_t *s, int64_t p) {
    const uint32_t v = (uint32_t)s[p] | (uint32_t)s[p + 1] << 8 | (uint32_t)s[p + 2] << 16 | (uint32_t)s[p + 3] << 24;
    return (v * 0x9E3779B1u) >> (32 - kHashBits);
}

// prev[p]: the distance back to the bucket's largest position q < chunk_start(p) (-1: none), 0 when there is none or it is
// more than 32 767 bytes back.  Following prev from p walks p's hash chain (at chunk granularity: positions of one chunk do
// not link to each other).
MSPA_HD uint16_t chain_link(int64_t p, int64_t q) { return (q >= 0 && p - q < kWindow) ? (uint16_t)(p - q) : (uint16_t)0; }

MSPA_HD int match_len(const uint8_t *s, int64_t p, int64_t d, int64_t lim) {
    int k = 0;
    while (k < lim && s[p + k] == s[p + k - d]) ++k;
    return k;
}

// Longest match at p, at most min(258, s1 - p) long, over the distances 1, 2, row, 2 row, then up to kChain links of p's hash
// chain; every candidate lies within the stream and within the 32 768-byte window; the first candidate wins a tie.  L = 0 when there is none of length >= 3 (or length 3 beyond
// kTooFar).
MSPA_HD void best_at(const uint8_t *s, const uint16_t *prev, int64_t p, int64_t s1, int64_t row, int &L, int &D) {
    L = 0;
    D = 0;
    const int64_t lim = s1 - p < 258 ? s1 - p : 258;
    if (lim < 3) return;
    int64_t q = p;
    for (int k = 0; k < 4 + kChain && L < lim; ++k) {
        int64_t d;
        if (k < 4) {
            d = k < 2 ? k + 1 : (k - 1) * row;
        } else {
            const int64_t link = prev[q];
            if (!link) break;
            q -= link;
            d = p - q;
            if (d > kWindow) break;
        }
        if (d > p || d > kWindow) continue;                 // before the stream, or beyond deflate's window (2 rows at w > 8191)
        if (L && s[p + L] != s[p + L - d]) continue;       // cannot be longer than L
        const int l = match_len(s, p, d, lim);
        if (l > L) {
            L = l;
            D = (int)d;
        }
    }
    if (L < 3 || (L == 3 && D > kTooFar)) L = 0;
}

// Tokens: a literal is its byte; a match is 0x80000000 | (length - 3) << 16 | (distance - 1), 3 <= length <= 258 and
// 1 <= distance <= 32 768 (best_at never returns more), so the distance fits its 15 bits.
MSPA_HD uint32_t match_token(int L, int D) { return 0x80000000u | (uint32_t)(L - 3) << 16 | (uint32_t)(D - 1); }

// The lazy parse of [s0, s1) into tok[0 ..); returns the token count.
MSPA_HD uint32_t parse_segment(const uint8_t *s, const uint16_t *prev, int64_t s0, int64_t s1, int64_t row, uint32_t *tok) {
    int64_t p = s0;
    uint32_t t = 0;
    int L, D;
    best_at(s, prev, p, s1, row, L, D);
    while (p < s1) {
        if (L) {
            if (L < kLazy && p + 1 < s1) {
                int L2, D2;
                best_at(s, prev, p + 1, s1, row, L2, D2);
                if (L2 > L) {
                    tok[t++] = s[p];
                    ++p;
                    L = L2;
                    D = D2;
                    continue;
                }
            }
            tok[t++] = match_token(L, D);
            p += L;
        } else {
            tok[t++] = s[p];
            ++p;
        }
        if (p < s1) best_at(s, prev, p, s1, row, L, D);
    }
    return t;
}

MSPA_HD int floor_log2(uint32_t v) {
    int k = 0;
    while (v >> (k + 1)) ++k;
    return k;
}

MSPA_HD int len_code(int L) {                   // 0..28 (symbol 257 + code)
    const int lm = L - 3;
    if (lm < 8) return lm;
    if (L == 258) return 28;
    const int k = floor_log2((uint32_t)lm);
    return 4 * k - 4 + ((lm >> (k - 2)) & 3);
}

MSPA_HD int dist_code(int D) {                  // 0..29
    const int dm = D - 1;
    if (dm < 4) return dm;
    const int k = floor_log2((uint32_t)dm);
    return 2 * k + ((dm >> (k - 1)) & 1);
}

// ---------------------------------------------------------------------------------------------------------------- blocks

enum : int32_t { kStored = 0, kDynamic = 2 };

struct Block {
    uint32_t freq[kLitSyms];
    uint32_t dfreq[kDistSyms];
    uint32_t clfreq[kClSyms];
    uint32_t key[kLitSyms];                     // Huffman scratch: (frequency << 9 | symbol), then lengths
    uint32_t depth[kLitSyms];
    int32_t num[48];                            // Huffman scratch: codes per length, then canonical-code counters
    uint16_t code[kLitSyms];                    // bit-reversed canonical codes
    uint16_t dcode[kDistSyms];
    uint16_t clcode[kClSyms];
    uint8_t len[kLitSyms];
    uint8_t dlen[kDistSyms];
    uint8_t cllen[kClSyms];
    uint8_t pad_[1];
    uint32_t ntok, adler_a, adler_b;
    int32_t type, hlit, hdist, hclen, pad2_;
    int64_t bits;                               // dynamic: exact; stored: the worst case 42 + 8 L
    int64_t off;                                // bit offset in the image's deflate stream
};

MSPA_HD void count_tokens(const uint32_t *tok, uint32_t ntok, Block &b) {
    for (int i = 0; i < kLitSyms; ++i) b.freq[i] = 0;
    for (int i = 0; i < kDistSyms; ++i) b.dfreq[i] = 0;
    for (uint32_t t = 0; t < ntok; ++t) {
        const uint32_t v = tok[t];
        if (v & 0x80000000u) {
            ++b.freq[257 + len_code((int)((v >> 16) & 255) + 3)];
            ++b.dfreq[dist_code((int)(v & 0x7FFF) + 1)];
        } else {
            ++b.freq[v];
        }
    }
    b.freq[256] = 1;
}

// Adler-32 partial sums of a segment: A = sum x_i, B = sum (L - i) x_i (mod 65521).
MSPA_HD void adler_partial(const uint8_t *x, int64_t L, uint32_t &A, uint32_t &B) {
    uint64_t a = 0, b = 0;
    for (int64_t i = 0; i < L; ++i) {
        a += x[i];
        b += (uint64_t)(L - i) * x[i];
    }
    A = (uint32_t)(a % kAdlerMod);
    B = (uint32_t)(b % kAdlerMod);
}

// The stream's Adler-32 from the segments' partial sums (segment s starts at s * kSeg).
MSPA_HD uint32_t adler_combine(const Block *blk, int64_t nseg, int64_t n) {
    uint64_t a = 1, b = (uint64_t)(n % kAdlerMod);
    for (int64_t s = 0; s < nseg; ++s) {
        const int64_t s0 = s * kSeg, L = (s0 + kSeg < n ? kSeg : n - s0);
        a += blk[s].adler_a;
        b += blk[s].adler_b + (uint64_t)((n - s0 - L) % kAdlerMod) * blk[s].adler_a;
        a %= kAdlerMod;
        b %= kAdlerMod;
    }
    return (uint32_t)(b << 16 | a);
}

// Code lengths (<= limit) for freq[0..n); `key` and `A` are n-entry scratch, `num` 33 entries.  Fewer than two used symbols get two 1-bit
// codes (the used one and the lowest unused), so every code is complete.
MSPA_HD void huff_lengths(const uint32_t *freq, int n, int limit, uint8_t *len, uint32_t *key, uint32_t *A, int32_t *num) {
    int m = 0;
    for (int i = 0; i < n; ++i) {
        len[i] = 0;
        if (freq[i]) key[m++] = freq[i] << 9 | (uint32_t)i;
    }
    if (m < 2) {
        const int used = m ? (int)(key[0] & 511) : -1;
        int other = 0;
        while (other == used) ++other;
        if (used >= 0) len[used] = 1;
        len[other] = 1;
        if (m == 0) len[other == 0 ? 1 : 0] = 1;
        return;
    }
    // heap sort of the keys, ascending
    for (int start = m / 2 - 1; start >= 0; --start) {
        int r = start;
        while (2 * r + 1 < m) {
            int c = 2 * r + 1;
            if (c + 1 < m && key[c + 1] > key[c]) ++c;
            if (key[r] >= key[c]) break;
            const uint32_t t = key[r]; key[r] = key[c]; key[c] = t;
            r = c;
        }
    }
    for (int end = m - 1; end > 0; --end) {
        const uint32_t t = key[0]; key[0] = key[end]; key[end] = t;
        int r = 0;
        while (2 * r + 1 < end) {
            int c = 2 * r + 1;
            if (c + 1 < end && key[c + 1] > key[c]) ++c;
            if (key[r] >= key[c]) break;
            const uint32_t u = key[r]; key[r] = key[c]; key[c] = u;
            r = c;
        }
    }
    // Moffat-Katajainen in-place minimum-redundancy code lengths over the sorted frequencies
    for (int i = 0; i < m; ++i) A[i] = key[i] >> 9;
    {
        int root = 0, leaf = 2, next;
        A[0] += A[1];
        for (next = 1; next < m - 1; ++next) {
            if (leaf >= m || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = (uint32_t)next; }
            else A[next] = A[leaf++];
            if (leaf >= m || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = (uint32_t)next; }
            else A[next] += A[leaf++];
        }
        A[m - 2] = 0;
        for (next = m - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
        int avbl = 1, used = 0, dpth = 0;
        root = m - 2;
        next = m - 1;
        while (avbl > 0) {
            while (root >= 0 && (int)A[root] == dpth) { ++used; --root; }
            while (avbl > used) { A[next--] = (uint32_t)dpth; --avbl; }
            avbl = 2 * used;
            ++dpth;
            used = 0;
        }
    }
    // lengths above the limit -> the limit, then repair the Kraft sum
    for (int i = 0; i <= 32; ++i) num[i] = 0;
    for (int i = 0; i < m; ++i) ++num[A[i] > (uint32_t)limit ? limit : (int)A[i]];
    uint32_t total = 0;
    for (int i = limit; i > 0; --i) total += (uint32_t)num[i] << (limit - i);
    while (total != (1u << limit)) {
        --num[limit];
        for (int i = limit - 1; i > 0; --i)
            if (num[i]) {
                --num[i];
                num[i + 1] += 2;
                break;
            }
        --total;
    }
    // the most frequent symbols take the shortest codes
    int j = m;
    for (int l = 1; l <= limit; ++l)
        for (int c = num[l]; c > 0; --c) len[key[--j] & 511] = (uint8_t)l;
}

MSPA_HD void canonical_codes(const uint8_t *len, int n, uint16_t *code, int32_t *scratch) {
    int32_t *count = scratch, *next = scratch + 16;
    for (int i = 0; i < 16; ++i) count[i] = 0;
    for (int i = 0; i < n; ++i) ++count[len[i]];
    count[0] = 0;
    int c = 0;
    next[0] = 0;
    for (int b = 1; b < 16; ++b) {
        c = (c + count[b - 1]) << 1;
        next[b] = c;
    }
    for (int i = 0; i < n; ++i) {
        const int l = len[i];
        uint32_t v = 0;
        if (l) {
            const uint32_t cv = (uint32_t)next[l]++;
            for (int k = 0; k < l; ++k) v |= ((cv >> k) & 1u) << (l - 1 - k);
        }
        code[i] = (uint16_t)v;
    }
}

// Run-length coding of the hlit + hdist code lengths (runs may cross from the literal / length into the distance lengths):
// emit(symbol, extra value, extra bits).  Zero runs: 18 while >= 11 (<= 138), then 17 for 3..10, then single zeros; other
// runs: the length itself, then 16 while >= 3 of the rest remain (<= 6), then single copies.
template <class F>
MSPA_HD void rle_lengths(const Block &b, F &&emit) {
    const int total = b.hlit + b.hdist;
    int i = 0;
    while (i < total) {
        const int v = i < b.hlit ? b.len[i] : b.dlen[i - b.hlit];
        int run = 1;
        while (i + run < total && (i + run < b.hlit ? b.len[i + run] : b.dlen[i + run - b.hlit]) == v) ++run;
        i += run;
        if (v == 0) {
            while (run >= 11) {
                const int r = run < 138 ? run : 138;
                emit(18, r - 11, 7);
                run -= r;
            }
            if (run >= 3) {
                emit(17, run - 3, 3);
                run = 0;
            }
            while (run > 0) { emit(0, 0, 0); --run; }
        } else {
            emit(v, 0, 0);
            --run;
            while (run >= 3) {
                const int r = run < 6 ? run : 6;
                emit(16, r - 3, 2);
                run -= r;
            }
            while (run > 0) { emit(v, 0, 0); --run; }
        }
    }
}

struct ClCounter {
    uint32_t *f;
    MSPA_HD void operator()(int sym, int, int) const { ++f[sym]; }
};

// Codes, block type and bit length of a segment of L bytes whose histograms are in b.freq / b.dfreq.
MSPA_HD void plan_block(Block &b, int64_t L) {
    huff_lengths(b.freq, kLitSyms, 15, b.len, b.key, b.depth, b.num);
    huff_lengths(b.dfreq, kDistSyms, 15, b.dlen, b.key, b.depth, b.num);
    b.hlit = kLitSyms;
    while (b.hlit > 257 && b.len[b.hlit - 1] == 0) --b.hlit;
    b.hdist = kDistSyms;
    while (b.hdist > 1 && b.dlen[b.hdist - 1] == 0) --b.hdist;
    for (int i = 0; i < kClSyms; ++i) b.clfreq[i] = 0;
    rle_lengths(b, ClCounter{b.clfreq});
    huff_lengths(b.clfreq, kClSyms, 7, b.cllen, b.key, b.depth, b.num);
    b.hclen = kClSyms;
    while (b.hclen > 4 && b.cllen[kClOrder[b.hclen - 1]] == 0) --b.hclen;
    canonical_codes(b.len, kLitSyms, b.code, b.num);
    canonical_codes(b.dlen, kDistSyms, b.dcode, b.num);
    canonical_codes(b.cllen, kClSyms, b.clcode, b.num);
    int64_t bits = 3 + 5 + 5 + 4 + 3 * (int64_t)b.hclen;
    for (int i = 0; i < kClSyms; ++i) bits += (int64_t)b.clfreq[i] * (b.cllen[i] + (i == 16 ? 2 : i == 17 ? 3 : i == 18 ? 7 : 0));
    for (int i = 0; i < kLitSyms; ++i) bits += (int64_t)b.freq[i] * (b.len[i] + (i >= 257 ? kLenExtra[i - 257] : 0));
    for (int i = 0; i < kDistSyms; ++i) bits += (int64_t)b.dfreq[i] * (b.dlen[i] + kDistExtra[i]);
    const int64_t stored = 42 + 8 * L;
    if (bits < stored) {
        b.type = kDynamic;
        b.bits = bits;
    } else {
        b.type = kStored;
        b.bits = stored;
    }
}

// The bits a block takes when it starts at bit `off`.
MSPA_HD int64_t block_bits_at(const Block &b, int64_t off, int64_t L) {
    if (b.type == kDynamic) return b.bits;
    return 3 + ((8 - ((off + 3) & 7)) & 7) + 32 + 8 * L;
}

template <class W>
struct ClEmitter {
    const Block &b;
    W &wr;
    MSPA_HD void operator()(int sym, int extra, int nextra) const {
        wr.put(b.clcode[sym], b.cllen[sym]);
        if (nextra) wr.put((uint32_t)extra, nextra);
    }
};

// Writes segment [s0, s0 + L) as one block; W has put(bits, n <= 16) and align() (to a byte boundary).
template <class W>
MSPA_HD void emit_block(const Block &b, const uint32_t *tok, const uint8_t *seg, int64_t L, bool last, W &wr) {
    wr.put(last ? 1u : 0u, 1);
    if (b.type == kStored) {
        wr.put(0, 2);
        wr.align();
        wr.put((uint32_t)L, 16);
        wr.put((uint32_t)(~L) & 0xFFFFu, 16);
        for (int64_t i = 0; i < L; ++i) wr.put(seg[i], 8);
        return;
    }
    wr.put(2, 2);
    wr.put((uint32_t)(b.hlit - 257), 5);
    wr.put((uint32_t)(b.hdist - 1), 5);
    wr.put((uint32_t)(b.hclen - 4), 4);
    for (int i = 0; i < b.hclen; ++i) wr.put(b.cllen[kClOrder[i]], 3);
    rle_lengths(b, ClEmitter<W>{b, wr});
    for (uint32_t t = 0; t < b.ntok; ++t) {
        const uint32_t v = tok[t];
        if (v & 0x80000000u) {
            const int L3 = (int)((v >> 16) & 255), D = (int)(v & 0x7FFF) + 1;
            const int lc = len_code(L3 + 3), dc = dist_code(D);
            wr.put(b.code[257 + lc], b.len[257 + lc]);
            if (kLenExtra[lc]) wr.put((uint32_t)(L3 + 3 - kLenBase[lc]), kLenExtra[lc]);
            wr.put(b.dcode[dc], b.dlen[dc]);
            if (kDistExtra[dc]) wr.put((uint32_t)(D - kDistBase[dc]), kDistExtra[dc]);
        } else {
            wr.put(b.code[v], b.len[v]);
        }
    }
    wr.put(b.code[256], b.len[256]);
}

// ---------------------------------------------------------------------------------------------------------------- container

struct FileInfo {
    int64_t dbytes;    // deflate stream bytes
    int64_t zlen;      // zlib stream bytes: 2 + dbytes + 4
    int64_t nchunk;    // IDAT chunks
    int64_t flen;      // file bytes
    uint32_t adler;
    uint32_t ihdr_crc;
};

MSPA_HD uint32_t crc_entry(uint32_t k) {
    uint32_t c = k;
    for (int i = 0; i < 8; ++i) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    return c;
}

MSPA_HD uint32_t crc_step(const uint32_t *tab, uint32_t c, uint32_t byte) { return tab[(c ^ byte) & 255] ^ (c >> 8); }

MSPA_HD uint32_t be_byte(uint32_t v, int64_t k) { return (v >> (8 * (3 - k))) & 255u; }

// IHDR's 17 CRC'd bytes ("IHDR" + 13 data bytes).
MSPA_HD uint32_t ihdr_byte(int32_t h, int32_t w, int i) {
    if (i < 4) return be_byte(0x49484452u, i);   // "IHDR"
    if (i < 8) return ((uint32_t)w >> (8 * (7 - i))) & 255u;
    if (i < 12) return ((uint32_t)h >> (8 * (11 - i))) & 255u;
    return i == 12 ? 16u : 0u;                  // depth 16; colour type, compression, filter, interlace 0
}

MSPA_HD uint32_t ihdr_crc(const uint32_t *tab, int32_t h, int32_t w) {
    uint32_t c = 0xFFFFFFFFu;
    for (int i = 0; i < 17; ++i) c = crc_step(tab, c, ihdr_byte(h, w, i));
    return ~c;
}

MSPA_HD FileInfo file_info(int64_t dbits, uint32_t adler, uint32_t ihdr_crc_value) {
    FileInfo f;
    f.dbytes = (dbits + 7) / 8;
    f.zlen = f.dbytes + 6;
    f.nchunk = (f.zlen + kIdat - 1) / kIdat;
    f.flen = kHead + 12 * f.nchunk + f.zlen + 12;
    f.adler = adler;
    f.ihdr_crc = ihdr_crc_value;
    return f;
}

// Byte i of the zlib stream: 78 9C, the deflate bytes, the Adler-32 (big-endian).
MSPA_HD uint32_t zlib_byte(const FileInfo &f, const uint8_t *dbuf, int64_t i) {
    if (i == 0) return 0x78;
    if (i == 1) return 0x9C;
    if (i < 2 + f.dbytes) return dbuf[i - 2];
    return (f.adler >> (8 * (3 - (i - 2 - f.dbytes)))) & 255u;
}

MSPA_HD int64_t chunk_len(const FileInfo &f, int64_t j) { return j + 1 < f.nchunk ? kIdat : f.zlen - j * kIdat; }

// CRC-32 of IDAT chunk j ("IDAT" + its zlib bytes).
MSPA_HD uint32_t chunk_crc(const uint32_t *tab, const FileInfo &f, const uint8_t *dbuf, int64_t j) {
    uint32_t c = 0xFFFFFFFFu;
    c = crc_step(tab, c, 'I');
    c = crc_step(tab, c, 'D');
    c = crc_step(tab, c, 'A');
    c = crc_step(tab, c, 'T');
    const int64_t z0 = j * kIdat, n = chunk_len(f, j);
    for (int64_t i = 0; i < n; ++i) c = crc_step(tab, c, zlib_byte(f, dbuf, z0 + i));
    return ~c;
}

// Byte i (< f.flen) of the file; crcs[j] = chunk_crc(j).
MSPA_HD uint32_t file_byte(int32_t h, int32_t w, const FileInfo &f, const uint8_t *dbuf, const uint32_t *crcs, int64_t i) {
    if (i < 8) return be_byte(i < 4 ? 0x89504E47u : 0x0D0A1A0Au, i & 3);   // the signature
    if (i < 12) return be_byte(13, i - 8);
    if (i < 29) return ihdr_byte(h, w, (int)(i - 12));
    if (i < kHead) return be_byte(f.ihdr_crc, i - 29);
    const int64_t iend = kHead + 12 * f.nchunk + f.zlen;
    if (i >= iend) {
        const int64_t r = i - iend;                 // IEND: length 0, "IEND", its CRC
        return r < 4 ? 0u : be_byte(r < 8 ? 0x49454E44u : 0xAE426082u, r & 3);
    }
    const int64_t r = i - kHead, j = r / (kIdat + 12), k = r % (kIdat + 12), n = chunk_len(f, j);
    if (k < 4) return be_byte((uint32_t)n, k);
    if (k < 8) return be_byte(0x49444154u, k - 4);   // "IDAT"
    if (k < 8 + n) return zlib_byte(f, dbuf, j * kIdat + k - 8);
    return be_byte(crcs[j], k - 8 - n);
}

// ---------------------------------------------------------------------------------------------------------------- host reference

#ifndef __HIP_DEVICE_COMPILE__
// Bit writer of the host reference: ORs LSB-first bits into a zeroed byte buffer.
struct HostBitWriter {
    uint8_t *dst;
    int64_t pos;
    MSPA_HD void put(uint32_t bits, int n) {
        for (int k = 0; k < n; ++k, ++pos)
            if ((bits >> k) & 1u) dst[pos >> 3] |= (uint8_t)(1u << (pos & 7));
    }
    MSPA_HD void align() { pos = (pos + 7) & ~(int64_t)7; }
};
#endif

}  // namespace pnge
}  // namespace mspa

#ifndef __HIP_DEVICE_COMPILE__
#include <vector>
namespace mspa {
namespace pnge {

// A whole file, serially: the reference form of what the kernels compute.  img = [h, w] uint16 stored as int16; dst holds
// at least geom(h, w).cap bytes.  Returns the file's length.  `filtered_out`, when given, receives the filtered stream.
inline int64_t encode_file_host(const int16_t *img, int32_t h, int32_t w, uint8_t *dst, uint8_t *filtered_out = nullptr) {
    const Geom g = geom(h, w);
    std::vector<uint8_t> s((size_t)g.n);
    for (int32_t y = 0; y < h; ++y)
        filter_row(img + (int64_t)y * w, y ? img + (int64_t)(y - 1) * w : nullptr, w, s.data() + y * g.row);
    if (filtered_out)
        for (int64_t i = 0; i < g.n; ++i) filtered_out[i] = s[(size_t)i];
    std::vector<uint16_t> prev((size_t)g.n);
    std::vector<uint32_t> tok((size_t)g.n);
    std::vector<int32_t> head((size_t)1 << kHashBits, -1);
    for (int64_t c0 = 0; c0 < g.n; c0 += kChunk) {
        const int64_t c1 = c0 + kChunk < g.n ? c0 + kChunk : g.n;
        for (int64_t p = c0; p < c1; ++p) prev[(size_t)p] = p + 4 <= g.n ? chain_link(p, head[hash4(s.data(), p)]) : 0;
        for (int64_t p = c0; p < c1; ++p)
            if (p + 4 <= g.n) head[hash4(s.data(), p)] = (int32_t)p;
    }
    std::vector<Block> blk((size_t)g.nseg);
    int64_t off = 0;
    for (int64_t sg = 0; sg < g.nseg; ++sg) {
        Block &b = blk[(size_t)sg];
        const int64_t s0 = sg * kSeg, L = s0 + kSeg < g.n ? kSeg : g.n - s0;
        b.ntok = parse_segment(s.data(), prev.data(), s0, s0 + L, g.row, tok.data() + s0);
        count_tokens(tok.data() + s0, b.ntok, b);
        adler_partial(s.data() + s0, L, b.adler_a, b.adler_b);
        plan_block(b, L);
        b.off = off;
        off += block_bits_at(b, off, L);
    }
    std::vector<uint8_t> dbuf((size_t)((off + 7) / 8), 0);
    for (int64_t sg = 0; sg < g.nseg; ++sg) {
        const Block &b = blk[(size_t)sg];
        const int64_t s0 = sg * kSeg, L = s0 + kSeg < g.n ? kSeg : g.n - s0;
        HostBitWriter wr{dbuf.data(), b.off};
        emit_block(b, tok.data() + s0, s.data() + s0, L, sg + 1 == g.nseg, wr);
    }
    uint32_t tab[256];
    for (uint32_t k = 0; k < 256; ++k) tab[k] = crc_entry(k);
    const FileInfo f = file_info(off, adler_combine(blk.data(), g.nseg, g.n), ihdr_crc(tab, h, w));
    std::vector<uint32_t> crcs((size_t)f.nchunk);
    for (int64_t j = 0; j < f.nchunk; ++j) crcs[(size_t)j] = chunk_crc(tab, f, dbuf.data(), j);
    for (int64_t i = 0; i < f.flen; ++i) dst[i] = (uint8_t)file_byte(h, w, f, dbuf.data(), crcs.data(), i);
    return f.flen;
}

}  // namespace pnge
}  // namespace mspa
#endif
