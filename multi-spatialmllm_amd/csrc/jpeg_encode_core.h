// Baseline JPEG encode: the per-image arithmetic shared by the device kernels of jpeg_encode.hip and the host header writer.
// Everything that decides an output byte is an MSPA_HD function here, so that a plain C++ build of this header can be checked
// against Pillow / libjpeg-turbo on a CPU.  The arithmetic restates libjpeg's documented default compression of an RGB image
// (`Image.fromarray(rgb).save(f, "JPEG", quality=q, subsampling=s)`):
//   * JFIF APP0 1.1 (density 1:1, no units), one DQT per table, SOF0, the four standard DHTs (DC0, AC0, DC1, AC1), SOS;
//   * the Annex K quantisation tables scaled by jpeg_quality_scaling, clamped to 255 (force_baseline);
//   * RGB -> YCbCr in 16-bit fixed point (jccolor.c: ONE_HALF rounding for Y, ONE_HALF - 1 for Cb / Cr);
//   * the edges replicated right to the downsampler's input width and down to a whole iMCU; h2v1 / h2v2 box downsampling with
//     the alternating biases 0/1 and 1/2 (jcsample.c); blocks past a component's width_in_blocks / height_in_blocks are dummy
//     blocks (zero ACs, the quantised DC of the preceding block of the MCU: jccoefct.c);
//   * the JDCT_ISLOW forward DCT (jfdctint.c: 13-bit constants, PASS1_BITS 2, input centred on 128);
//   * quantisation in libjpeg-turbo's reciprocal / correction / shift form with divisors q << 3 (jcdctmgr.c);
//   * Huffman coding with the Annex K tables, per-component DC prediction in MCU order, ZRL runs, EOB, 0xFF00 stuffing and
//     1-bit padding before EOI (jchuff.c).
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
#ifdef __HIPCC__
#define MSPA_UNROLL _Pragma("unroll")
#else
#define MSPA_UNROLL
#endif

namespace mspa {
namespace jpege {

enum : int32_t { k444 = 0, k422 = 1, k420 = 2 };      // Pillow's subsampling = 0 / 1 / 2

constexpr int kHeaderBytes = 623;                     // SOI + APP0 + 2 DQT + SOF0 + 4 DHT + SOS, every accepted (h, w, q, s)
constexpr int kMaxBlockBits = 1664;                   // >= 22 (DC) + 63 * 26 (AC: 16-bit code + 10 bits): 208 bytes a block

// zig-zag position -> natural (row-major) index
constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Annex K.1 / K.2, natural order
constexpr uint8_t kStdQuant[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
     14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// Annex K.3: code counts per length 1..16, then the symbols.  Index: 0 DC luma, 1 AC luma, 2 DC chroma, 3 AC chroma.
constexpr uint8_t kHuffBits[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                      {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
                                      {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
                                      {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr uint8_t kHuffValsDc[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kHuffValsAcLuma[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
constexpr uint8_t kHuffValsAcChroma[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

MSPA_HD const uint8_t *huff_vals(int t) {
    return (t & 1) ? (t == 1 ? kHuffValsAcLuma : kHuffValsAcChroma) : kHuffValsDc;
}

// Block geometry of one image (jcmaster.c's per-component sizes).  Component 0 is Y with (hm, vm); Cb and Cr are 1x1.
struct Geometry {
    int32_t h, w, hm, vm;
    int32_t mcus_x, mcus_y, blocks_per_mcu;
    int32_t bw[2], bh[2];          // width_in_blocks / height_in_blocks: [0] luma, [1] chroma (the real blocks)
};

MSPA_HD bool valid_args(int32_t h, int32_t w, int32_t quality, int32_t ss) {
    return h >= 1 && h <= 65535 && w >= 1 && w <= 65535 && quality >= 1 && quality <= 100 && ss >= k444 && ss <= k420;
}

MSPA_HD Geometry geometry(int32_t h, int32_t w, int32_t ss) {
    Geometry g;
    g.h = h;
    g.w = w;
    g.hm = ss == k444 ? 1 : 2;
    g.vm = ss == k420 ? 2 : 1;
    g.mcus_x = (w + 8 * g.hm - 1) / (8 * g.hm);
    g.mcus_y = (h + 8 * g.vm - 1) / (8 * g.vm);
    g.blocks_per_mcu = g.hm * g.vm + 2;
    g.bw[0] = (w + 7) / 8;
    g.bh[0] = (h + 7) / 8;
    const int32_t cw = (w + g.hm - 1) / g.hm, ch = (h + g.vm - 1) / g.vm;     // downsampled_width / height
    g.bw[1] = (cw + 7) / 8;
    g.bh[1] = (ch + 7) / 8;
    return g;
}

MSPA_HD int64_t mcus(const Geometry &g) { return (int64_t)g.mcus_x * g.mcus_y; }
MSPA_HD int64_t blocks(const Geometry &g) { return mcus(g) * g.blocks_per_mcu; }

// Worst case of one file: header, every block at kMaxBlockBits with every byte stuffed, EOI.
MSPA_HD int64_t capacity(const Geometry &g) { return kHeaderBytes + blocks(g) * (kMaxBlockBits / 8) * 2 + 2; }

// Quantisation and Huffman tables of one quality: what the kernels read.
struct Tables {
    uint16_t qval[2][64];          // natural order, force_baseline
    uint16_t recip[2][64];         // libjpeg-turbo's reciprocal of the divisor qval << 3
    uint16_t corr[2][64];          // its correction (rounding) term
    uint8_t shift[2][64];          // and the total right shift r
    uint16_t dc_code[2][12];
    uint8_t dc_len[2][12];
    uint16_t ac_code[2][256];
    uint8_t ac_len[2][256];
};

// jcparam.c: jpeg_quality_scaling, then jpeg_add_quant_table with force_baseline.
MSPA_HD int quality_scale(int quality) {
    if (quality <= 0) quality = 1;
    if (quality > 100) quality = 100;
    return quality < 50 ? 5000 / quality : 200 - quality * 2;
}

MSPA_HD uint16_t scaled_qval(int table, int i, int scale) {
    int64_t t = ((int64_t)kStdQuant[table][i] * scale + 50) / 100;
    if (t <= 0) t = 1;
    if (t > 255) t = 255;
    return (uint16_t)t;
}

// jcdctmgr.c compute_reciprocal for a 16-bit DCTELEM: divisor d >= 8 here, so the SIMD form applies.
MSPA_HD void reciprocal(uint32_t d, uint16_t &recip, uint16_t &corr, uint8_t &shift) {
    int b = 0;
    while ((d >> (b + 1)) != 0) ++b;                  // floor(log2 d)
    int r = 16 + b;
    uint32_t fq = (uint32_t)((1ull << r) / d), fr = (uint32_t)((1ull << r) % d);
    uint32_t c = d / 2;
    if (fr == 0) {                                    // a power of two: fq would not fit 16 bits
        fq >>= 1;
        --r;
    } else if (fr <= d / 2) {
        ++c;
    } else {
        ++fq;
    }
    recip = (uint16_t)fq;
    corr = (uint16_t)c;
    shift = (uint8_t)r;
}

MSPA_HD int16_t quantize(int32_t v, uint32_t recip, uint32_t corr, uint32_t shift) {
    const uint32_t a = (uint32_t)(v < 0 ? -v : v);
    const int32_t q = (int32_t)(((uint64_t)(a + corr) * recip) >> shift);
    return (int16_t)(v < 0 ? -q : q);
}

// jchuff.c jpeg_make_c_derived_tbl: canonical codes of the standard table t (0 DC luma, 1 AC luma, 2 DC chroma, 3 AC chroma).
MSPA_HD void derive_huff(int t, uint16_t *code_of, uint8_t *len_of) {
    const uint8_t *vals = huff_vals(t);
    uint32_t code = 0;
    int p = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < kHuffBits[t][l - 1]; ++i, ++p) {
            code_of[vals[p]] = (uint16_t)code++;
            len_of[vals[p]] = (uint8_t)l;
        }
        code <<= 1;
    }
}

MSPA_HD void make_tables(int quality, Tables &t) {
    const int scale = quality_scale(quality);
    for (int k = 0; k < 2; ++k) {
        for (int i = 0; i < 64; ++i) {
            t.qval[k][i] = scaled_qval(k, i, scale);
            reciprocal((uint32_t)t.qval[k][i] << 3, t.recip[k][i], t.corr[k][i], t.shift[k][i]);
        }
        for (int i = 0; i < 12; ++i) t.dc_code[k][i] = 0, t.dc_len[k][i] = 0;
        for (int i = 0; i < 256; ++i) t.ac_code[k][i] = 0, t.ac_len[k][i] = 0;
        derive_huff(2 * k, t.dc_code[k], t.dc_len[k]);
        derive_huff(2 * k + 1, t.ac_code[k], t.ac_len[k]);
    }
}

// The file's header up to the end of SOS: exactly kHeaderBytes bytes into dst.
MSPA_HD int write_header(int32_t h, int32_t w, int32_t quality, int32_t ss, uint8_t *dst) {
    int n = 0;
    auto b = [&](int v) { dst[n++] = (uint8_t)v; };
    auto w16 = [&](int v) { b(v >> 8); b(v & 255); };
    b(0xFF), b(0xD8);
    b(0xFF), b(0xE0), w16(16);                                        // APP0 JFIF 1.1, no units, density 1:1, no thumbnail
    b('J'), b('F'), b('I'), b('F'), b(0), b(1), b(1), b(0), w16(1), w16(1), b(0), b(0);
    const int scale = quality_scale(quality);
    for (int k = 0; k < 2; ++k) {                                     // DQT, 8-bit precision, zig-zag order
        b(0xFF), b(0xDB), w16(67), b(k);
        for (int i = 0; i < 64; ++i) b(scaled_qval(k, kZigzag[i], scale));
    }
    const Geometry g = geometry(h, w, ss);
    b(0xFF), b(0xC0), w16(17), b(8), w16(h), w16(w), b(3);           // SOF0
    b(1), b((g.hm << 4) | g.vm), b(0);
    b(2), b(0x11), b(1);
    b(3), b(0x11), b(1);
    for (int t = 0; t < 4; ++t) {                                     // DHT: DC0, AC0, DC1, AC1
        int count = 0;
        for (int l = 0; l < 16; ++l) count += kHuffBits[t][l];
        b(0xFF), b(0xC4), w16(2 + 1 + 16 + count), b(((t & 1) << 4) | (t >> 1));
        for (int l = 0; l < 16; ++l) b(kHuffBits[t][l]);
        const uint8_t *vals = huff_vals(t);
        for (int i = 0; i < count; ++i) b(vals[i]);
    }
    b(0xFF), b(0xDA), w16(12), b(3);                                  // SOS
    b(1), b(0x00), b(2), b(0x11), b(3), b(0x11);
    b(0), b(63), b(0);
    return n;
}

MSPA_HD int min_i(int a, int b) { return a < b ? a : b; }

// jccolor.c rgb_ycc_convert: SCALEBITS 16, FIX(x) = x * 65536 rounded
MSPA_HD void rgb_to_ycc(int r, int g, int b, int &y, int &cb, int &cr) {
    constexpr int32_t kHalf = 1 << 15, kOff = 128 << 16;
    y = (19595 * r + 38470 * g + 7471 * b + kHalf) >> 16;
    cb = (-11059 * r - 21709 * g + 32768 * b + kOff + kHalf - 1) >> 16;
    cr = (32768 * r - 27439 * g - 5329 * b + kOff + kHalf - 1) >> 16;
}

MSPA_HD int comp_of(const uint8_t *px, int c) {
    int y, cb, cr;
    rgb_to_ycc(px[0], px[1], px[2], y, cb, cr);
    return c == 0 ? y : c == 1 ? cb : cr;
}

// The centred 8x8 input of component c's block (bx, by) (a real block: bx < bw, by < bh), edges replicated and chroma
// downsampled as the preprocessing chain leaves it.
MSPA_HD void sample_block(const uint8_t *rgb, const Geometry &g, int c, int bx, int by, int32_t *blk) {
    const int64_t pitch = (int64_t)g.w * 3;
    const int H = g.h, W = g.w;
    if (c == 0 || (g.hm == 1 && g.vm == 1)) {
        MSPA_UNROLL
        for (int i = 0; i < 8; ++i) {
            const int y = min_i(by * 8 + i, H - 1);
            const uint8_t *row = rgb + y * pitch;
            MSPA_UNROLL
            for (int j = 0; j < 8; ++j) blk[i * 8 + j] = comp_of(row + 3 * min_i(bx * 8 + j, W - 1), c) - 128;
        }
        return;
    }
    const int ch = (H + g.vm - 1) / g.vm;                             // downsampled rows; later rows repeat the last
    MSPA_UNROLL
    for (int i = 0; i < 8; ++i) {
        const int cy = min_i(by * 8 + i, ch - 1);
        const int y0 = min_i(cy * g.vm, H - 1), y1 = min_i(cy * g.vm + g.vm - 1, H - 1);
        const uint8_t *r0 = rgb + y0 * pitch, *r1 = rgb + y1 * pitch;
        MSPA_UNROLL
        for (int j = 0; j < 8; ++j) {
            const int cx = bx * 8 + j;
            const int x0 = 3 * min_i(2 * cx, W - 1), x1 = 3 * min_i(2 * cx + 1, W - 1);
            int v;
            if (g.vm == 2) v = (comp_of(r0 + x0, c) + comp_of(r0 + x1, c) + comp_of(r1 + x0, c) + comp_of(r1 + x1, c) + 1 + (cx & 1)) >> 2;
            else v = (comp_of(r0 + x0, c) + comp_of(r0 + x1, c) + (cx & 1)) >> 1;
            blk[i * 8 + j] = v - 128;
        }
    }
}

// jfdctint.c: JDCT_ISLOW, rows then columns, in place.  Output scaled up by 8.
MSPA_HD void fdct_islow(int32_t *d) {
    constexpr int CB = 13, P1 = 2;
    constexpr int32_t F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633, F1501 = 12299,
                      F1847 = 15137, F1961 = 16069, F2053 = 16819, F2562 = 20995, F3072 = 25172;
    MSPA_UNROLL
    for (int pass = 0; pass < 2; ++pass) {
        const int step = pass == 0 ? 1 : 8, stride = pass == 0 ? 8 : 1;
        MSPA_UNROLL
        for (int r = 0; r < 8; ++r) {
            int32_t *p = d + r * stride;
            const int32_t tmp0 = p[0] + p[7 * step], tmp7 = p[0] - p[7 * step];
            const int32_t tmp1 = p[step] + p[6 * step], tmp6 = p[step] - p[6 * step];
            const int32_t tmp2 = p[2 * step] + p[5 * step], tmp5 = p[2 * step] - p[5 * step];
            const int32_t tmp3 = p[3 * step] + p[4 * step], tmp4 = p[3 * step] - p[4 * step];
            const int32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
            const int sh = pass == 0 ? CB - P1 : CB + P1;
            const int32_t rnd = 1 << (sh - 1);
            if (pass == 0) {
                p[0] = (tmp10 + tmp11) * (1 << P1);
                p[4 * step] = (tmp10 - tmp11) * (1 << P1);
            } else {
                p[0] = (tmp10 + tmp11 + (1 << (P1 - 1))) >> P1;
                p[4 * step] = (tmp10 - tmp11 + (1 << (P1 - 1))) >> P1;
            }
            int32_t z1 = (tmp12 + tmp13) * F0541;
            p[2 * step] = (z1 + tmp13 * F0765 + rnd) >> sh;
            p[6 * step] = (z1 - tmp12 * F1847 + rnd) >> sh;
            z1 = tmp4 + tmp7;
            int32_t z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
            const int32_t z5 = (z3 + z4) * F1175;
            const int32_t t4 = tmp4 * F0298, t5 = tmp5 * F2053, t6 = tmp6 * F3072, t7 = tmp7 * F1501;
            z1 = -z1 * F0899;
            z2 = -z2 * F2562;
            z3 = -z3 * F1961 + z5;
            z4 = -z4 * F0390 + z5;
            p[7 * step] = (t4 + z1 + z3 + rnd) >> sh;
            p[5 * step] = (t5 + z2 + z4 + rnd) >> sh;
            p[3 * step] = (t6 + z2 + z3 + rnd) >> sh;
            p[step] = (t7 + z1 + z4 + rnd) >> sh;
        }
    }
}

// One MCU's quantised blocks, natural order, in MCU order (Y blocks row by row, Cb, Cr); dummy blocks included.
MSPA_HD void mcu_coefs(const uint8_t *rgb, const Geometry &g, const Tables &t, int mx, int my, int16_t (*out)[64]) {
    int32_t blk[64];
    int n = 0;
    for (int c = 0; c < 3; ++c) {
        const int sh = c == 0 ? g.hm : 1, sv = c == 0 ? g.vm : 1, k = c == 0 ? 0 : 1;
        for (int yi = 0; yi < sv; ++yi)
            for (int xi = 0; xi < sh; ++xi, ++n) {
                const int bx = mx * sh + xi, by = my * sv + yi;
                if (bx >= g.bw[k] || by >= g.bh[k]) {          // dummy: the DC of the MCU's preceding block (same component)
                    for (int i = 1; i < 64; ++i) out[n][i] = 0;
                    out[n][0] = out[n - 1][0];
                    continue;
                }
                sample_block(rgb, g, c, bx, by, blk);
                fdct_islow(blk);
                for (int i = 0; i < 64; ++i) out[n][i] = quantize(blk[i], t.recip[k][i], t.corr[k][i], t.shift[k][i]);
            }
    }
}

MSPA_HD int bit_length(int32_t v) {
    int n = 0;
    while (v) ++n, v >>= 1;
    return n;
}

// jchuff.c encode_one_block: calls sink.put(bits, nbits) in stream order (nbits <= 16 each).  Returns the block's DC.
template <class Sink>
MSPA_HD void encode_block(const int16_t *blk, int32_t pred, const Tables &t, int k, Sink &sink) {
    int32_t v = blk[0] - pred, v2 = v;
    if (v < 0) v = -v, --v2;
    int nb = bit_length(v);
    sink.put(t.dc_code[k][nb], t.dc_len[k][nb]);
    if (nb) sink.put((uint32_t)v2 & ((1u << nb) - 1), nb);
    int run = 0;
    for (int i = 1; i < 64; ++i) {
        v = blk[kZigzag[i]];
        if (v == 0) {
            ++run;
            continue;
        }
        while (run > 15) {
            sink.put(t.ac_code[k][0xF0], t.ac_len[k][0xF0]);
            run -= 16;
        }
        v2 = v;
        if (v < 0) v = -v, --v2;
        nb = bit_length(v);
        const int sym = (run << 4) + nb;
        sink.put(t.ac_code[k][sym], t.ac_len[k][sym]);
        sink.put((uint32_t)v2 & ((1u << nb) - 1), nb);
        run = 0;
    }
    if (run > 0) sink.put(t.ac_code[k][0], t.ac_len[k][0]);
}

// The DC predictor of each component at MCU m: the DC of that component's last block in MCU m - 1 (0 at m = 0).  `prev` is
// MCU m - 1's blocks, or null.
MSPA_HD void mcu_preds(const int16_t (*prev)[64], const Geometry &g, int32_t pred[3]) {
    const int ny = g.hm * g.vm;
    pred[0] = prev ? prev[ny - 1][0] : 0;
    pred[1] = prev ? prev[ny][0] : 0;
    pred[2] = prev ? prev[ny + 1][0] : 0;
}

template <class Sink>
MSPA_HD void encode_mcu(const int16_t (*blk)[64], const int32_t pred_in[3], const Geometry &g, const Tables &t, Sink &sink) {
    const int ny = g.hm * g.vm;
    int32_t pred = pred_in[0];
    for (int i = 0; i < ny; ++i) {
        encode_block(blk[i], pred, t, 0, sink);
        pred = blk[i][0];
    }
    encode_block(blk[ny], pred_in[1], t, 1, sink);
    encode_block(blk[ny + 1], pred_in[2], t, 1, sink);
}

struct BitCount {
    int64_t n = 0;
    MSPA_HD void put(uint32_t, int nbits) { n += nbits; }
};

// Serial byte writer with 0xFF00 stuffing (the host restatement; the device stuffs in a pass of its own).
struct StuffedWriter {
    uint8_t *dst;
    int64_t n, cap;
    uint32_t acc;
    int nacc;
    MSPA_HD void byte(uint8_t v) {
        if (n < cap) dst[n] = v;
        ++n;
        if (v == 0xFF) {
            if (n < cap) dst[n] = 0;
            ++n;
        }
    }
    MSPA_HD void put(uint32_t bits, int nbits) {
        acc = (acc << nbits) | (bits & ((1u << nbits) - 1));
        nacc += nbits;
        while (nacc >= 8) {
            nacc -= 8;
            byte((uint8_t)(acc >> nacc));
        }
    }
    MSPA_HD void pad() {                                            // fill the last byte with 1-bits
        if (nacc) put(0x7F, 8 - nacc);
    }
};

// A whole file, serially: the reference form of what the kernels compute.  Returns the file's length (bytes past `cap` are
// counted, not written).
inline int64_t encode_file_host(const uint8_t *rgb, int32_t h, int32_t w, int32_t quality, int32_t ss, uint8_t *dst, int64_t cap) {
    static Tables t;
    make_tables(quality, t);
    const Geometry g = geometry(h, w, ss);
    uint8_t hdr[kHeaderBytes];
    write_header(h, w, quality, ss, hdr);
    StuffedWriter wr{dst, 0, cap, 0, 0};
    for (int i = 0; i < kHeaderBytes; ++i) {
        if (wr.n < cap) dst[wr.n] = hdr[i];
        ++wr.n;
    }
    int16_t cur[6][64], prev[6][64];
    bool first = true;
    for (int my = 0; my < g.mcus_y; ++my)
        for (int mx = 0; mx < g.mcus_x; ++mx) {
            mcu_coefs(rgb, g, t, mx, my, cur);
            int32_t pred[3];
            mcu_preds(first ? nullptr : prev, g, pred);
            encode_mcu(cur, pred, g, t, wr);
            for (int b = 0; b < g.blocks_per_mcu; ++b)
                for (int i = 0; i < 64; ++i) prev[b][i] = cur[b][i];
            first = false;
        }
    wr.pad();
    const uint8_t eoi[2] = {0xFF, 0xD9};
    for (int i = 0; i < 2; ++i) {
        if (wr.n < cap) dst[wr.n] = eoi[i];
        ++wr.n;
    }
    return wr.n;
}

}  // namespace jpege
}  // namespace mspa
