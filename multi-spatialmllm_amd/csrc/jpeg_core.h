// Baseline JPEG: the header parser (host) and the per-image decode arithmetic shared by the device kernels of jpeg_decode.hip.
// Everything that decides an output value is a __host__ __device__ function here, so that a plain C++ build of this header can
// be checked against libjpeg-turbo on a CPU.  The arithmetic restates libjpeg's documented default decompression:
//   * Huffman decode with the canonical (maxcode / valoffset) tables and an 8-bit lookahead (jdhuff.c's derived tables);
//   * dequantisation and the JDCT_ISLOW integer IDCT (jidctint.c: 13-bit constants, PASS1_BITS 2, DESCALE with rounding, the
//     post-IDCT range-limit table indexed with `& RANGE_MASK`);
//   * "fancy" triangular upsampling for h2v1 / h2v2 chroma (jdsample.c), replication when a chroma plane is <= 2 samples wide;
//   * YCbCr -> RGB with 16-bit fixed-point constants (jdcolor.c).
// A stream is accepted (status 0) only when it decodes EXACTLY: every MCU from real data bits, restart markers present and in
// sequence, valid codes only, no coefficient past index 63, and the segment consumed up to its final marker (EOI) with at most
// seven 1-bits of padding.  Anything libjpeg would merely warn about is declined, and the caller decodes that frame on the host.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>

#ifdef __HIPCC__
#define MSPA_HD __host__ __device__ __forceinline__
#else
#define MSPA_HD inline
#endif

namespace mspa {
namespace jpeg {

// per-image status (descriptor field `status` after the parse; the decode's status array after the decode)
enum : int32_t {
    kOk = 0,
    kNotJpeg = 1,          // no SOI, truncated or malformed header, a table that is not valid
    kUnsupported = 2,      // valid JPEG outside the accepted subset (progressive, arithmetic, 12-bit, CMYK, sampling, ...)
    kWrongSize = 3,        // decode: the image's (h, w) is not the call's
    kBadEntropy = 4,       // decode: invalid code, coefficient past 63, a DC out of range, or data ran out before the last MCU
    kBadRestart = 5,       // decode: a restart marker missing, out of sequence, or data left before it
    kBadEnd = 6,           // decode: data left after the last MCU, or the segment does not end with EOI
    kOutOfRange = 7,       // decode: a block's coefficients or IDCT intermediates outside the bounds every IDCT form agrees in
};

struct HuffTable {
    int32_t maxcode[18];       // largest code of length l (-1: none); [17] a sentinel
    int32_t valoffset[18];     // huffval index = code + valoffset[l]
    uint16_t look[256];        // 8-bit lookahead: (code length << 8) | symbol, 0 = longer than 8 bits
    uint8_t huffval[256];
};

// One fixed-size descriptor per image (MSPA_JPEG_DESC_BYTES).  The first 160 bytes are documented in include/mspa.h.
struct JpegDesc {
    int32_t status, h, w, ncomp;                        //   0
    int32_t restart_interval, hmax, vmax, mcus_x;        //  16
    int32_t mcus_y, total_blocks, adobe, jfif;           //  32
    int64_t scan_offset, scan_bytes;                     //  48: the entropy-coded data, relative to the payload's first byte
    int32_t samp_h[3], samp_v[3], tq[3], td[3], ta[3];   //  64
    int32_t bw[3], bh[3], block_off[3];                  // 124: block grid of each component (MCU-padded), first block
    int32_t dw[3], dh[3];                                // 160: downsampled_width / height (the real samples)
    uint8_t pad0[8];                                     // 184
    uint16_t qt[3][64];                                  // 192: each component's quantisation table, natural order
    HuffTable huff[4];                                   // 576: DC 0, DC 1, AC 0, AC 1
};
static_assert(sizeof(HuffTable) == 912, "HuffTable layout");
static_assert(offsetof(JpegDesc, scan_offset) == 48 && offsetof(JpegDesc, qt) == 192 && offsetof(JpegDesc, huff) == 576,
              "JpegDesc layout (include/mspa.h documents it)");
constexpr int kDescBytes = 4224;
static_assert(sizeof(JpegDesc) <= kDescBytes, "descriptor larger than MSPA_JPEG_DESC_BYTES");

// zig-zag position -> natural (row-major) index
constexpr uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                  41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                  30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Worst-case coefficient blocks of one image slot for (h, w): every accepted sampling fits 3 * (2 ceil(h/16)) * (2 ceil(w/16)).
MSPA_HD int64_t slot_blocks(int32_t h, int32_t w) {
    return 3ll * (2ll * ((h + 15) / 16)) * (2ll * ((w + 15) / 16));
}

// ------------------------------------------------------------------------------------------------------------------------
// Host: header parser.  Reads only [p, p + n); never trusts a length.

inline bool build_huff(HuffTable &t, const uint8_t bits[17], const uint8_t *vals, int nvals, bool dc) {
    memset(&t, 0, sizeof(t));
    int huffsize[257], huffcode[257];
    int p = 0;
    for (int l = 1; l <= 16; ++l)
        for (int i = 0; i < bits[l]; ++i) huffsize[p++] = l;
    huffsize[p] = 0;
    const int numsymbols = p;
    if (numsymbols != nvals || numsymbols > 256) return false;
    int code = 0, si = numsymbols ? huffsize[0] : 1;
    p = 0;
    while (huffsize[p]) {
        while (huffsize[p] == si) { huffcode[p++] = code++; }
        if (code >= (1 << si)) return false;          // over-subscribed
        code <<= 1;
        ++si;
    }
    p = 0;
    for (int l = 1; l <= 16; ++l) {
        if (bits[l]) {
            t.valoffset[l] = p - huffcode[p];
            p += bits[l];
            t.maxcode[l] = huffcode[p - 1];
        } else {
            t.maxcode[l] = -1;
        }
    }
    t.valoffset[17] = 0;
    t.maxcode[17] = 0xFFFFF;
    p = 0;
    for (int l = 1; l <= 8; ++l)
        for (int i = 1; i <= bits[l]; ++i, ++p) {
            int look = huffcode[p] << (8 - l);
            for (int c = 1 << (8 - l); c > 0; --c) t.look[look++] = (uint16_t)((l << 8) | vals[p]);
        }
    for (int i = 0; i < numsymbols; ++i) {
        t.huffval[i] = vals[i];
        if (dc && vals[i] > 11) return false;          // 8-bit baseline DC categories are 0..11
        if (!dc && (vals[i] & 15) > 10) return false;  // and AC magnitudes 1..10
    }
    return true;
}

// Parses one payload into `d`; returns (and stores) the status.
inline int32_t parse(const uint8_t *p, int64_t n, JpegDesc &d) {
    memset(&d, 0, sizeof(d));
    d.status = kNotJpeg;
    if (!p || n < 4 || p[0] != 0xFF || p[1] != 0xD8) return d.status;
    uint16_t qt[4][64];
    bool qt_ok[4] = {false, false, false, false}, ht_ok[4] = {false, false, false, false};
    bool sof = false;
    int comp_id[3] = {0, 0, 0};
    int64_t i = 2;
    auto done = [&](int32_t s) { d.status = s; return s; };
    while (true) {
        // next marker: 0xFF, optional 0xFF fill bytes, the code
        if (i >= n || p[i] != 0xFF) return done(kNotJpeg);
        while (i < n && p[i] == 0xFF) ++i;
        if (i >= n) return done(kNotJpeg);
        const int m = p[i++];
        if (m == 0xD8 || m == 0xD9 || m == 0x01 || (m >= 0xD0 && m <= 0xD7) || m == 0x00) return done(kNotJpeg);
        if (i + 2 > n) return done(kNotJpeg);
        const int len = (p[i] << 8) | p[i + 1];
        if (len < 2 || i + len > n) return done(kNotJpeg);
        const uint8_t *s = p + i + 2;
        const int sl = len - 2;
        if (m == 0xC0) {                                   // SOF0: baseline
            if (sof || sl < 6) return done(kNotJpeg);
            sof = true;
            if (s[0] != 8) return done(kUnsupported);
            d.h = (s[1] << 8) | s[2];
            d.w = (s[3] << 8) | s[4];
            const int nc = s[5];
            if (sl != 6 + 3 * nc || nc == 0) return done(kNotJpeg);
            if (nc != 1 && nc != 3) return done(kUnsupported);
            if (d.h == 0 || d.w == 0) return done(kUnsupported);   // DNL-defined height
            d.ncomp = nc;
            for (int c = 0; c < nc; ++c) {
                comp_id[c] = s[6 + 3 * c];
                d.samp_h[c] = s[7 + 3 * c] >> 4;
                d.samp_v[c] = s[7 + 3 * c] & 15;
                d.tq[c] = s[8 + 3 * c];
                if (d.samp_h[c] < 1 || d.samp_h[c] > 4 || d.samp_v[c] < 1 || d.samp_v[c] > 4 || d.tq[c] > 3) return done(kNotJpeg);
            }
        } else if ((m >= 0xC1 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC)) {
            return done(kUnsupported);                     // extended, progressive, lossless, arithmetic
        } else if (m == 0xCC) {
            return done(kUnsupported);                     // arithmetic conditioning
        } else if (m == 0xC4) {                            // DHT
            int k = 0;
            while (k < sl) {
                if (k + 17 > sl) return done(kNotJpeg);
                const int tc = s[k] >> 4, th = s[k] & 15;
                if (tc > 1 || th > 3) return done(kNotJpeg);
                uint8_t bits[17];
                bits[0] = 0;
                int cnt = 0;
                for (int l = 1; l <= 16; ++l) { bits[l] = s[k + l]; cnt += bits[l]; }
                if (cnt > 256 || k + 17 + cnt > sl) return done(kNotJpeg);
                if (th > 1) return done(kUnsupported);     // baseline: tables 0 and 1
                if (!build_huff(d.huff[tc * 2 + th], bits, s + k + 17, cnt, tc == 0)) return done(kNotJpeg);
                ht_ok[tc * 2 + th] = true;
                k += 17 + cnt;
            }
        } else if (m == 0xDB) {                            // DQT
            int k = 0;
            while (k < sl) {
                const int pq = s[k] >> 4, tq = s[k] & 15;
                if (tq > 3 || pq > 1) return done(kNotJpeg);
                const int sz = pq ? 128 : 64;
                if (k + 1 + sz > sl) return done(kNotJpeg);
                for (int z = 0; z < 64; ++z) {
                    const int v = pq ? ((s[k + 1 + 2 * z] << 8) | s[k + 2 + 2 * z]) : s[k + 1 + z];
                    qt[tq][kNatural[z]] = (uint16_t)v;
                }
                if (pq) return done(kUnsupported);         // 16-bit quantisers are not baseline
                qt_ok[tq] = true;
                k += 1 + sz;
            }
        } else if (m == 0xDD) {                            // DRI
            if (sl != 2) return done(kNotJpeg);
            d.restart_interval = (s[0] << 8) | s[1];
        } else if (m == 0xE0) {                            // APP0: JFIF?
            if (sl >= 5 && s[0] == 'J' && s[1] == 'F' && s[2] == 'I' && s[3] == 'F' && s[4] == 0) d.jfif = 1;
        } else if (m == 0xEE) {                            // APP14: Adobe (colour transform flag): declined
            if (sl >= 5 && s[0] == 'A' && s[1] == 'd' && s[2] == 'o' && s[3] == 'b' && s[4] == 'e') d.adobe = 1;
        } else if (m == 0xDA) {                            // SOS: the one scan
            if (!sof || sl < 1) return done(kNotJpeg);
            const int ns = s[0];
            if (sl != 4 + 2 * ns) return done(kNotJpeg);
            if (ns != d.ncomp) return done(kUnsupported);  // a multi-scan (non-interleaved) image
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != comp_id[c]) return done(kUnsupported);
                d.td[c] = s[2 + 2 * c] >> 4;
                d.ta[c] = s[2 + 2 * c] & 15;
                if (d.td[c] > 1 || d.ta[c] > 1) return done(kUnsupported);
                if (!ht_ok[d.td[c]] || !ht_ok[2 + d.ta[c]] || !qt_ok[d.tq[c]]) return done(kUnsupported);
            }
            const int ss = s[1 + 2 * ns], se = s[2 + 2 * ns], ah = s[3 + 2 * ns] >> 4, al = s[3 + 2 * ns] & 15;
            if (ss != 0 || se != 63 || ah != 0 || al != 0) return done(kNotJpeg);
            if (d.adobe) return done(kUnsupported);
            if (d.ncomp == 3) {
                if (!d.jfif && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B') return done(kUnsupported);
                const bool y11 = d.samp_h[0] == 1 && d.samp_v[0] == 1, y21 = d.samp_h[0] == 2 && d.samp_v[0] == 1,
                           y22 = d.samp_h[0] == 2 && d.samp_v[0] == 2;
                if (!(y11 || y21 || y22)) return done(kUnsupported);
                for (int c = 1; c < 3; ++c)
                    if (d.samp_h[c] != 1 || d.samp_v[c] != 1) return done(kUnsupported);
                d.hmax = d.samp_h[0];
                d.vmax = d.samp_v[0];
                d.mcus_x = (d.w + 8 * d.hmax - 1) / (8 * d.hmax);
                d.mcus_y = (d.h + 8 * d.vmax - 1) / (8 * d.vmax);
                int off = 0;
                for (int c = 0; c < 3; ++c) {
                    d.bw[c] = d.mcus_x * d.samp_h[c];
                    d.bh[c] = d.mcus_y * d.samp_v[c];
                    d.block_off[c] = off;
                    off += d.bw[c] * d.bh[c];
                    d.dw[c] = (int)(((int64_t)d.w * d.samp_h[c] + d.hmax - 1) / d.hmax);
                    d.dh[c] = (int)(((int64_t)d.h * d.samp_v[c] + d.vmax - 1) / d.vmax);
                }
                d.total_blocks = off;
            } else {
                // one component, non-interleaved: the MCU is one block whatever the sampling factors say
                d.samp_h[0] = d.samp_v[0] = d.hmax = d.vmax = 1;
                d.mcus_x = (d.w + 7) / 8;
                d.mcus_y = (d.h + 7) / 8;
                d.bw[0] = d.mcus_x;
                d.bh[0] = d.mcus_y;
                d.dw[0] = d.w;
                d.dh[0] = d.h;
                d.total_blocks = d.bw[0] * d.bh[0];
            }
            for (int c = 0; c < d.ncomp; ++c) memcpy(d.qt[c], qt[d.tq[c]], sizeof(d.qt[c]));
            d.scan_offset = i + len;
            d.scan_bytes = n - d.scan_offset;
            if (d.scan_bytes < 2) return done(kNotJpeg);  // not even room for the EOI: truncated
            return done(kOk);
        } else if (m == 0xDC) {                            // DNL
            return done(kUnsupported);
        }
        // APPn, COM and anything else with a length: skipped
        i += len;
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// Entropy decode of one image: coefficients (natural order, int16) into coef[block * 64 + k].  The caller zeroes coef first;
// only non-zero coefficients are stored.  The entropy-coded bytes [seg, seg + nbytes) lie in `src`, which is read as aligned
// 32-bit words: every word holding one of the segment's bytes (all inside `src`'s capacity, which the caller guarantees).

struct BitReader {
    const uint32_t *words;
    int64_t pos, end;        // next byte to load; one past the segment
    uint64_t buf;            // MSB-aligned bit buffer
    int32_t cnt;             // valid bits in buf
    int32_t pad;             // of those, zero bits inserted after the reader stopped (marker, end of data)
    bool stopped;            // at a marker (pos points at its 0xFF) or at the end of the data
    int64_t cached_idx;
    uint32_t cached;

    MSPA_HD int byte_at(int64_t b) {
        const int64_t wi = b >> 2;
        if (wi != cached_idx) { cached = words[wi]; cached_idx = wi; }
        return (int)((cached >> ((b & 3) * 8)) & 0xFFu);
    }
    MSPA_HD void reset(int64_t at) {
        pos = at;
        buf = 0;
        cnt = 0;
        pad = 0;
        stopped = false;
    }
    // fill to > 56 bits: real bytes while there are any, zero bits after a marker / the end
    MSPA_HD void fill() {
        while (cnt <= 56) {
            int b = 0;
            if (!stopped) {
                if (pos >= end) {
                    stopped = true;
                } else {
                    b = byte_at(pos);
                    if (b == 0xFF) {
                        const int b2 = pos + 1 < end ? byte_at(pos + 1) : -1;
                        if (b2 == 0x00) pos += 2;
                        else { stopped = true; b = 0; }
                    } else {
                        ++pos;
                    }
                }
            }
            if (stopped) pad += 8;
            buf |= (uint64_t)b << (56 - cnt);
            cnt += 8;
        }
    }
    MSPA_HD uint32_t peek(int n) const { return (uint32_t)(buf >> (64 - n)); }
    MSPA_HD void skip(int n) { buf <<= n; cnt -= n; }
    MSPA_HD bool overrun() const { return cnt < pad; }
    // The segment ends here: at most 7 real bits left, all ones, and the next bytes are the marker 0xFF `code`.
    MSPA_HD bool at_marker(int code) {
        const int real = cnt - pad;
        if (real < 0 || real > 7) return false;
        if (real && peek(real) != (1u << real) - 1u) return false;
        if (pos + 1 >= end) return false;
        return byte_at(pos) == 0xFF && byte_at(pos + 1) == code;
    }
};

// Huffman decode of one symbol (needs >= 16 bits in the buffer); -1 = no code matches
MSPA_HD int huff_decode(BitReader &br, const HuffTable *__restrict__ t) {
    const uint32_t look = t->look[br.peek(8)];
    if (look) {
        br.skip((int)(look >> 8));
        return (int)(look & 0xFFu);
    }
    const uint32_t w16 = br.peek(16);
    for (int l = 9; l <= 16; ++l) {
        const int code = (int)(w16 >> (16 - l));
        if (code <= t->maxcode[l]) {
            br.skip(l);
            const int idx = code + t->valoffset[l];
            if (idx < 0 || idx > 255) return -1;
            return t->huffval[idx];
        }
    }
    return -1;
}

MSPA_HD int extend(uint32_t r, int s) { return (int)r < (1 << (s - 1)) ? (int)r - (1 << s) + 1 : (int)r; }

MSPA_HD int32_t decode_entropy(const JpegDesc *__restrict__ d, const uint32_t *__restrict__ words, int64_t seg, int64_t nbytes,
                               int16_t *__restrict__ coef) {
    BitReader br;
    br.words = words;
    br.end = seg + nbytes;
    br.cached_idx = -1;
    br.cached = 0;
    br.reset(seg);
    const int nc = d->ncomp;
    const int ri = d->restart_interval;
    const int64_t total = (int64_t)d->mcus_x * d->mcus_y;
    int pred[3] = {0, 0, 0};
    int rst = 0, left = ri;
    int64_t mcu = 0;
    for (int my = 0; my < d->mcus_y; ++my) {
        for (int mx = 0; mx < d->mcus_x; ++mx) {
            for (int c = 0; c < nc; ++c) {
                const HuffTable *dct = &d->huff[d->td[c]];
                const HuffTable *act = &d->huff[2 + d->ta[c]];
                const int sh = d->samp_h[c], sv = d->samp_v[c];
                for (int by = 0; by < sv; ++by)
                    for (int bx = 0; bx < sh; ++bx) {
                        int16_t *blk = coef + 64ll * (d->block_off[c] + (int64_t)(my * sv + by) * d->bw[c] + mx * sh + bx);
                        br.fill();
                        int s = huff_decode(br, dct);
                        if (s < 0) return kBadEntropy;
                        if (s) {
                            const uint32_t r = br.peek(s);
                            br.skip(s);
                            s = extend(r, s);
                        }
                        const int dc = pred[c] + s;
                        if (dc < -32768 || dc > 32767) return kBadEntropy;
                        pred[c] = dc;
                        if (dc) blk[0] = (int16_t)dc;
                        for (int k = 1; k < 64; ++k) {
                            if (br.cnt < 32) br.fill();
                            const int rs = huff_decode(br, act);
                            if (rs < 0) return kBadEntropy;
                            const int r = rs >> 4, sz = rs & 15;
                            if (sz) {
                                k += r;
                                if (k > 63) return kBadEntropy;
                                const uint32_t v = br.peek(sz);
                                br.skip(sz);
                                blk[kNatural[k]] = (int16_t)extend(v, sz);
                            } else {
                                if (r != 15) break;            // EOB
                                k += 15;
                                if (k > 63) return kBadEntropy;
                            }
                        }
                    }
            }
            if (br.overrun()) return kBadEntropy;
            ++mcu;
            if (ri && --left == 0 && mcu < total) {
                if (!br.at_marker(0xD0 + (rst & 7))) return kBadRestart;
                br.reset(br.pos + 2);
                ++rst;
                left = ri;
                pred[0] = pred[1] = pred[2] = 0;
            }
        }
    }
    if (!br.at_marker(0xD9)) return kBadEnd;
    return kOk;
}

// ------------------------------------------------------------------------------------------------------------------------
// Dequantise + JDCT_ISLOW IDCT of one block (jidctint.c), output to out[y * stride + x].

constexpr int kConstBits = 13, kPass1Bits = 2;
MSPA_HD int range_limit(int x) {                  // sample_range_limit + CENTERJSAMPLE, indexed with & RANGE_MASK (1023)
    const int v = x & 1023;
    return v < 128 ? v + 128 : v < 512 ? 255 : v < 896 ? 0 : v - 896;
}

template <bool kPass2>
MSPA_HD void idct_1d(int64_t in0, int64_t in1, int64_t in2, int64_t in3, int64_t in4, int64_t in5, int64_t in6, int64_t in7,
                     int32_t o[8]) {
    // JLONG arithmetic (64-bit); pass 1 results are stored as int, as jidctint.c's work array is
    const int shift = kPass2 ? kConstBits + kPass1Bits + 3 : kConstBits - kPass1Bits;
    const int64_t round = 1ll << (shift - 1);
    int64_t z2 = in2, z3 = in6;
    int64_t z1 = (z2 + z3) * 4433;
    const int64_t tmp2e = z1 + z3 * -15137, tmp3e = z1 + z2 * 6270;
    const int64_t tmp0e = (in0 + in4) * (1ll << kConstBits), tmp1e = (in0 - in4) * (1ll << kConstBits);
    const int64_t tmp10 = tmp0e + tmp3e, tmp13 = tmp0e - tmp3e, tmp11 = tmp1e + tmp2e, tmp12 = tmp1e - tmp2e;
    int64_t t0 = in7, t1 = in5, t2 = in3, t3 = in1;
    z1 = t0 + t3;
    z2 = t1 + t2;
    z3 = t0 + t2;
    int64_t z4 = t1 + t3;
    const int64_t z5 = (z3 + z4) * 9633;
    t0 = t0 * 2446;
    t1 = t1 * 16819;
    t2 = t2 * 25172;
    t3 = t3 * 12299;
    z1 = z1 * -7373;
    z2 = z2 * -20995;
    z3 = z3 * -16069;
    z4 = z4 * -3196;
    z3 += z5;
    z4 += z5;
    t0 += z1 + z3;
    t1 += z2 + z4;
    t2 += z2 + z3;
    t3 += z1 + z4;
    o[0] = (int32_t)((tmp10 + t3 + round) >> shift);
    o[7] = (int32_t)((tmp10 - t3 + round) >> shift);
    o[1] = (int32_t)((tmp11 + t2 + round) >> shift);
    o[6] = (int32_t)((tmp11 - t2 + round) >> shift);
    o[2] = (int32_t)((tmp12 + t1 + round) >> shift);
    o[5] = (int32_t)((tmp12 - t1 + round) >> shift);
    o[3] = (int32_t)((tmp13 + t0 + round) >> shift);
    o[4] = (int32_t)((tmp13 - t0 + round) >> shift);
}

// Dequantised coefficients and IDCT intermediates of every decoded stream stay inside these bounds.  An 8-bit block's DCT
// coefficients are at most 1 024 in magnitude (the DC of a block of -128s) and quantising moves them by at most q / 2 <= 127;
// inside the bounds every intermediate of the 16-bit SIMD forms of the same IDCT (libjpeg-turbo's) fits its lane, so they
// and jidctint.c's C agree, and the range-limit mask equals a clamp.  A block outside them (damaged data) declines its image.
constexpr int32_t kMaxDequant = 1280, kMaxPass1 = 8191, kMaxPass2 = 511;

// c: 64 coefficients (natural order), q: 64 quantisers; the work array lives in registers once the loops are unrolled.
// Returns false when the block leaves the bounds above (its output is then unspecified).
MSPA_HD bool idct_islow(const int16_t *__restrict__ c, const uint16_t *__restrict__ q, uint8_t *__restrict__ out, int64_t stride) {
    int32_t ws[64];
    bool ok = true;
#pragma unroll
    for (int col = 0; col < 8; ++col) {
        int64_t in[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int32_t v = (int32_t)c[r * 8 + col] * (int32_t)q[r * 8 + col];
            ok = ok && v >= -kMaxDequant && v <= kMaxDequant;
            in[r] = v;
        }
        int32_t o[8];
        idct_1d<false>(in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7], o);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            ok = ok && o[r] >= -kMaxPass1 && o[r] <= kMaxPass1;
            ws[r * 8 + col] = o[r];
        }
    }
#pragma unroll
    for (int row = 0; row < 8; ++row) {
        const int32_t *w = ws + row * 8;
        int32_t o[8];
        idct_1d<true>(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], o);
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            ok = ok && o[x] >= -kMaxPass2 - 1 && o[x] <= kMaxPass2;
            out[row * stride + x] = (uint8_t)range_limit(o[x]);
        }
    }
    return ok;
}

// ------------------------------------------------------------------------------------------------------------------------
// Upsampling + colour conversion of one output pixel.  plane(c) is component c's IDCT output, pitch bw[c] * 8.

MSPA_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// the chroma sample of component plane `pl` (pitch `pitch`, dw x dh real samples) at output pixel (y, x)
MSPA_HD int chroma_at(const uint8_t *__restrict__ pl, int64_t pitch, int dw, int dh, int hmax, int vmax, int y, int x) {
    if (hmax == 1) return pl[(int64_t)y * pitch + x];
    const int ix = x >> 1;
    if (dw <= 2) {                                 // libjpeg: plain replication for planes at most 2 samples wide
        const int iy = vmax == 2 ? y >> 1 : y;
        return pl[(int64_t)iy * pitch + ix];
    }
    const int near_x = x & 1 ? clampi(ix + 1, 0, dw - 1) : clampi(ix - 1, 0, dw - 1);
    if (vmax == 1) {                               // h2v1: (3 near + far + 1 / 2) >> 2
        const int64_t r = (int64_t)y * pitch;
        return (3 * pl[r + ix] + pl[r + near_x] + (x & 1 ? 2 : 1)) >> 2;
    }
    // h2v2: column sums 3 * nearest row + next nearest row, then (3 * this + other + 8 / 7) >> 4
    const int iy = y >> 1;
    const int iy2 = y & 1 ? clampi(iy + 1, 0, dh - 1) : clampi(iy - 1, 0, dh - 1);
    const int64_t r0 = (int64_t)iy * pitch, r1 = (int64_t)iy2 * pitch;
    const int cs_this = 3 * pl[r0 + ix] + pl[r1 + ix];
    const int cs_other = 3 * pl[r0 + near_x] + pl[r1 + near_x];
    return (3 * cs_this + cs_other + (x & 1 ? 7 : 8)) >> 4;
}

MSPA_HD void ycc_to_rgb(int y, int cb, int cr, uint8_t *rgb) {
    const int cbp = cb - 128, crp = cr - 128;
    const int r = y + ((91881 * crp + 32768) >> 16);
    const int b = y + ((116130 * cbp + 32768) >> 16);
    const int g = y + ((-22554 * cbp - 46802 * crp + 32768) >> 16);
    rgb[0] = (uint8_t)clampi(r, 0, 255);
    rgb[1] = (uint8_t)clampi(g, 0, 255);
    rgb[2] = (uint8_t)clampi(b, 0, 255);
}

}  // namespace jpeg
}  // namespace mspa
