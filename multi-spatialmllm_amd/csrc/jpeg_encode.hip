// Annotated-image writes ON the MI355X: baseline JPEG encode byte-identical to Pillow / libjpeg-turbo's default compression of
// an RGB image (`Image.fromarray(rgb).save(f, "JPEG", quality=q, subsampling=s)`), and the two compositing passes of the dot
// annotator (discs as OpenCV spans, labels as Pillow's 8-bit glyph masks).  The arithmetic is csrc/jpeg_encode_core.h; this
// file holds the kernels and the C ABI.
//
// Unlike the decode, the encode is data-parallel up to the final byte layout, so it runs as six kernels over n images of one
// shape, quality and subsampling:
//   1. tables_kernel -- one lane derives the quantisation divisors, the Huffman codes and the 623-byte header into the workspace.
//   2. coef_kernel   -- one thread per 8x8 block (MCU order): colour conversion, edge replication, downsampling, JDCT_ISLOW and
//      quantisation into an int16 coefficient workspace.  A dummy block (past width_in_blocks / height_in_blocks) stores zero
//      ACs and the quantised DC of the MCU's last real block before it, which is what libjpeg's copy chain leaves there.
//   3. bits_kernel   -- one thread per MCU: the MCU's entropy-coded length in bits (DC predictors from the previous MCU).
//   4. scan_kernel   -- one workgroup per image: exclusive scan of the lengths in MCU order -> every MCU's bit offset.
//   5. write_kernel  -- one thread per MCU: Huffman codes at the MCU's bit offset into a zeroed raw buffer; whole 32-bit words
//      are stored, the (shared) first and last word of an MCU's span are OR-ed in atomically.
//   6. stuff_kernel  -- one workgroup per image: header, the raw bytes with 1-bit padding and a 0x00 after every 0xFF (a
//      per-tile scan of the 0xFF counts), EOI.  Bytes past the output pitch are counted, never written.
#include "mspa_common.h"
#include "jpeg_encode_core.h"

namespace mspa {
namespace jpege {

constexpr int64_t kTablesBytes = 4096;                // Tables + header at the start of the workspace
static_assert(sizeof(Tables) + kHeaderBytes <= kTablesBytes, "workspace table area");

MSPA_HD int64_t raw_bytes(const Geometry &g) { return (blocks(g) * (kMaxBlockBits / 8) + 8 + 15) / 16 * 16; }

struct Layout {
    int64_t coef, offs, totals, raw, end;             // byte offsets in the workspace
};

MSPA_HD Layout layout(int64_t n, const Geometry &g) {
    Layout l;
    l.coef = kTablesBytes;
    l.offs = l.coef + n * blocks(g) * 128;
    l.totals = l.offs + n * mcus(g) * 8;
    l.raw = l.totals + (n * 8 + 15) / 16 * 16;
    l.end = l.raw + n * raw_bytes(g);
    return l;
}

__global__ void tables_kernel(int32_t h, int32_t w, int32_t quality, int32_t ss, Tables *t, uint8_t *hdr) {
    if (threadIdx.x != 0) return;
    make_tables(quality, *t);
    write_header(h, w, quality, ss, hdr);
}

// Block j (0 .. blocks_per_mcu) of an MCU -> component, block column / row in that component's grid.
MSPA_HD void block_at(const Geometry &g, int mx, int my, int j, int &c, int &bx, int &by) {
    const int ny = g.hm * g.vm;
    if (j < ny) {
        c = 0;
        bx = mx * g.hm + j % g.hm;
        by = my * g.vm + j / g.hm;
    } else {
        c = j - ny + 1;
        bx = mx;
        by = my;
    }
}

__global__ void __launch_bounds__(256) coef_kernel(const uint8_t *__restrict__ rgb, Geometry g, const Tables *__restrict__ t,
                                                   int16_t *__restrict__ coef) {
    const int64_t k = blockIdx.y;
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= blocks(g)) return;
    const int64_t m = b / g.blocks_per_mcu;
    int j = (int)(b - m * g.blocks_per_mcu);
    const int my = (int)(m / g.mcus_x), mx = (int)(m - (int64_t)my * g.mcus_x);
    const uint8_t *img = rgb + k * (int64_t)g.h * g.w * 3;
    int16_t *out = coef + (k * blocks(g) + b) * 64;
    int c, bx, by;
    block_at(g, mx, my, j, c, bx, by);
    const int kt = c == 0 ? 0 : 1;
    bool dummy = bx >= g.bw[kt] || by >= g.bh[kt];
    int32_t blk[64];
    if (dummy) {
        // zero ACs; the DC is the one of the last real block before it in the MCU (block 0 of a luma MCU always is real)
        while (dummy) {
            --j;
            block_at(g, mx, my, j, c, bx, by);
            dummy = bx >= g.bw[0] || by >= g.bh[0];
        }
        sample_block(img, g, 0, bx, by, blk);
        fdct_islow(blk);
        const int16_t dc = quantize(blk[0], t->recip[0][0], t->corr[0][0], t->shift[0][0]);
        int4 *o = (int4 *)out;
        const int4 z = make_int4(0, 0, 0, 0);
        MSPA_UNROLL
        for (int i = 0; i < 8; ++i) o[i] = z;
        out[0] = dc;
        return;
    }
    sample_block(img, g, c, bx, by, blk);
    fdct_islow(blk);
    int4 *o = (int4 *)out;
    MSPA_UNROLL
    for (int i = 0; i < 8; ++i) {
        int16_t v[8];
        MSPA_UNROLL
        for (int e = 0; e < 8; ++e) v[e] = quantize(blk[8 * i + e], t->recip[kt][8 * i + e], t->corr[kt][8 * i + e], t->shift[kt][8 * i + e]);
        o[i] = make_int4((uint16_t)v[0] | ((uint32_t)(uint16_t)v[1] << 16), (uint16_t)v[2] | ((uint32_t)(uint16_t)v[3] << 16),
                         (uint16_t)v[4] | ((uint32_t)(uint16_t)v[5] << 16), (uint16_t)v[6] | ((uint32_t)(uint16_t)v[7] << 16));
    }
}

__global__ void __launch_bounds__(256) bits_kernel(Geometry g, const Tables *__restrict__ t, const int16_t *__restrict__ coef,
                                                   int64_t *__restrict__ offs) {
    const int64_t k = blockIdx.y;
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= mcus(g)) return;
    const int16_t(*blk)[64] = (const int16_t(*)[64])(coef + (k * blocks(g) + m * g.blocks_per_mcu) * 64);
    int32_t pred[3];
    mcu_preds(m ? blk - g.blocks_per_mcu : nullptr, g, pred);
    BitCount cnt;
    encode_mcu(blk, pred, g, *t, cnt);
    offs[k * mcus(g) + m] = cnt.n;
}

// Exclusive scan of one value per thread over a 1024-thread workgroup; `total` gets the sum.  lds: 32 int64.
__device__ int64_t block_scan(int64_t v, int64_t *lds, int64_t &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t x = v;
    MSPA_UNROLL
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) lds[wave] = x;
    __syncthreads();
    if (wave == 0) {
        int64_t s = lane < 16 ? lds[lane] : 0;
        MSPA_UNROLL
        for (int o = 1; o < 16; o <<= 1) {
            const int64_t y = __shfl_up(s, o, 64);
            if (lane >= o) s += y;
        }
        if (lane < 16) lds[16 + lane] = s;
    }
    __syncthreads();
    const int64_t before = wave ? lds[16 + wave - 1] : 0;
    total = lds[31];
    __syncthreads();
    return before + x - v;
}

__global__ void __launch_bounds__(1024) scan_kernel(int64_t n_mcus, int64_t *__restrict__ offs, int64_t *__restrict__ totals) {
    __shared__ int64_t lds[32];
    const int64_t k = blockIdx.x;
    int64_t *o = offs + k * n_mcus;
    int64_t run = 0;
    for (int64_t base = 0; base < n_mcus; base += 1024) {
        const int64_t i = base + threadIdx.x;
        const int64_t v = i < n_mcus ? o[i] : 0;
        int64_t tile = 0;
        const int64_t ex = block_scan(v, lds, tile);
        if (i < n_mcus) o[i] = run + ex;
        run += tile;
    }
    if (threadIdx.x == 0) totals[k] = run;
}

// Big-endian bit writer over 32-bit words; only the span's first and last word can be shared with a neighbouring MCU.
struct WordSink {
    uint32_t *words;
    int64_t nwords, wi, first, last;
    uint32_t cur;
    int used;                                          // bits of `cur` filled
    __device__ void flush() {
        if (wi < 0 || wi >= nwords) return;
        const uint32_t v = __builtin_bswap32(cur);
        if (wi == first || wi == last) atomicOr(words + wi, v);
        else words[wi] = v;
    }
    __device__ void put(uint32_t bits, int nbits) {
        bits &= (1u << nbits) - 1;
        const int room = 32 - used;
        if (nbits < room) {
            cur |= bits << (room - nbits);
            used += nbits;
        } else {
            const int rest = nbits - room;
            cur |= bits >> rest;
            flush();
            ++wi;
            cur = rest ? bits << (32 - rest) : 0u;
            used = rest;
        }
    }
};

__global__ void __launch_bounds__(256) write_kernel(Geometry g, const Tables *__restrict__ t, const int16_t *__restrict__ coef,
                                                    const int64_t *__restrict__ offs, const int64_t *__restrict__ totals,
                                                    uint8_t *__restrict__ raw) {
    const int64_t k = blockIdx.y;
    const int64_t nm = mcus(g);
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= nm) return;
    const int16_t(*blk)[64] = (const int16_t(*)[64])(coef + (k * blocks(g) + m * g.blocks_per_mcu) * 64);
    int32_t pred[3];
    mcu_preds(m ? blk - g.blocks_per_mcu : nullptr, g, pred);
    const int64_t start = offs[k * nm + m];
    const int64_t end = m + 1 < nm ? offs[k * nm + m + 1] : totals[k];
    if (end <= start) return;
    WordSink s;
    s.words = (uint32_t *)(raw + k * raw_bytes(g));
    s.nwords = raw_bytes(g) / 4;
    s.wi = start >> 5;
    s.first = start >> 5;
    s.last = (end - 1) >> 5;
    s.used = (int)(start & 31);
    s.cur = 0;
    encode_mcu(blk, pred, g, *t, s);
    if (s.used) s.flush();
}

__global__ void __launch_bounds__(1024) stuff_kernel(Geometry g, const uint8_t *__restrict__ hdr, const int64_t *__restrict__ totals,
                                                     const uint8_t *__restrict__ raw, uint8_t *__restrict__ out, int64_t pitch,
                                                     int64_t *__restrict__ out_bytes) {
    __shared__ int64_t lds[32];
    const int64_t k = blockIdx.x;
    uint8_t *o = out + k * pitch;
    for (int i = threadIdx.x; i < kHeaderBytes; i += 1024)
        if (i < pitch) o[i] = hdr[i];
    const int64_t bits = totals[k];
    const int64_t nraw = (bits + 7) >> 3;
    const int pad = (int)((8 - (bits & 7)) & 7);
    const uint8_t *r = raw + k * raw_bytes(g);
    int64_t pos = kHeaderBytes;
    for (int64_t base = 0; base < nraw; base += 4096) {
        const int64_t b0 = base + 4 * (int64_t)threadIdx.x;
        uint8_t v[4];
        int cnt = 0;
        if (b0 < nraw) {
            const uint32_t word = *(const uint32_t *)(r + b0);
            MSPA_UNROLL
            for (int e = 0; e < 4; ++e) {
                v[e] = (uint8_t)(word >> (8 * e));
                if (b0 + e < nraw) {
                    if (b0 + e == nraw - 1) v[e] |= (uint8_t)((1u << pad) - 1);
                    cnt += v[e] == 0xFF ? 2 : 1;
                }
            }
        }
        int64_t tile = 0;
        int64_t p = pos + block_scan(cnt, lds, tile);
        if (b0 < nraw) {
            for (int e = 0; e < 4 && b0 + e < nraw; ++e) {
                if (p < pitch) o[p] = v[e];
                ++p;
                if (v[e] == 0xFF) {
                    if (p < pitch) o[p] = 0;
                    ++p;
                }
            }
        }
        pos += tile;
    }
    if (threadIdx.x == 0) {
        if (pos < pitch) o[pos] = 0xFF;
        if (pos + 1 < pitch) o[pos + 1] = 0xD9;
        out_bytes[k] = pos + 2;
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// Compositing.  Spans arrive grouped by (image, row) with call order kept inside a group; the last span of a group that covers
// a pixel paints it.  Labels arrive grouped by image with call order kept inside a group; the first label covering a pixel
// blends every label of its group that covers the pixel, in order.

__global__ void __launch_bounds__(256) spans_kernel(const int32_t *__restrict__ spans, int64_t n_spans, int64_t n_images, int32_t h,
                                                    int32_t w, uint8_t *__restrict__ img) {
    const int64_t s = blockIdx.x;
    const int32_t *e = spans + s * 5;
    const int32_t im = e[0], y = e[1], x0 = e[2], x1 = e[3];
    const uint32_t rgb = (uint32_t)e[4];
    if (im < 0 || im >= n_images || y < 0 || y >= h) return;
    const int lo = x0 < 0 ? 0 : x0, hi = x1 >= w ? w - 1 : x1;
    for (int x = lo + (int)threadIdx.x; x <= hi; x += 256) {
        bool later = false;
        for (int64_t q = s + 1; q < n_spans; ++q) {
            const int32_t *f = spans + q * 5;
            if (f[0] != im || f[1] != y) break;
            if (f[2] <= x && x <= f[3]) {
                later = true;
                break;
            }
        }
        if (later) continue;
        uint8_t *p = img + (((int64_t)im * h + y) * w + x) * 3;
        p[0] = (uint8_t)(rgb >> 16);
        p[1] = (uint8_t)(rgb >> 8);
        p[2] = (uint8_t)rgb;
    }
}

// label entry: int64 [image, x, y, mask w, mask h, rgb, mask offset, 0]
__device__ __forceinline__ bool label_covers(const int64_t *e, int x, int y) {
    return x >= e[1] && x < e[1] + e[3] && y >= e[2] && y < e[2] + e[4];
}

MSPA_HD bool label_ok(const int64_t *e, int64_t masks_bytes, int64_t n_images) {
    return e[0] >= 0 && e[0] < n_images && e[3] >= 0 && e[4] >= 0 && e[3] <= 65535 && e[4] <= 65535 && e[6] >= 0 &&
           e[6] + e[3] * e[4] <= masks_bytes && e[1] > -(1ll << 30) && e[1] < (1ll << 30) && e[2] > -(1ll << 30) && e[2] < (1ll << 30);
}

__global__ void __launch_bounds__(256) masks_kernel(const int64_t *__restrict__ labels, int64_t n_labels, const uint8_t *__restrict__ masks,
                                                    int64_t masks_bytes, int64_t n_images, int32_t h, int32_t w, uint8_t *__restrict__ img) {
    const int64_t j = blockIdx.x;
    const int64_t *e = labels + j * 8;
    if (!label_ok(e, masks_bytes, n_images)) return;
    const int64_t im = e[0];
    const int64_t mw = e[3], mh = e[4];
    for (int64_t i = threadIdx.x; i < mw * mh; i += 256) {
        const int yy = (int)(i / mw), xx = (int)(i - yy * mw);
        const int x = (int)e[1] + xx, y = (int)e[2] + yy;
        if (x < 0 || x >= w || y < 0 || y >= h) continue;
        bool earlier = false;
        for (int64_t q = j - 1; q >= 0 && labels[q * 8] == im; --q)
            if (label_ok(labels + q * 8, masks_bytes, n_images) && label_covers(labels + q * 8, x, y)) {
                earlier = true;
                break;
            }
        if (earlier) continue;
        uint8_t *p = img + ((im * h + y) * w + x) * 3;
        int px[3] = {p[0], p[1], p[2]};
        for (int64_t q = j; q < n_labels && labels[q * 8] == im; ++q) {
            const int64_t *f = labels + q * 8;
            if (!label_ok(f, masks_bytes, n_images) || !label_covers(f, x, y)) continue;
            const int mv = masks[f[6] + (int64_t)(y - f[2]) * f[3] + (x - f[1])];
            const uint32_t ink = (uint32_t)f[5];
            MSPA_UNROLL
            for (int c = 0; c < 3; ++c) {
                const int ic = (int)((ink >> (16 - 8 * c)) & 255);
                const int tt = ic * mv + px[c] * (255 - mv) + 128;
                px[c] = ((tt >> 8) + tt) >> 8;
            }
        }
        p[0] = (uint8_t)px[0];
        p[1] = (uint8_t)px[1];
        p[2] = (uint8_t)px[2];
    }
}

}  // namespace jpege
}  // namespace mspa

using namespace mspa;

extern "C" int64_t mspa_jpeg_encode_capacity(int32_t h, int32_t w, int32_t subsampling) {
    if (!jpege::valid_args(h, w, 50, subsampling)) return -1;
    return jpege::capacity(jpege::geometry(h, w, subsampling));
}

extern "C" int64_t mspa_jpeg_encode_workspace_bytes(int64_t n_images, int32_t h, int32_t w, int32_t subsampling) {
    if (n_images < 0 || !jpege::valid_args(h, w, 50, subsampling)) return -1;
    return jpege::layout(n_images, jpege::geometry(h, w, subsampling)).end;
}

extern "C" int mspa_jpeg_encode_header_host(int32_t h, int32_t w, int32_t quality, int32_t subsampling, uint8_t *dst,
                                            int64_t capacity, int64_t *nbytes) {
    if (!jpege::valid_args(h, w, quality, subsampling)) return fail(MSPA_EINVAL, "mspa_jpeg_encode_header_host: bad size, quality or subsampling");
    if (!dst || !nbytes) return fail(MSPA_EINVAL, "mspa_jpeg_encode_header_host: null pointer");
    if (capacity < jpege::kHeaderBytes) return fail(MSPA_EINVAL, "mspa_jpeg_encode_header_host: capacity below the header's size");
    *nbytes = jpege::write_header(h, w, quality, subsampling, dst);
    return MSPA_OK;
}

extern "C" int mspa_jpeg_encode_device(const uint8_t *rgb_dev, int64_t n_images, int32_t h, int32_t w, int32_t quality,
                                       int32_t subsampling, uint8_t *out_dev, int64_t out_pitch, int64_t *out_bytes_dev,
                                       void *workspace, int64_t workspace_bytes, void *stream) {
    if (n_images < 0 || !jpege::valid_args(h, w, quality, subsampling))
        return fail(MSPA_EINVAL, "mspa_jpeg_encode_device: bad size, quality or subsampling");
    if (n_images == 0) return MSPA_OK;
    if (n_images > 65535) return fail(MSPA_EINVAL, "mspa_jpeg_encode_device: more than 65 535 images in one call");
    if (!rgb_dev || !out_dev || !out_bytes_dev || !workspace) return fail(MSPA_EINVAL, "mspa_jpeg_encode_device: null pointer");
    if (out_pitch < 0) return fail(MSPA_EINVAL, "mspa_jpeg_encode_device: negative pitch");
    const jpege::Geometry g = jpege::geometry(h, w, subsampling);
    const jpege::Layout l = jpege::layout(n_images, g);
    if (workspace_bytes < l.end) return fail(MSPA_EINVAL, "mspa_jpeg_encode_device: workspace smaller than mspa_jpeg_encode_workspace_bytes()");
    if ((uintptr_t)workspace & 15u) return fail(MSPA_EINVAL, "mspa_jpeg_encode_device: workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    uint8_t *ws = (uint8_t *)workspace;
    auto *tables = (jpege::Tables *)ws;
    uint8_t *hdr = ws + sizeof(jpege::Tables);
    auto *coef = (int16_t *)(ws + l.coef);
    auto *offs = (int64_t *)(ws + l.offs);
    auto *totals = (int64_t *)(ws + l.totals);
    uint8_t *raw = ws + l.raw;
    hipError_t e = hipMemsetAsync(raw, 0, (size_t)(l.end - l.raw), st);
    if (e != hipSuccess) return check_hip(e, "mspa_jpeg_encode_device: memset");
    const unsigned ny = (unsigned)n_images;
    hipLaunchKernelGGL(jpege::tables_kernel, dim3(1), dim3(64), 0, st, h, w, quality, subsampling, tables, hdr);
    const int64_t nb = jpege::blocks(g), nm = jpege::mcus(g);
    hipLaunchKernelGGL(jpege::coef_kernel, dim3((unsigned)((nb + 255) / 256), ny), dim3(256), 0, st, rgb_dev, g,
                       (const jpege::Tables *)tables, coef);
    hipLaunchKernelGGL(jpege::bits_kernel, dim3((unsigned)((nm + 255) / 256), ny), dim3(256), 0, st, g, (const jpege::Tables *)tables,
                       (const int16_t *)coef, offs);
    hipLaunchKernelGGL(jpege::scan_kernel, dim3(ny), dim3(1024), 0, st, nm, offs, totals);
    hipLaunchKernelGGL(jpege::write_kernel, dim3((unsigned)((nm + 255) / 256), ny), dim3(256), 0, st, g, (const jpege::Tables *)tables,
                       (const int16_t *)coef, (const int64_t *)offs, (const int64_t *)totals, raw);
    hipLaunchKernelGGL(jpege::stuff_kernel, dim3(ny), dim3(1024), 0, st, g, (const uint8_t *)hdr, (const int64_t *)totals,
                       (const uint8_t *)raw, out_dev, out_pitch, out_bytes_dev);
    return check_hip(hipGetLastError(), "mspa_jpeg_encode_device");
}

extern "C" int mspa_draw_spans_device(const int32_t *spans_dev, int64_t n_spans, uint8_t *images_dev, int64_t n_images, int32_t h,
                                      int32_t w, void *stream) {
    if (n_spans < 0 || n_images < 0 || h <= 0 || w <= 0) return fail(MSPA_EINVAL, "mspa_draw_spans_device: bad size");
    if (n_spans == 0) return MSPA_OK;
    if (!spans_dev || !images_dev) return fail(MSPA_EINVAL, "mspa_draw_spans_device: null pointer");
    if (n_spans > 0x7FFFFFFF) return fail(MSPA_EINVAL, "mspa_draw_spans_device: too many spans");
    hipLaunchKernelGGL(jpege::spans_kernel, dim3((unsigned)n_spans), dim3(256), 0, (hipStream_t)stream, spans_dev, n_spans, n_images, h, w,
                       images_dev);
    return check_hip(hipGetLastError(), "mspa_draw_spans_device");
}

extern "C" int mspa_blend_masks_device(const int64_t *labels_dev, int64_t n_labels, const uint8_t *masks_dev, int64_t masks_bytes,
                                       uint8_t *images_dev, int64_t n_images, int32_t h, int32_t w, void *stream) {
    if (n_labels < 0 || n_images < 0 || masks_bytes < 0 || h <= 0 || w <= 0) return fail(MSPA_EINVAL, "mspa_blend_masks_device: bad size");
    if (n_labels == 0) return MSPA_OK;
    if (!labels_dev || !masks_dev || !images_dev) return fail(MSPA_EINVAL, "mspa_blend_masks_device: null pointer");
    if (n_labels > 0x7FFFFFFF) return fail(MSPA_EINVAL, "mspa_blend_masks_device: too many labels");
    hipLaunchKernelGGL(jpege::masks_kernel, dim3((unsigned)n_labels), dim3(256), 0, (hipStream_t)stream, labels_dev, n_labels, masks_dev,
                       masks_bytes, n_images, h, w, images_dev);
    return check_hip(hipGetLastError(), "mspa_blend_masks_device");
}
