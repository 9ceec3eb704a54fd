// Colour-frame decode ON the MI355X: baseline JPEG (SOF0, 8-bit, Huffman, one interleaved scan; greyscale or YCbCr 4:4:4 /
// 4:2:2 / 4:2:0) decoded bit-identically to libjpeg-turbo's default decompression -- what `Image.open(f).convert("RGB")` and
// `cv2.imread` + BGR->RGB (ops.py:265-266) give.  The arithmetic is csrc/jpeg_core.h; this file holds the kernels and the C ABI.
//
// Three phases, each its own kernel:
//   1. entropy_kernel -- the Huffman decode is serial inside an entropy-coded segment, so the parallelism is ACROSS images: one
//      lane per image walks its whole scan (restart markers checked in line) and scatters the non-zero coefficients, natural
//      order, into the zeroed int16 coefficient slot of its image.  A wave takes `lanes` images (1 .. 64, chosen from the batch
//      size so that the batch spreads over every SIMD of the chip before lanes of one wave are shared: a lane's time is its
//      chain of dependent table loads, and 64 lanes in lock step only pay off once every SIMD already holds a wave).
//   2. idct_kernel -- one thread per 8x8 block: dequantise, JDCT_ISLOW, range limit, into the image's component planes
//      (MCU-padded, pitch bw * 8).  A block outside the bounds every IDCT form agrees in declines its image (status 7).
//   3. color_kernel -- one thread per 4 output pixels: fancy upsampling of the chroma planes, YCbCr -> RGB, [H, W, 3] uint8
//      stores (three dwords when the 12 bytes are aligned).
// A declined image's phases 2 and 3 are skipped; its output is unspecified and the caller decodes it on the host.
#include "mspa_common.h"
#include "jpeg_core.h"

#include <algorithm>

namespace mspa {
namespace jpeg {

// The descriptor's geometry is re-derived from (h, w) and the sampling factors before a single coefficient is stored: whatever
// a caller passes as a descriptor, the decode never writes outside its image's slot.
__device__ bool geometry_ok(const JpegDesc *d, int32_t h, int32_t w) {
    if (d->h != h || d->w != w) return false;
    const int nc = d->ncomp;
    if (nc != 1 && nc != 3) return false;
    const int hm = d->hmax, vm = d->vmax;
    if (hm < 1 || hm > 2 || vm < 1 || vm > 2) return false;
    if (d->mcus_x != (w + 8 * hm - 1) / (8 * hm) || d->mcus_y != (h + 8 * vm - 1) / (8 * vm)) return false;
    int off = 0;
    for (int c = 0; c < nc; ++c) {
        const int sh = d->samp_h[c], sv = d->samp_v[c];
        if (sh < 1 || sv < 1 || sh > hm || sv > vm) return false;
        if (d->bw[c] != d->mcus_x * sh || d->bh[c] != d->mcus_y * sv || d->block_off[c] != off) return false;
        if (d->dw[c] < 1 || d->dw[c] > d->bw[c] * 8 || d->dh[c] < 1 || d->dh[c] > d->bh[c] * 8) return false;
        if (d->td[c] < 0 || d->td[c] > 1 || d->ta[c] < 0 || d->ta[c] > 1) return false;
        off += d->bw[c] * d->bh[c];
    }
    if (nc == 1 && (hm != 1 || vm != 1)) return false;
    if (nc == 3 && (d->samp_h[0] != hm || d->samp_v[0] != vm || d->samp_h[1] != 1 || d->samp_v[1] != 1 || d->samp_h[2] != 1 ||
                    d->samp_v[2] != 1)) return false;
    return off == d->total_blocks && (int64_t)off <= slot_blocks(h, w) && d->restart_interval >= 0;
}

__global__ void __launch_bounds__(64) entropy_kernel(const uint8_t *__restrict__ src, int64_t src_words, const int64_t *__restrict__ offsets,
                                                     const int64_t *__restrict__ nbytes, const JpegDesc *__restrict__ desc, int64_t n,
                                                     int32_t h, int32_t w, int lanes, int16_t *__restrict__ coef, int32_t *__restrict__ status) {
    const int lane = threadIdx.x;
    if (lane >= lanes) return;
    const int64_t k = (int64_t)blockIdx.x * lanes + lane;
    if (k >= n) return;
    const JpegDesc *d = desc + k;
    int32_t st = d->status;
    if (st == kOk && !geometry_ok(d, h, w)) st = kWrongSize;
    const int64_t off = offsets[k], len = nbytes[k];
    if (st == kOk && (off < 0 || len < 0 || d->scan_offset < 0 || d->scan_offset > len || ((off + len + 3) >> 2) > src_words))
        st = kNotJpeg;
    if (st == kOk)
        st = decode_entropy(d, (const uint32_t *)src, off + d->scan_offset, len - d->scan_offset, coef + k * slot_blocks(h, w) * 64);
    status[k] = st;
}

__global__ void __launch_bounds__(256) idct_kernel(const JpegDesc *__restrict__ desc, int32_t h, int32_t w, const int16_t *__restrict__ coef,
                                                   uint8_t *__restrict__ planes, int32_t *__restrict__ status) {
    const int64_t k = blockIdx.y;
    if (status[k] != kOk) return;
    const JpegDesc *d = desc + k;
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= d->total_blocks) return;
    int c = 0;
    if (d->ncomp == 3) c = b >= d->block_off[2] ? 2 : b >= d->block_off[1] ? 1 : 0;
    const int rel = b - d->block_off[c], bw = d->bw[c];
    const int by = rel / bw, bx = rel - by * bw;
    const int64_t slot = slot_blocks(h, w) * 64;
    uint8_t *out = planes + k * slot + (int64_t)d->block_off[c] * 64 + (int64_t)by * 8 * (bw * 8) + bx * 8;
    int16_t blk[64];
    const int4 *src = (const int4 *)(coef + k * slot + (int64_t)b * 64);
#pragma unroll
    for (int i = 0; i < 8; ++i) *(int4 *)(blk + 8 * i) = src[i];
    if (!idct_islow(blk, d->qt[c], out, (int64_t)bw * 8)) status[k] = kOutOfRange;
}

__global__ void __launch_bounds__(256) color_kernel(const JpegDesc *__restrict__ desc, int32_t h, int32_t w, const uint8_t *__restrict__ planes,
                                                    uint8_t *__restrict__ out, const int32_t *__restrict__ status) {
    const int64_t k = blockIdx.y;
    if (status[k] != kOk) return;
    const JpegDesc *d = desc + k;
    const int64_t npix = (int64_t)h * w;
    const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 >= npix) return;
    const uint8_t *pl = planes + k * slot_blocks(h, w) * 64;
    const int64_t pitch0 = (int64_t)d->bw[0] * 8;
    uint8_t px[12];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t p = p0 + i < npix ? p0 + i : npix - 1;
        const int y = (int)(p / w), x = (int)(p - (int64_t)y * w);
        const int Y = pl[(int64_t)y * pitch0 + x];
        if (d->ncomp == 1) {
            px[3 * i] = px[3 * i + 1] = px[3 * i + 2] = (uint8_t)Y;
        } else {
            const int cb = chroma_at(pl + (int64_t)d->block_off[1] * 64, (int64_t)d->bw[1] * 8, d->dw[1], d->dh[1], d->hmax, d->vmax, y, x);
            const int cr = chroma_at(pl + (int64_t)d->block_off[2] * 64, (int64_t)d->bw[2] * 8, d->dw[2], d->dh[2], d->hmax, d->vmax, y, x);
            ycc_to_rgb(Y, cb, cr, px + 3 * i);
        }
    }
    uint8_t *o = out + (k * npix + p0) * 3;
    if (p0 + 4 <= npix && ((uintptr_t)o & 3u) == 0) {
        uint32_t *o32 = (uint32_t *)o;
#pragma unroll
        for (int j = 0; j < 3; ++j)
            o32[j] = px[4 * j] | (px[4 * j + 1] << 8) | (px[4 * j + 2] << 16) | ((uint32_t)px[4 * j + 3] << 24);
    } else {
        for (int i = 0; i < 4 && p0 + i < npix; ++i) {
            o[3 * i] = px[3 * i];
            o[3 * i + 1] = px[3 * i + 1];
            o[3 * i + 2] = px[3 * i + 2];
        }
    }
}

int simd_count() {
    static int n = [] {
        int dev = 0, cu = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 1024;
        return cu * 4;
    }();
    return n;
}

}  // namespace jpeg
}  // namespace mspa

using namespace mspa;

static_assert(MSPA_JPEG_DESC_BYTES == jpeg::kDescBytes, "include/mspa.h and jpeg_core.h disagree on the descriptor size");

extern "C" int mspa_jpeg_parse_host(const void *const *src_host, const int64_t *nbytes_host, int64_t n, void *desc_host,
                                    int32_t *status_host) {
    if (n < 0) return fail(MSPA_EINVAL, "mspa_jpeg_parse_host: bad size");
    if (n == 0) return MSPA_OK;
    if (!src_host || !nbytes_host || !desc_host || !status_host) return fail(MSPA_EINVAL, "mspa_jpeg_parse_host: null pointer");
    for (int64_t k = 0; k < n; ++k) {
        jpeg::JpegDesc d;
        const int64_t len = nbytes_host[k];
        status_host[k] = jpeg::parse(len > 0 ? (const uint8_t *)src_host[k] : nullptr, len, d);
        uint8_t *dst = (uint8_t *)desc_host + k * (int64_t)MSPA_JPEG_DESC_BYTES;
        memset(dst, 0, MSPA_JPEG_DESC_BYTES);
        memcpy(dst, &d, sizeof(d));
    }
    return MSPA_OK;
}

extern "C" int64_t mspa_jpeg_workspace_bytes(int64_t n_images, int32_t h, int32_t w) {
    if (n_images < 0 || h <= 0 || w <= 0) return -1;
    return n_images * jpeg::slot_blocks(h, w) * 64 * 3;          // int16 coefficients + uint8 component planes
}

extern "C" int mspa_jpeg_decode_device(const void *src_dev, const int64_t *src_offsets_dev, const int64_t *src_bytes_dev,
                                       int64_t src_capacity, const void *desc_dev, int64_t n_images, int32_t h, int32_t w,
                                       uint8_t *out_dev, int32_t *status_dev, void *workspace, int64_t workspace_bytes, void *stream) {
    if (n_images < 0 || h <= 0 || w <= 0 || src_capacity < 0) return fail(MSPA_EINVAL, "mspa_jpeg_decode_device: bad size");
    if (n_images == 0) return MSPA_OK;
    if (!src_dev || !src_offsets_dev || !src_bytes_dev || !desc_dev || !out_dev || !status_dev || !workspace)
        return fail(MSPA_EINVAL, "mspa_jpeg_decode_device: null pointer");
    if (n_images > 65535) return fail(MSPA_EINVAL, "mspa_jpeg_decode_device: more than 65 535 images in one call");
    if (workspace_bytes < mspa_jpeg_workspace_bytes(n_images, h, w))
        return fail(MSPA_EINVAL, "mspa_jpeg_decode_device: workspace smaller than mspa_jpeg_workspace_bytes()");
    if (((uintptr_t)src_dev & 3u) || ((uintptr_t)workspace & 15u) || ((uintptr_t)desc_dev & 15u))
        return fail(MSPA_EINVAL, "mspa_jpeg_decode_device: src must be 4-byte, workspace and descriptors 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int64_t slot = jpeg::slot_blocks(h, w) * 64;
    int16_t *coef = (int16_t *)workspace;
    uint8_t *planes = (uint8_t *)workspace + n_images * slot * 2;
    hipError_t e = hipMemsetAsync(coef, 0, (size_t)(n_images * slot * 2), st);
    if (e != hipSuccess) return check_hip(e, "mspa_jpeg_decode_device: memset");
    const int64_t simds = jpeg::simd_count();
    const int lanes = (int)std::min<int64_t>(64, std::max<int64_t>(1, (n_images + simds - 1) / simds));
    const auto *desc = (const jpeg::JpegDesc *)desc_dev;
    hipLaunchKernelGGL(jpeg::entropy_kernel, dim3((unsigned)((n_images + lanes - 1) / lanes)), dim3(64), 0, st, (const uint8_t *)src_dev,
                       src_capacity >> 2, src_offsets_dev, src_bytes_dev, desc, n_images, h, w, lanes, coef, status_dev);
    hipLaunchKernelGGL(jpeg::idct_kernel, dim3((unsigned)((slot / 64 + 255) / 256), (unsigned)n_images), dim3(256), 0, st, desc, h, w,
                       (const int16_t *)coef, planes, status_dev);
    const int64_t quads = ((int64_t)h * w + 3) / 4;
    hipLaunchKernelGGL(jpeg::color_kernel, dim3((unsigned)((quads + 255) / 256), (unsigned)n_images), dim3(256), 0, st, desc, h, w,
                       (const uint8_t *)planes, out_dev, (const int32_t *)status_dev);
    return check_hip(hipGetLastError(), "mspa_jpeg_decode_device");
}
