// Frame sharpness ON the MI355X: the variance of the Laplacian of a frame's grey image (the reference's
// calculate_image_sharpness, handler/ops.py:22-34: cv2.imread(IMREAD_GRAYSCALE), cv2.Laplacian(CV_64F), .var()).
//
//   mspa_jpeg_decode_luma_device -- the grey image of a baseline JPEG is its component 0 after the IDCT, at the image's size
//     (libjpeg's out_color_space = JCS_GRAYSCALE).  The entropy phase is jpeg_decode.hip's entropy_kernel as it stands (chroma is
//     walked: the scan is one interleaved bit stream); the IDCT runs over the blocks of component 0 only, and a copy crops the
//     MCU-padded plane to [h, w].  Same workspace, same status codes as mspa_jpeg_decode_device.
//   mspa_laplacian_moments_device -- L = I(y-1,x) + I(y+1,x) + I(y,x-1) + I(y,x+1) - 4 I(y,x) with reflect-101 borders (-1 -> 1,
//     len -> len - 2; a dimension of length 1 maps every index to 0), and per image and block of kRows rows S1 = sum L and
//     S2 = sum L^2 as int64: |L| <= 1020, so a 32-bit sum of squares would overflow after some 2 000 pixels.  No atomics: a
//     workgroup owns its slot, lanes add in a fixed order.  The host adds the blocks in integers.
#include "mspa_common.h"
#include "jpeg_core.h"

#include <algorithm>

namespace mspa {
namespace jpeg {

// csrc/jpeg_decode.hip
__global__ void entropy_kernel(const uint8_t *__restrict__ src, int64_t src_words, const int64_t *__restrict__ offsets,
                               const int64_t *__restrict__ nbytes, const JpegDesc *__restrict__ desc, int64_t n, int32_t h, int32_t w, int lanes,
                               int16_t *__restrict__ coef, int32_t *__restrict__ status);
int simd_count();

}  // namespace jpeg

namespace image_ops {

constexpr int kRows = 8;             // rows of one block of the moments
constexpr int kThreads = 256;

// One thread per 8x8 block of component 0 (entropy_kernel has checked the descriptor's geometry against (h, w)).
__global__ void __launch_bounds__(256) luma_idct_kernel(const jpeg::JpegDesc *__restrict__ desc, int32_t h, int32_t w,
                                                        const int16_t *__restrict__ coef, uint8_t *__restrict__ planes,
                                                        int32_t *__restrict__ status) {
    const int64_t k = blockIdx.y;
    if (status[k] != jpeg::kOk) return;
    const jpeg::JpegDesc *d = desc + k;
    const int b = blockIdx.x * 256 + threadIdx.x;
    const int bw = d->bw[0];
    if (b >= bw * d->bh[0]) return;
    const int by = b / bw, bx = b - by * bw;
    const int64_t slot = jpeg::slot_blocks(h, w) * 64;
    uint8_t *out = planes + k * slot + (int64_t)by * 8 * (bw * 8) + bx * 8;
    int16_t blk[64];
    const int4 *src = (const int4 *)(coef + k * slot + (int64_t)b * 64);
#pragma unroll
    for (int i = 0; i < 8; ++i) *(int4 *)(blk + 8 * i) = src[i];
    if (!jpeg::idct_islow(blk, d->qt[0], out, (int64_t)bw * 8)) status[k] = jpeg::kOutOfRange;
}

__global__ void __launch_bounds__(256) luma_crop_kernel(const jpeg::JpegDesc *__restrict__ desc, int32_t h, int32_t w,
                                                        const uint8_t *__restrict__ planes, uint8_t *__restrict__ out,
                                                        const int32_t *__restrict__ status) {
    const int64_t k = blockIdx.y;
    if (status[k] != jpeg::kOk) return;
    const int64_t npix = (int64_t)h * w;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const int y = (int)(p / w), x = (int)(p - (int64_t)y * w);
    out[k * npix + p] = planes[k * jpeg::slot_blocks(h, w) * 64 + (int64_t)y * (desc[k].bw[0] * 8) + x];
}

__device__ __forceinline__ int reflect101(int i, int len) { return len == 1 ? 0 : i < 0 ? -i : i >= len ? 2 * len - 2 - i : i; }

__global__ void __launch_bounds__(kThreads) laplacian_moments_kernel(const uint8_t *__restrict__ luma, int32_t h, int32_t w, int32_t blocks,
                                                                     int64_t *__restrict__ partials) {
    const int64_t k = blockIdx.y;
    const uint8_t *img = luma + k * (int64_t)h * w;
    const int y0 = blockIdx.x * kRows, rows = min(kRows, h - y0);
    long long s1 = 0, s2 = 0;
    for (int p = threadIdx.x; p < rows * w; p += kThreads) {
        const int y = y0 + p / w, x = p % w;
        const int64_t row = (int64_t)y * w;
        const int L = (int)img[(int64_t)reflect101(y - 1, h) * w + x] + (int)img[(int64_t)reflect101(y + 1, h) * w + x] +
                      (int)img[row + reflect101(x - 1, w)] + (int)img[row + reflect101(x + 1, w)] - 4 * (int)img[row + x];
        s1 += L;
        s2 += L * L;
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        s1 += __shfl_down(s1, off, kWave);
        s2 += __shfl_down(s2, off, kWave);
    }
    __shared__ long long part[kThreads / kWave][2];
    if ((threadIdx.x & (kWave - 1)) == 0) {
        part[threadIdx.x / kWave][0] = s1;
        part[threadIdx.x / kWave][1] = s2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long a = 0, b = 0;
        for (int i = 0; i < kThreads / kWave; ++i) {
            a += part[i][0];
            b += part[i][1];
        }
        int64_t *o = partials + (k * blocks + blockIdx.x) * 2;
        o[0] = a;
        o[1] = b;
    }
}

}  // namespace image_ops
}  // namespace mspa

using namespace mspa;

extern "C" int mspa_jpeg_decode_luma_device(const void *src_dev, const int64_t *src_offsets_dev, const int64_t *src_bytes_dev,
                                            int64_t src_capacity, const void *desc_dev, int64_t n_images, int32_t h, int32_t w,
                                            uint8_t *out_dev, int32_t *status_dev, void *workspace, int64_t workspace_bytes, void *stream) {
    if (n_images < 0 || h <= 0 || w <= 0 || src_capacity < 0) return fail(MSPA_EINVAL, "mspa_jpeg_decode_luma_device: bad size");
    if (n_images == 0) return MSPA_OK;
    if (!src_dev || !src_offsets_dev || !src_bytes_dev || !desc_dev || !out_dev || !status_dev || !workspace)
        return fail(MSPA_EINVAL, "mspa_jpeg_decode_luma_device: null pointer");
    if (n_images > 65535) return fail(MSPA_EINVAL, "mspa_jpeg_decode_luma_device: more than 65 535 images in one call");
    if (workspace_bytes < mspa_jpeg_workspace_bytes(n_images, h, w))
        return fail(MSPA_EINVAL, "mspa_jpeg_decode_luma_device: workspace smaller than mspa_jpeg_workspace_bytes()");
    if (((uintptr_t)src_dev & 3u) || ((uintptr_t)workspace & 15u) || ((uintptr_t)desc_dev & 15u))
        return fail(MSPA_EINVAL, "mspa_jpeg_decode_luma_device: src must be 4-byte, workspace and descriptors 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int64_t slot = jpeg::slot_blocks(h, w) * 64;
    int16_t *coef = (int16_t *)workspace;
    uint8_t *planes = (uint8_t *)workspace + n_images * slot * 2;
    hipError_t e = hipMemsetAsync(coef, 0, (size_t)(n_images * slot * 2), st);
    if (e != hipSuccess) return check_hip(e, "mspa_jpeg_decode_luma_device: memset");
    const int64_t simds = jpeg::simd_count();
    const int lanes = (int)std::min<int64_t>(64, std::max<int64_t>(1, (n_images + simds - 1) / simds));
    const auto *desc = (const jpeg::JpegDesc *)desc_dev;
    hipLaunchKernelGGL(jpeg::entropy_kernel, dim3((unsigned)((n_images + lanes - 1) / lanes)), dim3(64), 0, st, (const uint8_t *)src_dev,
                       src_capacity >> 2, src_offsets_dev, src_bytes_dev, desc, n_images, h, w, lanes, coef, status_dev);
    // component 0 has at most ceil(h / 8 / vmax) * vmax x ceil(w / 8 / hmax) * hmax blocks, hmax, vmax <= 2
    const int64_t luma_blocks = (int64_t)((h + 15) / 16 * 2) * ((w + 15) / 16 * 2);
    hipLaunchKernelGGL(image_ops::luma_idct_kernel, dim3((unsigned)((luma_blocks + 255) / 256), (unsigned)n_images), dim3(256), 0, st, desc, h,
                       w, (const int16_t *)coef, planes, status_dev);
    hipLaunchKernelGGL(image_ops::luma_crop_kernel, dim3((unsigned)(((int64_t)h * w + 255) / 256), (unsigned)n_images), dim3(256), 0, st, desc,
                       h, w, (const uint8_t *)planes, out_dev, (const int32_t *)status_dev);
    return check_hip(hipGetLastError(), "mspa_jpeg_decode_luma_device");
}

extern "C" int32_t mspa_laplacian_blocks(int32_t h, int32_t w) {
    if (h <= 0 || w <= 0) return -1;
    return (h + image_ops::kRows - 1) / image_ops::kRows;
}

extern "C" int mspa_laplacian_moments_device(const uint8_t *luma_dev, int64_t n, int32_t h, int32_t w, int64_t *partials_dev, void *stream) {
    if (n < 0 || h <= 0 || w <= 0 || (int64_t)image_ops::kRows * w > INT32_MAX) return fail(MSPA_EINVAL, "mspa_laplacian_moments_device: bad size");
    if (n == 0) return MSPA_OK;
    if (!luma_dev || !partials_dev) return fail(MSPA_EINVAL, "mspa_laplacian_moments_device: null pointer");
    if (n > 65535) return fail(MSPA_EINVAL, "mspa_laplacian_moments_device: more than 65 535 images in one call");
    const int32_t blocks = mspa_laplacian_blocks(h, w);
    hipLaunchKernelGGL(image_ops::laplacian_moments_kernel, dim3((unsigned)blocks, (unsigned)n), dim3(image_ops::kThreads), 0,
                       (hipStream_t)stream, luma_dev, h, w, blocks, partials_dev);
    return check_hip(hipGetLastError(), "mspa_laplacian_moments_device");
}
