// Image resizing ON the MI355X, bit-identical to Pillow's `Image.resize((W, H), BICUBIC | BILINEAR)` of an 8-bit RGB image.
// The arithmetic is csrc/resize_core.h; this file holds the two kernels and the C ABI.
//
// n images of one source shape go to one target shape per call, in Pillow's order:
//   1. horizontal_kernel -- [rows, w, 3] -> [rows, W, 3] over the source rows the vertical pass reads only.  A workgroup owns a
//      tile of 64 output columns x 16 rows: it stages the rows' source window (the taps of its 64 columns) and the 64 coefficient
//      rows in LDS, then every thread resamples 4 neighbouring pixels of one row and stores them as 3 dwords.  The intermediate
//      lives in the workspace with a 16-byte-aligned row pitch, so those stores and the next pass's loads are aligned.
//   2. vertical_kernel   -- [rows, W * 3] -> [H, W * 3], channel-blind (a row is W * 3 independent byte columns).  A workgroup
//      owns 256 byte columns x 16 output rows: it stages the window of source rows and the 16 coefficient rows in LDS; a wave
//      takes 4 of the output rows, a lane one dword of each.
// A pass whose size does not change is skipped, as in Pillow; then the remaining pass reads the caller's source (any pitch,
// any alignment) or writes the caller's destination directly, which is why both kernels stage through one loader that takes
// whole aligned dwords where a row has them and single bytes at its ragged ends, and store dwords only where the address and
// the row allow it.
//
// The tables arrive in device memory from the caller (mspa_resize_coeffs_host builds them), so the kernels trust nothing in
// them: every bound is clamped to the staged window and to ksize before it addresses LDS.  With the tables of resize_core.h
// no clamp ever changes a value: window_cap() is an upper bound of a tile's window.
#include "mspa_common.h"
#include "resize_core.h"

#include <vector>

namespace mspa {
namespace resize {

constexpr int kTileCols = 64;                         // horizontal pass: output columns of a tile
constexpr int kTileRows = 16;                         // both passes: rows of a tile
constexpr int kTileBytes = 256;                       // vertical pass: byte columns of a tile (one dword per lane)
constexpr int kThreads = 256;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// LDS row r (pitch lds_pitch, a multiple of 4) <- bytes [byte0, byte0 + nbytes) of source row r (`base` + r * pitch, valid for
// row_bytes bytes), placed so that aligned global dwords land on aligned LDS dwords: byte i of the span sits at LDS byte
// skew(r) + i with skew(r) = (address of the span's first byte) & 3.  lds_pitch >= nbytes + 3 rounded up to 4.
__device__ __forceinline__ void stage_rows(const uint8_t *__restrict__ base, int64_t pitch, int nrows, int64_t byte0, int nbytes,
                                           int64_t row_bytes, uint32_t *__restrict__ lds, int lds_pitch) {
    const int ndw = lds_pitch >> 2;
    for (int i = threadIdx.x; i < nrows * ndw; i += kThreads) {
        const int r = i / ndw, d = i - r * ndw;
        const uint8_t *row = base + (int64_t)r * pitch;
        const uint8_t *first = row + byte0, *last = first + nbytes, *end = row + row_bytes;
        const uint8_t *q = (const uint8_t *)(((uintptr_t)first & ~(uintptr_t)3) + 4u * (uint32_t)d);
        uint32_t v = 0;
        if (q < last) {
            if (q >= row && q + 4 <= end) {
                v = *(const uint32_t *)q;
            } else {
                MSPA_UNROLL
                for (int e = 0; e < 4; ++e)
                    if (q + e >= row && q + e < end) v |= (uint32_t)q[e] << (8 * e);
            }
        }
        lds[i] = v;
    }
}

// 4 bytes -> memory at p (byte `off` of a row that may be written up to row_cap and holds row_valid meaningful bytes).
__device__ __forceinline__ void store4(uint8_t *__restrict__ p, int64_t off, int64_t row_cap, int64_t row_valid, uint32_t v) {
    if ((((uintptr_t)p & 3) == 0) && off + 4 <= row_cap) {
        *(uint32_t *)p = v;
    } else {
        MSPA_UNROLL
        for (int e = 0; e < 4; ++e)
            if (off + e < row_valid) p[e] = (uint8_t)(v >> (8 * e));
    }
}

struct Pass {
    const uint8_t *src;                               // row 0 of image 0 of what this pass reads
    int64_t src_row_pitch, src_image_pitch;
    uint8_t *dst;
    int64_t dst_row_pitch, dst_image_pitch, dst_row_cap;   // dst_row_cap: bytes of a destination row that may be written
    const int32_t *bounds, *coef;                     // the pass's axis: [2 * out], [out * ksize]
    int32_t in, out, ksize;                           // the pass's axis
    int32_t rows;                                     // horizontal: rows to resample; vertical: source rows present
    int32_t other;                                    // horizontal: unused; vertical: bytes of a row (W * 3)
    int32_t shift;                                    // vertical: source row 0 is row `shift` of the table's numbering
    int32_t cap, lds_pitch;                           // LDS window: samples (rows) at most, bytes per staged row
};

// LDS: window [16 rows][lds_pitch] | coefficients [64][ksize] | bounds [64][2]
__global__ void __launch_bounds__(kThreads) horizontal_kernel(Pass p) {
    extern __shared__ uint32_t lds[];
    uint32_t *win = lds;
    int32_t *coef = (int32_t *)(win + kTileRows * (p.lds_pitch >> 2));
    int32_t *bnd = coef + kTileCols * p.ksize;
    const int c0 = blockIdx.x * kTileCols, r0 = blockIdx.y * kTileRows;
    const int ncols = min(kTileCols, p.out - c0), nrows = min(kTileRows, p.rows - r0);
    const int64_t k = blockIdx.z;
    const int win0 = clampi(p.bounds[2 * c0], 0, p.in);
    const int wend = clampi(p.bounds[2 * (c0 + ncols - 1)] + p.bounds[2 * (c0 + ncols - 1) + 1], win0, p.in);
    const int nwin = min(wend - win0, p.cap);
    for (int i = threadIdx.x; i < ncols * p.ksize; i += kThreads) coef[i] = p.coef[(int64_t)c0 * p.ksize + i];
    for (int i = threadIdx.x; i < ncols; i += kThreads) {
        const int xmin = clampi(p.bounds[2 * (c0 + i)], win0, win0 + nwin);
        bnd[2 * i] = xmin - win0;
        bnd[2 * i + 1] = clampi(p.bounds[2 * (c0 + i) + 1], 0, min(p.ksize, win0 + nwin - xmin));
    }
    const uint8_t *base = p.src + k * p.src_image_pitch + (int64_t)r0 * p.src_row_pitch;
    stage_rows(base, p.src_row_pitch, nrows, (int64_t)win0 * 3, nwin * 3, (int64_t)p.in * 3, win, p.lds_pitch);
    __syncthreads();
    const int cg = threadIdx.x & 15, rr = threadIdx.x >> 4;
    if (rr >= nrows || cg * 4 >= ncols) return;
    const int skew = (int)((uintptr_t)(base + (int64_t)rr * p.src_row_pitch + (int64_t)win0 * 3) & 3);
    const uint8_t *row = (const uint8_t *)win + rr * p.lds_pitch + skew;
    uint8_t px[12];
    MSPA_UNROLL
    for (int q = 0; q < 4; ++q) {
        const int c = min(cg * 4 + q, ncols - 1);          // a column past the tile repeats the last one; its bytes are not kept
        const int xmin = bnd[2 * c], xmax = bnd[2 * c + 1];
        const int32_t *kk = coef + c * p.ksize;
        const uint8_t *s = row + xmin * 3;
        int32_t a0 = kHalf, a1 = kHalf, a2 = kHalf;
        for (int j = 0; j < xmax; ++j) {
            const int32_t w = kk[j];
            a0 += s[3 * j] * w;
            a1 += s[3 * j + 1] * w;
            a2 += s[3 * j + 2] * w;
        }
        px[3 * q] = clip8(a0);
        px[3 * q + 1] = clip8(a1);
        px[3 * q + 2] = clip8(a2);
    }
    const int64_t off = (int64_t)(c0 + cg * 4) * 3;
    uint8_t *o = p.dst + k * p.dst_image_pitch + (int64_t)(r0 + rr) * p.dst_row_pitch + off;
    const int64_t valid = (int64_t)p.out * 3;
    MSPA_UNROLL
    for (int d = 0; d < 3; ++d)
        store4(o + 4 * d, off + 4 * d, p.dst_row_cap, valid,
               px[4 * d] | ((uint32_t)px[4 * d + 1] << 8) | ((uint32_t)px[4 * d + 2] << 16) | ((uint32_t)px[4 * d + 3] << 24));
}

// LDS: window [cap rows][lds_pitch = 260] | coefficients [16][ksize] | bounds [16][2]
// kAligned: every staged row starts on a dword (source base and pitches are multiples of 4), so no row has a skew.
template <bool kAligned>
__global__ void __launch_bounds__(kThreads) vertical_kernel(Pass p) {
    extern __shared__ uint32_t lds[];
    uint32_t *win = lds;
    int32_t *coef = (int32_t *)(win + p.cap * (p.lds_pitch >> 2));
    int32_t *bnd = coef + kTileRows * p.ksize;
    const int64_t b0 = (int64_t)blockIdx.x * kTileBytes;
    const int y0 = blockIdx.y * kTileRows;
    const int nbytes = (int)min((int64_t)kTileBytes, p.other - b0), nout = min(kTileRows, p.out - y0);
    const int64_t k = blockIdx.z;
    const int win0 = clampi(p.bounds[2 * y0] - p.shift, 0, p.rows);
    const int wend = clampi(p.bounds[2 * (y0 + nout - 1)] - p.shift + p.bounds[2 * (y0 + nout - 1) + 1], win0, p.rows);
    const int nwin = min(wend - win0, p.cap);
    for (int i = threadIdx.x; i < nout * p.ksize; i += kThreads) coef[i] = p.coef[(int64_t)y0 * p.ksize + i];
    for (int i = threadIdx.x; i < nout; i += kThreads) {
        const int ymin = clampi(p.bounds[2 * (y0 + i)] - p.shift, win0, win0 + nwin);
        bnd[2 * i] = ymin - win0;
        bnd[2 * i + 1] = clampi(p.bounds[2 * (y0 + i) + 1], 0, min(p.ksize, win0 + nwin - ymin));
    }
    const uint8_t *base = p.src + k * p.src_image_pitch + (int64_t)win0 * p.src_row_pitch;
    stage_rows(base, p.src_row_pitch, nwin, b0, nbytes, p.other, win, p.lds_pitch);
    __syncthreads();
    const int col = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (col * 4 >= nbytes) return;
    const int ndw = p.lds_pitch >> 2;
    // a staged row's skew: (address of its first byte) & 3, which moves with the row when the pitch is not a multiple of 4
    const uint32_t skew0 = (uint32_t)((uintptr_t)(base + b0) & 3), skew_step = (uint32_t)(p.src_row_pitch & 3);
    for (int yy = wave; yy < nout; yy += kThreads / 64) {
        const int ymin = bnd[2 * yy], ymax = bnd[2 * yy + 1];
        const int32_t *kk = coef + yy * p.ksize;
        int32_t a0 = kHalf, a1 = kHalf, a2 = kHalf, a3 = kHalf;
        for (int j = 0; j < ymax; ++j) {
            const uint32_t *s = win + (ymin + j) * ndw + col;
            uint32_t v = s[0];
            if (!kAligned) v = __builtin_amdgcn_alignbyte(s[1], v, (skew0 + (uint32_t)(ymin + j) * skew_step) & 3);
            const int32_t w = kk[j];
            a0 += (int32_t)(v & 255) * w;
            a1 += (int32_t)((v >> 8) & 255) * w;
            a2 += (int32_t)((v >> 16) & 255) * w;
            a3 += (int32_t)(v >> 24) * w;
        }
        const int64_t off = b0 + col * 4;
        uint8_t *o = p.dst + k * p.dst_image_pitch + (int64_t)(y0 + yy) * p.dst_row_pitch + off;
        store4(o, off, p.dst_row_cap, p.other,
               clip8(a0) | ((uint32_t)clip8(a1) << 8) | ((uint32_t)clip8(a2) << 16) | ((uint32_t)clip8(a3) << 24));
    }
}

MSPA_HD int64_t tmp_pitch(int32_t W) { return ((int64_t)W * 3 + 15) / 16 * 16; }

static int64_t horizontal_lds(const Axis &ax, int32_t &cap, int32_t &pitch) {
    cap = window_cap(ax, kTileCols);
    pitch = (cap * 3 + 3 + 3) / 4 * 4;
    return (int64_t)kTileRows * pitch + (int64_t)kTileCols * ax.ksize * 4 + kTileCols * 8;
}

static int64_t vertical_lds(const Axis &ay, int32_t &cap, int32_t &pitch) {
    cap = window_cap(ay, kTileRows);
    pitch = kTileBytes + 4;
    return (int64_t)cap * pitch + (int64_t)kTileRows * ay.ksize * 4 + kTileRows * 8;
}

}  // namespace resize
}  // namespace mspa

using namespace mspa;

extern "C" int mspa_resize_coeffs_host(int32_t in, int32_t out, int32_t filter, int32_t *bounds, int32_t *coeffs, int32_t *ksize) {
    if (in < 1 || out < 1 || in > 65535 || out > 65535) return fail(MSPA_EINVAL, "mspa_resize_coeffs_host: sizes must be in 1..65535");
    if (!resize::valid_filter(filter)) return fail(MSPA_EINVAL, "mspa_resize_coeffs_host: filter must be 2 (bilinear) or 3 (bicubic)");
    if (!ksize) return fail(MSPA_EINVAL, "mspa_resize_coeffs_host: null pointer");
    const resize::Axis a = resize::axis(in, out, filter);
    *ksize = a.ksize;
    if (!bounds && !coeffs) return MSPA_OK;                // a sizing call
    if (!bounds) return fail(MSPA_EINVAL, "mspa_resize_coeffs_host: null pointer");
    std::vector<double> w((size_t)a.ksize);
    std::vector<int32_t> krow((size_t)a.ksize);
    if (resize::coeffs(a, bounds, coeffs, w.data(), krow.data()) < 0)
        return fail(MSPA_EUNSUPPORTED, "mspa_resize_coeffs_host: a coefficient row exceeds the 32-bit accumulator's bound");
    return MSPA_OK;
}

extern "C" int64_t mspa_resize_workspace_bytes(int64_t n_images, int32_t h, int32_t w, int32_t H, int32_t W) {
    if (n_images < 0 || h < 1 || w < 1 || H < 1 || W < 1 || h > 65535 || w > 65535 || H > 65535 || W > 65535) return -1;
    if (h == H || w == W) return 0;                        // one pass at most: no intermediate
    return n_images * (int64_t)h * resize::tmp_pitch(W);   // every source row: an upper bound of the rows the vertical pass reads
}

extern "C" int mspa_resize_rgb_device(const uint8_t *src_dev, int64_t n_images, int32_t h, int32_t w, int64_t src_row_pitch,
                                      int64_t src_image_pitch, uint8_t *dst_dev, int32_t H, int32_t W, int32_t filter,
                                      const int32_t *bounds_x_dev, const int32_t *coeffs_x_dev, const int32_t *bounds_y_dev,
                                      const int32_t *coeffs_y_dev, void *workspace, int64_t workspace_bytes, void *stream) {
    if (n_images < 0 || h < 1 || w < 1 || H < 1 || W < 1 || h > 65535 || w > 65535 || H > 65535 || W > 65535)
        return fail(MSPA_EINVAL, "mspa_resize_rgb_device: sizes must be in 1..65535");
    if (!resize::valid_filter(filter)) return fail(MSPA_EINVAL, "mspa_resize_rgb_device: filter must be 2 (bilinear) or 3 (bicubic)");
    if (n_images == 0) return MSPA_OK;
    if (n_images > 65535) return fail(MSPA_EINVAL, "mspa_resize_rgb_device: more than 65 535 images in one call");
    if (!src_dev || !dst_dev) return fail(MSPA_EINVAL, "mspa_resize_rgb_device: null pointer");
    if (src_row_pitch < (int64_t)w * 3 || src_image_pitch < (int64_t)(h - 1) * src_row_pitch + (int64_t)w * 3)
        return fail(MSPA_EINVAL, "mspa_resize_rgb_device: pitch smaller than a row / an image");
    if (!resize::in_range(h, H) || !resize::in_range(w, W))
        return fail(MSPA_EUNSUPPORTED, "mspa_resize_rgb_device: a per-axis factor outside 1/8 .. 8");
    const bool need_h = w != W, need_v = h != H;
    if ((need_h && (!bounds_x_dev || !coeffs_x_dev)) || (need_v && (!bounds_y_dev || !coeffs_y_dev)))
        return fail(MSPA_EINVAL, "mspa_resize_rgb_device: null table of a pass that runs");
    const int64_t ws_need = mspa_resize_workspace_bytes(n_images, h, w, H, W);
    if (ws_need > 0 && (!workspace || workspace_bytes < ws_need))
        return fail(MSPA_EINVAL, "mspa_resize_rgb_device: workspace smaller than mspa_resize_workspace_bytes()");
    if (ws_need > 0 && ((uintptr_t)workspace & 15u)) return fail(MSPA_EINVAL, "mspa_resize_rgb_device: workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const unsigned nz = (unsigned)n_images;
    const int64_t dst_row = (int64_t)W * 3, dst_image = (int64_t)H * dst_row;
    if (!need_h && !need_v) {                              // Pillow returns a copy
        const bool dense = src_image_pitch == (int64_t)h * src_row_pitch;
        for (int64_t k = 0; k < (dense ? 1 : n_images); ++k) {
            const hipError_t e = hipMemcpy2DAsync(dst_dev + k * dst_image, (size_t)dst_row, src_dev + k * src_image_pitch, (size_t)src_row_pitch,
                                                  (size_t)dst_row, (size_t)h * (size_t)(dense ? n_images : 1), hipMemcpyDeviceToDevice, st);
            if (e != hipSuccess) return check_hip(e, "mspa_resize_rgb_device: copy");
        }
        return MSPA_OK;
    }
    const resize::Axis ax = resize::axis(w, W, filter), ay = resize::axis(h, H, filter);
    int32_t first = 0, rows = h;
    if (need_v) resize::rows_read(ay, first, rows);
    if (first < 0 || rows < 1 || first + rows > h) return fail(MSPA_EINVAL, "mspa_resize_rgb_device: internal: vertical window outside the source");
    const int64_t tpitch = resize::tmp_pitch(W);
    if (need_h) {
        resize::Pass p{};
        p.src = src_dev + (need_v ? (int64_t)first * src_row_pitch : 0);
        p.src_row_pitch = src_row_pitch;
        p.src_image_pitch = src_image_pitch;
        p.dst = need_v ? (uint8_t *)workspace : dst_dev;
        p.dst_row_pitch = need_v ? tpitch : dst_row;
        p.dst_image_pitch = need_v ? (int64_t)rows * tpitch : dst_image;
        p.dst_row_cap = p.dst_row_pitch;
        p.bounds = bounds_x_dev;
        p.coef = coeffs_x_dev;
        p.in = w;
        p.out = W;
        p.ksize = ax.ksize;
        p.rows = need_v ? rows : h;
        const int64_t lds = resize::horizontal_lds(ax, p.cap, p.lds_pitch);
        if (lds > 65536) return fail(MSPA_EUNSUPPORTED, "mspa_resize_rgb_device: horizontal window exceeds LDS");
        hipLaunchKernelGGL(resize::horizontal_kernel, dim3((unsigned)((W + resize::kTileCols - 1) / resize::kTileCols),
                                                           (unsigned)((p.rows + resize::kTileRows - 1) / resize::kTileRows), nz),
                           dim3(resize::kThreads), (size_t)lds, st, p);
    }
    if (need_v) {
        resize::Pass p{};
        p.src = need_h ? (const uint8_t *)workspace : src_dev + (int64_t)first * src_row_pitch;
        p.src_row_pitch = need_h ? tpitch : src_row_pitch;
        p.src_image_pitch = need_h ? (int64_t)rows * tpitch : src_image_pitch;
        p.dst = dst_dev;
        p.dst_row_pitch = dst_row;
        p.dst_image_pitch = dst_image;
        p.dst_row_cap = dst_row;
        p.bounds = bounds_y_dev;
        p.coef = coeffs_y_dev;
        p.in = h;
        p.out = H;
        p.ksize = ay.ksize;
        p.rows = rows;
        p.other = (int32_t)dst_row;
        p.shift = first;
        const int64_t lds = resize::vertical_lds(ay, p.cap, p.lds_pitch);
        if (lds > 65536) return fail(MSPA_EUNSUPPORTED, "mspa_resize_rgb_device: vertical window exceeds LDS");
        const dim3 grid((unsigned)((dst_row + resize::kTileBytes - 1) / resize::kTileBytes),
                        (unsigned)((H + resize::kTileRows - 1) / resize::kTileRows), nz);
        if ((((uintptr_t)p.src | (uintptr_t)p.src_row_pitch | (uintptr_t)p.src_image_pitch) & 3) == 0)
            hipLaunchKernelGGL(resize::vertical_kernel<true>, grid, dim3(resize::kThreads), (size_t)lds, st, p);
        else
            hipLaunchKernelGGL(resize::vertical_kernel<false>, grid, dim3(resize::kThreads), (size_t)lds, st, p);
    }
    return check_hip(hipGetLastError(), "mspa_resize_rgb_device");
}
