// Instance-mask decode ON the MI355X: ScanNet's `instance-filt/<image>.png` files are 8-bit greyscale PNGs, one label per pixel.
// The reference reads one per (image, object) with `cv2.imread(path, -1)` (info_handler.py get_instance_mask); here the host packs
// the files' scanline zlib streams (mspa_png_pack_idat8_host, the 8-bit twin of mspa_png_pack_idat_host), the existing inflate
// kernel (mspa_inflate_blocks_device, block_bytes = h * (w + 1)) inflates them, and this file undoes the row filters with
// bytes-per-pixel 1 -- the rule of csrc/png_unfilter8_core.h -- into the [n, h, w] uint8 label block the instance split reads.
//
// mspa::mask::png_unfilter8_kernel -- one wave per image, the byte-wise band pipeline of png_unfilter_hard_kernel with one byte
// per pixel: 64 rows per band, lane l works on row y0 + l and is one column behind lane l - 1 (at step t it is at column t - l),
// so its upper neighbour is the byte the lane above produced one step earlier (a DPP wave shift), its upper-left neighbour
// the one it received the step before, its left neighbour its own last output.  Lane 0's upper neighbour is the last row of the
// previous band, written by this wave: it is re-read after a workgroup-scope fence, kUpChunk bytes at a time into LDS, so the
// step itself never waits for memory on lane 0's behalf.  A row's raw bytes arrive as aligned dwords, each requested one dword
// (four steps) ahead.  Any mix of the five filters, any width and height: the kernel declines nothing that is well formed.
#include "mspa_common.h"
#include "png_unfilter8_core.h"

namespace mspa {
namespace mask {

constexpr int kUpChunk = 1024;                                   // bytes of the row above the band held in LDS at a time

__global__ __launch_bounds__(64) void png_unfilter8_kernel(const uint8_t *__restrict__ raw_base, int64_t raw_pitch, int32_t h, int32_t w,
                                                           uint8_t *__restrict__ out_base, int32_t *__restrict__ status) {
    __shared__ uint8_t up_row[kUpChunk];
    const int64_t k = blockIdx.x;
    if (status[k] != 0) return;
    const int lane = (int)threadIdx.x;
    const uint8_t *raw = raw_base + k * raw_pitch;
    uint8_t *out = out_base + k * (int64_t)h * w;
    const int64_t stride = (int64_t)w + 1;
    bool bad = false;
    for (int y = lane; y < h; y += 64) bad = bad || raw[(int64_t)y * stride] > 4;
    if (__any(bad)) {
        if (lane == 0) status[k] = 3;
        return;
    }
    const int64_t last = (raw_pitch - 4) & ~(int64_t)3;          // the image's last whole dword: no load past its own block
    for (int y0 = 0; y0 < h; y0 += 64) {
        const int y = y0 + lane;
        const bool row = y < h;
        const int64_t a0 = (int64_t)(row ? y : 0) * stride + 1;  // the row's first sample byte
        const int ft = row ? (int)raw[a0 - 1] : 0;
        uint8_t *op = out + (int64_t)(row ? y : 0) * w;
        const uint8_t *up = y0 > 0 ? out + (int64_t)(y0 - 1) * w : nullptr;        // the row above the band (lane 0's neighbour)
        if (y0 > 0) {                                                              // written by this wave in the previous band
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
        auto ld = [&](int64_t byte) {                            // the aligned dword that holds byte `byte` of the image's block
            int64_t o = byte & ~(int64_t)3;
            o = o < 0 ? 0 : (o < last ? o : last);
            return *(const uint32_t *)(raw + o);
        };
        // this lane's column at step t is t - lane: its stream position is a0 + t - lane; `cur` holds the dword of the current
        // position, `nxt` the one behind it (requested when `cur` was taken over)
        int64_t pos = a0 - lane;
        uint32_t cur = ld(pos), nxt = ld(pos + 4);
        int a = 0;                           // left neighbour: this lane's last output
        int x = 0;                           // this lane's most recent output (what the lane below reads as "up")
        int c = 0;                           // the upper neighbour received one step earlier: upper-left of the current column
        const int steps = w + 63;
        for (int t = 0; t < steps; ++t, ++pos) {
            if (up != nullptr && (t & (kUpChunk - 1)) == 0 && t < w) {             // (wave-uniform) the next chunk of the row above
                wave_lds_fence();
                for (int i = lane; i < kUpChunk; i += 64) up_row[i] = t + i < w ? up[t + i] : (uint8_t)0;
                wave_lds_fence();
            }
            const int col = t - lane;
            const bool on = row && col >= 0 && col < w;
            int top = 0;
            if (up != nullptr && t < w) top = up_row[t & (kUpChunk - 1)];          // (one LDS broadcast read)
            // the lane above worked on this very column one step ago: its latest output is our "up"
            int b = __builtin_amdgcn_update_dpp(0, x, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
            b = lane == 0 ? top : b;
            if ((pos & 3) == 0 && t > 0) {                       // crossed into the next dword
                cur = nxt;
                nxt = ld(pos + 4);
            }
            if (on) {
                const int r = (int)((cur >> (8 * (int)(pos & 3))) & 0xFFu);
                x = png8::unfilter_byte(ft, r, a, y > 0 ? b : 0, (y > 0 && col > 0) ? c : 0);
                a = x;
                op[col] = (uint8_t)x;
            }
            c = b;
        }
    }
}

}  // namespace mask
}  // namespace mspa

using namespace mspa;

extern "C" int mspa_png_pack_idat8_host(const char *const *paths_host, int64_t n_files, int32_t h, int32_t w, void *dst_host,
                                        int64_t dst_capacity, int64_t *offsets_host, int64_t *bytes_host, int32_t *status_host,
                                        int64_t *capacity_needed, int32_t n_threads) {
    return png_pack_idat_files("mspa_png_pack_idat8_host", 8, paths_host, n_files, h, w, dst_host, dst_capacity, offsets_host, bytes_host,
                               status_host, capacity_needed, n_threads);
}

extern "C" int mspa_png_unfilter8_device(const void *raw_dev, int64_t raw_pitch, int64_t n_images, int32_t h, int32_t w,
                                         uint8_t *out_dev, int32_t *status_dev, mspa_stream_t stream) {
    if (n_images < 0 || h <= 0 || w <= 0 || raw_pitch < (int64_t)h * ((int64_t)w + 1))
        return fail(MSPA_EINVAL, "mspa_png_unfilter8_device: bad size");
    // the rows' bytes are loaded as aligned dwords clamped to the image's last one, (raw_pitch - 4) & ~3
    if (raw_pitch & 3) return fail(MSPA_EINVAL, "mspa_png_unfilter8_device: raw_pitch must be a multiple of 4");
    if (n_images == 0) return MSPA_OK;
    if (!raw_dev || !out_dev || !status_dev) return fail(MSPA_EINVAL, "mspa_png_unfilter8_device: null pointer");
    if ((uintptr_t)raw_dev & 3u) return fail(MSPA_EINVAL, "mspa_png_unfilter8_device: raw_dev must be 4-byte aligned");
    if (n_images > 0x7fffffffll) return fail(MSPA_EINVAL, "mspa_png_unfilter8_device: too many images");
    hipLaunchKernelGGL(mask::png_unfilter8_kernel, dim3((unsigned)n_images), dim3(64), 0, (hipStream_t)stream, (const uint8_t *)raw_dev,
                       raw_pitch, h, w, out_dev, status_dev);
    return check_hip(hipGetLastError(), "mspa_png_unfilter8_device");
}

extern "C" int mspa_png_unfilter8_host(const void *raw_host, int64_t raw_pitch, int64_t n_images, int32_t h, int32_t w,
                                       uint8_t *out_host, int32_t *status_host) {
    if (n_images < 0 || h <= 0 || w <= 0 || raw_pitch < (int64_t)h * ((int64_t)w + 1))
        return fail(MSPA_EINVAL, "mspa_png_unfilter8_host: bad size");
    if (n_images == 0) return MSPA_OK;
    if (!raw_host || !out_host || !status_host) return fail(MSPA_EINVAL, "mspa_png_unfilter8_host: null pointer");
    for (int64_t k = 0; k < n_images; ++k) {
        if (status_host[k] != 0) continue;
        status_host[k] = png8::unfilter_image((const uint8_t *)raw_host + k * raw_pitch, h, w, out_host + k * (int64_t)h * w);
    }
    return MSPA_OK;
}
