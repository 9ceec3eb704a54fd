// The PNG row filters (PNG 9.2) for 8-bit greyscale images: bytes per pixel = 1, so the left neighbour a, the upper neighbour b
// and the upper-left neighbour c of a byte are the bytes one column / one row / both away (0 outside the image).  ONE statement of
// the rule for the device kernel (csrc/mask_ingest.hip), the host entry point behind the CPU tests and the host fallback.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MSPA_PNG8_HD __host__ __device__ __forceinline__
#else
#define MSPA_PNG8_HD inline
#endif

namespace mspa {
namespace png8 {

// Paeth's predictor: the neighbour closest to a + b - c, ties in the order a, b, c
MSPA_PNG8_HD int paeth(int a, int b, int c) {
    const int t = b - c, u = a - c;                               // p - a, p - b for p = a + b - c
    const int pa = t < 0 ? -t : t, pb = u < 0 ? -u : u, pc = t + u < 0 ? -(t + u) : t + u;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// the reconstructed byte: raw + predictor(filter type 0 .. 4), modulo 256
MSPA_PNG8_HD int unfilter_byte(int ft, int raw, int a, int b, int c) {
    const int pred = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : paeth(a, b, c);
    return (raw + pred) & 0xFF;
}

// One image on the host: raw = h rows of 1 filter byte + w sample bytes -> out[h * w].  0 done; 3 a filter byte > 4 (then out
// is not written at all: the check runs over every row first, as the kernel's does).
inline int unfilter_image(const uint8_t *raw, int32_t h, int32_t w, uint8_t *out) {
    const int64_t stride = (int64_t)w + 1;
    for (int32_t y = 0; y < h; ++y)
        if (raw[(int64_t)y * stride] > 4) return 3;
    for (int32_t y = 0; y < h; ++y) {
        const uint8_t *row = raw + (int64_t)y * stride + 1;
        const int ft = row[-1];
        uint8_t *cur = out + (int64_t)y * w;
        const uint8_t *up = y > 0 ? cur - w : nullptr;
        int a = 0, c = 0;
        for (int32_t x = 0; x < w; ++x) {
            const int b = up ? up[x] : 0;
            a = unfilter_byte(ft, row[x], a, b, c);
            cur[x] = (uint8_t)a;
            c = b;
        }
    }
    return 0;
}

}  // namespace png8
}  // namespace mspa
