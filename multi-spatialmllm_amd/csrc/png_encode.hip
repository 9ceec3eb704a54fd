// Depth-PNG writes ON the MI355X: 16-bit greyscale PNG files of n frames of one shape.  The arithmetic is
// csrc/png_encode_core.h (whose host build is the reference this file equals byte for byte); this file holds the kernels and
// the C ABI.  Nine kernels over n frames:
//   1. filter_kernel -- one thread per row: Pillow's filter choice, then the filtered row into the stream workspace.
//   2. match_kernel  -- one wave per (frame, segment): walks the 32 KiB before the segment and the segment itself in chunks of
//      64 positions, with the hash heads in LDS (atomicMax per bucket, so the largest position wins whatever the order); writes
//      every position's chain link.
//   3. parse_kernel  -- one thread per segment: the lazy parse over the chain links into tokens.
//   4. hist_kernel   -- one workgroup per segment: symbol histograms (LDS atomics) and the Adler-32 partial sums.
//   5. huff_kernel   -- one thread per segment: Huffman code lengths and codes, block type and bit length.
//   6. scan_kernel   -- one thread per frame: block bit offsets in segment order, the Adler-32, the file length.
//   7. write_kernel  -- one thread per segment: the block at its bit offset into a zeroed buffer; whole 32-bit words are
//      stored, the (shared) first and last word of a block are OR-ed in atomically.
//   8. crc_kernel    -- one thread per IDAT chunk: its CRC-32 (table in LDS).
//   9. copy_kernel   -- one thread per 4 output bytes: signature, IHDR, chunk framing, zlib bytes, IEND as dword stores.
#include "mspa_common.h"
#include "png_encode_core.h"

namespace mspa {
namespace pnge {

constexpr int64_t kMaxImages = 65535;

MSPA_HD int64_t round16(int64_t v) { return (v + 15) / 16 * 16; }

struct Layout {
    int64_t spitch, ppitch, tpitch, bpitch, dpitch, cpitch;   // per-frame bytes of each area
    int64_t stream, prev, tok, blk, dbuf, crc, info, end;    // byte offsets in the workspace
};

MSPA_HD Layout layout(int64_t n, const Geom &g) {
    Layout l;
    l.spitch = round16(g.n);
    l.ppitch = round16(2 * g.n);
    l.tpitch = round16(4 * g.n);
    l.bpitch = round16(g.nseg * (int64_t)sizeof(Block));
    l.dpitch = round16(g.dcap + 8);
    l.cpitch = round16(4 * g.nchunk);
    l.stream = 0;
    l.prev = l.stream + n * l.spitch;
    l.tok = l.prev + n * l.ppitch;
    l.blk = l.tok + n * l.tpitch;
    l.dbuf = l.blk + n * l.bpitch;
    l.crc = l.dbuf + n * l.dpitch;
    l.info = l.crc + n * l.cpitch;
    l.end = l.info + round16(n * (int64_t)sizeof(FileInfo));
    return l;
}

MSPA_HD int64_t seg_len(const Geom &g, int64_t sg) { return sg * kSeg + kSeg < g.n ? kSeg : g.n - sg * kSeg; }

__global__ void filter_kernel(const int16_t *__restrict__ depth, int64_t n, Geom g, uint8_t *__restrict__ stream, int64_t spitch) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * g.h) return;
    const int64_t k = idx / g.h, y = idx % g.h;
    const int16_t *img = depth + k * g.h * (int64_t)g.w;
    filter_row(img + y * g.w, y ? img + (y - 1) * g.w : nullptr, g.w, stream + k * spitch + y * g.row);
}

__global__ void __launch_bounds__(kChunk) match_kernel(Geom g, const uint8_t *__restrict__ stream, int64_t spitch, uint16_t *prev,
                                                       int64_t ppitch) {
    __shared__ int32_t head[1 << kHashBits];
    const int64_t k = blockIdx.y, sg = blockIdx.x;
    const uint8_t *s = stream + k * spitch;
    uint16_t *pv = (uint16_t *)((uint8_t *)prev + k * ppitch);
    for (int i = threadIdx.x; i < (1 << kHashBits); i += kChunk) head[i] = -1;
    __syncthreads();
    const int64_t s0 = sg * kSeg, s1 = s0 + seg_len(g, sg);
    for (int64_t c0 = s0 > kWindow ? s0 - kWindow : 0; c0 < s1; c0 += kChunk) {
        const int64_t p = c0 + threadIdx.x;
        const bool has = p + 4 <= g.n;
        const uint32_t hv = has ? hash4(s, p) : 0u;
        if (p >= s0 && p < s1) pv[p] = has ? chain_link(p, head[hv]) : (uint16_t)0;
        __syncthreads();
        if (has) atomicMax(&head[hv], (int32_t)p);
        __syncthreads();
    }
}

__global__ void parse_kernel(int64_t n, Geom g, const uint8_t *__restrict__ stream, int64_t spitch, const uint16_t *__restrict__ prev,
                             int64_t ppitch, uint32_t *__restrict__ tok, int64_t tpitch, Block *blk, int64_t bpitch) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * g.nseg) return;
    const int64_t k = idx / g.nseg, sg = idx % g.nseg, s0 = sg * kSeg;
    Block *b = (Block *)((uint8_t *)blk + k * bpitch) + sg;
    b->ntok = parse_segment(stream + k * spitch, (const uint16_t *)((const uint8_t *)prev + k * ppitch), s0, s0 + seg_len(g, sg),
                            g.row, (uint32_t *)((uint8_t *)tok + k * tpitch) + s0);
}

__global__ void __launch_bounds__(256) hist_kernel(Geom g, const uint8_t *__restrict__ stream, int64_t spitch,
                                                   const uint32_t *__restrict__ tok, int64_t tpitch, Block *blk, int64_t bpitch) {
    __shared__ uint32_t hist[kLitSyms + kDistSyms];
    __shared__ uint64_t sa[256], sb[256];
    const int64_t k = blockIdx.y, sg = blockIdx.x, s0 = sg * kSeg, L = seg_len(g, sg);
    Block *b = (Block *)((uint8_t *)blk + k * bpitch) + sg;
    const uint32_t *t = (const uint32_t *)((const uint8_t *)tok + k * tpitch) + s0;
    const uint8_t *x = stream + k * spitch + s0;
    for (int i = threadIdx.x; i < kLitSyms + kDistSyms; i += 256) hist[i] = 0;
    __syncthreads();
    const uint32_t ntok = b->ntok;
    for (uint32_t i = threadIdx.x; i < ntok; i += 256) {
        const uint32_t v = t[i];
        if (v & 0x80000000u) {
            atomicAdd(&hist[257 + len_code((int)((v >> 16) & 255) + 3)], 1u);
            atomicAdd(&hist[kLitSyms + dist_code((int)(v & 0x7FFF) + 1)], 1u);
        } else {
            atomicAdd(&hist[v], 1u);
        }
    }
    uint64_t a = 0, bb = 0;
    for (int64_t i = threadIdx.x; i < L; i += 256) {
        a += x[i];
        bb += (uint64_t)(L - i) * x[i];
    }
    sa[threadIdx.x] = a;
    sb[threadIdx.x] = bb;
    __syncthreads();
    for (int i = threadIdx.x; i < kLitSyms; i += 256) b->freq[i] = i == 256 ? 1u : hist[i];
    for (int i = threadIdx.x; i < kDistSyms; i += 256) b->dfreq[i] = hist[kLitSyms + i];
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            sa[threadIdx.x] += sa[threadIdx.x + w];
            sb[threadIdx.x] += sb[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        b->adler_a = (uint32_t)(sa[0] % kAdlerMod);
        b->adler_b = (uint32_t)(sb[0] % kAdlerMod);
    }
}

__global__ void huff_kernel(int64_t n, Geom g, Block *blk, int64_t bpitch) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * g.nseg) return;
    const int64_t k = idx / g.nseg, sg = idx % g.nseg;
    plan_block(((Block *)((uint8_t *)blk + k * bpitch))[sg], seg_len(g, sg));
}

__global__ void scan_kernel(int64_t n, Geom g, Block *blk, int64_t bpitch, uint32_t ihdr, FileInfo *info, int64_t *nbytes) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    Block *b = (Block *)((uint8_t *)blk + k * bpitch);
    int64_t off = 0;
    for (int64_t sg = 0; sg < g.nseg; ++sg) {
        b[sg].off = off;
        off += block_bits_at(b[sg], off, seg_len(g, sg));
    }
    const FileInfo f = file_info(off, adler_combine(b, g.nseg, g.n), ihdr);
    info[k] = f;
    nbytes[k] = f.flen;
}

struct WordWriter {
    uint32_t *words;
    int64_t widx;
    uint64_t acc;
    int nacc;
    bool first;
    __device__ void store() {
        if (first) atomicOr(words + widx, (uint32_t)acc);
        else words[widx] = (uint32_t)acc;
        first = false;
        ++widx;
        acc >>= 32;
        nacc -= 32;
    }
    __device__ void put(uint32_t bits, int nb) {
        acc |= (uint64_t)bits << nacc;
        nacc += nb;
        if (nacc >= 32) store();
    }
    __device__ void align() {
        nacc = (nacc + 7) & ~7;
        if (nacc >= 32) store();
    }
    __device__ void finish() {
        if (nacc > 0) atomicOr(words + widx, (uint32_t)acc);
    }
};

__global__ void write_kernel(int64_t n, Geom g, const uint8_t *__restrict__ stream, int64_t spitch, const uint32_t *__restrict__ tok,
                             int64_t tpitch, const Block *__restrict__ blk, int64_t bpitch, uint8_t *dbuf, int64_t dpitch) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * g.nseg) return;
    const int64_t k = idx / g.nseg, sg = idx % g.nseg, s0 = sg * kSeg;
    const Block &b = ((const Block *)((const uint8_t *)blk + k * bpitch))[sg];
    WordWriter wr{(uint32_t *)(dbuf + k * dpitch), b.off >> 5, 0, (int)(b.off & 31), true};
    emit_block(b, (const uint32_t *)((const uint8_t *)tok + k * tpitch) + s0, stream + k * spitch + s0, seg_len(g, sg),
               sg + 1 == g.nseg, wr);
    wr.finish();
}

__global__ void __launch_bounds__(256) crc_kernel(int64_t max_chunks, const uint8_t *__restrict__ dbuf, int64_t dpitch,
                                                  const FileInfo *__restrict__ info, uint32_t *crcs, int64_t cpitch) {
    __shared__ uint32_t tab[256];
    tab[threadIdx.x] = crc_entry(threadIdx.x);
    __syncthreads();
    const int64_t k = blockIdx.y, j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const FileInfo f = info[k];
    if (j >= max_chunks || j >= f.nchunk) return;
    ((uint32_t *)((uint8_t *)crcs + k * cpitch))[j] = chunk_crc(tab, f, dbuf + k * dpitch, j);
}

__global__ void __launch_bounds__(256) copy_kernel(Geom g, const uint8_t *__restrict__ dbuf, int64_t dpitch,
                                                   const FileInfo *__restrict__ info, const uint32_t *__restrict__ crcs,
                                                   int64_t cpitch, uint8_t *out, int64_t out_pitch) {
    const int64_t k = blockIdx.y, i = 4 * ((int64_t)blockIdx.x * 256 + threadIdx.x);
    const FileInfo f = info[k];
    if (i >= f.flen) return;
    const uint8_t *d = dbuf + k * dpitch;
    const uint32_t *c = (const uint32_t *)((const uint8_t *)crcs + k * cpitch);
    uint32_t v = 0;
    for (int b = 0; b < 4; ++b)
        if (i + b < f.flen) v |= file_byte(g.h, g.w, f, d, c, i + b) << (8 * b);
    *(uint32_t *)(out + k * out_pitch + i) = v;
}

}  // namespace pnge
}  // namespace mspa

using namespace mspa;

extern "C" int64_t mspa_png_encode_capacity(int32_t h, int32_t w) {
    if (!pnge::valid_size(h, w)) return -1;
    return pnge::geom(h, w).cap;
}

extern "C" int64_t mspa_png_encode_workspace_bytes(int64_t n, int32_t h, int32_t w) {
    if (n < 0 || n > pnge::kMaxImages || !pnge::valid_size(h, w)) return -1;
    return pnge::layout(n, pnge::geom(h, w)).end;
}

extern "C" int mspa_png_encode_device(const int16_t *depth_dev, int64_t n, int32_t h, int32_t w, uint8_t *out_dev, int64_t out_pitch,
                                      int64_t *nbytes_dev, void *workspace, int64_t workspace_bytes, void *stream) {
    if (n < 0 || n > pnge::kMaxImages || !pnge::valid_size(h, w))
        return fail(MSPA_EINVAL, "mspa_png_encode_device: bad size (1 <= h, w <= 8192, 0 <= n <= 65535)");
    if (n == 0) return MSPA_OK;
    if (!depth_dev || !out_dev || !nbytes_dev || !workspace) return fail(MSPA_EINVAL, "mspa_png_encode_device: null pointer");
    if ((uintptr_t)depth_dev & 1u) return fail(MSPA_EINVAL, "mspa_png_encode_device: depth_dev must be 2-byte aligned");
    if ((uintptr_t)out_dev & 3u) return fail(MSPA_EINVAL, "mspa_png_encode_device: out_dev must be 4-byte aligned");
    if ((uintptr_t)nbytes_dev & 7u) return fail(MSPA_EINVAL, "mspa_png_encode_device: nbytes_dev must be 8-byte aligned");
    if ((uintptr_t)workspace & 15u) return fail(MSPA_EINVAL, "mspa_png_encode_device: workspace must be 16-byte aligned");
    const pnge::Geom g = pnge::geom(h, w);
    if (out_pitch < g.cap || (out_pitch & 3))
        return fail(MSPA_EINVAL, "mspa_png_encode_device: out_pitch must be a multiple of 4 and at least mspa_png_encode_capacity()");
    const pnge::Layout l = pnge::layout(n, g);
    if (workspace_bytes < l.end)
        return fail(MSPA_EINVAL, "mspa_png_encode_device: workspace smaller than mspa_png_encode_workspace_bytes()");
    hipStream_t st = (hipStream_t)stream;
    uint8_t *ws = (uint8_t *)workspace;
    uint8_t *s = ws + l.stream, *dbuf = ws + l.dbuf;
    auto *prev = (uint16_t *)(ws + l.prev);
    auto *tok = (uint32_t *)(ws + l.tok);
    auto *blk = (pnge::Block *)(ws + l.blk);
    auto *crcs = (uint32_t *)(ws + l.crc);
    auto *info = (pnge::FileInfo *)(ws + l.info);
    uint32_t tab[256];
    for (uint32_t k = 0; k < 256; ++k) tab[k] = pnge::crc_entry(k);
    const uint32_t ihdr = pnge::ihdr_crc(tab, h, w);
    hipError_t e = hipMemsetAsync(dbuf, 0, (size_t)(n * l.dpitch), st);
    if (e != hipSuccess) return check_hip(e, "mspa_png_encode_device: memset");
    const int64_t rows = n * h, segs = n * g.nseg;
    const unsigned ny = (unsigned)n;
    hipLaunchKernelGGL(pnge::filter_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, depth_dev, n, g, s, l.spitch);
    hipLaunchKernelGGL(pnge::match_kernel, dim3((unsigned)g.nseg, ny), dim3(pnge::kChunk), 0, st, g, (const uint8_t *)s, l.spitch,
                       prev, l.ppitch);
    hipLaunchKernelGGL(pnge::parse_kernel, dim3((unsigned)((segs + 63) / 64)), dim3(64), 0, st, n, g, (const uint8_t *)s, l.spitch,
                       (const uint16_t *)prev, l.ppitch, tok, l.tpitch, blk, l.bpitch);
    hipLaunchKernelGGL(pnge::hist_kernel, dim3((unsigned)g.nseg, ny), dim3(256), 0, st, g, (const uint8_t *)s, l.spitch,
                       (const uint32_t *)tok, l.tpitch, blk, l.bpitch);
    hipLaunchKernelGGL(pnge::huff_kernel, dim3((unsigned)((segs + 63) / 64)), dim3(64), 0, st, n, g, blk, l.bpitch);
    hipLaunchKernelGGL(pnge::scan_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, n, g, blk, l.bpitch, ihdr, info, nbytes_dev);
    hipLaunchKernelGGL(pnge::write_kernel, dim3((unsigned)((segs + 63) / 64)), dim3(64), 0, st, n, g, (const uint8_t *)s, l.spitch,
                       (const uint32_t *)tok, l.tpitch, (const pnge::Block *)blk, l.bpitch, dbuf, l.dpitch);
    hipLaunchKernelGGL(pnge::crc_kernel, dim3((unsigned)((g.nchunk + 255) / 256), ny), dim3(256), 0, st, g.nchunk,
                       (const uint8_t *)dbuf, l.dpitch, (const pnge::FileInfo *)info, crcs, l.cpitch);
    const int64_t words = (g.cap + 3) / 4;
    hipLaunchKernelGGL(pnge::copy_kernel, dim3((unsigned)((words + 255) / 256), ny), dim3(256), 0, st, g, (const uint8_t *)dbuf,
                       l.dpitch, (const pnge::FileInfo *)info, (const uint32_t *)crcs, l.cpitch, out_dev, out_pitch);
    return check_hip(hipGetLastError(), "mspa_png_encode_device");
}
