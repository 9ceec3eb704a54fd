// K12: the visibility index's `values` column chunk as parquet v1 data pages (PLAIN BYTE_ARRAY, RLE definition levels, Snappy),
// written ON the MI355X from the text K10 (format_lists.hip) leaves in arrow's string layout.
//
// What it replaces: pyarrow's page assembly and Snappy compression of ~80 MB of JSON text per 320-frame scene on an encoder thread,
// and the copy of that text over PCIe.  Every output byte is defined by csrc/snappy_core.h; a g++ build of that header is the
// reference these kernels equal byte for byte (tests/test_gpu_parquet_pages.py).
//
// This file is the writer; the way back is csrc/snappy_decode.hip (streams -> bytes) and csrc/index_rows.hip (pages -> bitsets).
//
// Three passes around the caller's prefix sums (torch.cumsum: the caller's plumbing, as for K10):
//   pack      every thread writes 16 consecutive payload bytes: one binary search for the value its first byte falls into, then a
//             walk forward.  Bytes are distributed, not values -- one image_to_points value is ~300 KB of text.
//   compress  one wave per 64 KiB block of a stream.  The hash table (uint16[16384], 32 KiB) lives in LDS.  The wave hashes 64
//             positions at a time: each lane reads the table as it was before the chunk, takes the nearest earlier lane of the chunk
//             with an equal hash instead when there is one (a 64-step readlane loop: the lists repeat at distances 7 - 9, so
//             matches inside a chunk carry most of the ratio), then the last lane of every hash inserts.  The greedy parse walks
//             the chunk with ballot + ctz, extends a match 64 bytes a step, the lanes copy literal bytes and lane 0 writes tags.
//             Output goes to the block's worst-case slot, its byte count to a size array.
//   compact   block outputs -> contiguous streams behind their varint(uncompressed) preambles (two kernels: blocks, preambles).
// No load goes beyond a stream's last byte and no store beyond a slot: every index is guarded, nothing relies on padding.
#include "mspa_common.h"
#include "snappy_core.h"

namespace mspa {
namespace snappy {

__global__ __launch_bounds__(64) void compress_blocks_kernel(const uint8_t *__restrict__ src, int64_t src_bytes,
                                                             const int64_t *__restrict__ offsets, const int64_t *__restrict__ nbytes,
                                                             int64_t n_streams, const int64_t *__restrict__ block_prefix,
                                                             uint8_t *__restrict__ slots, int64_t *__restrict__ sizes) {
    __shared__ uint16_t table[kTable];
    const int lane = (int)threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t s = last_at_or_below(block_prefix, n_streams, b);      // block b's stream (streams without blocks share their successor's entry)
    const int64_t k = b - block_prefix[s], n = nbytes[s], off = offsets[s];
    // a table that does not describe streams inside src: nothing is read, the size says so
    if (off < 0 || n < 0 || n > kMaxStream || off > src_bytes - n || k < 0 || k * kBlock >= n) {
        if (lane == 0) sizes[b] = -1;
        return;
    }
    const uint8_t *__restrict__ sp = src + off + k * kBlock;
    const int32_t nb = (int32_t)(n - k * kBlock < kBlock ? n - k * kBlock : kBlock);
    uint8_t *__restrict__ out = slots + b * kSlot;

    for (int i = lane; i < kTable; i += 64) table[i] = (uint16_t)kEmpty;
    wave_lds_fence();

    int32_t o = 0, lit = 0, cursor = 0;                          // wave-uniform
    bool overflow = false;

    // literal bytes [lit, end) in front of whatever comes next
    auto flush = [&](int32_t end) {
        const int32_t L = end - lit;
        if (L <= 0) return;
        const int32_t hd = L <= 60 ? 1 : L <= 256 ? 2 : 3;
        if ((int64_t)o + hd + L > kSlot) {
            overflow = true;
            return;
        }
        if (lane == 0) put_literal_head(out + o, L);
        for (int32_t i = lane; i < L; i += 64) out[o + hd + i] = sp[lit + i];
        o += hd + L;
    };

    for (int32_t c0 = 0; c0 < nb && !overflow; c0 += kChunk) {
        const int32_t pos = c0 + lane;
        const bool has = pos + 3 < nb;
        uint32_t v = 0, h = 0xFFFFFFFFu, before = kEmpty;
        if (has) {
            v = load32(sp + pos);
            h = hash(v);
            before = table[h];
        }
        int32_t near = -1;
        bool later = false;
#pragma unroll
        for (int j = 0; j < kChunk; ++j) {
            const uint32_t hj = (uint32_t)__builtin_amdgcn_readlane((int)h, j);
            const bool eq = hj == h;
            near = (eq && j < lane) ? j : near;
            later = later || (eq && j > lane);
        }
        if (has && !later) table[h] = (uint16_t)pos;
        wave_lds_fence();
        if (c0 + kChunk <= cursor) continue;                     // a match covers the whole chunk: its positions were inserted, no more
        const int32_t q = near >= 0 ? c0 + near : (before != kEmpty ? (int32_t)before : -1);
        const bool valid = has && q >= 0 && load32(sp + q) == v;
        for (;;) {
            const unsigned long long m = __ballot(valid && pos >= cursor);
            if (m == 0ull) break;
            const int l = __builtin_ctzll(m);
            const int32_t mp = c0 + l, mq = __shfl(q, l);
            int32_t len = 4;
            for (;;) {
                const int32_t i = len + lane;
                const bool same = mp + i < nb && sp[mq + i] == sp[mp + i];
                const unsigned long long bal = __ballot(same);
                if (bal == ~0ull) {
                    len += 64;
                    continue;
                }
                len += __builtin_ctzll(~bal);
                break;
            }
            flush(mp);
            const int32_t offset = mp - mq;
            const int32_t pieces = (len <= 11 && offset < 2048) ? 0 : (len + 63) / 64;
            if (overflow || (int64_t)o + (pieces ? 3 * pieces : 2) > kSlot) {
                overflow = true;
                break;
            }
            int32_t cb = 0;
            if (lane == 0) cb = put_copy(out + o, offset, len);
            o += __shfl(cb, 0);
            cursor = mp + len;
            lit = cursor;
        }
    }
    if (!overflow) flush(nb);
    if (lane == 0) sizes[b] = overflow ? -1 : (int64_t)o;
}

// Stream s's preamble goes to size_prefix[block_prefix[s]] + vprefix[s]; block b's elements to size_prefix[b] + vprefix[s + 1]
// (vprefix: exclusive prefix sum of the preambles' lengths).
__global__ __launch_bounds__(256) void compact_blocks_kernel(const int64_t *__restrict__ block_prefix, int64_t n_streams,
                                                             const uint8_t *__restrict__ slots, const int64_t *__restrict__ size_prefix,
                                                             const int64_t *__restrict__ vprefix, uint8_t *__restrict__ out,
                                                             int64_t out_bytes, int32_t *__restrict__ bad) {
    const int64_t b = blockIdx.x;
    const int64_t s = last_at_or_below(block_prefix, n_streams, b);      // block b's stream (streams without blocks share their successor's entry)
    const int64_t size = size_prefix[b + 1] - size_prefix[b], dst = size_prefix[b] + vprefix[s + 1];
    if (size < 0 || size > kSlot || dst < 0 || dst > out_bytes - size) {
        if (threadIdx.x == 0) atomicOr(bad, 1);
        return;
    }
    const uint8_t *__restrict__ from = slots + b * kSlot;
    for (int64_t i = threadIdx.x; i < size; i += 256) out[dst + i] = from[i];
}

__global__ __launch_bounds__(256) void preambles_kernel(const int64_t *__restrict__ nbytes, const int64_t *__restrict__ block_prefix,
                                                        int64_t n_streams, int64_t n_blocks, const int64_t *__restrict__ size_prefix,
                                                        const int64_t *__restrict__ vprefix, uint8_t *__restrict__ out, int64_t out_bytes,
                                                        int32_t *__restrict__ bad) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_streams) return;
    const int64_t n = nbytes[s], first = block_prefix[s];
    if (n < 0 || n > kMaxStream || first < 0 || first > n_blocks) {
        atomicOr(bad, 1);
        return;
    }
    const int64_t dst = size_prefix[first] + vprefix[s];
    if (dst < 0 || dst > out_bytes - varint_len((uint64_t)n)) {
        atomicOr(bad, 1);
        return;
    }
    put_varint(out + dst, (uint64_t)n);
}

// 16 payload bytes per thread.  pay_off[p]: where page p's payload starts (n_pages + 1 entries); cuts[p]: its first value.
__global__ __launch_bounds__(256) void pack_pages_kernel(const int32_t *__restrict__ offsets, int64_t rows, const uint8_t *__restrict__ data,
                                                         int64_t data_bytes, const int64_t *__restrict__ cuts,
                                                         const int64_t *__restrict__ pay_off, int64_t n_pages, int64_t total,
                                                         uint8_t *__restrict__ payload, int32_t *__restrict__ bad) {
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    if (i0 >= total) return;
    // the page its first byte falls into (no page is empty: no ties)
    int64_t p = last_at_or_below(pay_off, n_pages, i0), v0 = 0, v1 = 0, k = 0, start = 0, end = 0;
    int32_t head = 0;
    bool fresh = true, ok = true;
    const int64_t stop = i0 + 16 < total ? i0 + 16 : total;
    for (int64_t i = i0; i < stop; ++i) {
        while (fresh || i >= end) {
            if (!fresh) ++p;
            if (p >= n_pages) {
                ok = false;
                break;
            }
            v0 = cuts[p];
            v1 = cuts[p + 1];
            start = pay_off[p];
            end = pay_off[p + 1];
            // the page table must describe this text: values in order and inside the offsets, payload lengths as the header says
            if (v0 < 0 || v1 <= v0 || v1 > rows || start > i || end - start != page_payload_len(offsets, v0, v1) || offsets[v0] < 0 ||
                (int64_t)offsets[v1] > data_bytes) {
                ok = false;
                break;
            }
            head = page_head_len(v1 - v0);
            if (fresh) {
                // the value the first byte falls into: the last k in [v0, v1) with plain_start(k) <= r
                const int64_t r = i - start - head;
                int64_t a = v0, z = v1;
                while (r > 0 && z - a > 1) {
                    const int64_t mid = (a + z) >> 1;
                    if (plain_start(offsets, v0, mid) <= r) a = mid;
                    else z = mid;
                }
                k = a;
            } else {
                k = v0;
            }
            fresh = false;
        }
        if (!ok) break;
        const int64_t r = i - start;
        uint32_t byte;
        if (r < head) {
            byte = page_head_byte(v1 - v0, (int32_t)r);
        } else {
            const int64_t rp = r - head;
            while (k + 1 < v1 && plain_start(offsets, v0, k + 1) <= rp) ++k;
            if (offsets[k + 1] < offsets[k]) {                   // offsets that go backwards: not arrow's layout
                ok = false;
                break;
            }
            const int64_t at = (int64_t)offsets[k] + (rp - plain_start(offsets, v0, k)) - 4;
            if (at >= data_bytes) {
                ok = false;
                break;
            }
            byte = plain_byte(offsets, data, v0, k, rp);
        }
        payload[i] = (uint8_t)byte;
    }
    if (!ok) atomicOr(bad, 1);
}

}  // namespace snappy
}  // namespace mspa

using namespace mspa;

extern "C" int64_t mspa_snappy_capacity(int64_t n) { return (n < 0 || n > snappy::kMaxStream) ? -1 : snappy::capacity(n); }

extern "C" int64_t mspa_snappy_compress_host(const uint8_t *src, int64_t n, uint8_t *dst, int64_t dst_capacity) {
    if (n < 0 || n > snappy::kMaxStream) return fail(MSPA_EINVAL, "mspa_snappy_compress_host: 0 <= n < 2^31");
    if ((n > 0 && !src) || !dst) return fail(MSPA_EINVAL, "mspa_snappy_compress_host: null pointer");
    if (dst_capacity < snappy::capacity(n)) return fail(MSPA_EINVAL, "mspa_snappy_compress_host: dst smaller than mspa_snappy_capacity(n)");
    return snappy::compress_host(src, n, dst);
}

extern "C" int64_t mspa_snappy_workspace_bytes(int64_t n_blocks) {
    if (n_blocks < 0 || n_blocks > 0x7fffffffLL) return -1;
    return n_blocks * snappy::kSlot;
}

extern "C" int mspa_snappy_compress_device(const uint8_t *src_dev, int64_t src_bytes, const int64_t *offsets_dev, const int64_t *nbytes_dev,
                                           int64_t n_streams, const int64_t *block_prefix_dev, int64_t n_blocks, uint8_t *slots_dev,
                                           int64_t slots_bytes, int64_t *out_block_sizes_dev, void *stream) {
    if (src_bytes < 0 || n_streams < 0 || n_blocks < 0 || n_blocks > 0x7fffffffLL)
        return fail(MSPA_EINVAL, "mspa_snappy_compress_device: bad size");
    if (n_blocks == 0) return MSPA_OK;
    if (n_streams == 0) return fail(MSPA_EINVAL, "mspa_snappy_compress_device: blocks without streams");
    if (!src_dev || !offsets_dev || !nbytes_dev || !block_prefix_dev || !slots_dev || !out_block_sizes_dev)
        return fail(MSPA_EINVAL, "mspa_snappy_compress_device: null pointer");
    if (slots_bytes < n_blocks * snappy::kSlot)
        return fail(MSPA_EINVAL, "mspa_snappy_compress_device: slots smaller than mspa_snappy_workspace_bytes(n_blocks)");
    hipLaunchKernelGGL(snappy::compress_blocks_kernel, dim3((unsigned)n_blocks), dim3(64), 0, (hipStream_t)stream, src_dev, src_bytes,
                       offsets_dev, nbytes_dev, n_streams, block_prefix_dev, slots_dev, out_block_sizes_dev);
    return check_hip(hipGetLastError(), "mspa_snappy_compress_device");
}

extern "C" int mspa_snappy_compact_device(const int64_t *nbytes_dev, int64_t n_streams, const int64_t *block_prefix_dev, int64_t n_blocks,
                                          const uint8_t *slots_dev, int64_t slots_bytes, const int64_t *size_prefix_dev,
                                          const int64_t *preamble_prefix_dev, uint8_t *out_dev, int64_t out_bytes, int32_t *bad_flag_dev,
                                          void *stream) {
    if (n_streams < 0 || n_blocks < 0 || n_blocks > 0x7fffffffLL || out_bytes < 0 || n_streams > (int64_t)0x7fffffff * 256)
        return fail(MSPA_EINVAL, "mspa_snappy_compact_device: bad size");
    if (n_streams == 0) return n_blocks == 0 ? MSPA_OK : fail(MSPA_EINVAL, "mspa_snappy_compact_device: blocks without streams");
    if (!nbytes_dev || !block_prefix_dev || !size_prefix_dev || !preamble_prefix_dev || !out_dev || !bad_flag_dev ||
        (n_blocks > 0 && !slots_dev))
        return fail(MSPA_EINVAL, "mspa_snappy_compact_device: null pointer");
    if (slots_bytes < n_blocks * snappy::kSlot)
        return fail(MSPA_EINVAL, "mspa_snappy_compact_device: slots smaller than mspa_snappy_workspace_bytes(n_blocks)");
    hipStream_t st = (hipStream_t)stream;
    if (n_blocks > 0)
        hipLaunchKernelGGL(snappy::compact_blocks_kernel, dim3((unsigned)n_blocks), dim3(256), 0, st, block_prefix_dev, n_streams, slots_dev,
                           size_prefix_dev, preamble_prefix_dev, out_dev, out_bytes, bad_flag_dev);
    hipLaunchKernelGGL(snappy::preambles_kernel, dim3((unsigned)((n_streams + 255) / 256)), dim3(256), 0, st, nbytes_dev, block_prefix_dev,
                       n_streams, n_blocks, size_prefix_dev, preamble_prefix_dev, out_dev, out_bytes, bad_flag_dev);
    return check_hip(hipGetLastError(), "mspa_snappy_compact_device");
}

extern "C" int64_t mspa_parquet_page_cuts_host(const int32_t *offsets, int64_t rows, int64_t page_bytes, int64_t *out_cuts,
                                               int64_t cuts_capacity) {
    if (rows < 0 || page_bytes < 1) return fail(MSPA_EINVAL, "mspa_parquet_page_cuts_host: rows >= 0, page_bytes >= 1");
    if (!offsets) return fail(MSPA_EINVAL, "mspa_parquet_page_cuts_host: null pointer");
    for (int64_t k = 0; k < rows; ++k)
        if (offsets[k + 1] < offsets[k] || offsets[k] < 0) return fail(MSPA_EINVAL, "mspa_parquet_page_cuts_host: offsets must not decrease");
    const int64_t pages = snappy::page_cuts(offsets, rows, page_bytes, out_cuts, cuts_capacity);
    if (pages < 0) return fail(MSPA_EINVAL, "mspa_parquet_page_cuts_host: out_cuts too small");
    return pages;
}

extern "C" int64_t mspa_parquet_page_payload_bytes_host(const int32_t *offsets, int64_t v0, int64_t v1) {
    if (!offsets || v0 < 0 || v1 <= v0) return fail(MSPA_EINVAL, "mspa_parquet_page_payload_bytes_host: 0 <= v0 < v1");
    return snappy::page_payload_len(offsets, v0, v1);
}

extern "C" int mspa_parquet_page_payload_host(const int32_t *offsets, const uint8_t *data, int64_t v0, int64_t v1, uint8_t *dst,
                                              int64_t dst_capacity) {
    if (!offsets || !dst || v0 < 0 || v1 <= v0) return fail(MSPA_EINVAL, "mspa_parquet_page_payload_host: 0 <= v0 < v1, no null pointer");
    if (offsets[v1] > offsets[v0] && !data) return fail(MSPA_EINVAL, "mspa_parquet_page_payload_host: null data");
    if (dst_capacity < snappy::page_payload_len(offsets, v0, v1)) return fail(MSPA_EINVAL, "mspa_parquet_page_payload_host: dst too small");
    snappy::page_payload_host(offsets, data, v0, v1, dst);
    return MSPA_OK;
}

extern "C" int mspa_parquet_string_pages_device(const int32_t *text_offsets_dev, int64_t rows, const uint8_t *data_dev, int64_t data_bytes,
                                                const int64_t *cuts_dev, const int64_t *payload_offsets_dev, int64_t n_pages,
                                                int64_t payload_bytes, uint8_t *out_payload_dev, int32_t *bad_flag_dev, void *stream) {
    if (rows < 0 || data_bytes < 0 || n_pages < 0 || payload_bytes < 0 || data_bytes > 0x7fffffffLL)
        return fail(MSPA_EINVAL, "mspa_parquet_string_pages_device: bad size");
    if (n_pages == 0) return payload_bytes == 0 ? MSPA_OK : fail(MSPA_EINVAL, "mspa_parquet_string_pages_device: payload without pages");
    if (n_pages > rows) return fail(MSPA_EINVAL, "mspa_parquet_string_pages_device: more pages than rows");
    if (payload_bytes < 10 * n_pages) return fail(MSPA_EINVAL, "mspa_parquet_string_pages_device: payload too small for its pages");
    if (!text_offsets_dev || !cuts_dev || !payload_offsets_dev || !out_payload_dev || !bad_flag_dev || (data_bytes > 0 && !data_dev))
        return fail(MSPA_EINVAL, "mspa_parquet_string_pages_device: null pointer");
    const int64_t threads = (payload_bytes + 15) / 16;
    if (threads > (int64_t)0x7fffffff * 256) return fail(MSPA_EINVAL, "mspa_parquet_string_pages_device: payload too large");
    hipLaunchKernelGGL(snappy::pack_pages_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, text_offsets_dev,
                       rows, data_dev, data_bytes, cuts_dev, payload_offsets_dev, n_pages, payload_bytes, out_payload_dev, bad_flag_dev);
    return check_hip(hipGetLastError(), "mspa_parquet_string_pages_device");
}
