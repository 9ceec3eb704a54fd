// K12: the visibility index's `values` column chunk as parquet v1 data pages (PLAIN BYTE_ARRAY, RLE definition levels, Snappy),
// written ON the MI355X from the text K10 (format_lists.hip) leaves in arrow's string layout.
//
// What it replaces: pyarrow's page assembly and Snappy compression of ~80 MB of JSON text per 320-frame scene on an encoder thread,
// and the copy of that text over PCIe.  Every output byte is defined by csrc/snappy_core.h; a g++ build of that header is the
// reference these kernels equal byte for byte (tests/test_gpu_parquet_pages.py).
//
// Three kernels around the caller's prefix sums (torch.cumsum: the caller's plumbing, as for K10):
//   pack      every thread writes 16 consecutive payload bytes: one binary search for the value its first byte falls into, then a
//             walk forward.  Bytes are distributed, not values -- one image_to_points value is ~300 KB of text.
//   compress  one wave per 64 KiB block of a stream.  The hash table (uint16[16384], 32 KiB) lives in LDS.  The wave hashes 64
//             positions at a time: each lane reads the table as it was before the chunk, takes the nearest earlier lane of the chunk
//             with an equal hash instead when there is one (a 64-step readlane loop: the lists repeat at distances 7 - 9, so
//             matches inside a chunk carry most of the ratio), then the last lane of every hash inserts.  The greedy parse walks
//             the chunk with ballot + ctz, extends a match 64 bytes a step, the lanes copy literal bytes and lane 0 writes tags.
//             Output goes to the block's worst-case slot, its byte count to a size array.
//   compact   block outputs -> contiguous streams behind their varint(uncompressed) preambles.
// No load goes beyond a stream's last byte and no store beyond a slot: every index is guarded, nothing relies on padding.
#include "mspa_common.h"
#include "snappy_core.h"

namespace mspa {
namespace snappy {

// The stream block b belongs to: the last s with block_prefix[s] <= b (streams without blocks share their successor's entry).
__device__ __forceinline__ int64_t stream_of_block(const int64_t *__restrict__ block_prefix, int64_t n_streams, int64_t b) {
    int64_t lo = 0, hi = n_streams;                              // invariant: block_prefix[lo] <= b < block_prefix[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (block_prefix[mid] <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(64) void compress_blocks_kernel(const uint8_t *__restrict__ src, int64_t src_bytes,
                                                             const int64_t *__restrict__ offsets, const int64_t *__restrict__ nbytes,
                                                             int64_t n_streams, const int64_t *__restrict__ block_prefix,
                                                             uint8_t *__restrict__ slots, int64_t *__restrict__ sizes) {
    __shared__ uint16_t table[kTable];
    const int lane = (int)threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t s = stream_of_block(block_prefix, n_streams, b);
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
    const int64_t s = stream_of_block(block_prefix, n_streams, b);
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
    int64_t lo = 0, hi = n_pages;                                // invariant: pay_off[lo] <= i0 < pay_off[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (pay_off[mid] <= i0) lo = mid;
        else hi = mid;
    }
    int64_t p = lo, v0 = 0, v1 = 0, k = 0, start = 0, end = 0;
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

// ------------------------------------------------------------------------------------------------------------------ reading
// The way back: a values chunk's pages -> the image_to_points rows' bitsets, without the text ever leaving the device.
//
//   decompress   one wave per Snappy stream (a page of ~1 MiB).  The element chain is sequential, so input position p, output
//                position o and every element's fields are WAVE-UNIFORM (the head's words come through readfirstlane; every
//                branch on them is scalar); the 64 lanes only move an element's bytes, one byte each (no element but a long
//                literal writes more than 64).  Rules and status codes are snappy_core.h's, in decompress()'s order.
//                - the compressed bytes sit in two registers as a sliding window of 128 aligned words (lane l holds word
//                  base + l and base + 64 + l), filled by coalesced dword loads every 256 input bytes.  A head (<= 5 bytes)
//                  comes out of them with v_readlane, a literal of up to 64 bytes with ds_bpermute; longer literals go from
//                  global memory to global memory;
//                - a copy reads the wave's own earlier output.  The last kRing = 32 KiB of it are kept in LDS (every output
//                  byte is stored there as well as in global memory), so a copy with offset <= kRing is an LDS gather -- lane i
//                  takes byte i mod offset of the period, which covers the overlapping (run-like) copies -- ordered behind the
//                  stores by wave_lds_fence() (a wave's LDS operations execute in order).  A copy that reaches further back
//                  (pyarrow's and this library's blocks allow 64 KiB, a copy-4 anything) loads from the output in global
//                  memory behind `s_waitcnt vmcnt(0)` between a workgroup-scope release / acquire fence pair (which keeps the
//                  compiler from moving the stores and the load across it; on gfx950 the pair alone emits no wait).  The wait
//                  returns when every store of the wave has been acknowledged, i.e. has gone through the write-through L1 of
//                  the CU the wave runs on to L2, and the load that follows is served by that same L1 or the L2 behind it; the
//                  lines it reads lie at least 32 KiB behind the write front, so no line is read before it was written whole.
//                  So no offset is declined;
//                - 32 KiB of LDS per wave: five waves to a CU, 1 280 on the chip.  A scene has 30 - 90 pages; the ring's size does
//                  not decide the occupancy of such a launch, its hit rate does (the lists repeat 7 - 9 bytes back).
//   spans        one lane per needed page walks the PLAIN u32 length chain from the page's first value to its last needed row: a
//                dependent-load chain as long as the values in front of that row.  In this project's files a scene's
//                image_to_points rows open the chunk (a few values per ~1 MiB page); a row group that mixes scenes may put
//                ~20 k short point_to_images rows of the scene before in front of them -- 20 k dependent L2 loads, a few
//                milliseconds for that one lane (not measured on such a file).
//   brackets     one lane per row: '[' and ']' behind / in front of JSON white space.
//   gather       the texts between the brackets back to back (what K11's list parser takes), one byte per lane.
//   lists->bits  one lane per parsed value.  A list ascends, so the values of one 64-bit word are neighbours in the value array:
//                the lane whose predecessor lies in another word (or that opens the row) ORs the run and stores the word with a
//                plain store into the zeroed row.  A value below its predecessor or outside [0, n_points) declines the row
//                (plain stores of a constant: lanes that race write the same thing); a duplicate is harmless.
// No atomics; every load and store is checked against the buffer it goes to.
constexpr int kRing = 32768;
constexpr uint32_t kRingMask = kRing - 1;

__global__ __launch_bounds__(64) void decompress_kernel(const uint8_t *__restrict__ src, int64_t src_bytes,
                                                        const int64_t *__restrict__ offsets, const int64_t *__restrict__ nbytes,
                                                        uint8_t *out, int64_t out_bytes, const int64_t *__restrict__ out_offsets,
                                                        const int64_t *__restrict__ out_sizes, int32_t *__restrict__ status) {
    __shared__ uint8_t ring[kRing];
    const int lane = (int)threadIdx.x;
    const int64_t s = blockIdx.x;
    const int64_t off = offsets[s], n = nbytes[s], oo = out_offsets[s], expected = out_sizes[s];
    if (off < 0 || n < 0 || n > kMaxStream || off > src_bytes - n || oo < 0 || expected < 0 || expected > kMaxStream ||
        oo > out_bytes - expected) {
        if (lane == 0) status[s] = MSPA_EINVAL;                  // the tables do not describe spans inside src / out: nothing is touched
        return;
    }
    const uint8_t *__restrict__ sp = src + off;
    uint8_t *dp = out + oo;
    int64_t p = 0, o = 0;                                        // wave-uniform
    int rc = 0;
    constexpr bool kPreamble = true;
#include "snappy_decode_loop.inc"
    if (lane == 0) status[s] = rc;
}

// The block route's last pass, over the same stream table.  `serial`: the per-stream flags of the passes in front -- a stream whose
// flag is 0 was decoded by its blocks' waves and only gets its status and its route here; a flagged one is decoded from scratch,
// as decompress_kernel does it.
__global__ __launch_bounds__(64) void decompress_flagged_kernel(const uint8_t *__restrict__ src, int64_t src_bytes,
                                                                const int64_t *__restrict__ offsets, const int64_t *__restrict__ nbytes,
                                                                uint8_t *out, int64_t out_bytes, const int64_t *__restrict__ out_offsets,
                                                                const int64_t *__restrict__ out_sizes, int32_t *__restrict__ status,
                                                                const int32_t *__restrict__ serial, const int64_t *__restrict__ block_prefix,
                                                                int32_t *__restrict__ route) {
    __shared__ uint8_t ring[kRing];
    const int lane = (int)threadIdx.x;
    const int64_t s = blockIdx.x;
    const bool by_blocks = serial[s] == 0;
    if (lane == 0) route[s] = by_blocks ? (int32_t)(block_prefix[s + 1] - block_prefix[s]) : 0;
    if (by_blocks) {
        if (lane == 0) status[s] = 0;
        return;
    }
    const int64_t off = offsets[s], n = nbytes[s], oo = out_offsets[s], expected = out_sizes[s];
    if (off < 0 || n < 0 || n > kMaxStream || off > src_bytes - n || oo < 0 || expected < 0 || expected > kMaxStream ||
        oo > out_bytes - expected) {
        if (lane == 0) status[s] = MSPA_EINVAL;
        return;
    }
    const uint8_t *__restrict__ sp = src + off;
    uint8_t *dp = out + oo;
    int64_t p = 0, o = 0;                                        // wave-uniform
    int rc = 0;
    constexpr bool kPreamble = true;
#include "snappy_decode_loop.inc"
    if (lane == 0) status[s] = rc;
}

// --------------------------------------------------------------------------------------------------------- decoding by blocks
// One wave per 64 KiB block of a blockwise stream (snappy_core.h), so that one 29 MB page is 450 waves' work and not one's.
// Where a block's elements begin in the compressed bytes is found without a walk of the whole element chain:
//
//   prefix       one wave: the exclusive prefix sum of the streams' compressed sizes (where each stream's tables lie in the
//                workspace) and every stream's flag -- `serial` = 1 for a stream the block route does not take from the start:
//                a table entry outside src / out, fewer than `min_blocks` blocks, a block table that is not ceil(size / 64 Ki),
//                tables that do not fit the workspace.  Such a stream takes no table space.
//   tables       one wave per segment of kSeg = 2 KiB of compressed bytes.  EVERY byte position i of the segment is treated as an
//                element start: its advance in the input (head + literal bytes) and its output length give next[i] and sum[i];
//                then pointer jumping in LDS, ceil(log2 kSeg) rounds at most, until next[i] is the first position at or beyond
//                the segment's end on the chain from i (a literal may jump whole segments) and sum[i] the output bytes on the
//                way.  A position that is no real element start holds a garbage tag: an element that is cut off, runs past the
//                stream or is longer than a stream may be gives kLeave, and kLeave absorbs; sums saturate.  A round reads all
//                of a lane's 32 entries into registers before it writes any (one wave: its LDS operations execute in order),
//                so a round sees the round before, whole.  (next, sum) pairs go to the workspace: 8 bytes per compressed byte.
//   walk         one lane per stream: from the preamble's end, (entry, output offset) of every segment the chain enters -- one
//                dependent 8-byte load per segment, the only serial chain over a stream.  The chain must end exactly at the
//                stream's end with `expected` bytes; the stream's last start (its end) is written here.
//   starts       one lane per segment walks the true chain from the segment's entry to its end: an element that begins at output
//                b * 64 Ki gives starts[b]; one that straddles such a multiple, or a copy that reaches in front of its block,
//                flags the stream.
//   blocks       one wave per (stream, block): the element loop over [starts[b], starts[b + 1]) into the block's own bytes.  A
//                block that does not decode to exactly its size from exactly its range flags the stream.
//   (serial)     decompress_flagged_kernel over the same stream table: flagged streams from scratch, the others get status 0.
// Flags are only ever raised, with plain stores of the constant 1, and read by the kernels behind; the scan decides routes and
// never a status: whatever is wrong with a stream sends it to the one-wave kernel, whose code and bytes are the host's.
constexpr int kSeg = 2048;
constexpr int kSegRounds = 11;                          // 2^11 = kSeg: a chain inside a segment has at most kSeg steps
constexpr int kSegPerLane = kSeg / 64;
constexpr uint32_t kLeave = 0xFFFFFFFFu;                // next: the chain leaves the stream (or is no chain at all)
constexpr uint64_t kNoEntry = ~0ull;                    // a segment the chain does not enter (the tables are cleared to this)

struct BlocksWorkspace {                                // the caller's workspace, cut up (byte offsets, every one a multiple of 16)
    int64_t prefix, serial, entry, table, starts, total;
    int64_t seg_slots;
};

__host__ __device__ inline BlocksWorkspace blocks_workspace(int64_t stream_bytes, int64_t n_streams, int64_t n_blocks) {
    BlocksWorkspace w;
    auto up = [](int64_t v) { return (v + 15) / 16 * 16; };
    w.seg_slots = stream_bytes / kSeg + n_streams;      // stream s's segments start at slot prefix[s] / kSeg + s
    w.prefix = 0;
    w.serial = w.prefix + up(8 * (n_streams + 1));
    w.entry = w.serial + up(4 * n_streams);
    w.table = w.entry + up(8 * w.seg_slots);
    w.starts = w.table + up(8 * stream_bytes);
    w.total = w.starts + up(8 * (n_blocks + n_streams));
    return w;
}

__device__ __forceinline__ int64_t seg_base(const int64_t *__restrict__ prefix, int64_t s) { return prefix[s] / kSeg + s; }

__global__ __launch_bounds__(64) void blocks_prefix_kernel(int64_t src_bytes, const int64_t *__restrict__ offsets,
                                                           const int64_t *__restrict__ nbytes, int64_t n_streams, int64_t out_bytes,
                                                           const int64_t *__restrict__ out_offsets, const int64_t *__restrict__ out_sizes,
                                                           const int64_t *__restrict__ block_prefix, int64_t n_blocks, int64_t min_blocks,
                                                           int64_t stream_bytes, int64_t *__restrict__ prefix, int32_t *__restrict__ serial) {
    const int lane = (int)threadIdx.x;
    int64_t carry = 0;                                           // wave-uniform
    if (lane == 0) prefix[0] = 0;
    for (int64_t s0 = 0; s0 < n_streams; s0 += 64) {
        const int64_t s = s0 + lane;
        int64_t take = 0;
        if (s < n_streams) {
            const int64_t off = offsets[s], n = nbytes[s], expected = out_sizes[s], b0 = block_prefix[s], b1 = block_prefix[s + 1];
            const bool inside = !(off < 0 || n < 0 || n > kMaxStream || off > src_bytes - n || expected < 0 || expected > kMaxStream);
            bool out_ok = true;
            if (out_offsets) out_ok = out_offsets[s] >= 0 && inside && out_offsets[s] <= out_bytes - expected;
            if (inside && out_ok && b0 >= 0 && b1 <= n_blocks && b1 - b0 == block_count(expected) && b1 - b0 >= min_blocks) take = n;
        }
        int64_t incl = take;
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        const int64_t begin = carry + incl - take;
        // the tables of a stream that is taken lie at [begin, begin + n) of the workspace's: they must fit what the caller gave
        if (s < n_streams) {
            const bool fits = begin + take <= stream_bytes;
            const bool by_blocks = take > 0 && fits;
            serial[s] = by_blocks ? 0 : 1;
            prefix[s + 1] = carry + incl;
        }
        carry += __shfl(incl, 63);
    }
}

// The stream segment slot g belongs to: the last s with seg_base(s) <= g (seg_base ascends strictly).
__device__ __forceinline__ int64_t stream_of_segment(const int64_t *__restrict__ prefix, int64_t n_streams, int64_t g) {
    int64_t lo = 0, hi = n_streams;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (seg_base(prefix, mid) <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint64_t pair_of(uint32_t next, uint32_t sum) { return (uint64_t)next | (uint64_t)sum << 32; }

__global__ __launch_bounds__(64) void segment_tables_kernel(const uint8_t *__restrict__ src, const int64_t *__restrict__ offsets,
                                                            const int64_t *__restrict__ nbytes, int64_t n_streams,
                                                            const int64_t *__restrict__ prefix, const int32_t *__restrict__ serial,
                                                            int64_t stream_bytes, uint64_t *__restrict__ table) {
    __shared__ uint32_t raw[kSeg / 4 + 1];
    __shared__ uint64_t tab[kSeg];
    const int lane = (int)threadIdx.x;
    const int64_t g = blockIdx.x;
    const int64_t s = stream_of_segment(prefix, n_streams, g);
    if (serial[s] != 0) return;                                  // (an unflagged stream's table entries were checked by the prefix kernel)
    const int64_t n = nbytes[s], base = (g - seg_base(prefix, s)) * kSeg, at = prefix[s];
    if (base >= n || at < 0 || at > stream_bytes - n) return;
    const uint8_t *__restrict__ sp = src + offsets[s];
    const int64_t seg_end = base + kSeg < n ? base + kSeg : n;

    for (int i = lane; i < kSeg / 4 + 1; i += 64) {              // the segment's bytes and the 4 behind them; zero beyond the stream
        uint32_t v = 0;
        for (int j = 0; j < 4; ++j) {
            const int64_t q = base + 4 * i + j;
            if (q < n) v |= (uint32_t)sp[q] << (8 * j);
        }
        raw[i] = v;
    }
    wave_lds_fence();
    for (int k = 0; k < kSegPerLane; ++k) {
        const int i = k * 64 + lane;
        const int64_t q = base + i;
        uint64_t entry = pair_of(kLeave, 0);
        if (q < n) {
            const uint64_t bytes = ((uint64_t)raw[i >> 2] | (uint64_t)raw[(i >> 2) + 1] << 32) >> (8 * (i & 3));
            Element e;
            const int rc = parse_element(bytes, n - q, e);
            const int64_t advance = e.head + (e.literal ? e.len : 0);
            if (rc == 0 && advance <= n - q && e.len <= kMaxStream) entry = pair_of((uint32_t)(q + advance), (uint32_t)e.len);
        }
        tab[i] = entry;
    }
    for (int r = 0; r < kSegRounds; ++r) {
        wave_lds_fence();
        uint64_t theirs[kSegPerLane];
        uint32_t inside = 0;                                     // bit k: entry k's chain has not left the segment yet
#pragma unroll
        for (int k = 0; k < kSegPerLane; ++k) {
            const uint32_t next = (uint32_t)tab[k * 64 + lane];
            const bool in = next != kLeave && (int64_t)next < seg_end;
            theirs[k] = in ? tab[(int64_t)next - base] : 0;      // base <= q < next < seg_end: inside tab
            inside |= (in ? 1u : 0u) << k;
        }
        wave_lds_fence();
        if (__ballot(inside != 0) == 0ull) break;
#pragma unroll
        for (int k = 0; k < kSegPerLane; ++k) {
            if (!(inside >> k & 1u)) continue;
            const uint64_t sum = (tab[k * 64 + lane] >> 32) + (theirs[k] >> 32);     // a lane's own entry: nobody else writes it
            tab[k * 64 + lane] = pair_of((uint32_t)theirs[k], sum > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)sum);
        }
    }
    wave_lds_fence();
    for (int k = 0; k < kSegPerLane; ++k) {
        const int i = k * 64 + lane;
        if (base + i < n) table[at + base + i] = tab[i];
    }
}

__global__ __launch_bounds__(64) void segment_walk_kernel(const uint8_t *__restrict__ src, const int64_t *__restrict__ offsets,
                                                          const int64_t *__restrict__ nbytes, const int64_t *__restrict__ out_sizes,
                                                          int64_t n_streams, const int64_t *__restrict__ prefix,
                                                          const int64_t *__restrict__ block_prefix, const uint64_t *__restrict__ table,
                                                          uint64_t *__restrict__ entry, int64_t seg_slots, int64_t *__restrict__ starts,
                                                          int64_t n_starts, int32_t *__restrict__ serial) {
    const int64_t s = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (s >= n_streams || serial[s] != 0) return;
    const int64_t n = nbytes[s], expected = out_sizes[s], at = prefix[s], slot0 = seg_base(prefix, s);
    const uint8_t *__restrict__ sp = src + offsets[s];
    const int pre = parse_preamble(load_le(sp, 0, n), n, expected);
    bool ok = pre > 0;
    int64_t p = ok ? pre : 0, o = 0;
    while (ok && p < n) {
        const int64_t slot = slot0 + p / kSeg;
        if (slot >= seg_slots) {
            ok = false;
            break;
        }
        entry[slot] = pair_of((uint32_t)p, (uint32_t)o);
        const uint64_t hop = table[at + p];                      // p < n: inside the stream's part of the table
        const uint32_t next = (uint32_t)hop;
        o += (int64_t)(hop >> 32);
        ok = next != kLeave && (int64_t)next > p && (int64_t)next <= n && o <= expected;
        p = next;
    }
    ok = ok && p == n && o == expected;
    const int64_t last = block_prefix[s + 1] + s;                // the stream's starts: [block_prefix[s] + s, block_prefix[s + 1] + s]
    if (ok && last >= 0 && last < n_starts) starts[last] = n;
    else ok = false;
    if (!ok) serial[s] = 1;
}

__global__ __launch_bounds__(64) void block_starts_kernel(const uint8_t *__restrict__ src, const int64_t *__restrict__ offsets,
                                                          const int64_t *__restrict__ nbytes, const int64_t *__restrict__ out_sizes,
                                                          int64_t n_streams, const int64_t *__restrict__ prefix,
                                                          const int64_t *__restrict__ block_prefix, const uint64_t *__restrict__ entry,
                                                          int64_t seg_slots, int64_t *__restrict__ starts, int64_t n_starts,
                                                          int32_t *__restrict__ serial) {
    const int64_t g = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (g >= seg_slots) return;
    const int64_t s = stream_of_segment(prefix, n_streams, g);
    if (serial[s] != 0 || entry[g] == kNoEntry) return;
    const int64_t n = nbytes[s], expected = out_sizes[s], k = g - seg_base(prefix, s), first = block_prefix[s] + s;
    const int64_t seg_end = (k + 1) * kSeg < n ? (k + 1) * kSeg : n;
    const uint8_t *__restrict__ sp = src + offsets[s];
    int64_t p = (int64_t)(uint32_t)entry[g], o = (int64_t)(entry[g] >> 32);
    bool ok = p >= k * kSeg;
    while (ok && p < seg_end) {
        Element e;
        int rc = parse_element(load_le(sp, p, n), n - p, e);
        if (rc == 0 && e.literal && e.len > n - p - e.head) rc = kErrTruncated;
        const int64_t in_block = o % kBlock, b = first + o / kBlock;
        if (rc != 0 || o >= expected || e.len > expected - o || in_block + e.len > kBlock ||
            (!e.literal && (e.offset == 0 || e.offset > in_block)) || b < 0 || b >= n_starts) {
            ok = false;
            break;
        }
        if (in_block == 0) starts[b] = p;
        p += e.head + (e.literal ? e.len : 0);
        o += e.len;
    }
    if (!ok) serial[s] = 1;
}

// route[s] of the scan alone (mspa_snappy_block_starts_device): the stream's block count, or 0.
__global__ __launch_bounds__(64) void scan_route_kernel(const int32_t *__restrict__ serial, const int64_t *__restrict__ block_prefix,
                                                        int64_t n_streams, int32_t *__restrict__ route) {
    const int64_t s = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (s < n_streams) route[s] = serial[s] == 0 ? (int32_t)(block_prefix[s + 1] - block_prefix[s]) : 0;
}

__global__ __launch_bounds__(64) void decompress_blocks_kernel(const uint8_t *__restrict__ src, const int64_t *__restrict__ offsets,
                                                               const int64_t *__restrict__ nbytes, int64_t n_streams,
                                                               const int64_t *__restrict__ block_prefix, uint8_t *out,
                                                               const int64_t *__restrict__ out_offsets, const int64_t *__restrict__ out_sizes,
                                                               const int64_t *__restrict__ starts, int64_t n_starts, int32_t *__restrict__ serial) {
    __shared__ uint8_t ring[kRing];
    const int lane = (int)threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t s = stream_of_block(block_prefix, n_streams, b);
    if (serial[s] != 0) return;                                  // (an unflagged stream's table entries were checked by the prefix kernel)
    const int64_t k = b - block_prefix[s], size = out_sizes[s], at = b + s;
    if (k < 0 || k * kBlock >= size || at < 0 || at + 1 >= n_starts) {
        if (lane == 0) serial[s] = 1;
        return;
    }
    const int64_t p0 = starts[at], p1 = starts[at + 1], nb = size - k * kBlock < kBlock ? size - k * kBlock : kBlock;
    if (p0 < 1 || p1 < p0 || p1 > nbytes[s]) {                   // a start the scan did not find reads as -1
        if (lane == 0) serial[s] = 1;
        return;
    }
    const uint8_t *__restrict__ sp = src + offsets[s];
    uint8_t *dp = out + out_offsets[s] + k * kBlock;
    const int64_t n = p1, expected = nb;                         // the loop's names: this block's input end and size
    int64_t p = p0, o = 0;
    int rc = 0;
    constexpr bool kPreamble = false;
#include "snappy_decode_loop.inc"
    if (rc != 0 && lane == 0) serial[s] = 1;
}

constexpr int32_t kPageBounds = 1;       // a length runs past the page, or the tables do not describe it
constexpr int32_t kPageLevels = 2;       // the definition levels are not one run of ones
constexpr int32_t kRowBrackets = 1;      // a row's text is not [ ... ]
constexpr int32_t kRowOrder = 32;        // lists->bits: a value below its predecessor     (K11's parser owns bits 2 .. 16)
constexpr int32_t kRowRange = 64;        // lists->bits: a value outside [0, n_points)

__device__ __forceinline__ bool json_space(uint8_t c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }

__global__ __launch_bounds__(64) void plain_spans_kernel(const uint8_t *__restrict__ pages, int64_t pages_bytes,
                                                         const int64_t *__restrict__ page_off, const int64_t *__restrict__ page_size,
                                                         const int64_t *__restrict__ page_values, int64_t n_pages, int32_t has_levels,
                                                         const int64_t *__restrict__ row_begin, const int64_t *__restrict__ row_index,
                                                         int64_t n_rows, int64_t *__restrict__ out_start, int64_t *__restrict__ out_len,
                                                         int32_t *__restrict__ page_status) {
    const int64_t pg = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (pg >= n_pages) return;
    const int64_t off = page_off[pg], size = page_size[pg], nv = page_values[pg];
    int64_t r0 = row_begin[pg], r1 = row_begin[pg + 1];
    int32_t bad = 0;
    if (r0 < 0 || r1 < r0 || r1 > n_rows) {
        page_status[pg] = kPageBounds;
        return;
    }
    if (off < 0 || size < 0 || off > pages_bytes - size || nv < 0) bad = kPageBounds;
    const uint8_t *__restrict__ q = pages + off;
    int64_t pos = 0;
    if (!bad && has_levels) {
        const int32_t head = page_head_len(nv);
        if (head > size) bad = kPageBounds;
        for (int32_t r = 0; !bad && r < head; ++r)
            if (q[r] != page_head_byte(nv, r)) bad = kPageLevels;
        pos = head;
    }
    int64_t v = 0, r = r0;
    for (; !bad && r < r1; ++r) {
        const int64_t target = row_index[r];
        if (target < v || target >= nv) {
            bad = kPageBounds;
            break;
        }
        for (;; ++v) {
            if (pos > size - 4) {
                bad = kPageBounds;
                break;
            }
            const int64_t len = load32(q + pos);
            if (len > size - pos - 4) {
                bad = kPageBounds;
                break;
            }
            if (v == target) {
                out_start[r] = off + pos + 4;
                out_len[r] = len;
            }
            pos += 4 + len;
            if (v == target) break;
        }
        if (bad) break;
        ++v;
    }
    for (; bad && r < r1; ++r) {                                 // the rows this page did not give
        out_start[r] = 0;
        out_len[r] = 0;
    }
    page_status[pg] = bad;
}

__global__ __launch_bounds__(64) void row_brackets_kernel(const uint8_t *__restrict__ pages, int64_t pages_bytes,
                                                          const int64_t *__restrict__ start, const int64_t *__restrict__ len, int64_t n_rows,
                                                          int64_t *__restrict__ inner_start, int64_t *__restrict__ inner_len,
                                                          int32_t *__restrict__ row_status) {
    const int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (r >= n_rows) return;
    int64_t a = start[r], z = a + len[r];
    bool ok = a >= 0 && len[r] >= 2 && len[r] <= pages_bytes && a <= pages_bytes - len[r];
    if (ok) {
        while (a < z && json_space(pages[a])) ++a;
        while (z > a && json_space(pages[z - 1])) --z;
        ok = z - a >= 2 && pages[a] == '[' && pages[z - 1] == ']';
    }
    inner_start[r] = ok ? a + 1 : 0;
    inner_len[r] = ok ? z - a - 2 : 0;
    row_status[r] = ok ? 0 : kRowBrackets;
}

__global__ __launch_bounds__(256) void row_gather_kernel(const uint8_t *__restrict__ pages, int64_t pages_bytes,
                                                         const int64_t *__restrict__ inner_start, const int64_t *__restrict__ prefix,
                                                         int64_t n_rows, int64_t total, uint8_t *__restrict__ text) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    int64_t lo = 0, hi = n_rows;                                 // invariant: prefix[lo] <= i < prefix[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (prefix[mid] <= i) lo = mid;
        else hi = mid;
    }
    const int64_t from = inner_start[lo] + (i - prefix[lo]);
    text[i] = (from >= 0 && from < pages_bytes) ? pages[from] : (uint8_t)0;      // a 0 byte is no list: the parser declines the row
}

__global__ __launch_bounds__(256) void lists_to_bits_kernel(const int32_t *__restrict__ values, int64_t n_values,
                                                            const int64_t *__restrict__ offsets, int64_t n_rows, int64_t n_points,
                                                            uint64_t *__restrict__ bits, int64_t n_words, int32_t *__restrict__ row_status) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_values) return;
    int64_t lo = 0, hi = n_rows;                                 // the row: the last one with offsets[row] <= i
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (offsets[mid] <= i) lo = mid;
        else hi = mid;
    }
    const int64_t first = offsets[lo];
    int64_t end = offsets[lo + 1];
    if (end > n_values) end = n_values;
    if (i < first || i >= end) return;                           // offsets that do not hold this value: no row's
    const int64_t v = values[i], prev = (i > first && i > 0) ? (int64_t)values[i - 1] : -1;
    if (v < prev) row_status[lo] = kRowOrder;
    if (v < 0 || v >= n_points) {
        row_status[lo] = kRowRange;
        return;
    }
    if (prev >= 0 && (prev >> 6) == (v >> 6)) return;            // the lane in front owns this word
    uint64_t w = 0;
    for (int64_t j = i; j < end; ++j) {
        const int64_t u = values[j];
        if (u < 0 || (u >> 6) != (v >> 6)) break;
        w |= 1ull << (u & 63);
    }
    bits[lo * n_words + (v >> 6)] = w;                           // v < n_points <= 64 n_words
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

extern "C" int64_t mspa_snappy_decompress_host(const uint8_t *src, int64_t src_len, uint8_t *dst, int64_t expected) {
    if (src_len < 0 || src_len > snappy::kMaxStream || expected < 0 || expected > snappy::kMaxStream)
        return fail(MSPA_EINVAL, "mspa_snappy_decompress_host: 0 <= src_len, expected < 2^31");
    if ((src_len > 0 && !src) || (expected > 0 && !dst)) return fail(MSPA_EINVAL, "mspa_snappy_decompress_host: null pointer");
    return snappy::decompress(src, src_len, dst, expected);
}

extern "C" int mspa_snappy_decompress_device(const uint8_t *src_dev, int64_t src_bytes, const int64_t *offsets_dev, const int64_t *nbytes_dev,
                                             int64_t n_streams, uint8_t *out_dev, int64_t out_bytes, const int64_t *out_offsets_dev,
                                             const int64_t *out_bytes_dev, int32_t *status_dev, void *stream) {
    if (src_bytes < 0 || out_bytes < 0 || n_streams < 0 || n_streams > 0x7fffffffLL)
        return fail(MSPA_EINVAL, "mspa_snappy_decompress_device: bad size");
    if (n_streams == 0) return MSPA_OK;
    if (!offsets_dev || !nbytes_dev || !out_offsets_dev || !out_bytes_dev || !status_dev || (src_bytes > 0 && !src_dev) ||
        (out_bytes > 0 && !out_dev))
        return fail(MSPA_EINVAL, "mspa_snappy_decompress_device: null pointer");
    hipLaunchKernelGGL(snappy::decompress_kernel, dim3((unsigned)n_streams), dim3(64), 0, (hipStream_t)stream, src_dev, src_bytes, offsets_dev,
                       nbytes_dev, out_dev, out_bytes, out_offsets_dev, out_bytes_dev, status_dev);
    return check_hip(hipGetLastError(), "mspa_snappy_decompress_device");
}

extern "C" int64_t mspa_snappy_block_starts_host(const uint8_t *src, int64_t src_len, int64_t expected, int64_t *out_starts,
                                                 int64_t starts_capacity) {
    if (src_len < 0 || src_len > snappy::kMaxStream || expected < 0 || expected > snappy::kMaxStream)
        return fail(MSPA_EINVAL, "mspa_snappy_block_starts_host: 0 <= src_len, expected < 2^31");
    if ((src_len > 0 && !src) || !out_starts) return fail(MSPA_EINVAL, "mspa_snappy_block_starts_host: null pointer");
    if (starts_capacity < snappy::block_count(expected) + 1)
        return fail(MSPA_EINVAL, "mspa_snappy_block_starts_host: out_starts holds fewer than ceil(expected / 65536) + 1 entries");
    return snappy::block_starts(src, src_len, expected, out_starts, starts_capacity);
}

extern "C" int64_t mspa_snappy_blocks_workspace_bytes(int64_t stream_bytes, int64_t n_streams, int64_t n_blocks) {
    if (stream_bytes < 0 || n_streams < 0 || n_blocks < 0 || n_streams > 0x7fffffffLL || n_blocks > 0x7fffffffLL ||
        stream_bytes > ((int64_t)1 << 40))
        return -1;
    return snappy::blocks_workspace(stream_bytes, n_streams, n_blocks).total;
}

// The scan (prefix, tables, walk, starts) of a batch, enqueued on st; `starts` has n_blocks + n_streams entries.
static int enqueue_block_scan(const char *what, const uint8_t *src_dev, int64_t src_bytes, const int64_t *offsets_dev, const int64_t *nbytes_dev,
                              int64_t n_streams, int64_t out_bytes, const int64_t *out_offsets_dev, const int64_t *out_sizes_dev,
                              const int64_t *block_prefix_dev, int64_t n_blocks, int64_t min_blocks, int64_t stream_bytes, uint8_t *ws,
                              const snappy::BlocksWorkspace &w, int64_t *starts, hipStream_t st) {
    int64_t *prefix = (int64_t *)(ws + w.prefix);
    int32_t *serial = (int32_t *)(ws + w.serial);
    uint64_t *entry = (uint64_t *)(ws + w.entry), *table = (uint64_t *)(ws + w.table);
    const int64_t n_starts = n_blocks + n_streams;
    int rc = check_hip(hipMemsetAsync(entry, 0xFF, (size_t)w.seg_slots * 8, st), what);
    if (rc == MSPA_OK) rc = check_hip(hipMemsetAsync(starts, 0xFF, (size_t)n_starts * 8, st), what);
    if (rc) return rc;
    hipLaunchKernelGGL(snappy::blocks_prefix_kernel, dim3(1), dim3(64), 0, st, src_bytes, offsets_dev, nbytes_dev, n_streams, out_bytes,
                       out_offsets_dev, out_sizes_dev, block_prefix_dev, n_blocks, min_blocks, stream_bytes, prefix, serial);
    hipLaunchKernelGGL(snappy::segment_tables_kernel, dim3((unsigned)w.seg_slots), dim3(64), 0, st, src_dev, offsets_dev, nbytes_dev, n_streams,
                       (const int64_t *)prefix, (const int32_t *)serial, stream_bytes, table);
    hipLaunchKernelGGL(snappy::segment_walk_kernel, dim3((unsigned)((n_streams + 63) / 64)), dim3(64), 0, st, src_dev, offsets_dev, nbytes_dev,
                       out_sizes_dev, n_streams, (const int64_t *)prefix, block_prefix_dev, (const uint64_t *)table, entry, w.seg_slots, starts,
                       n_starts, serial);
    hipLaunchKernelGGL(snappy::block_starts_kernel, dim3((unsigned)((w.seg_slots + 63) / 64)), dim3(64), 0, st, src_dev, offsets_dev, nbytes_dev,
                       out_sizes_dev, n_streams, (const int64_t *)prefix, block_prefix_dev, (const uint64_t *)entry, w.seg_slots, starts, n_starts,
                       serial);
    return check_hip(hipGetLastError(), what);
}

static int check_blocks_args(const char *what, int64_t src_bytes, int64_t n_streams, int64_t n_blocks, int64_t stream_bytes, const void *workspace,
                             int64_t workspace_bytes) {
    if (src_bytes < 0 || n_streams < 0 || n_streams > 0x7fffffffLL || n_blocks < 0 || n_blocks > 0x7fffffffLL || stream_bytes < 0 ||
        stream_bytes > ((int64_t)1 << 40) || workspace_bytes < 0)
        return fail(MSPA_EINVAL, what);
    if (n_streams == 0) return MSPA_OK;
    const snappy::BlocksWorkspace w = snappy::blocks_workspace(stream_bytes, n_streams, n_blocks);
    if (w.seg_slots > 0x7fffffffLL) return fail(MSPA_EINVAL, what);
    if (!workspace || ((uintptr_t)workspace & 15) != 0 || workspace_bytes < w.total) return fail(MSPA_EINVAL, what);
    return MSPA_OK;
}

extern "C" int mspa_snappy_block_starts_device(const uint8_t *src_dev, int64_t src_bytes, const int64_t *offsets_dev, const int64_t *nbytes_dev,
                                               int64_t n_streams, const int64_t *out_bytes_dev, const int64_t *block_prefix_dev, int64_t n_blocks,
                                               int64_t stream_bytes, void *workspace, int64_t workspace_bytes, int64_t *starts_dev,
                                               int32_t *route_dev, void *stream) {
    const int bad = check_blocks_args("mspa_snappy_block_starts_device: bad size, or a workspace that is null, not 16-byte aligned or smaller than "
                                      "mspa_snappy_blocks_workspace_bytes", src_bytes, n_streams, n_blocks, stream_bytes, workspace, workspace_bytes);
    if (bad) return bad;
    if (n_streams == 0) return MSPA_OK;
    if (!offsets_dev || !nbytes_dev || !out_bytes_dev || !block_prefix_dev || !starts_dev || !route_dev || (src_bytes > 0 && !src_dev))
        return fail(MSPA_EINVAL, "mspa_snappy_block_starts_device: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const snappy::BlocksWorkspace w = snappy::blocks_workspace(stream_bytes, n_streams, n_blocks);
    const int rc = enqueue_block_scan("mspa_snappy_block_starts_device", src_dev, src_bytes, offsets_dev, nbytes_dev, n_streams, 0, nullptr,
                                      out_bytes_dev, block_prefix_dev, n_blocks, 1, stream_bytes, (uint8_t *)workspace, w, starts_dev, st);
    if (rc) return rc;
    hipLaunchKernelGGL(snappy::scan_route_kernel, dim3((unsigned)((n_streams + 63) / 64)), dim3(64), 0, st,
                       (const int32_t *)((uint8_t *)workspace + w.serial), block_prefix_dev, n_streams, route_dev);
    return check_hip(hipGetLastError(), "mspa_snappy_block_starts_device");
}

extern "C" int mspa_snappy_decompress_blocks_device(const uint8_t *src_dev, int64_t src_bytes, const int64_t *offsets_dev,
                                                    const int64_t *nbytes_dev, int64_t n_streams, uint8_t *out_dev, int64_t out_bytes,
                                                    const int64_t *out_offsets_dev, const int64_t *out_bytes_dev,
                                                    const int64_t *block_prefix_dev, int64_t n_blocks, int64_t stream_bytes, void *workspace,
                                                    int64_t workspace_bytes, int32_t *status_dev, int32_t *route_dev, void *stream) {
    if (out_bytes < 0) return fail(MSPA_EINVAL, "mspa_snappy_decompress_blocks_device: bad size");
    const int bad = check_blocks_args("mspa_snappy_decompress_blocks_device: bad size, or a workspace that is null, not 16-byte aligned or smaller "
                                      "than mspa_snappy_blocks_workspace_bytes", src_bytes, n_streams, n_blocks, stream_bytes, workspace,
                                      workspace_bytes);
    if (bad) return bad;
    if (n_streams == 0) return MSPA_OK;
    if (!offsets_dev || !nbytes_dev || !out_offsets_dev || !out_bytes_dev || !block_prefix_dev || !status_dev || !route_dev ||
        (src_bytes > 0 && !src_dev) || (out_bytes > 0 && !out_dev))
        return fail(MSPA_EINVAL, "mspa_snappy_decompress_blocks_device: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const snappy::BlocksWorkspace w = snappy::blocks_workspace(stream_bytes, n_streams, n_blocks);
    uint8_t *ws = (uint8_t *)workspace;
    int64_t *starts = (int64_t *)(ws + w.starts);
    int32_t *serial = (int32_t *)(ws + w.serial);
    const int rc = enqueue_block_scan("mspa_snappy_decompress_blocks_device", src_dev, src_bytes, offsets_dev, nbytes_dev, n_streams, out_bytes,
                                      out_offsets_dev, out_bytes_dev, block_prefix_dev, n_blocks, 2, stream_bytes, ws, w, starts, st);
    if (rc) return rc;
    if (n_blocks > 0)
        hipLaunchKernelGGL(snappy::decompress_blocks_kernel, dim3((unsigned)n_blocks), dim3(64), 0, st, src_dev, offsets_dev, nbytes_dev, n_streams,
                           block_prefix_dev, out_dev, out_offsets_dev, out_bytes_dev, (const int64_t *)starts, n_blocks + n_streams, serial);
    hipLaunchKernelGGL(snappy::decompress_flagged_kernel, dim3((unsigned)n_streams), dim3(64), 0, st, src_dev, src_bytes, offsets_dev, nbytes_dev,
                       out_dev, out_bytes, out_offsets_dev, out_bytes_dev, status_dev, (const int32_t *)serial, block_prefix_dev, route_dev);
    return check_hip(hipGetLastError(), "mspa_snappy_decompress_blocks_device");
}

extern "C" int mspa_parquet_plain_spans_device(const uint8_t *pages_dev, int64_t pages_bytes, const int64_t *page_offsets_dev,
                                               const int64_t *page_bytes_dev, const int64_t *page_values_dev, int64_t n_pages,
                                               int32_t has_levels, const int64_t *row_begin_dev, const int64_t *row_index_dev, int64_t n_rows,
                                               int64_t *out_start_dev, int64_t *out_len_dev, int32_t *page_status_dev, void *stream) {
    if (pages_bytes < 0 || n_pages < 0 || n_rows < 0 || n_pages > (int64_t)0x7fffffff * 64 || (has_levels != 0 && has_levels != 1))
        return fail(MSPA_EINVAL, "mspa_parquet_plain_spans_device: bad size");
    if (n_pages == 0) return n_rows == 0 ? MSPA_OK : fail(MSPA_EINVAL, "mspa_parquet_plain_spans_device: rows without pages");
    if (!page_offsets_dev || !page_bytes_dev || !page_values_dev || !row_begin_dev || !page_status_dev || (pages_bytes > 0 && !pages_dev) ||
        (n_rows > 0 && (!row_index_dev || !out_start_dev || !out_len_dev)))
        return fail(MSPA_EINVAL, "mspa_parquet_plain_spans_device: null pointer");
    hipLaunchKernelGGL(snappy::plain_spans_kernel, dim3((unsigned)((n_pages + 63) / 64)), dim3(64), 0, (hipStream_t)stream, pages_dev, pages_bytes,
                       page_offsets_dev, page_bytes_dev, page_values_dev, n_pages, has_levels, row_begin_dev, row_index_dev, n_rows, out_start_dev,
                       out_len_dev, page_status_dev);
    return check_hip(hipGetLastError(), "mspa_parquet_plain_spans_device");
}

extern "C" int mspa_index_rows_brackets_device(const uint8_t *pages_dev, int64_t pages_bytes, const int64_t *start_dev, const int64_t *len_dev,
                                               int64_t n_rows, int64_t *out_inner_start_dev, int64_t *out_inner_len_dev, int32_t *row_status_dev,
                                               void *stream) {
    if (pages_bytes < 0 || n_rows < 0 || n_rows > (int64_t)0x7fffffff * 64) return fail(MSPA_EINVAL, "mspa_index_rows_brackets_device: bad size");
    if (n_rows == 0) return MSPA_OK;
    if (!start_dev || !len_dev || !out_inner_start_dev || !out_inner_len_dev || !row_status_dev || (pages_bytes > 0 && !pages_dev))
        return fail(MSPA_EINVAL, "mspa_index_rows_brackets_device: null pointer");
    hipLaunchKernelGGL(snappy::row_brackets_kernel, dim3((unsigned)((n_rows + 63) / 64)), dim3(64), 0, (hipStream_t)stream, pages_dev, pages_bytes,
                       start_dev, len_dev, n_rows, out_inner_start_dev, out_inner_len_dev, row_status_dev);
    return check_hip(hipGetLastError(), "mspa_index_rows_brackets_device");
}

extern "C" int mspa_index_rows_gather_device(const uint8_t *pages_dev, int64_t pages_bytes, const int64_t *inner_start_dev,
                                             const int64_t *inner_prefix_dev, int64_t n_rows, uint8_t *out_text_dev, int64_t text_bytes,
                                             void *stream) {
    if (pages_bytes < 0 || n_rows < 0 || text_bytes < 0 || text_bytes > 0x7fffffffLL)
        return fail(MSPA_EINVAL, "mspa_index_rows_gather_device: bad size (less than 2 GiB of text a call)");
    if (text_bytes == 0) return MSPA_OK;
    if (n_rows == 0) return fail(MSPA_EINVAL, "mspa_index_rows_gather_device: text without rows");
    if (!pages_dev || !inner_start_dev || !inner_prefix_dev || !out_text_dev) return fail(MSPA_EINVAL, "mspa_index_rows_gather_device: null pointer");
    hipLaunchKernelGGL(snappy::row_gather_kernel, dim3((unsigned)((text_bytes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pages_dev,
                       pages_bytes, inner_start_dev, inner_prefix_dev, n_rows, text_bytes, out_text_dev);
    return check_hip(hipGetLastError(), "mspa_index_rows_gather_device");
}

extern "C" int mspa_index_lists_to_bits_device(const int32_t *values_dev, int64_t n_values, const int64_t *offsets_dev, int64_t n_rows,
                                               int64_t n_points, uint64_t *out_bits_dev, int64_t n_words, int32_t *row_status_dev, void *stream) {
    if (n_values < 0 || n_rows < 0 || n_points < 0 || n_words < 0 || n_values > (int64_t)0x7fffffff * 256 || n_points > 64 * n_words ||
        (n_words > 0 && n_rows > ((int64_t)1 << 40) / n_words))
        return fail(MSPA_EINVAL, "mspa_index_lists_to_bits_device: bad size (n_points <= 64 n_words)");
    if (n_rows == 0) return n_values == 0 ? MSPA_OK : fail(MSPA_EINVAL, "mspa_index_lists_to_bits_device: values without rows");
    if (!offsets_dev || !row_status_dev || (n_values > 0 && !values_dev) || (n_words > 0 && !out_bits_dev))
        return fail(MSPA_EINVAL, "mspa_index_lists_to_bits_device: null pointer");
    hipStream_t st = (hipStream_t)stream;
    int rc = check_hip(hipMemsetAsync(row_status_dev, 0, (size_t)n_rows * 4, st), "mspa_index_lists_to_bits_device: clearing the status");
    if (rc == MSPA_OK && n_words > 0)
        rc = check_hip(hipMemsetAsync(out_bits_dev, 0, (size_t)n_rows * (size_t)n_words * 8, st), "mspa_index_lists_to_bits_device: clearing the rows");
    if (rc) return rc;
    if (n_values > 0)
        hipLaunchKernelGGL(snappy::lists_to_bits_kernel, dim3((unsigned)((n_values + 255) / 256)), dim3(256), 0, st, values_dev, n_values, offsets_dev,
                           n_rows, n_points, out_bits_dev, n_words, row_status_dev);
    return check_hip(hipGetLastError(), "mspa_index_lists_to_bits_device");
}
