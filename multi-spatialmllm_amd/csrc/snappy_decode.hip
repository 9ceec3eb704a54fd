// The Snappy decoder of the visibility index's `values` pages, ON the MI355X: the first half of the way back from a column chunk's
// pages to the image_to_points rows' bitsets (csrc/index_rows.hip is the other half; csrc/parquet_pages.hip wrote the pages).
// Every status code and every accepted stream is defined by csrc/snappy_core.h, whose decompress() on the host is the reference.
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
// No atomics; every load and store is checked against the buffer it goes to.
#include "mspa_common.h"
#include "snappy_core.h"

namespace mspa {
namespace snappy {

constexpr int kRing = 32768;
constexpr uint32_t kRingMask = kRing - 1;

// FLAGGED = false: every stream of the table is decoded; the last three parameters are unused.  FLAGGED = true: the block route's
// last pass, over the same stream table.  `serial`: the per-stream flags of the passes in front -- a stream whose flag is 0 was
// decoded by its blocks' waves and only gets its status and its route here; a flagged one is decoded from scratch.
template <bool FLAGGED>
__global__ __launch_bounds__(64) void decompress_kernel(const uint8_t *__restrict__ src, int64_t src_bytes,
                                                        const int64_t *__restrict__ offsets, const int64_t *__restrict__ nbytes,
                                                        uint8_t *out, int64_t out_bytes, const int64_t *__restrict__ out_offsets,
                                                        const int64_t *__restrict__ out_sizes, int32_t *__restrict__ status,
                                                        const int32_t *__restrict__ serial, const int64_t *__restrict__ block_prefix,
                                                        int32_t *__restrict__ route) {
    __shared__ uint8_t ring[kRing];
    const int lane = (int)threadIdx.x;
    const int64_t s = blockIdx.x;
    if constexpr (FLAGGED) {
        const bool by_blocks = serial[s] == 0;
        if (lane == 0) route[s] = by_blocks ? (int32_t)(block_prefix[s + 1] - block_prefix[s]) : 0;
        if (by_blocks) {
            if (lane == 0) status[s] = 0;
            return;
        }
    }
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
//   (serial)     decompress_kernel<true> over the same stream table: flagged streams from scratch, the others get status 0.
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
    return last_at_or_below(n_streams, g, [prefix](int64_t s) { return seg_base(prefix, s); });
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
    const int64_t s = last_at_or_below(block_prefix, n_streams, b);      // block b's stream (streams without blocks share their successor's entry)
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

}  // namespace snappy
}  // namespace mspa

using namespace mspa;

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
    hipLaunchKernelGGL(snappy::decompress_kernel<false>, dim3((unsigned)n_streams), dim3(64), 0, (hipStream_t)stream, src_dev, src_bytes,
                       offsets_dev, nbytes_dev, out_dev, out_bytes, out_offsets_dev, out_bytes_dev, status_dev, nullptr, nullptr, nullptr);
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

// The sizes and the workspace of entry point `name`'s call; `w`: the workspace's layout, computed here once (untouched when n_streams == 0).
static int check_blocks_args(const char *name, int64_t src_bytes, int64_t n_streams, int64_t n_blocks, int64_t stream_bytes, const void *workspace,
                             int64_t workspace_bytes, snappy::BlocksWorkspace &w) {
    const std::string what = std::string(name) + ": bad size, or a workspace that is null, not 16-byte aligned or smaller than "
                                                 "mspa_snappy_blocks_workspace_bytes";
    if (src_bytes < 0 || n_streams < 0 || n_streams > 0x7fffffffLL || n_blocks < 0 || n_blocks > 0x7fffffffLL || stream_bytes < 0 ||
        stream_bytes > ((int64_t)1 << 40) || workspace_bytes < 0)
        return fail(MSPA_EINVAL, what);
    if (n_streams == 0) return MSPA_OK;
    w = snappy::blocks_workspace(stream_bytes, n_streams, n_blocks);
    if (w.seg_slots > 0x7fffffffLL) return fail(MSPA_EINVAL, what);
    if (!workspace || ((uintptr_t)workspace & 15) != 0 || workspace_bytes < w.total) return fail(MSPA_EINVAL, what);
    return MSPA_OK;
}

extern "C" int mspa_snappy_block_starts_device(const uint8_t *src_dev, int64_t src_bytes, const int64_t *offsets_dev, const int64_t *nbytes_dev,
                                               int64_t n_streams, const int64_t *out_bytes_dev, const int64_t *block_prefix_dev, int64_t n_blocks,
                                               int64_t stream_bytes, void *workspace, int64_t workspace_bytes, int64_t *starts_dev,
                                               int32_t *route_dev, void *stream) {
    snappy::BlocksWorkspace w;
    const int bad = check_blocks_args("mspa_snappy_block_starts_device", src_bytes, n_streams, n_blocks, stream_bytes, workspace, workspace_bytes, w);
    if (bad) return bad;
    if (n_streams == 0) return MSPA_OK;
    if (!offsets_dev || !nbytes_dev || !out_bytes_dev || !block_prefix_dev || !starts_dev || !route_dev || (src_bytes > 0 && !src_dev))
        return fail(MSPA_EINVAL, "mspa_snappy_block_starts_device: null pointer");
    hipStream_t st = (hipStream_t)stream;
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
    snappy::BlocksWorkspace w;
    const int bad = check_blocks_args("mspa_snappy_decompress_blocks_device", src_bytes, n_streams, n_blocks, stream_bytes, workspace,
                                      workspace_bytes, w);
    if (bad) return bad;
    if (n_streams == 0) return MSPA_OK;
    if (!offsets_dev || !nbytes_dev || !out_offsets_dev || !out_bytes_dev || !block_prefix_dev || !status_dev || !route_dev ||
        (src_bytes > 0 && !src_dev) || (out_bytes > 0 && !out_dev))
        return fail(MSPA_EINVAL, "mspa_snappy_decompress_blocks_device: null pointer");
    hipStream_t st = (hipStream_t)stream;
    uint8_t *ws = (uint8_t *)workspace;
    int64_t *starts = (int64_t *)(ws + w.starts);
    int32_t *serial = (int32_t *)(ws + w.serial);
    const int rc = enqueue_block_scan("mspa_snappy_decompress_blocks_device", src_dev, src_bytes, offsets_dev, nbytes_dev, n_streams, out_bytes,
                                      out_offsets_dev, out_bytes_dev, block_prefix_dev, n_blocks, 2, stream_bytes, ws, w, starts, st);
    if (rc) return rc;
    if (n_blocks > 0)
        hipLaunchKernelGGL(snappy::decompress_blocks_kernel, dim3((unsigned)n_blocks), dim3(64), 0, st, src_dev, offsets_dev, nbytes_dev, n_streams,
                           block_prefix_dev, out_dev, out_offsets_dev, out_bytes_dev, (const int64_t *)starts, n_blocks + n_streams, serial);
    hipLaunchKernelGGL(snappy::decompress_kernel<true>, dim3((unsigned)n_streams), dim3(64), 0, st, src_dev, src_bytes, offsets_dev, nbytes_dev,
                       out_dev, out_bytes, out_offsets_dev, out_bytes_dev, status_dev, (const int32_t *)serial, block_prefix_dev, route_dev);
    return check_hip(hipGetLastError(), "mspa_snappy_decompress_blocks_device");
}
