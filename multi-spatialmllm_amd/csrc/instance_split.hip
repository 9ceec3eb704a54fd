// Per-object point clouds of a batch of frames in ONE pass: the stable split of every frame's valid pixels by instance label.
//
// What it replaces: the reference builds an object's cloud per (image, object) -- `np.where(mask_image == target_id + 1)`
// (info_handler.py get_instance_mask), then project_mask_to_3d over that mask (ops.py:235-329) -- so a frame with 30 objects is
// decoded and back-projected 30 times.  Here K3 exact runs once per frame (xyz_f64 + valid_u8 of every pixel) and these kernels
// sort the valid pixels' rows into (frame, label) segments, each in ascending pixel index: the rows `project_mask_to_3d`
// returns for that object's mask, in its order.  The rule and the decomposition are stated in csrc/instance_split_core.h.
//
//   split_count_kernel    one workgroup per tile of 4 096 pixels: histogram of the selected pixels' labels (LDS integer atomics:
//                         a count does not depend on arrival order) -> workspace [F, tiles, 256].
//   split_scan_kernel     one workgroup per frame, thread v = label v: exclusive scan of the tile histograms over the tiles (in
//                         place: the workspace then holds tile bases) and the segment sizes counts [F, 256].
//   split_scatter_kernel  one workgroup per tile, 16 rounds of 256 pixels.  A wave ranks its lanes per distinct label with ballots
//                         (a loop over the labels present in the wave, leader by leader: at most 64 turns, a handful for real
//                         masks), the waves' per-label counts of the round meet in LDS, a running per-label position carries from
//                         round to round.  No atomic takes part in placing a row.
//   split_extents_kernel  one workgroup per segment: min / max of its rows (pure selection; an empty segment gets +inf / -inf).
#include "mspa_common.h"
#include "instance_split_core.h"

namespace mspa {
namespace split {

__global__ __launch_bounds__(kBlock) void split_count_kernel(const uint8_t *__restrict__ labels, const uint8_t *__restrict__ valid, int64_t P,
                                                             int64_t T, int32_t *__restrict__ work) {
    __shared__ int32_t hist[kLabels];
    const int tid = (int)threadIdx.x;
    const int64_t tile = blockIdx.x, f = blockIdx.y;
    hist[tid] = 0;
    __syncthreads();
    for (int r = 0; r < kRounds; ++r) {
        const int64_t p = tile * kTile + (int64_t)r * kBlock + tid;
        if (p < P) {
            const uint8_t l = labels[f * P + p];
            if (selected(l, valid[f * P + p])) atomicAdd(&hist[l], 1);
        }
    }
    __syncthreads();
    work[(f * T + tile) * kLabels + tid] = hist[tid];
}

__global__ __launch_bounds__(kLabels) void split_scan_kernel(int64_t T, int32_t *__restrict__ work, int32_t *__restrict__ counts) {
    const int v = (int)threadIdx.x;
    const int64_t f = blockIdx.x;
    int32_t run = 0;
    for (int64_t t = 0; t < T; ++t) {
        const int64_t at = (f * T + t) * kLabels + v;
        const int32_t n = work[at];
        work[at] = run;
        run += n;
    }
    counts[f * kLabels + v] = run;
}

__global__ __launch_bounds__(kBlock) void split_scatter_kernel(const uint8_t *__restrict__ labels, const uint8_t *__restrict__ valid,
                                                               const double *__restrict__ xyz, const uint8_t *__restrict__ rgb, int64_t P,
                                                               int64_t T, const int64_t *__restrict__ offsets, const int32_t *__restrict__ work,
                                                               double *__restrict__ out_xyz, uint8_t *__restrict__ out_rgb,
                                                               int32_t *__restrict__ out_pixel) {
    __shared__ int64_t run[kLabels];                             // next row of every label's segment, at the start of the round
    __shared__ int32_t wcnt[kWaves][kLabels];                    // the round's selected pixels per wave and label
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t tile = blockIdx.x, f = blockIdx.y;
    run[tid] = offsets[f * kLabels + tid] + work[(f * T + tile) * kLabels + tid];
#pragma unroll
    for (int e = 0; e < kWaves; ++e) wcnt[e][tid] = 0;
    __syncthreads();
    for (int r = 0; r < kRounds; ++r) {
        const int64_t p0 = tile * kTile + (int64_t)r * kBlock;
        if (p0 >= P) break;                                      // (the whole workgroup: the rounds left hold no pixel)
        const int64_t p = p0 + tid;
        const bool in = p < P;
        const int l = in ? (int)labels[f * P + p] : 0;
        const bool sel = in && selected((uint8_t)l, valid[f * P + p]);
        double x = 0.0, y = 0.0, z = 0.0;
        if (sel) {                                               // on their way while the wave ranks its lanes
            const double *q = xyz + (f * P + p) * 3;
            x = q[0]; y = q[1]; z = q[2];
        }
        int rank = 0;
        uint64_t todo = __ballot(sel);
        while (todo) {                                           // wave-uniform: one turn per distinct label of the wave
            const int leader = __builtin_ctzll(todo);
            const int v = __builtin_amdgcn_readlane(l, leader);
            const bool mine = sel && l == v;
            const uint64_t m = __ballot(mine);
            if (mine) rank = rank_below(m, lane);
            if (lane == leader) wcnt[w][v] = __popcll(m);
            todo &= ~m;
        }
        __syncthreads();
        if (sel) {
            int64_t row = run[l] + rank;
#pragma unroll
            for (int e = 0; e < kWaves - 1; ++e) row += e < w ? wcnt[e][l] : 0;
            double *o = out_xyz + row * 3;
            o[0] = x; o[1] = y; o[2] = z;
            if (out_rgb) {
                const uint8_t *c = rgb + (f * P + p) * 3;
                uint8_t *oc = out_rgb + row * 3;
                oc[0] = c[0]; oc[1] = c[1]; oc[2] = c[2];
            }
            out_pixel[row] = (int32_t)p;
        }
        __syncthreads();
        {
            int32_t s = 0;
#pragma unroll
            for (int e = 0; e < kWaves; ++e) { s += wcnt[e][tid]; wcnt[e][tid] = 0; }
            run[tid] += s;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kBlock) void split_extents_kernel(const int64_t *__restrict__ offsets, const double *__restrict__ rows,
                                                               double *__restrict__ out_lo, double *__restrict__ out_hi) {
    __shared__ double part[kWaves][6];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t seg = blockIdx.x;
    const int64_t beg = offsets[seg] * 3, n = (offsets[seg + 1] - offsets[seg]) * 3;
    const double inf = __builtin_inf();
    double lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    for (int64_t j = tid; j < n; j += kBlock) {
        const double c = rows[beg + j];
        const int k = (int)(j % 3);
#pragma unroll
        for (int a = 0; a < 3; ++a)
            if (k == a) { lo[a] = c < lo[a] ? c : lo[a]; hi[a] = c > hi[a] ? c : hi[a]; }
    }
    if (n > 0) {                                                 // (uniform per workgroup)
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) {
                const double ol = __shfl_xor(lo[a], s, 64), oh = __shfl_xor(hi[a], s, 64);
                lo[a] = ol < lo[a] ? ol : lo[a];
                hi[a] = oh > hi[a] ? oh : hi[a];
            }
        if (lane == 0) {
#pragma unroll
            for (int a = 0; a < 3; ++a) { part[w][a] = lo[a]; part[w][3 + a] = hi[a]; }
        }
        __syncthreads();
        if (tid < 3) {
            double l = part[0][tid], h = part[0][3 + tid];
#pragma unroll
            for (int e = 1; e < kWaves; ++e) {
                l = part[e][tid] < l ? part[e][tid] : l;
                h = part[e][3 + tid] > h ? part[e][3 + tid] : h;
            }
            lo[0] = l; hi[0] = h;
        }
    }
    if (tid < 3) {
        out_lo[seg * 3 + tid] = n > 0 ? lo[0] : inf;
        out_hi[seg * 3 + tid] = n > 0 ? hi[0] : -inf;
    }
}

}  // namespace split
}  // namespace mspa

using namespace mspa;

static int split_sizes_ok(int64_t F, int64_t P) { return F >= 0 && P >= 0 && F <= 65535 && P <= 0x7fffffffll; }

extern "C" int64_t mspa_instance_split_workspace_bytes(int64_t F, int64_t P) {
    if (!split_sizes_ok(F, P)) return -1;
    const int64_t b = split::workspace_words(F, P) * 4;
    return b < 16 ? 16 : b;
}

extern "C" int mspa_instance_split_count(const uint8_t *labels, const uint8_t *valid, int64_t F, int64_t P, int32_t *out_counts,
                                         void *workspace, int64_t workspace_bytes, mspa_stream_t stream) {
    if (!split_sizes_ok(F, P)) return fail(MSPA_EINVAL, "mspa_instance_split_count: bad size (F <= 65535 frames of P < 2^31 pixels)");
    if (F == 0) return MSPA_OK;
    if (!out_counts || !workspace || (P > 0 && (!labels || !valid))) return fail(MSPA_EINVAL, "mspa_instance_split_count: null pointer");
    if (workspace_bytes < mspa_instance_split_workspace_bytes(F, P) || ((uintptr_t)workspace & 3u))
        return fail(MSPA_EINVAL, "mspa_instance_split_count: workspace smaller than mspa_instance_split_workspace_bytes or misaligned");
    const int64_t T = split::tiles(P);
    hipStream_t st = (hipStream_t)stream;
    if (T > 0)
        hipLaunchKernelGGL(split::split_count_kernel, dim3((unsigned)T, (unsigned)F), dim3(split::kBlock), 0, st, labels, valid, P, T,
                           (int32_t *)workspace);
    hipLaunchKernelGGL(split::split_scan_kernel, dim3((unsigned)F), dim3(split::kLabels), 0, st, T, (int32_t *)workspace, out_counts);
    return check_hip(hipGetLastError(), "mspa_instance_split_count");
}

extern "C" int mspa_instance_split_scatter(const uint8_t *labels, const uint8_t *valid, const double *xyz_f64, const uint8_t *rgb_or_null,
                                           int64_t F, int64_t P, int32_t H, int32_t W, const int64_t *offsets, const void *workspace,
                                           double *out_xyz, uint8_t *out_rgb, int32_t *out_pixel, double *out_lo, double *out_hi,
                                           mspa_stream_t stream) {
    if (!split_sizes_ok(F, P) || H < 0 || W < 0 || (int64_t)H * W != P)
        return fail(MSPA_EINVAL, "mspa_instance_split_scatter: bad size (F <= 65535 frames of P = H * W < 2^31 pixels)");
    if (F == 0) return MSPA_OK;
    if (!offsets || !workspace || !out_lo || !out_hi || (P > 0 && (!labels || !valid || !xyz_f64 || !out_xyz || !out_pixel)))
        return fail(MSPA_EINVAL, "mspa_instance_split_scatter: null pointer");
    if ((rgb_or_null == nullptr) != (out_rgb == nullptr))
        return fail(MSPA_EINVAL, "mspa_instance_split_scatter: rgb and out_rgb go together");
    const int64_t T = split::tiles(P);
    hipStream_t st = (hipStream_t)stream;
    if (T > 0)
        hipLaunchKernelGGL(split::split_scatter_kernel, dim3((unsigned)T, (unsigned)F), dim3(split::kBlock), 0, st, labels, valid, xyz_f64,
                           rgb_or_null, P, T, offsets, (const int32_t *)workspace, out_xyz, out_rgb, out_pixel);
    hipLaunchKernelGGL(split::split_extents_kernel, dim3((unsigned)(F * split::kLabels)), dim3(split::kBlock), 0, st, offsets,
                       (const double *)out_xyz, out_lo, out_hi);
    return check_hip(hipGetLastError(), "mspa_instance_split_scatter");
}

extern "C" int mspa_instance_split_host(const uint8_t *labels, const uint8_t *valid, const double *xyz_f64, const uint8_t *rgb_or_null,
                                        int64_t F, int64_t P, int32_t *out_counts, int64_t *out_offsets, int32_t *workspace,
                                        double *out_xyz, uint8_t *out_rgb, int32_t *out_pixel, double *out_lo, double *out_hi,
                                        int32_t reversed) {
    if (!split_sizes_ok(F, P)) return fail(MSPA_EINVAL, "mspa_instance_split_host: bad size");
    if (!out_counts || !out_offsets || !workspace || (P > 0 && F > 0 && (!labels || !valid)))
        return fail(MSPA_EINVAL, "mspa_instance_split_host: null pointer");
    split::count_host(labels, valid, F, P, out_counts, workspace);
    out_offsets[0] = 0;
    for (int64_t s = 0; s < F * split::kLabels; ++s) out_offsets[s + 1] = out_offsets[s] + out_counts[s];
    if (!out_xyz) return MSPA_OK;                                 // the size-only first call
    if (!xyz_f64 || !out_pixel || !out_lo || !out_hi || ((rgb_or_null == nullptr) != (out_rgb == nullptr)))
        return fail(MSPA_EINVAL, "mspa_instance_split_host: null pointer");
    split::scatter_host(labels, valid, xyz_f64, rgb_or_null, F, P, out_offsets, workspace, out_xyz, out_rgb, out_pixel, out_lo, out_hi,
                        reversed != 0);
    return MSPA_OK;
}
