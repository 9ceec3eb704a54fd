// K7b: average linkage + fcluster of a batch of K7 matrices (rigid_body_segmentation, OM_C:80-92), identical to SciPy.
// The arithmetic and every tie rule live in linkage_core.h, which also builds with a plain C++ compiler; this file supplies the
// device team: one workgroup of 256 lanes per matrix, the matrices of a batch in parallel across the CUs.
//
// The chain of merges is sequential, and stays so inside its workgroup: the lanes share each nearest-neighbour scan (a strided
// pass over one row of the working matrix, a wave shuffle argmin, one barrier to combine the four waves) and each row update.
// Barriers per matrix: one per scan (below 4 P of them), two per merge (P - 1), five around the sort / relabel / walk tail.
// The relabelling union-find and fcluster's tree walk are serial by nature and run on lane 0, over LDS only.
// The working copy of the matrix lives in the caller's workspace (P * P float64 per matrix; at P = 2048 it would not fit LDS);
// the small state (cluster sizes, the chain, the union-find, the walk's stack) is 6 P int32 of LDS.  Workgroups never talk to
// each other, nothing waits on global memory, and a wrong tie rule ends in a status code after 4 P scans, not in a hang.
#include "mspa_common.h"

#include "linkage_core.h"

namespace mspa {

constexpr int kLinkageThreads = 256;
constexpr int kLinkageWaves = kLinkageThreads / kWave;
static_assert(linkage::kMaxPoints == MSPA_LINKAGE_MAX_POINTS, "header and core disagree on the largest matrix");
static_assert(linkage::kOk == MSPA_LINKAGE_OK && linkage::kNonFinite == MSPA_LINKAGE_NONFINITE &&
              linkage::kIterationCap == MSPA_LINKAGE_ITERATION_CAP, "header and core disagree on the status codes");

// The team of linkage_core.h on the device.  argmin: lowest index among the smallest values; every lane gets the result.
// The per-wave results go through one of two LDS slot sets, alternating, so one barrier per call is enough: a lane that writes
// set s for call r + 2 has passed the barrier of call r + 1, which every lane reaches only after reading set s for call r.
struct TeamCtx {
    int tid, nthr;
    double *slot_v;     // [2][kLinkageWaves]
    int *slot_i;        // [2][kLinkageWaves]
    int turn;

    __device__ __forceinline__ void sync() { __syncthreads(); }

    __device__ __forceinline__ void argmin(double &v, int &i) {
#pragma unroll
        for (int off = kWave / 2; off >= 1; off >>= 1) {
            const double ov = __shfl_down(v, off, kWave);
            const int oi = __shfl_down(i, off, kWave);
            if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
        }
        double *sv = slot_v + turn * kLinkageWaves;
        int *si = slot_i + turn * kLinkageWaves;
        if ((tid & (kWave - 1)) == 0) { sv[tid / kWave] = v; si[tid / kWave] = i; }
        __syncthreads();
        v = sv[0];
        i = si[0];
#pragma unroll
        for (int w = 1; w < kLinkageWaves; ++w) {
            const double ov = sv[w];
            const int oi = si[w];
            if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
        }
        turn ^= 1;
    }

    __device__ __forceinline__ bool any(bool b) {
        double v = b ? 0.0 : 1.0;
        int i = 0;
        argmin(v, i);
        return v == 0.0;
    }
};

__global__ __launch_bounds__(kLinkageThreads) void track_linkage_kernel(const double *loss, int n, double threshold,
                                                                        char *workspace, int64_t scratch_stride, double *Z,
                                                                        int32_t *labels, int32_t *status) {
    extern __shared__ int32_t linkage_shared[];          // linkage::shared_words(n) int32
    __shared__ double slot_v[2 * kLinkageWaves];
    __shared__ int slot_i[2 * kLinkageWaves];
    const int64_t b = blockIdx.x;
    TeamCtx c{(int)threadIdx.x, kLinkageThreads, slot_v, slot_i, 0};
    linkage::block(c, loss + b * n * n, n, threshold, workspace + b * scratch_stride, linkage_shared, Z + b * (n - 1) * 4,
                   labels + b * n, status + b);
}

}  // namespace mspa

using namespace mspa;

extern "C" int64_t mspa_track_linkage_workspace_bytes(int64_t n_blocks, int32_t P) {
    if (n_blocks < 0 || P < 0 || P > linkage::kMaxPoints || n_blocks > 0x7fffffffLL) return -1;
    if (n_blocks == 0 || P < 2) return 0;
    return n_blocks * linkage::scratch_bytes(P);
}

extern "C" int mspa_track_linkage(const double *loss, int64_t n_blocks, int32_t P, double threshold, double *out_Z,
                                  int32_t *out_labels, int32_t *out_status, void *workspace, int64_t workspace_bytes,
                                  mspa_stream_t stream) {
    if (n_blocks < 0 || P < 0 || workspace_bytes < 0) return fail(MSPA_EINVAL, "mspa_track_linkage: bad size");
    if (P > linkage::kMaxPoints) return fail(MSPA_EINVAL, "mspa_track_linkage: more than MSPA_LINKAGE_MAX_POINTS points");
    if (n_blocks > 0x7fffffffLL) return fail(MSPA_EINVAL, "mspa_track_linkage: too many blocks for one launch");
    if (n_blocks == 0 || P < 2) return MSPA_OK;
    if (!loss || !out_Z || !out_labels || !out_status || !workspace) return fail(MSPA_EINVAL, "mspa_track_linkage: null pointer");
    if (workspace_bytes < mspa_track_linkage_workspace_bytes(n_blocks, P))
        return fail(MSPA_EINVAL, "mspa_track_linkage: workspace smaller than mspa_track_linkage_workspace_bytes()");
    if ((uintptr_t)workspace & 15u) return fail(MSPA_EINVAL, "mspa_track_linkage: workspace must be 16-byte aligned");
    hipLaunchKernelGGL(track_linkage_kernel, dim3((uint32_t)n_blocks), dim3(kLinkageThreads),
                       (size_t)linkage::shared_words(P) * sizeof(int32_t), (hipStream_t)stream, loss, (int)P, threshold,
                       (char *)workspace, linkage::scratch_bytes(P), out_Z, out_labels, out_status);
    return check_hip(hipGetLastError(), "track_linkage_kernel launch");
}
