// The intersection over union of upright boxes ON the MI355X, as pairs and as matrices, with the host twin's bits and the same bits on
// every run.  The rule, its window and its forward-error bound are csrc/upright_iou_core.h; this file holds the one kernel, the host
// twin's entry point and the C ABI.
//
//   upright_iou_kernel   one lane per output element, workgroups of 128.  operands_of turns the element's index into the rows of a
//     and b it reads, for both launch shapes (pairs are G = P matrices of 1 x 1, with either side possibly a single box).  The
//     polygon of the clipping (at most 8 vertices, two copies used in turn) lives in a per-lane slice of LDS, vertex i of a lane at
//     [i][lane]: a vertex array indexed at run time in registers would go to scratch.  32 KiB of LDS per workgroup; no barrier, no
//     atomic, no lane reads another lane's slice.
#include "mspa_common.h"
#include "upright_iou_core.h"

namespace mspa {
namespace uiou {

constexpr int kIouBlock = 128;

__global__ void __launch_bounds__(kIouBlock) upright_iou_kernel(const double *__restrict__ a, const double *__restrict__ b, int64_t outputs, int64_t A,
                                                                int64_t B, int a_one, int b_one, double *__restrict__ out,
                                                                double *__restrict__ parts) {
    __shared__ double poly[4][kMaxVertices][kIouBlock];          // x0, y0, x1, y1
    const int tid = (int)threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * kIouBlock + tid;
    if (i >= outputs) return;
    int64_t ia, ib;
    operands_of(i, A, B, a_one != 0, b_one != 0, ia, ib);
    const Result r = pair_iou(a + ia * kBoxValues, b + ib * kBoxValues, &poly[0][0][tid], &poly[1][0][tid], &poly[2][0][tid], &poly[3][0][tid],
                              kIouBlock);
    out[i] = r.iou;
    if (parts) {
        parts[2 * i] = r.area;
        parts[2 * i + 1] = r.dz;
    }
}

bool misaligned8(const void *p) { return ((uintptr_t)p & 7u) != 0; }

// The checks both entry points share: the shape, or outputs < 0 with the error text set.
Shape checked_shape(const char *who, const void *a, int64_t Pa, const void *b, int64_t Pb, int64_t G, int64_t A, int64_t B, int32_t mode,
                    const void *out, const void *parts) {
    Shape sh = shape_of(Pa, Pb, G, A, B, mode);
    if (sh.outputs < 0) {
        fail(MSPA_EINVAL, std::string(who) + ": counts must be non-negative and fit the mode (pairs: Pa == Pb or one of them 1, G = A = B = 0; "
                                             "matrix: Pa == G * A, Pb == G * B), with at most 2^31 outputs");
        return sh;
    }
    if ((Pa > 0 && !a) || (Pb > 0 && !b) || (sh.outputs > 0 && !out)) {
        fail(MSPA_EINVAL, std::string(who) + ": null pointer");
        sh.outputs = -1;
        return sh;
    }
    if (misaligned8(a) || misaligned8(b) || misaligned8(out) || misaligned8(parts)) {
        fail(MSPA_EINVAL, std::string(who) + ": a buffer is not aligned to its element");
        sh.outputs = -1;
    }
    return sh;
}

}  // namespace uiou
}  // namespace mspa

using namespace mspa;

extern "C" int mspa_upright_iou_device(const double *a_dev, int64_t Pa, const double *b_dev, int64_t Pb, int64_t G, int64_t A, int64_t B, int32_t mode,
                                       double *out_dev, double *parts_dev, void *stream) {
    const char *who = "mspa_upright_iou_device";
    const uiou::Shape sh = uiou::checked_shape(who, a_dev, Pa, b_dev, Pb, G, A, B, mode, out_dev, parts_dev);
    if (sh.outputs < 0) return MSPA_EINVAL;
    if (sh.outputs == 0) return MSPA_OK;
    const unsigned blocks = (unsigned)((sh.outputs + uiou::kIouBlock - 1) / uiou::kIouBlock);
    hipLaunchKernelGGL(uiou::upright_iou_kernel, dim3(blocks), dim3(uiou::kIouBlock), 0, (hipStream_t)stream, a_dev, b_dev, sh.outputs, sh.A, sh.B,
                       sh.a_one ? 1 : 0, sh.b_one ? 1 : 0, out_dev, parts_dev);
    return check_hip(hipGetLastError(), who);
}

extern "C" int mspa_upright_iou_host(const double *a_host, int64_t Pa, const double *b_host, int64_t Pb, int64_t G, int64_t A, int64_t B, int32_t mode,
                                     double *out_host, double *parts_host) {
    const char *who = "mspa_upright_iou_host";
    const uiou::Shape sh = uiou::checked_shape(who, a_host, Pa, b_host, Pb, G, A, B, mode, out_host, parts_host);
    if (sh.outputs < 0) return MSPA_EINVAL;
    uiou::iou_all(a_host, b_host, sh, out_host, parts_host);
    return MSPA_OK;
}

extern "C" int mspa_upright_iou_bound_host(const double *a_host, const double *b_host, int64_t P, double *area_bound_out, double *iou_bound_out) {
    const char *who = "mspa_upright_iou_bound_host";
    if (P < 0 || P > uiou::kMaxOutputs) return fail(MSPA_EINVAL, std::string(who) + ": P must be between 0 and 2^31");
    if (P > 0 && (!a_host || !b_host || !area_bound_out || !iou_bound_out)) return fail(MSPA_EINVAL, std::string(who) + ": null pointer");
    for (int64_t i = 0; i < P; ++i)
        uiou::pair_bounds(a_host + i * uiou::kBoxValues, b_host + i * uiou::kBoxValues, area_bound_out[i], iou_bound_out[i]);
    return MSPA_OK;
}
