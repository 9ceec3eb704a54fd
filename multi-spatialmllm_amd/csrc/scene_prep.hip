// K11: ScanNet instance data from raw scans (utils/scannet_utils/batch_load_scannet_data.py + scannet_utils.py), batched over scenes.
//
// What it replaces: per scan, a Python loop over every vertex (read_segmentation, SU:38-50), one fancy assignment per segment
// (BL:82-93), np.dot over [N, 4] (BL:66-69) and one boolean pass over ALL vertices per object, twice (extract_bbox, SU:73-92).
// On the device that is a gather through two small per-segment tables, an affine map, a segmented min / max and a stable split.
//
// Every kernel serves MANY scenes with ragged sizes in one launch.  The unit of work is a wave = 64 consecutive vertices of ONE
// scene: word_off[s] (prefix sum of ceil(N_s / 64)) tells a wave its scene by a wave-uniform binary search, vert_off[s] where
// the scene's vertices start in the concatenated arrays.  A wave therefore also owns one 64-bit word of every (scene, object)
// membership row, which is what makes the stable split a plain store:
//   mspa_prep_labels    instance_ids[v] = seg2inst[seg[v]], label index li = seg2label[seg[v]], label_ids[v] = label_value[li]
//   mspa_prep_align     [N, 6] float32 -> [N, 6] float64, xyz through the scene's axis alignment in NumPy's K = 4 order
//   mspa_prep_objects   per distinct object in the wave: a ballot is the object's membership word (-> K9's popcount / expand give
//                       the vertex lists in vertex order), a butterfly over the wave folds count and the 12 extrema, lane 0 adds
//                       them with the native float64 atomic min / max.  Pure selection: bit-exact whatever the atomics' order.
//                       float32 extrema travel as float64 (exact) and are narrowed on the host.
//   mspa_parse_int_list_{flags_,}device   the inverse of K10 (csrc/format_lists.hip): one lane per byte of the JSON text.
// Bandwidth-trivial, latency-bound; nothing here is tuned beyond this first form.
#include "mspa_common.h"

namespace mspa {
namespace prep {

constexpr int kWavesPerBlock = 4;

struct WaveSpan {
    int64_t scene, word, v;          // scene, word within the scene, this lane's vertex in the concatenated arrays
    bool live;
};

__device__ __forceinline__ bool wave_span(const int64_t *__restrict__ vert_off, const int64_t *__restrict__ word_off, int64_t n_scenes,
                                          WaveSpan &w) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (g >= word_off[n_scenes]) return false;
    w.scene = last_at_or_below(word_off, n_scenes, g);             // the wave's scene (scenes without vertices share their successor's offset)
    w.word = g - word_off[w.scene];
    const int64_t local = w.word * 64 + lane;
    w.live = local < vert_off[w.scene + 1] - vert_off[w.scene];
    w.v = vert_off[w.scene] + local;
    return true;
}

__global__ __launch_bounds__(256) void labels_kernel(const int32_t *__restrict__ seg, const int64_t *__restrict__ vert_off,
                                                     const int64_t *__restrict__ word_off, int64_t n_scenes,
                                                     const int64_t *__restrict__ tab_off, const int32_t *__restrict__ seg2inst,
                                                     const int32_t *__restrict__ seg2label, const int64_t *__restrict__ lab_off,
                                                     const uint32_t *__restrict__ label_value, uint32_t *__restrict__ out_inst,
                                                     uint32_t *__restrict__ out_label, int32_t *__restrict__ out_label_idx) {
    WaveSpan w;
    if (!wave_span(vert_off, word_off, n_scenes, w) || !w.live) return;
    const int64_t t0 = tab_off[w.scene], n_tab = tab_off[w.scene + 1] - t0;
    const int64_t l0 = lab_off[w.scene], n_lab = lab_off[w.scene + 1] - l0;
    const int32_t s = seg[w.v];
    int32_t inst = 0, li = 0;
    if (s >= 0 && s < n_tab) {                   // a segment beyond the table is one no object lists
        inst = seg2inst[t0 + s];
        li = seg2label[t0 + s];
    }
    if (li < 0 || li >= n_lab) li = 0;           // the tables are the caller's: never index outside label_value
    out_inst[w.v] = (uint32_t)inst;
    out_label_idx[w.v] = li;
    out_label[w.v] = n_lab > 0 ? label_value[l0 + li] : 0u;
}

__global__ __launch_bounds__(256) void align_kernel(const float *__restrict__ verts, const int64_t *__restrict__ vert_off,
                                                    const int64_t *__restrict__ word_off, int64_t n_scenes,
                                                    const double *__restrict__ mats, double *__restrict__ out) {
    WaveSpan w;
    if (!wave_span(vert_off, word_off, n_scenes, w) || !w.live) return;
    const double *__restrict__ m = mats + 16 * w.scene;          // wave-uniform: scalar loads
    const float *__restrict__ p = verts + 6 * w.v;
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    double *__restrict__ o = out + 6 * w.v;
    if (vert_off[w.scene + 1] - vert_off[w.scene] == 1) {
        // a scene of ONE vertex: np.dot hands a [1, 4] operand to BLAS as a vector (gemv, not gemm), whose kernel rounds the four
        // products on their own and adds them as (k0 + k2) + (k1 + k3).  -ffp-contract=off keeps this as written.
        for (int r = 0; r < 3; ++r) o[r] = (m[4 * r + 0] * x + m[4 * r + 2] * z) + (m[4 * r + 1] * y + m[4 * r + 3]);
    } else {
        o[0] = affine_row_w(m + 0, x, y, z, 1.0);
        o[1] = affine_row_w(m + 4, x, y, z, 1.0);
        o[2] = affine_row_w(m + 8, x, y, z, 1.0);
    }
    o[3] = (double)p[3];
    o[4] = (double)p[4];
    o[5] = (double)p[5];
}

__global__ __launch_bounds__(256) void objects_init_kernel(double *__restrict__ lo_un, double *__restrict__ hi_un,
                                                           double *__restrict__ lo_al, double *__restrict__ hi_al,
                                                           int32_t *__restrict__ count, int64_t n_slots, int32_t *__restrict__ zero_count,
                                                           int64_t n_scenes) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const double inf = __builtin_inf();
    if (k < n_slots) {
        for (int c = 0; c < 3; ++c) {
            lo_un[3 * k + c] = inf; hi_un[3 * k + c] = -inf;
            lo_al[3 * k + c] = inf; hi_al[3 * k + c] = -inf;
        }
        count[k] = 0;
    }
    if (k < n_scenes) zero_count[k] = 0;
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(256) void objects_kernel(const uint32_t *__restrict__ inst, const float *__restrict__ verts,
                                                      const double *__restrict__ aligned, const int64_t *__restrict__ vert_off,
                                                      const int64_t *__restrict__ word_off, int64_t n_scenes,
                                                      const int64_t *__restrict__ obj_off, uint64_t *__restrict__ bits, int64_t n_words,
                                                      int32_t *__restrict__ count, double *__restrict__ lo_un, double *__restrict__ hi_un,
                                                      double *__restrict__ lo_al, double *__restrict__ hi_al,
                                                      int32_t *__restrict__ zero_count) {
    WaveSpan w;
    if (!wave_span(vert_off, word_off, n_scenes, w)) return;
    const int lane = threadIdx.x & 63;
    const int64_t o0 = obj_off[w.scene], n_obj = obj_off[w.scene + 1] - o0;
    const uint32_t k = w.live ? inst[w.v] : 0u;
    const double inf = __builtin_inf();
    double u[3] = {0.0, 0.0, 0.0}, a[3] = {0.0, 0.0, 0.0};
    if (w.live) {
        for (int c = 0; c < 3; ++c) {
            u[c] = (double)verts[6 * w.v + c];
            a[c] = aligned[6 * w.v + c];
        }
    }
    const uint64_t zeros = __ballot(w.live && k == 0u);
    if (lane == 0 && zeros) atomicAdd(zero_count + w.scene, (int32_t)__popcll(zeros));
    uint64_t rem = __ballot(w.live && k >= 1u && (int64_t)k <= n_obj);       // ids beyond the scene's objects are the caller's error: skipped
    while (rem) {                                                            // wave-uniform: one turn per distinct object of these 64 vertices
        const int leader = __ffsll((unsigned long long)rem) - 1;
        const uint32_t kk = (uint32_t)__shfl((int)k, leader, 64);
        const uint64_t m = __ballot(w.live && k == kk) & rem;
        rem &= ~m;
        const bool in = (m >> lane) & 1;
        double mn_u[3], mx_u[3], mn_a[3], mx_a[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            mn_u[c] = wave_min(in ? u[c] : inf);
            mx_u[c] = wave_max(in ? u[c] : -inf);
            mn_a[c] = wave_min(in ? a[c] : inf);
            mx_a[c] = wave_max(in ? a[c] : -inf);
        }
        if (lane == 0) {
            const int64_t r = o0 + (int64_t)kk - 1;
            if (w.word < n_words) bits[r * n_words + w.word] = m;            // this wave alone owns the word
            atomicAdd(count + r, (int32_t)__popcll(m));
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                unsafeAtomicMin(lo_un + 3 * r + c, mn_u[c]);
                unsafeAtomicMax(hi_un + 3 * r + c, mx_u[c]);
                unsafeAtomicMin(lo_al + 3 * r + c, mn_a[c]);
                unsafeAtomicMax(hi_al + 3 * r + c, mx_a[c]);
            }
        }
    }
}

// len(np.unique(instance_ids)) per scene: the objects that own a vertex, plus one for the unannotated id 0 when it occurs
__global__ __launch_bounds__(256) void unique_kernel(const int64_t *__restrict__ obj_off, int64_t n_scenes, const int32_t *__restrict__ count,
                                                     const int32_t *__restrict__ zero_count, int32_t *__restrict__ out_unique) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_scenes) return;
    int32_t n = zero_count[s] > 0 ? 1 : 0;
    for (int64_t r = obj_off[s]; r < obj_off[s + 1]; ++r) n += count[r] > 0 ? 1 : 0;
    out_unique[s] = n;
}

// ---- the JSON integer lists ------------------------------------------------------------------------------------------------------
// status bits of an array (0 = parsed; anything else: declined, the host parser decides)
constexpr int32_t kBadByte = 1, kBadRange = 2, kBadZero = 4, kBadGrammar = 8, kBadCount = 16;

__device__ __forceinline__ bool is_digit(unsigned char c) { return (unsigned)(c - '0') < 10u; }

__global__ __launch_bounds__(256) void int_list_flags_kernel(const unsigned char *__restrict__ text, const int64_t *__restrict__ text_off,
                                                             int64_t n_arrays, int64_t n_bytes, int64_t *__restrict__ flags,
                                                             int32_t *__restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_bytes) return;
    const int64_t a = last_at_or_below(text_off, n_arrays, i);               // byte i's array (empty texts in front of it share its offset)
    const unsigned char c = text[i];
    const bool next_digit = i + 1 < text_off[a + 1] && is_digit(text[i + 1]);
    int64_t f = 0;
    if (is_digit(c)) f = next_digit ? 0 : 1;                                  // a number ends here
    else if (c == ',') f = (int64_t)1 << 32;
    else if (!(c == ' ' || c == '\t' || c == '\n' || c == '\r')) atomicOr(status + a, kBadByte);
    flags[i] = f;
}

__global__ __launch_bounds__(256) void int_list_values_kernel(const unsigned char *__restrict__ text, const int64_t *__restrict__ text_off,
                                                              int64_t n_arrays, int64_t n_bytes, const int64_t *__restrict__ T,
                                                              int32_t *__restrict__ out, int64_t out_capacity, int32_t *__restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_bytes) return;
    const int64_t t = T[i];
    if (((T[i + 1] - t) & 0xffffffffLL) != 1) return;                        // not the last digit of a number
    const int64_t a = last_at_or_below(text_off, n_arrays, i);               // byte i's array (empty texts in front of it share its offset)
    const int64_t base = text_off[a], tb = T[base];
    const int64_t e = t & 0xffffffffLL;                                      // numbers in front of this one, over all arrays: its slot
    int32_t bad = 0;
    if ((t >> 32) - (tb >> 32) != e - (tb & 0xffffffffLL)) bad |= kBadGrammar;     // commas in front != numbers in front (within the array)
    uint64_t value = 0, scale = 1;
    int len = 0;
    int64_t j = i;
    for (; j >= base && len < 10 && is_digit(text[j]); --j, ++len) {
        value += scale * (uint64_t)(text[j] - '0');
        scale *= 10;
    }
    if (j >= base && is_digit(text[j])) bad |= kBadRange;                     // an eleventh digit
    else if (len > 1 && text[j + 1] == '0') bad |= kBadZero;                   // JSON has no leading zeros
    if (value > 0x7fffffffULL) bad |= kBadRange;
    if (bad) atomicOr(status + a, bad);
    if (e < out_capacity) out[e] = bad ? 0 : (int32_t)value;
}

__global__ __launch_bounds__(256) void int_list_finish_kernel(const int64_t *__restrict__ text_off, int64_t n_arrays, const int64_t *__restrict__ T,
                                                              const int64_t *__restrict__ expected, int64_t *__restrict__ out_offsets,
                                                              int32_t *__restrict__ status) {
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (a > n_arrays) return;
    const int64_t t0 = T[text_off[a]];
    out_offsets[a] = t0 & 0xffffffffLL;
    if (a == n_arrays) return;
    const int64_t t1 = T[text_off[a + 1]];
    const int64_t n = (t1 & 0xffffffffLL) - (t0 & 0xffffffffLL), commas = (t1 >> 32) - (t0 >> 32);
    int32_t bad = 0;
    if (commas != (n > 0 ? n - 1 : 0)) bad |= kBadGrammar;
    if (expected != nullptr && expected[a] >= 0 && expected[a] != n) bad |= kBadCount;
    if (bad) atomicOr(status + a, bad);
}

}  // namespace prep
}  // namespace mspa

using namespace mspa;

static inline unsigned wave_blocks(int64_t n_waves) { return (unsigned)((n_waves + prep::kWavesPerBlock - 1) / prep::kWavesPerBlock); }

// n_vertices / n_waves are the totals the caller's offset tables end with (vert_off[n_scenes], word_off[n_scenes]): the grid is
// sized from them, the kernels bound themselves by the tables.
static int check_spans(const char *who, int64_t n_scenes, int64_t n_vertices, int64_t n_waves) {
    if (n_scenes < 0 || n_vertices < 0 || n_waves < 0) return fail(MSPA_EINVAL, std::string(who) + ": negative size");
    if (n_waves > n_vertices || n_waves * 64 < n_vertices) return fail(MSPA_EINVAL, std::string(who) + ": wave count does not fit the vertex count");
    if (n_waves > (int64_t)0x7fffffff * prep::kWavesPerBlock) return fail(MSPA_EINVAL, std::string(who) + ": too many vertices; split the batch");
    return MSPA_OK;
}

extern "C" int mspa_prep_labels(const int32_t *seg, const int64_t *vert_off, const int64_t *word_off, int64_t n_scenes, int64_t n_vertices,
                                int64_t n_waves, const int64_t *tab_off, const int32_t *seg2inst, const int32_t *seg2label,
                                const int64_t *lab_off, const uint32_t *label_value, uint32_t *out_instance_ids, uint32_t *out_label_ids,
                                int32_t *out_label_index, mspa_stream_t stream) {
    if (int rc = check_spans("mspa_prep_labels", n_scenes, n_vertices, n_waves)) return rc;
    if (n_scenes == 0 || n_vertices == 0) return MSPA_OK;
    if (!seg || !vert_off || !word_off || !tab_off || !seg2inst || !seg2label || !lab_off || !label_value || !out_instance_ids ||
        !out_label_ids || !out_label_index)
        return fail(MSPA_EINVAL, "mspa_prep_labels: null pointer");
    hipLaunchKernelGGL(prep::labels_kernel, dim3(wave_blocks(n_waves)), dim3(256), 0, (hipStream_t)stream, seg, vert_off, word_off, n_scenes,
                       tab_off, seg2inst, seg2label, lab_off, label_value, out_instance_ids, out_label_ids, out_label_index);
    return check_hip(hipGetLastError(), "mspa_prep_labels");
}

extern "C" int mspa_prep_align(const float *vertices, const int64_t *vert_off, const int64_t *word_off, int64_t n_scenes, int64_t n_vertices,
                               int64_t n_waves, const double *axis_align, double *out_aligned, mspa_stream_t stream) {
    if (int rc = check_spans("mspa_prep_align", n_scenes, n_vertices, n_waves)) return rc;
    if (n_scenes == 0 || n_vertices == 0) return MSPA_OK;
    if (!vertices || !vert_off || !word_off || !axis_align || !out_aligned) return fail(MSPA_EINVAL, "mspa_prep_align: null pointer");
    hipLaunchKernelGGL(prep::align_kernel, dim3(wave_blocks(n_waves)), dim3(256), 0, (hipStream_t)stream, vertices, vert_off, word_off, n_scenes,
                       axis_align, out_aligned);
    return check_hip(hipGetLastError(), "mspa_prep_align");
}

extern "C" int mspa_prep_objects(const uint32_t *instance_ids, const float *vertices, const double *aligned, const int64_t *vert_off,
                                 const int64_t *word_off, int64_t n_scenes, int64_t n_vertices, int64_t n_waves, const int64_t *obj_off,
                                 int64_t n_objects, uint64_t *out_bits, int64_t n_words, int32_t *out_count, double *out_lo_unaligned,
                                 double *out_hi_unaligned, double *out_lo_aligned, double *out_hi_aligned, int32_t *out_zero_count,
                                 int32_t *out_unique, mspa_stream_t stream) {
    if (int rc = check_spans("mspa_prep_objects", n_scenes, n_vertices, n_waves)) return rc;
    if (n_objects < 0 || n_words < 0) return fail(MSPA_EINVAL, "mspa_prep_objects: negative size");
    if (n_scenes == 0) return MSPA_OK;
    if (!vert_off || !word_off || !obj_off || !out_zero_count || !out_unique || (n_vertices > 0 && (!instance_ids || !vertices || !aligned)) ||
        (n_objects > 0 && (!out_count || !out_lo_unaligned || !out_hi_unaligned || !out_lo_aligned || !out_hi_aligned)) ||
        (n_objects > 0 && n_words > 0 && !out_bits))
        return fail(MSPA_EINVAL, "mspa_prep_objects: null pointer");
    if (n_words > n_waves) return fail(MSPA_EINVAL, "mspa_prep_objects: membership rows longer than the batch");
    if (n_objects > 0 && n_words > 0 && n_objects > ((int64_t)1 << 40) / n_words) return fail(MSPA_EINVAL, "mspa_prep_objects: membership table too large; split the batch");
    hipStream_t st = (hipStream_t)stream;
    if (n_objects > 0 && n_words > 0) {
        const int rc = check_hip(hipMemsetAsync(out_bits, 0, (size_t)n_objects * (size_t)n_words * 8, st), "mspa_prep_objects: clearing the membership rows");
        if (rc) return rc;
    }
    const int64_t slots = n_objects > n_scenes ? n_objects : n_scenes;
    hipLaunchKernelGGL(prep::objects_init_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, out_lo_unaligned, out_hi_unaligned,
                       out_lo_aligned, out_hi_aligned, out_count, n_objects, out_zero_count, n_scenes);
    if (n_vertices > 0)
        hipLaunchKernelGGL(prep::objects_kernel, dim3(wave_blocks(n_waves)), dim3(256), 0, st, instance_ids, vertices, aligned, vert_off, word_off,
                           n_scenes, obj_off, out_bits, n_words, out_count, out_lo_unaligned, out_hi_unaligned, out_lo_aligned, out_hi_aligned,
                           out_zero_count);
    hipLaunchKernelGGL(prep::unique_kernel, dim3((unsigned)((n_scenes + 255) / 256)), dim3(256), 0, st, obj_off, n_scenes, out_count, out_zero_count,
                       out_unique);
    return check_hip(hipGetLastError(), "mspa_prep_objects");
}

static int check_text(const char *who, int64_t n_arrays, int64_t n_bytes) {
    if (n_arrays < 0 || n_bytes < 0) return fail(MSPA_EINVAL, std::string(who) + ": negative size");
    if (n_bytes > 0x7fffffffLL) return fail(MSPA_EINVAL, std::string(who) + ": more than 2 GiB of text; split the batch");
    return MSPA_OK;
}

extern "C" int mspa_parse_int_list_flags_device(const char *text_dev, const int64_t *text_offsets_dev, int64_t n_arrays, int64_t n_bytes,
                                                int64_t *out_flags_dev, int32_t *status_dev, mspa_stream_t stream) {
    if (int rc = check_text("mspa_parse_int_list_flags_device", n_arrays, n_bytes)) return rc;
    if (n_arrays == 0) return MSPA_OK;
    if (!text_offsets_dev || !status_dev || (n_bytes > 0 && (!text_dev || !out_flags_dev)))
        return fail(MSPA_EINVAL, "mspa_parse_int_list_flags_device: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int rc = check_hip(hipMemsetAsync(status_dev, 0, (size_t)n_arrays * 4, st), "mspa_parse_int_list_flags_device: clearing the status");
    if (rc) return rc;
    if (n_bytes > 0)
        hipLaunchKernelGGL(prep::int_list_flags_kernel, dim3((unsigned)((n_bytes + 255) / 256)), dim3(256), 0, st, (const unsigned char *)text_dev,
                           text_offsets_dev, n_arrays, n_bytes, out_flags_dev, status_dev);
    return check_hip(hipGetLastError(), "mspa_parse_int_list_flags_device");
}

extern "C" int mspa_parse_int_list_device(const char *text_dev, const int64_t *text_offsets_dev, int64_t n_arrays, int64_t n_bytes,
                                          const int64_t *flags_prefix_dev, const int64_t *expected_counts_dev, int32_t *out_values_dev,
                                          int64_t out_capacity, int64_t *out_offsets_dev, int32_t *status_dev, mspa_stream_t stream) {
    if (int rc = check_text("mspa_parse_int_list_device", n_arrays, n_bytes)) return rc;
    if (out_capacity < 0) return fail(MSPA_EINVAL, "mspa_parse_int_list_device: negative size");
    if (n_arrays == 0) return MSPA_OK;
    if (!text_offsets_dev || !flags_prefix_dev || !out_offsets_dev || !status_dev || (n_bytes > 0 && !text_dev) ||
        (out_capacity > 0 && !out_values_dev))
        return fail(MSPA_EINVAL, "mspa_parse_int_list_device: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (n_bytes > 0)
        hipLaunchKernelGGL(prep::int_list_values_kernel, dim3((unsigned)((n_bytes + 255) / 256)), dim3(256), 0, st, (const unsigned char *)text_dev,
                           text_offsets_dev, n_arrays, n_bytes, flags_prefix_dev, out_values_dev, out_capacity, status_dev);
    hipLaunchKernelGGL(prep::int_list_finish_kernel, dim3((unsigned)((n_arrays + 1 + 255) / 256)), dim3(256), 0, st, text_offsets_dev, n_arrays,
                       flags_prefix_dev, expected_counts_dev, out_offsets_dev, status_dev);
    return check_hip(hipGetLastError(), "mspa_parse_int_list_device");
}
