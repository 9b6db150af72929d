// head_metrics.hip -- the network-head metrics of a validation step, on the device: per-image cross-entropy of the class logits,
// weighted smooth-L1 loss of the vector field, segmentation precision and recall, for a batch in one call.  The whole of
// libpvnet_head.so; C ABI: pvnet_head_metrics in include/pvnet_head.h.
//
// Restates what the reference's NetWrapper.forward computes after the backbone (tools/train_linemod.py:85-91 with
// lib/utils/net_utils.py:54-79 and :329-348), term for term in float64 on the inputs as stored.  Its oracle is the float64
// restatement of tests/test_head_metrics_device.py and the reference's own recorded outputs (tests/golden/head_metrics.npz).
//
//   head_partial_kernel   grid (segments of 1 024 pixels, images).  A workgroup streams its run of pixels through every plane -- the
//     (fast path)         class logits, the 2 vn predicted and 2 vn target planes, the weights, the mask -- eight consecutive pixels
//                         per lane, 16 bytes per load wherever the element is 2 bytes or wider: 164 bytes per pixel with float32
//                         predictions and int64 masks, each read once.  The planes must be contiguous in the pixels and 16-byte
//                         aligned, h * w a multiple of 8 (what a backbone and a dataset deliver).  The targets, the weights and
//                         the mask are loaded non-temporally -- nobody reads them again --, the predictions plainly: the vote reads
//                         them next (profiles/head_metrics_probe.txt holds the A/B).
//   head_partial_general_kernel   the same record from any element strides, any alignment, any h * w: a pixel per lane and load
//                         (mirrors the mask_linear split of k1_mask.hip).
//   head_final_kernel     a workgroup per image: sums the image's records in a fixed order, finalises, writes the outputs.
//
// No atomics; every sum has a fixed order (lane-sequential, then an xor butterfly over the wave, then the waves in order), so two
// calls on the same inputs agree bit for bit.  float64 throughout: at 164 bytes per pixel the float64 vector rate is far above
// what the memory system can feed, the kernel is bound by HBM reads.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "head_common.h"   // the per-pixel helpers, the records and the per-image body the head's translation units share
#include "pvnet_head.h"

// no contraction: the sums round as the float64 restatement's separate multiplies and adds do
#pragma clang fp contract(off)

namespace {

using namespace pvh;

constexpr int HM_T = HC_T;                // lanes of a pass-1 workgroup
constexpr int HM_PPL = HC_PPL;            // consecutive pixels per lane (fast path)
constexpr int HM_SEG = HC_SEG;            // pixels per workgroup = per partial record
constexpr int HM_FT = HC_FT;              // lanes of the final workgroup
constexpr int HM_MAX_B = HC_MAX_B;
constexpr int HM_MAX_PIXELS = HC_MAX_PIXELS;
// the spare-VGPR granule of each kernel (PVNET_SPARE_VGPRS in vote_common.h; tools/check_kernel_resources.py holds them to it)
#define HM_FAST_SPARE 119
#define HM_GENERAL_SPARE 87
#define HM_FINAL_SPARE 71

struct HeadArgs {
    const void* seg;
    const void* vp;
    const float* vt;
    const float* vw;
    const void* mask;
    int64_t ss[4], vs[4], ts[4], ws[3], ms[3];
    int seg_type, vp_type, mask_dtype, num_classes, planes;
    int h, w, npix, nseg;
    double hs, inv, half;   // sigma^2 / 2, 1 / sigma^2, 0.5 / sigma^2
    double* losses;
    int64_t* counts;
    int32_t* status;
    HeadPartial* partial;
};

template <int VT, int NT>
__global__ __launch_bounds__(HM_T) void head_partial_kernel(HeadArgs A) {
    PVNET_SPARE_VGPRS(HM_FAST_SPARE);
    constexpr bool NT_P = NT == NT_ALL, NT_T = NT != NT_NONE;   // predictions, targets / weights / mask
    const int bi = blockIdx.y;
    const int p0 = blockIdx.x * HM_SEG + (int)threadIdx.x * HM_PPL;
    Acc acc;
    if (p0 < A.npix) {   // (npix is a multiple of 8 here: the lane's eight pixels are all inside)
        int lab[HM_PPL];
        load8_labels<NT_T>(A.mask_dtype, A.mask, (int64_t)bi * A.ms[0] + p0, A.num_classes, lab);
        // ---- class logits: maximum and arg-max in one pass, then sum exp(s - max) in a second (the planes are in cache) -------------
        const int64_t soff = (int64_t)bi * A.ss[0] + p0;
        float best[HM_PPL], sl[HM_PPL], s[HM_PPL];
        bool pfg[HM_PPL];
        load8_rt<NT_P>(A.seg_type, A.seg, soff, best);
#pragma unroll
        for (int i = 0; i < HM_PPL; ++i) {
            pfg[i] = false;
            sl[i] = best[i];   // label 0, or a bad label (not used then)
        }
        for (int c = 1; c < A.num_classes; ++c) {
            load8_rt<NT_P>(A.seg_type, A.seg, soff + (int64_t)c * A.ss[1], s);
#pragma unroll
            for (int i = 0; i < HM_PPL; ++i) {
                const bool take = takes_over(best[i], s[i]);
                best[i] = take ? s[i] : best[i];
                pfg[i] = take ? true : pfg[i];
                sl[i] = lab[i] == c ? s[i] : sl[i];
            }
        }
        double sum[HM_PPL];
#pragma unroll
        for (int i = 0; i < HM_PPL; ++i) sum[i] = 0.0;
        for (int c = 0; c < A.num_classes; ++c) {
            load8_rt<NT_P>(A.seg_type, A.seg, soff + (int64_t)c * A.ss[1], s);
#pragma unroll
            for (int i = 0; i < HM_PPL; ++i) sum[i] = sum[i] + exp((double)s[i] - (double)best[i]);
        }
#pragma unroll
        for (int i = 0; i < HM_PPL; ++i) {
            if (lab[i] >= 0) acc.ce = acc.ce + cross_entropy(sum[i], sl[i], best[i]);
            acc.packed += confusion(pfg[i], lab[i]);
        }
        // ---- the field: 2 vn planes of prediction and target under one plane of weights ---------------------------------------------
        float wf[HM_PPL];
        double wd[HM_PPL];
        load8<VT_F32, NT_T>(A.vw, (int64_t)bi * A.ws[0] + p0, wf);
#pragma unroll
        for (int i = 0; i < HM_PPL; ++i) {
            wd[i] = (double)wf[i];
            acc.wsum = acc.wsum + wd[i];
        }
        const int64_t poff = (int64_t)bi * A.vs[0] + p0, toff = (int64_t)bi * A.ts[0] + p0;
#pragma unroll 2
        for (int k = 0; k < A.planes; ++k) {
            float p[HM_PPL], t[HM_PPL];
            load8<VT, NT_P>(A.vp, poff + (int64_t)k * A.vs[1], p);
            load8<VT_F32, NT_T>(A.vt, toff + (int64_t)k * A.ts[1], t);
#pragma unroll
            for (int i = 0; i < HM_PPL; ++i) acc.sl1 = acc.sl1 + smooth_l1(A, wd[i], p[i], t[i]);
        }
    }
    if (block_reduce<HM_T>(acc)) store_partial(A, acc);
}

__global__ __launch_bounds__(HM_T) void head_partial_general_kernel(HeadArgs A) {
    PVNET_SPARE_VGPRS(HM_GENERAL_SPARE);
    const int bi = blockIdx.y;
    Acc acc;
    for (int j = 0; j < HM_PPL; ++j) {
        const int p = blockIdx.x * HM_SEG + j * HM_T + (int)threadIdx.x;
        if (p >= A.npix) break;
        const int y = p / A.w, x = p - y * A.w;
        const int lab = label_of(load_label_rt(A.mask_dtype, A.mask, (int64_t)bi * A.ms[0] + (int64_t)y * A.ms[1] + (int64_t)x * A.ms[2]),
                                 A.num_classes);
        const int64_t soff = (int64_t)bi * A.ss[0] + (int64_t)y * A.ss[2] + (int64_t)x * A.ss[3];
        float best = pvd::ld_elem_rt(A.seg_type, A.seg, soff);
        float sl = best;
        bool pfg = false;
        for (int c = 1; c < A.num_classes; ++c) {
            const float s = pvd::ld_elem_rt(A.seg_type, A.seg, soff + (int64_t)c * A.ss[1]);
            const bool take = takes_over(best, s);
            best = take ? s : best;
            pfg = take ? true : pfg;
            sl = lab == c ? s : sl;
        }
        double sum = 0.0;
        for (int c = 0; c < A.num_classes; ++c)
            sum = sum + exp((double)pvd::ld_elem_rt(A.seg_type, A.seg, soff + (int64_t)c * A.ss[1]) - (double)best);
        if (lab >= 0) acc.ce = acc.ce + cross_entropy(sum, sl, best);
        acc.packed += confusion(pfg, lab);
        const double wd = (double)A.vw[(int64_t)bi * A.ws[0] + (int64_t)y * A.ws[1] + (int64_t)x * A.ws[2]];
        acc.wsum = acc.wsum + wd;
        const int64_t poff = (int64_t)bi * A.vs[0] + (int64_t)y * A.vs[2] + (int64_t)x * A.vs[3];
        const int64_t toff = (int64_t)bi * A.ts[0] + (int64_t)y * A.ts[2] + (int64_t)x * A.ts[3];
        for (int k = 0; k < A.planes; ++k)
            acc.sl1 = acc.sl1 + smooth_l1(A, wd, pvd::ld_elem_rt(A.vp_type, A.vp, poff + (int64_t)k * A.vs[1]),
                                          A.vt[toff + (int64_t)k * A.ts[1]]);
    }
    if (block_reduce<HM_T>(acc)) store_partial(A, acc);
}

__global__ __launch_bounds__(HM_FT) void head_final_kernel(HeadArgs A) {
    PVNET_SPARE_VGPRS(HM_FINAL_SPARE);
    head_final_image(A);
}

template <int VT>
void launch_fast(int nt, dim3 grid, hipStream_t s, const HeadArgs& A) {
    if (nt == NT_NONE) hipLaunchKernelGGL((head_partial_kernel<VT, NT_NONE>), grid, dim3(HM_T), 0, s, A);
    else if (nt == NT_ALL) hipLaunchKernelGGL((head_partial_kernel<VT, NT_ALL>), grid, dim3(HM_T), 0, s, A);
    else hipLaunchKernelGGL((head_partial_kernel<VT, NT_TARGETS>), grid, dim3(HM_T), 0, s, A);
}

}  // namespace

extern "C" {

int pvnet_head_abi_version(void) { return PVNET_HEAD_ABI_VERSION; }

size_t pvnet_head_metrics_workspace_bytes(int b, int h, int w) {
    if (b <= 0 || h <= 0 || w <= 0 || b > HM_MAX_B || (long long)h * w > HM_MAX_PIXELS) return 0;
    const size_t nseg = ((size_t)h * w + HM_SEG - 1) / HM_SEG;
    return ((size_t)b * nseg * sizeof(HeadPartial) + 255) / 256 * 256;
}

int pvnet_head_metrics(const void* seg_pred, const int64_t seg_strides[4], int num_classes, const void* vertex_pred,
                       const int64_t vp_strides[4], const float* vertex_target, const int64_t vt_strides[4],
                       const float* vertex_weights, const int64_t w_strides[3], const void* mask, int mask_dtype,
                       const int64_t mask_strides[3], int b, int h, int w, int vn, double sigma, uint32_t flags, double* losses,
                       int64_t* counts, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    constexpr uint32_t KNOWN = PVNET_HEAD_F_VERTEX_F16 | PVNET_HEAD_F_VERTEX_BF16 | PVNET_HEAD_F_LOGITS_F16 | PVNET_HEAD_F_LOGITS_BF16 |
                               PVNET_HEAD_F_NT_NONE | PVNET_HEAD_F_NT_ALL;
    if (!seg_pred || !seg_strides || !vertex_pred || !vp_strides || !vertex_target || !vt_strides || !vertex_weights || !w_strides ||
        !mask || !mask_strides || !losses || !counts)
        return PVNET_E_BADARG;
    if (b < 0 || h <= 0 || w <= 0 || vn <= 0 || num_classes < 2 || !(sigma > 0.0) || !isfinite(sigma) || (flags & ~KNOWN) != 0)
        return PVNET_E_BADARG;
    if (((flags & PVNET_HEAD_F_VERTEX_F16) && (flags & PVNET_HEAD_F_VERTEX_BF16)) ||
        ((flags & PVNET_HEAD_F_LOGITS_F16) && (flags & PVNET_HEAD_F_LOGITS_BF16)) ||
        ((flags & PVNET_HEAD_F_NT_NONE) && (flags & PVNET_HEAD_F_NT_ALL)))
        return PVNET_E_BADARG;
    if (mask_dtype == PVNET_MASK_I16 || mask_dtype == PVNET_MASK_F32 || mask_dtype == PVNET_MASK_LOGITS_F32) return PVNET_E_UNSUPPORTED;
    if (mask_dtype != PVNET_MASK_U8 && mask_dtype != PVNET_MASK_I32 && mask_dtype != PVNET_MASK_I64) return PVNET_E_BADARG;
    if (b > HM_MAX_B || (long long)h * w > HM_MAX_PIXELS || vn > (1 << 20)) return PVNET_E_UNSUPPORTED;
    if (b == 0) return 0;
    if (!workspace || workspace_bytes < pvnet_head_metrics_workspace_bytes(b, h, w)) return PVNET_E_WORKSPACE;
    if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0) return PVNET_E_BADARG;
    HeadArgs A;
    A.seg = seg_pred;
    A.vp = vertex_pred;
    A.vt = vertex_target;
    A.vw = vertex_weights;
    A.mask = mask;
    for (int i = 0; i < 4; ++i) {
        A.ss[i] = seg_strides[i];
        A.vs[i] = vp_strides[i];
        A.ts[i] = vt_strides[i];
    }
    for (int i = 0; i < 3; ++i) {
        A.ws[i] = w_strides[i];
        A.ms[i] = mask_strides[i];
    }
    A.seg_type = type_of(flags, PVNET_HEAD_F_LOGITS_F16, PVNET_HEAD_F_LOGITS_BF16);
    A.vp_type = type_of(flags, PVNET_HEAD_F_VERTEX_F16, PVNET_HEAD_F_VERTEX_BF16);
    A.mask_dtype = mask_dtype;
    A.num_classes = num_classes;
    A.planes = 2 * vn;
    A.h = h;
    A.w = w;
    A.npix = h * w;
    A.nseg = (A.npix + HM_SEG - 1) / HM_SEG;
    const double s2 = sigma * sigma;
    A.hs = s2 / 2.0;
    A.inv = 1.0 / s2;
    A.half = 0.5 / s2;
    A.losses = losses;
    A.counts = counts;
    A.status = status;
    A.partial = static_cast<HeadPartial*>(workspace);
    const bool fast = A.npix % HM_PPL == 0 && plane_linear(seg_pred, b, A.ss[0], A.ss[1], A.ss[2], A.ss[3], w) &&
                      plane_linear(vertex_pred, b, A.vs[0], A.vs[1], A.vs[2], A.vs[3], w) &&
                      plane_linear(vertex_target, b, A.ts[0], A.ts[1], A.ts[2], A.ts[3], w) &&
                      plane_linear(vertex_weights, b, A.ws[0], 0, A.ws[1], A.ws[2], w) &&
                      plane_linear(mask, b, A.ms[0], 0, A.ms[1], A.ms[2], w);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)A.nseg, (unsigned)b);
    if (fast) {
        const int nt = (flags & PVNET_HEAD_F_NT_NONE) ? NT_NONE : (flags & PVNET_HEAD_F_NT_ALL) ? NT_ALL : NT_TARGETS;
        if (A.vp_type == VT_F16) launch_fast<VT_F16>(nt, grid, s, A);
        else if (A.vp_type == VT_BF16) launch_fast<VT_BF16>(nt, grid, s, A);
        else launch_fast<VT_F32>(nt, grid, s, A);
    } else {
        hipLaunchKernelGGL(head_partial_general_kernel, grid, dim3(HM_T), 0, s, A);
    }
    hipLaunchKernelGGL(head_final_kernel, dim3((unsigned)b), dim3(HM_FT), 0, s, A);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

}  // extern "C"
