// head_grad.hip -- the backward of the network-head losses of a training step, on the device: the gradient of the per-image
// cross-entropy with respect to the class logits and of the weighted smooth-L1 loss with respect to the predicted field, for a batch
// in one call.  The whole of libpvnet_train.so; C ABI: pvnet_head_grad in include/pvnet_train.h (the formulas are stated there).
//
// The forward is pvnet_head_metrics (head_metrics.hip, libpvnet_head.so), which stays as it is; the loss is the reference's
// (tools/train_linemod.py:85-91, lib/utils/net_utils.py:54-79).  Both gradients have a closed form per element, so nothing of the
// forward is saved: this file reads the forward's inputs again and writes the two gradient tensors.  Its oracle is the float64
// restatement tests/head_grad_restatement.py and the reference's own autograd, recorded in tests/golden/head_grad.npz.
//
//   head_grad_wsum_kernel<FAST>   grid (segments of 1 024 pixels, images): the segment's sum of the weights, in the forward's order
//                                 (so D_i = 2vn sum w + 1e-3 is the forward's denominator bit for bit).  4 bytes per pixel, loaded
//                                 plainly: the gradient kernel reads them again.  Skipped without a field gradient.
//   head_grad_final_kernel        a workgroup per image: sums the records in a fixed order and writes the image's two coefficients
//                                 u_s / (h w) and u_v / D_i to the workspace.
//   head_grad_kernel<VT, NT>      grid (segments, images), the fast path: eight consecutive pixels per lane, 16 bytes per load and
//                                 store wherever the element is 2 bytes or wider.  Reads every input byte once -- targets, weights
//                                 and mask non-temporally, as the forward does --, writes every gradient byte once, plainly: the
//                                 backbone's backward reads them next.  244 bytes per pixel with float32 predictions, int64 masks,
//                                 C = 2 and vn = 9.  Needs what the forward's fast path needs, of the gradient tensors too.
//   head_grad_general_kernel      the same from any element strides, any alignment, any h * w: a pixel per lane and access.
//   head_grad_status_kernel       a workgroup per image: ORs the segments' bad-label flags into status (only when status is asked
//                                 for; 0 where the logits' half did not run).
//
// No atomics; every sum has a fixed order, every output element is a function of its own pixel and the image's two coefficients:
// two calls agree bit for bit.  float64 after the load; each element is rounded ONCE to its tensor's type (float16 / bfloat16 through
// a round-to-odd float32, which makes the second rounding exact).
//
// The load and store helpers, the two formulas and the per-image bodies are head_common.h's, shared with head_metrics.hip.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "head_common.h"   // the per-pixel helpers and the per-image bodies the head's translation units share
#include "pvnet_train.h"

// no contraction: every product and sum rounds as the float64 restatement's separate operations do
#pragma clang fp contract(off)

namespace {

using namespace pvh;

constexpr int HG_T = HC_T;                // lanes of a workgroup of the per-pixel kernels
constexpr int HG_PPL = HC_PPL;            // consecutive pixels per lane (fast path)
constexpr int HG_SEG = HC_SEG;            // pixels per workgroup
constexpr int HG_FT = HC_FT;              // lanes of the per-image workgroups
constexpr int HG_MAX_B = HC_MAX_B;
constexpr int HG_MAX_PIXELS = HC_MAX_PIXELS;
// the spare-VGPR granule of each kernel (PVNET_SPARE_VGPRS in vote_common.h; tools/check_kernel_resources.py holds them to it)
#define HG_FAST_SPARE 135
#define HG_GENERAL_SPARE 79
#define HG_WSUM_SPARE 31
#define HG_FINAL_SPARE 31
#define HG_STATUS_SPARE 23

struct GradArgs {
    const void* seg;
    const void* vp;
    const float* vt;
    const float* vw;
    const void* mask;
    void* gs;   // NULL: the logits' half is skipped
    void* gv;   // NULL: the field's half is skipped
    int64_t ss[4], vs[4], ts[4], ws[3], ms[3], gss[4], gvs[4];
    int seg_type, vp_type, mask_dtype, num_classes, planes;
    int h, w, npix, nseg;
    double s2, inv;   // sigma^2, 1 / sigma^2
    const double* upstream;
    double* coef;     // [b][2]: u_s / (h w), u_v / D_i
    double* wpart;    // [b][nseg]: a segment's sum of the weights
    int32_t* bad;     // [b][nseg]: the segment holds a label outside 0 .. C-1
    int32_t* status;
};

template <bool FAST>
__global__ __launch_bounds__(HG_T) void head_grad_wsum_kernel(GradArgs A) {
    PVNET_SPARE_VGPRS(HG_WSUM_SPARE);
    const int bi = blockIdx.y;
    double acc = 0.0;
    if (FAST) {
        const int p0 = blockIdx.x * HG_SEG + (int)threadIdx.x * HG_PPL;
        if (p0 < A.npix) {   // (npix is a multiple of 8 here: the lane's eight pixels are all inside)
            float wf[HG_PPL];
            load8<VT_F32, false>(A.vw, (int64_t)bi * A.ws[0] + p0, wf);
#pragma unroll
            for (int i = 0; i < HG_PPL; ++i) acc = acc + (double)wf[i];
        }
    } else {
        for (int j = 0; j < HG_PPL; ++j) {
            const int p = blockIdx.x * HG_SEG + j * HG_T + (int)threadIdx.x;
            if (p >= A.npix) break;
            const int y = p / A.w, x = p - y * A.w;
            acc = acc + (double)A.vw[(int64_t)bi * A.ws[0] + (int64_t)y * A.ws[1] + (int64_t)x * A.ws[2]];
        }
    }
    acc = block_sum<HG_T>(acc);
    if (threadIdx.x == 0) A.wpart[(size_t)bi * A.nseg + blockIdx.x] = acc;
}

__global__ __launch_bounds__(HG_FT) void head_grad_final_kernel(GradArgs A) {
    PVNET_SPARE_VGPRS(HG_FINAL_SPARE);
    head_grad_final_image(A);
}

template <int VT, int NT>
__global__ __launch_bounds__(HG_T) void head_grad_kernel(GradArgs A) {
    PVNET_SPARE_VGPRS(HG_FAST_SPARE);
    constexpr bool NT_P = NT == NT_ALL, NT_T = NT != NT_NONE, NT_S = NT == NT_ALL;   // predictions, targets / weights / mask, stores
    const int bi = blockIdx.y;
    const int p0 = blockIdx.x * HG_SEG + (int)threadIdx.x * HG_PPL;
    const bool inside = p0 < A.npix;   // (npix is a multiple of 8 here: the lane's eight pixels are all inside)
    int bad = 0;
    if (inside && A.gs) {
        const double ks = A.coef[2 * bi];
        int lab[HG_PPL];
        load8_labels<NT_T>(A.mask_dtype, A.mask, (int64_t)bi * A.ms[0] + p0, A.num_classes, lab);
        // ---- the maximum, then sum exp(s - max) and the share of the classes other than the label's, then the gradients: the planes
        //      are in cache after the first pass -----------------------------------------------------------------------------------
        const int64_t soff = (int64_t)bi * A.ss[0] + p0, goff = (int64_t)bi * A.gss[0] + p0;
        float best[HG_PPL], s[HG_PPL];
        load8_rt<NT_P>(A.seg_type, A.seg, soff, best);
        for (int c = 1; c < A.num_classes; ++c) {
            load8_rt<NT_P>(A.seg_type, A.seg, soff + (int64_t)c * A.ss[1], s);
#pragma unroll
            for (int i = 0; i < HG_PPL; ++i) best[i] = takes_over(best[i], s[i]) ? s[i] : best[i];
        }
        double sum[HG_PPL], rest[HG_PPL];
#pragma unroll
        for (int i = 0; i < HG_PPL; ++i) {
            sum[i] = 0.0;
            rest[i] = 0.0;
            bad |= lab[i] < 0;
        }
        for (int c = 0; c < A.num_classes; ++c) {
            load8_rt<NT_P>(A.seg_type, A.seg, soff + (int64_t)c * A.ss[1], s);
#pragma unroll
            for (int i = 0; i < HG_PPL; ++i) {
                const double e = exp((double)s[i] - (double)best[i]);
                sum[i] = sum[i] + e;
                rest[i] = rest[i] + (lab[i] == c ? 0.0 : e);
            }
        }
        for (int c = 0; c < A.num_classes; ++c) {
            load8_rt<NT_P>(A.seg_type, A.seg, soff + (int64_t)c * A.ss[1], s);
            double g[HG_PPL];
#pragma unroll
            for (int i = 0; i < HG_PPL; ++i)
                g[i] = logit_grad(lab[i], c, exp((double)s[i] - (double)best[i]), sum[i], rest[i], ks);
            store8_rt<NT_S>(A.seg_type, A.gs, goff + (int64_t)c * A.gss[1], g);
        }
    }
    if (inside && A.gv) {
        // ---- the field: 2 vn planes of prediction and target under one plane of weights -----------------------------------------------
        const double kv = A.coef[2 * bi + 1];
        float wf[HG_PPL];
        double wd[HG_PPL];
        load8<VT_F32, NT_T>(A.vw, (int64_t)bi * A.ws[0] + p0, wf);
#pragma unroll
        for (int i = 0; i < HG_PPL; ++i) wd[i] = (double)wf[i];
        const int64_t poff = (int64_t)bi * A.vs[0] + p0, toff = (int64_t)bi * A.ts[0] + p0, goff = (int64_t)bi * A.gvs[0] + p0;
#pragma unroll 2
        for (int k = 0; k < A.planes; ++k) {
            float p[HG_PPL], t[HG_PPL];
            double g[HG_PPL];
            load8<VT, NT_P>(A.vp, poff + (int64_t)k * A.vs[1], p);
            load8<VT_F32, NT_T>(A.vt, toff + (int64_t)k * A.ts[1], t);
#pragma unroll
            for (int i = 0; i < HG_PPL; ++i) g[i] = field_grad(A, wd[i], p[i], t[i], kv);
            store8<VT, NT_S>(A.gv, goff + (int64_t)k * A.gvs[1], g);
        }
    }
    if (A.gs) {   // (uniform over the grid: every lane reaches the barrier)
        const int any = __syncthreads_or(bad);
        if (threadIdx.x == 0) A.bad[(size_t)bi * A.nseg + blockIdx.x] = any ? 1 : 0;
    }
}

__global__ __launch_bounds__(HG_T) void head_grad_general_kernel(GradArgs A) {
    PVNET_SPARE_VGPRS(HG_GENERAL_SPARE);
    const int bi = blockIdx.y;
    int bad = 0;
    for (int j = 0; j < HG_PPL; ++j) {
        const int p = blockIdx.x * HG_SEG + j * HG_T + (int)threadIdx.x;
        if (p >= A.npix) break;
        const int y = p / A.w, x = p - y * A.w;
        if (A.gs) {
            const double ks = A.coef[2 * bi];
            const int lab = label_of(load_label_rt(A.mask_dtype, A.mask, (int64_t)bi * A.ms[0] + (int64_t)y * A.ms[1] + (int64_t)x * A.ms[2]),
                                     A.num_classes);
            bad |= lab < 0;
            const int64_t soff = (int64_t)bi * A.ss[0] + (int64_t)y * A.ss[2] + (int64_t)x * A.ss[3];
            const int64_t goff = (int64_t)bi * A.gss[0] + (int64_t)y * A.gss[2] + (int64_t)x * A.gss[3];
            float best = pvd::ld_elem_rt(A.seg_type, A.seg, soff);
            for (int c = 1; c < A.num_classes; ++c) {
                const float s = pvd::ld_elem_rt(A.seg_type, A.seg, soff + (int64_t)c * A.ss[1]);
                best = takes_over(best, s) ? s : best;
            }
            double sum = 0.0, rest = 0.0;
            for (int c = 0; c < A.num_classes; ++c) {
                const double e = exp((double)pvd::ld_elem_rt(A.seg_type, A.seg, soff + (int64_t)c * A.ss[1]) - (double)best);
                sum = sum + e;
                rest = rest + (lab == c ? 0.0 : e);
            }
            for (int c = 0; c < A.num_classes; ++c) {
                const double e = exp((double)pvd::ld_elem_rt(A.seg_type, A.seg, soff + (int64_t)c * A.ss[1]) - (double)best);
                store_elem_rt(A.seg_type, A.gs, goff + (int64_t)c * A.gss[1], logit_grad(lab, c, e, sum, rest, ks));
            }
        }
        if (A.gv) {
            const double kv = A.coef[2 * bi + 1];
            const double wd = (double)A.vw[(int64_t)bi * A.ws[0] + (int64_t)y * A.ws[1] + (int64_t)x * A.ws[2]];
            const int64_t poff = (int64_t)bi * A.vs[0] + (int64_t)y * A.vs[2] + (int64_t)x * A.vs[3];
            const int64_t toff = (int64_t)bi * A.ts[0] + (int64_t)y * A.ts[2] + (int64_t)x * A.ts[3];
            const int64_t goff = (int64_t)bi * A.gvs[0] + (int64_t)y * A.gvs[2] + (int64_t)x * A.gvs[3];
            for (int k = 0; k < A.planes; ++k)
                store_elem_rt(A.vp_type, A.gv, goff + (int64_t)k * A.gvs[1],
                              field_grad(A, wd, pvd::ld_elem_rt(A.vp_type, A.vp, poff + (int64_t)k * A.vs[1]), A.vt[toff + (int64_t)k * A.ts[1]], kv));
        }
    }
    if (A.gs) {
        const int any = __syncthreads_or(bad);
        if (threadIdx.x == 0) A.bad[(size_t)bi * A.nseg + blockIdx.x] = any ? 1 : 0;
    }
}

__global__ __launch_bounds__(HG_FT) void head_grad_status_kernel(GradArgs A) {
    PVNET_SPARE_VGPRS(HG_STATUS_SPARE);
    head_grad_status_image(A);
}

template <int VT>
void launch_fast(int nt, dim3 grid, hipStream_t s, const GradArgs& A) {
    if (nt == NT_NONE) hipLaunchKernelGGL((head_grad_kernel<VT, NT_NONE>), grid, dim3(HG_T), 0, s, A);
    else if (nt == NT_ALL) hipLaunchKernelGGL((head_grad_kernel<VT, NT_ALL>), grid, dim3(HG_T), 0, s, A);
    else hipLaunchKernelGGL((head_grad_kernel<VT, NT_TARGETS>), grid, dim3(HG_T), 0, s, A);
}

}  // namespace

extern "C" {

int pvnet_train_abi_version(void) { return PVNET_TRAIN_ABI_VERSION; }

size_t pvnet_head_grad_workspace_bytes(int b, int h, int w) {
    if (b <= 0 || h <= 0 || w <= 0 || b > HG_MAX_B || (long long)h * w > HG_MAX_PIXELS) return 0;
    const size_t nseg = ((size_t)h * w + HG_SEG - 1) / HG_SEG;
    return round256((size_t)b * 2 * sizeof(double)) + round256((size_t)b * nseg * sizeof(double)) + round256((size_t)b * nseg * sizeof(int32_t));
}

int pvnet_head_grad(const void* seg_pred, const int64_t seg_strides[4], int num_classes, const void* vertex_pred,
                    const int64_t vp_strides[4], const float* vertex_target, const int64_t vt_strides[4], const float* vertex_weights,
                    const int64_t w_strides[3], const void* mask, int mask_dtype, const int64_t mask_strides[3], int b, int h, int w,
                    int vn, double sigma, uint32_t flags, const double* upstream, void* grad_seg, const int64_t gs_strides[4],
                    void* grad_vertex, const int64_t gv_strides[4], int32_t* status, void* workspace, size_t workspace_bytes,
                    void* stream) {
    constexpr uint32_t KNOWN = PVNET_HEAD_F_VERTEX_F16 | PVNET_HEAD_F_VERTEX_BF16 | PVNET_HEAD_F_LOGITS_F16 | PVNET_HEAD_F_LOGITS_BF16 |
                               PVNET_HEAD_F_NT_NONE | PVNET_HEAD_F_NT_ALL;
    if (!seg_pred || !seg_strides || !vertex_pred || !vp_strides || !vertex_target || !vt_strides || !vertex_weights || !w_strides ||
        !mask || !mask_strides || !upstream)
        return PVNET_E_BADARG;
    if ((!grad_seg && !grad_vertex) || (grad_seg && !gs_strides) || (grad_vertex && !gv_strides)) return PVNET_E_BADARG;
    if (b < 0 || h <= 0 || w <= 0 || vn <= 0 || num_classes < 2 || !(sigma > 0.0) || !isfinite(sigma) || (flags & ~KNOWN) != 0)
        return PVNET_E_BADARG;
    if (((flags & PVNET_HEAD_F_VERTEX_F16) && (flags & PVNET_HEAD_F_VERTEX_BF16)) ||
        ((flags & PVNET_HEAD_F_LOGITS_F16) && (flags & PVNET_HEAD_F_LOGITS_BF16)) ||
        ((flags & PVNET_HEAD_F_NT_NONE) && (flags & PVNET_HEAD_F_NT_ALL)))
        return PVNET_E_BADARG;
    if (mask_dtype == PVNET_MASK_I16 || mask_dtype == PVNET_MASK_F32 || mask_dtype == PVNET_MASK_LOGITS_F32) return PVNET_E_UNSUPPORTED;
    if (mask_dtype != PVNET_MASK_U8 && mask_dtype != PVNET_MASK_I32 && mask_dtype != PVNET_MASK_I64) return PVNET_E_BADARG;
    if (b > HG_MAX_B || (long long)h * w > HG_MAX_PIXELS || vn > (1 << 20)) return PVNET_E_UNSUPPORTED;
    if (b == 0) return 0;
    if (!workspace || workspace_bytes < pvnet_head_grad_workspace_bytes(b, h, w)) return PVNET_E_WORKSPACE;
    if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0) return PVNET_E_BADARG;
    GradArgs A;
    A.seg = seg_pred;
    A.vp = vertex_pred;
    A.vt = vertex_target;
    A.vw = vertex_weights;
    A.mask = mask;
    A.gs = grad_seg;
    A.gv = grad_vertex;
    for (int i = 0; i < 4; ++i) {
        A.ss[i] = seg_strides[i];
        A.vs[i] = vp_strides[i];
        A.ts[i] = vt_strides[i];
        A.gss[i] = grad_seg ? gs_strides[i] : 0;
        A.gvs[i] = grad_vertex ? gv_strides[i] : 0;
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
    A.nseg = (A.npix + HG_SEG - 1) / HG_SEG;
    A.s2 = sigma * sigma;
    A.inv = 1.0 / A.s2;
    A.upstream = upstream;
    char* ws = static_cast<char*>(workspace);
    A.coef = reinterpret_cast<double*>(ws);
    ws += round256((size_t)b * 2 * sizeof(double));
    A.wpart = reinterpret_cast<double*>(ws);
    ws += round256((size_t)b * A.nseg * sizeof(double));
    A.bad = reinterpret_cast<int32_t*>(ws);
    A.status = status;
    // each half asks the fast path's shape of its own tensors only: the other half's are not touched
    const bool lin_w = plane_linear(vertex_weights, b, A.ws[0], 0, A.ws[1], A.ws[2], w);
    const bool fast = A.npix % HG_PPL == 0 &&
                      (!grad_seg || (plane_linear(seg_pred, b, A.ss[0], A.ss[1], A.ss[2], A.ss[3], w) &&
                                     plane_linear(mask, b, A.ms[0], 0, A.ms[1], A.ms[2], w) &&
                                     plane_linear(grad_seg, b, A.gss[0], A.gss[1], A.gss[2], A.gss[3], w))) &&
                      (!grad_vertex || (plane_linear(vertex_pred, b, A.vs[0], A.vs[1], A.vs[2], A.vs[3], w) &&
                                        plane_linear(vertex_target, b, A.ts[0], A.ts[1], A.ts[2], A.ts[3], w) && lin_w &&
                                        plane_linear(grad_vertex, b, A.gvs[0], A.gvs[1], A.gvs[2], A.gvs[3], w)));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)A.nseg, (unsigned)b);
    if (grad_vertex) {
        if (A.npix % HG_PPL == 0 && lin_w) hipLaunchKernelGGL(head_grad_wsum_kernel<true>, grid, dim3(HG_T), 0, s, A);
        else hipLaunchKernelGGL(head_grad_wsum_kernel<false>, grid, dim3(HG_T), 0, s, A);
    }
    hipLaunchKernelGGL(head_grad_final_kernel, dim3((unsigned)b), dim3(HG_FT), 0, s, A);
    if (fast) {
        const int nt = (flags & PVNET_HEAD_F_NT_NONE) ? NT_NONE : (flags & PVNET_HEAD_F_NT_ALL) ? NT_ALL : NT_TARGETS;
        if (A.vp_type == VT_F16) launch_fast<VT_F16>(nt, grid, s, A);
        else if (A.vp_type == VT_BF16) launch_fast<VT_BF16>(nt, grid, s, A);
        else launch_fast<VT_F32>(nt, grid, s, A);
    } else {
        hipLaunchKernelGGL(head_grad_general_kernel, grid, dim3(HG_T), 0, s, A);
    }
    if (status) hipLaunchKernelGGL(head_grad_status_kernel, dim3((unsigned)b), dim3(HG_FT), 0, s, A);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

}  // extern "C"
