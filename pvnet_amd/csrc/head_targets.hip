// head_targets.hip -- the training targets of the vector field made on the device from the key-points, and the network head's forward
// and backward fused with them.  The whole of libpvnet_targets.so; C ABI: include/pvnet_targets.h (the definition is stated there).
//
// The reference makes `vertex` and `vertex_weights` on the host, per sample (compute_vertex_hcoords, lib/datasets/linemod_dataset.py
// :68-81 and :224-227), and ships 76 bytes per pixel to the device; both are a function of the mask and of 27 numbers per image.
// kp_target (kp_target.h) is that function for one pixel and one key-point; nothing else here makes a target.
//
// This file holds the key-point target source, KpSource -- the policy of head_common.h's per-pixel bodies that computes a pixel's
// weight and targets in registers where MemSource loads them --, the one kernel that writes the targets out, and the head's kernels
// instantiated on that source.  It holds none of the head's arithmetic: the bodies are head_common.h's, the same source text that
// head_metrics.hip and head_grad.hip instantiate on MemSource, so the fused forms equal the head on materialised targets bit for bit.
//
//   vertex_targets_kernel<FAST>      grid (segments of 1 024 pixels, images).  Reads the mask, writes the 2 vn target planes and the
//                                    weights: 76 bytes per pixel written at vn = 9, plainly -- the head reads them next.  Fast path:
//                                    eight consecutive pixels per lane, 16 bytes per store (mask and outputs contiguous in the
//                                    pixels, 16-byte aligned, h * w a multiple of 8); else a pixel per lane and store, any strides.
//   head_partial_kp_kernel<VT, NT>   the forward (head_partial8 / head_partial1 / head_final_image): 88 bytes per pixel read instead
//   head_partial_kp_general_kernel   of 164 (float32 predictions, int64 masks, vn = 9).  Same grid, segments, records and summation
//   head_final_kp_kernel             order as on loaded targets.
//   head_grad_kp_wsum_kernel<FAST>   the backward (head_grad_wsum / head_grad_final_image / head_grad8 / head_grad1 /
//   head_grad_kp_final_kernel        head_grad_status_image): 88 bytes read and 80 written per pixel instead of 244 moved.  The
//   head_grad_kp_kernel<VT, NT>      weights' sum reads the mask (the weight of a pixel is its mask value times the image's scale),
//   head_grad_kp_general_kernel      and so does the field's half: the mask is read whichever half is asked for.
//   head_grad_kp_status_kernel
//
// The image's key-points are held in SGPRs.  They reach the kernels as an argument of their own, `const double* __restrict__`, not
// through the argument struct: a pointer in a struct passed by value is not noalias, and beside the kernels' stores the compiler then
// read it with per-lane vector loads.  As a noalias argument at a uniform address (blockIdx.y, the loop counter) the three doubles are
// one s_load_dwordx4 and one s_load_dwordx2 per key-point.  A lane whose eight pixels hold no mask == 1 takes no float64 square root
// or divide, and a wave of such lanes branches over them; its targets are zeros.  The predictions are still read at every pixel -- a
// NaN at a background pixel reaches the loss and the gradient as 0 * NaN.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "head_common.h"
#include "kp_target.h"
#include "pvnet_targets.h"

// no contraction: vx vx + vy vy and hx - x hz round as the reference's separate numpy operations do
#pragma clang fp contract(off)

namespace {

using namespace pvh;

// the spare-VGPR granule of each kernel (PVNET_SPARE_VGPRS in vote_common.h; tools/check_kernel_resources.py holds them to it)
#define KP_TARGETS_FAST_SPARE 95
#define KP_TARGETS_GENERAL_SPARE 39
#define KP_HEAD_FAST_SPARE 119      // float32 predictions: the forward on loaded targets' allocation, four waves per SIMD
#define KP_HEAD_FAST16_SPARE 135    // float16 / bfloat16: their conversions beside the float64 divides pass 111 VGPRs
#define KP_HEAD_GENERAL_SPARE 95
#define KP_HEAD_FINAL_SPARE 71
#define KP_GRAD_FAST_SPARE 143        // three waves per SIMD, as at 135
#define KP_GRAD_GENERAL_SPARE 87
#define KP_GRAD_WSUM_SPARE 39
#define KP_GRAD_FINAL_SPARE 31
#define KP_GRAD_STATUS_SPARE 23

// (THE definition of a target, kp_target, and the weight of a pixel, kp_weight: kp_target.h, shared with class_targets.hip)

// ---- the key-point source: where the mask is, and the target source made of it (the interface is stated at MemSource) -------------
struct KpSource {
    const void* mask;
    const float* __restrict__ wscale;   // NULL or [b]
    int64_t ms[3];
    int mask_dtype, vn, motion;
    int w, npix, nseg;

    __device__ __forceinline__ float scale(int bi) const { return wscale ? wscale[bi] : 1.0f; }
    __device__ __forceinline__ long long mask_at(int bi, int x, int y) const {
        return load_label_rt(mask_dtype, mask, (int64_t)bi * ms[0] + (int64_t)y * ms[1] + (int64_t)x * ms[2]);
    }

    // a lane's eight mask values -> labels, weights, the mask == 1 bits
    template <bool NT>
    __device__ __forceinline__ unsigned kp_pixels8(int bi, int p0, int C, int* lab, float* wf) const {
        long long mv[HC_PPL];
        load8_mask<NT>(mask_dtype, mask, (int64_t)bi * ms[0] + p0, mv);
        const float sc = scale(bi);
        unsigned fg = 0;
#pragma unroll
        for (int i = 0; i < HC_PPL; ++i) {
            lab[i] = label_of(mv[i], C);
            wf[i] = kp_weight(mv[i], sc);
            fg |= mv[i] == 1 ? 1u << i : 0u;
        }
        return fg;
    }

    // the targets of one key-point for a lane's eight consecutive pixels from (x0, y0) on; fg: bit i set where mask == 1.  A lane
    // without such a pixel skips the float64 work (and so does a wave of such lanes).
    __device__ __forceinline__ void kp_targets8(const double* __restrict__ hc, int x0, int y0, unsigned fg, float* tx, float* ty) const {
        const double hx = hc[0], hy = hc[1], hz = hc[2];
#pragma unroll
        for (int i = 0; i < HC_PPL; ++i) tx[i] = ty[i] = 0.0f;
        if (fg == 0) return;
        int x = x0, y = y0;
#pragma unroll
        for (int i = 0; i < HC_PPL; ++i) {
            float ax, ay;
            kp_target(hx, hy, hz, x, y, motion != 0, ax, ay);
            tx[i] = (fg >> i) & 1u ? ax : 0.0f;
            ty[i] = (fg >> i) & 1u ? ay : 0.0f;
            if (++x == w) {
                x = 0;
                ++y;
            }
        }
    }

    // -- as a target source: the mask is read whether or not the labels are asked for (the weights and the targets depend on it)
    struct Lane8 {
        float wf[HC_PPL];
        unsigned fg = 0;
    };
    struct Image {
        float scale;
    };
    struct Pixel {
        long long m;
    };

    template <bool NT>
    __device__ __forceinline__ void pixels8(int bi, int p0, int C, bool, int* lab, Lane8& L) const {
        L.fg = kp_pixels8<NT>(bi, p0, C, lab, L.wf);
    }
    template <bool NT>
    __device__ __forceinline__ void weights8(int, int, const Lane8& L, double* wd) const {
#pragma unroll
        for (int i = 0; i < HC_PPL; ++i) wd[i] = (double)L.wf[i];
    }
    // the x and the y plane of a key-point per step.  BOTH: the two predictions are loaded before the targets are made (the backward:
    // their latency hides behind the float64 work); else each when it is used (the forward, which keeps to 128 VGPRs so)
    template <bool NT, bool BOTH, typename LOAD, typename USE>
    __device__ __forceinline__ void planes8(const double* __restrict__ hcb, int, int p0, int, const Lane8& L, LOAD load, USE use) const {
        const int y0 = p0 / w, x0 = p0 - y0 * w;
        for (int k = 0; k < vn; ++k) {
            float p[HC_PPL], q[HC_PPL], tx[HC_PPL], ty[HC_PPL];
            if (BOTH) {
                load(2 * k, p);
                load(2 * k + 1, q);
            }
            kp_targets8(hcb + 3 * k, x0, y0, L.fg, tx, ty);
            if (!BOTH) load(2 * k, p);
            use(2 * k, p, tx);
            if (!BOTH) load(2 * k + 1, q);
            use(2 * k + 1, q, ty);
        }
    }

    __device__ __forceinline__ Image image(int bi) const { return Image{scale(bi)}; }
    __device__ __forceinline__ Pixel pixel1(int bi, int x, int y) const { return Pixel{mask_at(bi, x, y)}; }
    __device__ __forceinline__ int label1(int, int, int, int C, const Pixel& P) const { return label_of(P.m, C); }
    __device__ __forceinline__ double weight1(const Image& I, int, int, int, const Pixel& P) const { return (double)kp_weight(P.m, I.scale); }
    template <typename USE>
    __device__ __forceinline__ void planes1(const double* __restrict__ hcb, int, int x, int y, int, const Pixel& P, USE use) const {
        for (int k = 0; k < vn; ++k) {
            float tx = 0.0f, ty = 0.0f;
            if (P.m == 1) {
                const double* hc = hcb + 3 * k;
                kp_target(hc[0], hc[1], hc[2], x, y, motion != 0, tx, ty);
            }
            use(2 * k, tx);
            use(2 * k + 1, ty);
        }
    }
};

struct TargetArgs {
    KpSource K;
    float* vt;   // NULL: not asked for
    float* vw;   // NULL: not asked for
    int64_t ts[4], ws[3];
};

typedef HeadArgs<KpSource> KpHeadArgs;
typedef GradArgs<KpSource> KpGradArgs;

// the image's key-points, from the kernel's own noalias argument
__device__ __forceinline__ const double* image_hcoords(const KpSource& K, const double* __restrict__ hcoords) {
    return hcoords + (size_t)blockIdx.y * K.vn * 3;
}

__device__ __forceinline__ void st8(float* base, int64_t off, const float* v) {
    f32x4 a, b;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        a[i] = v[i];
        b[i] = v[4 + i];
    }
    stv<false, f32x4>(base + off, a);
    stv<false, f32x4>(base + off + 4, b);
}

// ---- the materialising kernel ------------------------------------------------------------------------------------------------------
template <bool FAST>
__global__ __launch_bounds__(HC_T) void vertex_targets_kernel(TargetArgs A, const double* __restrict__ hcoords) {
    const KpSource& K = A.K;
    const int bi = blockIdx.y;
    const double* __restrict__ hcb = hcoords + (size_t)bi * K.vn * 3;
    if (FAST) {
        PVNET_SPARE_VGPRS(KP_TARGETS_FAST_SPARE);
        const int p0 = blockIdx.x * HC_SEG + (int)threadIdx.x * HC_PPL;
        if (p0 >= K.npix) return;   // (npix is a multiple of 8 here: the lane's eight pixels are all inside)
        int lab[HC_PPL];
        float wf[HC_PPL];
        const unsigned fg = K.kp_pixels8<false>(bi, p0, 2, lab, wf);
        if (A.vw) st8(A.vw, (int64_t)bi * A.ws[0] + p0, wf);
        if (!A.vt) return;
        const int y0 = p0 / K.w, x0 = p0 - y0 * K.w;
        const int64_t toff = (int64_t)bi * A.ts[0] + p0;
        for (int k = 0; k < K.vn; ++k) {
            float tx[HC_PPL], ty[HC_PPL];
            K.kp_targets8(hcb + 3 * k, x0, y0, fg, tx, ty);
            st8(A.vt, toff + (int64_t)(2 * k) * A.ts[1], tx);
            st8(A.vt, toff + (int64_t)(2 * k + 1) * A.ts[1], ty);
        }
    } else {
        PVNET_SPARE_VGPRS(KP_TARGETS_GENERAL_SPARE);
        const float scale = K.scale(bi);
        for (int j = 0; j < HC_PPL; ++j) {
            const int p = blockIdx.x * HC_SEG + j * HC_T + (int)threadIdx.x;
            if (p >= K.npix) break;
            const int y = p / K.w, x = p - y * K.w;
            const long long m = K.mask_at(bi, x, y);
            if (A.vw) A.vw[(int64_t)bi * A.ws[0] + (int64_t)y * A.ws[1] + (int64_t)x * A.ws[2]] = kp_weight(m, scale);
            if (!A.vt) continue;
            const int64_t toff = (int64_t)bi * A.ts[0] + (int64_t)y * A.ts[2] + (int64_t)x * A.ts[3];
            for (int k = 0; k < K.vn; ++k) {
                float tx = 0.0f, ty = 0.0f;
                if (m == 1) {
                    const double* hc = hcb + 3 * k;
                    kp_target(hc[0], hc[1], hc[2], x, y, K.motion != 0, tx, ty);
                }
                A.vt[toff + (int64_t)(2 * k) * A.ts[1]] = tx;
                A.vt[toff + (int64_t)(2 * k + 1) * A.ts[1]] = ty;
            }
        }
    }
}

// ---- the head on the key-point source: head_common.h's bodies, the spare-VGPR constants, nothing else --------------------------------
template <int VT, int NT>
__global__ __launch_bounds__(HC_T) void head_partial_kp_kernel(KpHeadArgs A, const double* __restrict__ hcoords) {
    if (VT == VT_F32) PVNET_SPARE_VGPRS(KP_HEAD_FAST_SPARE);
    else PVNET_SPARE_VGPRS(KP_HEAD_FAST16_SPARE);
    head_partial8<VT, NT>(A, image_hcoords(A.T, hcoords));
}

__global__ __launch_bounds__(HC_T) void head_partial_kp_general_kernel(KpHeadArgs A, const double* __restrict__ hcoords) {
    PVNET_SPARE_VGPRS(KP_HEAD_GENERAL_SPARE);
    head_partial1(A, image_hcoords(A.T, hcoords));
}

__global__ __launch_bounds__(HC_FT) void head_final_kp_kernel(KpHeadArgs A) {
    PVNET_SPARE_VGPRS(KP_HEAD_FINAL_SPARE);
    head_final_image(A);
}

template <bool FAST>
__global__ __launch_bounds__(HC_T) void head_grad_kp_wsum_kernel(KpGradArgs A) {
    PVNET_SPARE_VGPRS(KP_GRAD_WSUM_SPARE);
    head_grad_wsum<FAST>(A);
}

__global__ __launch_bounds__(HC_FT) void head_grad_kp_final_kernel(KpGradArgs A) {
    PVNET_SPARE_VGPRS(KP_GRAD_FINAL_SPARE);
    head_grad_final_image(A);
}

template <int VT, int NT>
__global__ __launch_bounds__(HC_T) void head_grad_kp_kernel(KpGradArgs A, const double* __restrict__ hcoords) {
    PVNET_SPARE_VGPRS(KP_GRAD_FAST_SPARE);
    head_grad8<VT, NT>(A, image_hcoords(A.T, hcoords));
}

__global__ __launch_bounds__(HC_T) void head_grad_kp_general_kernel(KpGradArgs A, const double* __restrict__ hcoords) {
    PVNET_SPARE_VGPRS(KP_GRAD_GENERAL_SPARE);
    head_grad1(A, image_hcoords(A.T, hcoords));
}

__global__ __launch_bounds__(HC_FT) void head_grad_kp_status_kernel(KpGradArgs A) {
    PVNET_SPARE_VGPRS(KP_GRAD_STATUS_SPARE);
    head_grad_status_image(A);
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
KpSource make_source(const void* mask, int mask_dtype, const int64_t* mask_strides, const float* weight_scale,
                     int h, int w, int vn, uint32_t flags) {
    KpSource K;
    K.mask = mask;
    K.wscale = weight_scale;
    for (int i = 0; i < 3; ++i) K.ms[i] = mask_strides[i];
    K.mask_dtype = mask_dtype;
    K.vn = vn;
    K.motion = (flags & PVNET_TARGETS_F_MOTION) ? 1 : 0;
    K.w = w;
    K.npix = h * w;
    K.nseg = (int)segments((size_t)K.npix);
    return K;
}

}  // namespace

extern "C" {

int pvnet_targets_abi_version(void) { return PVNET_TARGETS_ABI_VERSION; }

int pvnet_vertex_targets(const void* mask, int mask_dtype, const int64_t mask_strides[3], const double* hcoords,
                         const float* weight_scale, int b, int h, int w, int vn, uint32_t flags, float* vertex,
                         const int64_t v_strides[4], float* vertex_weights, const int64_t w_strides[3], void* stream) {
    const bool pointers = mask && mask_strides && hcoords && (vertex || vertex_weights) && (!vertex || v_strides) &&
                          (!vertex_weights || w_strides);
    if (const int rc = check_args(pointers, mask_dtype, b, h, w, vn, 2, 1.0, flags, PVNET_TARGETS_F_MOTION)) return rc;
    if (b == 0) return 0;
    TargetArgs A;
    A.K = make_source(mask, mask_dtype, mask_strides, weight_scale, h, w, vn, flags);
    A.vt = vertex;
    A.vw = vertex_weights;
    for (int i = 0; i < 4; ++i) A.ts[i] = vertex ? v_strides[i] : 0;
    for (int i = 0; i < 3; ++i) A.ws[i] = vertex_weights ? w_strides[i] : 0;
    const bool fast = A.K.npix % HC_PPL == 0 && linear3(mask, b, A.K.ms, w) && (!vertex || linear4(vertex, b, A.ts, w)) &&
                      (!vertex_weights || linear3(vertex_weights, b, A.ws, w));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)A.K.nseg, (unsigned)b);
    if (fast) hipLaunchKernelGGL(vertex_targets_kernel<true>, grid, dim3(HC_T), 0, s, A, hcoords);
    else hipLaunchKernelGGL(vertex_targets_kernel<false>, grid, dim3(HC_T), 0, s, A, hcoords);
    return launched();
}

size_t pvnet_head_metrics_kp_workspace_bytes(int b, int h, int w) { return head_workspace_bytes(b, h, w); }

int pvnet_head_metrics_kp(const void* seg_pred, const int64_t seg_strides[4], int num_classes, const void* vertex_pred,
                          const int64_t vp_strides[4], const double* hcoords, const float* weight_scale, const void* mask,
                          int mask_dtype, const int64_t mask_strides[3], int b, int h, int w, int vn, double sigma, uint32_t flags,
                          double* losses, int64_t* counts, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    const bool pointers = seg_pred && seg_strides && vertex_pred && vp_strides && hcoords && mask && mask_strides && losses && counts;
    if (const int rc = check_args(pointers, mask_dtype, b, h, w, vn, num_classes, sigma, flags, HEAD_FLAGS | PVNET_TARGETS_F_MOTION)) return rc;
    if (b == 0) return 0;
    if (const int rc = check_workspace(workspace, workspace_bytes, head_workspace_bytes(b, h, w))) return rc;
    KpHeadArgs A;
    A.T = make_source(mask, mask_dtype, mask_strides, weight_scale, h, w, vn, flags);
    fill_inputs(A, seg_pred, seg_strides, num_classes, vertex_pred, vp_strides, h, w, vn, sigma, flags);
    fill_head(A, losses, counts, status, workspace);
    const bool fast = A.npix % HC_PPL == 0 && linear4(seg_pred, b, A.ss, w) && linear4(vertex_pred, b, A.vs, w) && linear3(mask, b, A.T.ms, w);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)A.nseg, (unsigned)b);
    if (fast)
        launch_fast(A.vp_type, flags, [&](auto vt, auto nt) {
            hipLaunchKernelGGL((head_partial_kp_kernel<decltype(vt)::value, decltype(nt)::value>), grid, dim3(HC_T), 0, s, A, hcoords);
        });
    else
        hipLaunchKernelGGL(head_partial_kp_general_kernel, grid, dim3(HC_T), 0, s, A, hcoords);
    hipLaunchKernelGGL(head_final_kp_kernel, dim3((unsigned)b), dim3(HC_FT), 0, s, A);
    return launched();
}

size_t pvnet_head_grad_kp_workspace_bytes(int b, int h, int w) { return grad_workspace_bytes(b, h, w); }

int pvnet_head_grad_kp(const void* seg_pred, const int64_t seg_strides[4], int num_classes, const void* vertex_pred,
                       const int64_t vp_strides[4], const double* hcoords, const float* weight_scale, const void* mask,
                       int mask_dtype, const int64_t mask_strides[3], int b, int h, int w, int vn, double sigma, uint32_t flags,
                       const double* upstream, void* grad_seg, const int64_t gs_strides[4], void* grad_vertex,
                       const int64_t gv_strides[4], int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    const bool pointers = seg_pred && seg_strides && vertex_pred && vp_strides && hcoords && mask && mask_strides && upstream &&
                          (grad_seg || grad_vertex) && (!grad_seg || gs_strides) && (!grad_vertex || gv_strides);
    if (const int rc = check_args(pointers, mask_dtype, b, h, w, vn, num_classes, sigma, flags, HEAD_FLAGS | PVNET_TARGETS_F_MOTION)) return rc;
    if (b == 0) return 0;
    if (const int rc = check_workspace(workspace, workspace_bytes, grad_workspace_bytes(b, h, w))) return rc;
    KpGradArgs A;
    A.T = make_source(mask, mask_dtype, mask_strides, weight_scale, h, w, vn, flags);
    fill_inputs(A, seg_pred, seg_strides, num_classes, vertex_pred, vp_strides, h, w, vn, sigma, flags);
    fill_grad(A, b, upstream, grad_seg, gs_strides, grad_vertex, gv_strides, status, workspace);
    // the mask is read by either half; each half asks the fast path's shape of its own tensors beyond it
    const bool lin_m = linear3(mask, b, A.T.ms, w);
    const bool fast = A.npix % HC_PPL == 0 && lin_m && (!grad_seg || (linear4(seg_pred, b, A.ss, w) && linear4(grad_seg, b, A.gss, w))) &&
                      (!grad_vertex || (linear4(vertex_pred, b, A.vs, w) && linear4(grad_vertex, b, A.gvs, w)));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)A.nseg, (unsigned)b);
    if (grad_vertex) {
        if (A.npix % HC_PPL == 0 && lin_m) hipLaunchKernelGGL(head_grad_kp_wsum_kernel<true>, grid, dim3(HC_T), 0, s, A);
        else hipLaunchKernelGGL(head_grad_kp_wsum_kernel<false>, grid, dim3(HC_T), 0, s, A);
    }
    hipLaunchKernelGGL(head_grad_kp_final_kernel, dim3((unsigned)b), dim3(HC_FT), 0, s, A);
    if (fast)
        launch_fast(A.vp_type, flags, [&](auto vt, auto nt) {
            hipLaunchKernelGGL((head_grad_kp_kernel<decltype(vt)::value, decltype(nt)::value>), grid, dim3(HC_T), 0, s, A, hcoords);
        });
    else
        hipLaunchKernelGGL(head_grad_kp_general_kernel, grid, dim3(HC_T), 0, s, A, hcoords);
    if (status) hipLaunchKernelGGL(head_grad_kp_status_kernel, dim3((unsigned)b), dim3(HC_FT), 0, s, A);
    return launched();
}

}  // extern "C"
