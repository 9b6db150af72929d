// head_targets.hip -- the training targets of the vector field made on the device from the key-points, and the network head's forward
// and backward fused with them.  The whole of libpvnet_targets.so; C ABI: include/pvnet_targets.h (the definition is stated there).
//
// The reference makes `vertex` and `vertex_weights` on the host, per sample (compute_vertex_hcoords, lib/datasets/linemod_dataset.py
// :68-81 and :224-227), and ships 76 bytes per pixel to the device; both are a function of the mask and of 27 numbers per image.
// kp_target below is that function for one pixel and one key-point; the three entry points call nothing else for a target:
//
//   vertex_targets_kernel<FAST>      grid (segments of 1 024 pixels, images).  Reads the mask, writes the 2 vn target planes and the
//                                    weights: 76 bytes per pixel written at vn = 9, plainly -- the head reads them next.  Fast path:
//                                    eight consecutive pixels per lane, 16 bytes per store (mask and outputs contiguous in the
//                                    pixels, 16-byte aligned, h * w a multiple of 8); else a pixel per lane and store, any strides.
//   head_partial_kp_kernel<VT, NT>   head_metrics.hip's head_partial_kernel / head_partial_general_kernel / head_final_kernel with the
//   head_partial_kp_general_kernel   target and the weight of a pixel computed in registers instead of loaded: 88 bytes per pixel read
//   head_final_kp_kernel             instead of 164 (float32 predictions, int64 masks, vn = 9).  Same grid, segments, records and
//                                    summation order, the same float32 targets into the same float64 terms: equal bit for bit.
//   head_grad_kp_wsum_kernel<FAST>   head_grad.hip's five kernels likewise: 88 bytes read and 80 written per pixel instead of 244
//   head_grad_kp_final_kernel        moved.  The weights' sum reads the mask (the weight of a pixel is its mask value times the
//   head_grad_kp_kernel<VT, NT>      image's scale).
//   head_grad_kp_general_kernel
//   head_grad_kp_status_kernel
//
// The image's key-points are held in SGPRs.  They reach the kernels as an argument of their own, `const double* __restrict__`, not
// through the argument struct: a pointer in a struct passed by value is not noalias, and beside the kernels' stores the compiler then
// read it with per-lane vector loads.  As a noalias argument at a uniform address (blockIdx.y, the loop counter) the three doubles are
// one s_load_dwordx4 and one s_load_dwordx2 per key-point.  A lane whose eight pixels hold no mask == 1 takes no float64 square root
// or divide, and a wave of such lanes branches over them; its targets are zeros.  The predictions are still read at every pixel -- a NaN at a background pixel reaches the loss and the gradient as 0 * NaN.
//
// The per-pixel helpers, the records and the per-image bodies are head_common.h's, shared with head_metrics.hip and head_grad.hip.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "head_common.h"
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
#define KP_GRAD_FAST_SPARE 135
#define KP_GRAD_GENERAL_SPARE 87
#define KP_GRAD_WSUM_SPARE 39
#define KP_GRAD_FINAL_SPARE 31
#define KP_GRAD_STATUS_SPARE 23

// what the three entry points share: where the mask and the key-points are
struct KpSource {
    const void* mask;
    const float* __restrict__ wscale;   // NULL or [b]
    int64_t ms[3];
    int mask_dtype, vn, motion;
    int h, w, npix, nseg;
};

struct TargetArgs {
    KpSource K;
    float* vt;   // NULL: not asked for
    float* vw;   // NULL: not asked for
    int64_t ts[4], ws[3];
};

struct KpHeadArgs {
    KpSource K;
    const void* seg;
    const void* vp;
    int64_t ss[4], vs[4];
    int seg_type, vp_type, num_classes, planes;
    int npix, nseg;
    double hs, inv, half;   // sigma^2 / 2, 1 / sigma^2, 0.5 / sigma^2
    double* losses;
    int64_t* counts;
    int32_t* status;
    HeadPartial* partial;
};

struct KpGradArgs {
    KpSource K;
    const void* seg;
    const void* vp;
    void* gs;   // NULL: the logits' half is skipped
    void* gv;   // NULL: the field's half is skipped
    int64_t ss[4], vs[4], gss[4], gvs[4];
    int seg_type, vp_type, num_classes, planes;
    int npix, nseg;
    double s2, inv;   // sigma^2, 1 / sigma^2
    const double* upstream;
    double* coef;     // [b][2]: u_s / (h w), u_v / D_i
    double* wpart;    // [b][nseg]: a segment's sum of the weights
    int32_t* bad;     // [b][nseg]: the segment holds a label outside 0 .. C-1
    int32_t* status;
};

// ---- THE definition (linemod_dataset.py:72-77): the target of the pixel (x, y) with mask == 1 for the key-point (hx, hy, hz).  Every
//      operation is one IEEE float64 operation, in the reference's order; the result is rounded once to float32 ----------------------
__device__ __forceinline__ void kp_target(double hx, double hy, double hz, int x, int y, bool motion, float& tx, float& ty) {
    double vx = hx - (double)x * hz, vy = hy - (double)y * hz;
    if (!motion) {
        double n = sqrt(vx * vx + vy * vy);
        if (n < 1e-3) n = n + 1e-3;
        vx = vx / n;
        vy = vy / n;
    }
    tx = (float)vx;
    ty = (float)vy;
}

// the weight of a pixel: the mask's value as float32 (mask.float()) times the image's scale
__device__ __forceinline__ float kp_weight(long long m, float scale) { return (float)m * scale; }

__device__ __forceinline__ float kp_scale(const KpSource& K, int bi) { return K.wscale ? K.wscale[bi] : 1.0f; }

// the targets of key-point k for a lane's eight consecutive pixels from (x0, y0) on; fg: bit i set where mask == 1.  A lane without
// such a pixel skips the float64 work (and so does a wave of such lanes).
__device__ __forceinline__ void kp_targets8(const KpSource& K, const double* __restrict__ hc, int x0, int y0, unsigned fg, float* tx, float* ty) {
    const double hx = hc[0], hy = hc[1], hz = hc[2];
#pragma unroll
    for (int i = 0; i < HC_PPL; ++i) tx[i] = ty[i] = 0.0f;
    if (fg == 0) return;
    int x = x0, y = y0;
#pragma unroll
    for (int i = 0; i < HC_PPL; ++i) {
        float ax, ay;
        kp_target(hx, hy, hz, x, y, K.motion != 0, ax, ay);
        tx[i] = (fg >> i) & 1u ? ax : 0.0f;
        ty[i] = (fg >> i) & 1u ? ay : 0.0f;
        if (++x == K.w) {
            x = 0;
            ++y;
        }
    }
}

// a lane's eight mask values -> labels, weights, the mask == 1 bits
template <bool NT>
__device__ __forceinline__ unsigned kp_pixels8(const KpSource& K, int bi, int p0, int C, int* lab, float* wf) {
    long long mv[HC_PPL];
    load8_mask<NT>(K.mask_dtype, K.mask, (int64_t)bi * K.ms[0] + p0, mv);
    const float scale = kp_scale(K, bi);
    unsigned fg = 0;
#pragma unroll
    for (int i = 0; i < HC_PPL; ++i) {
        lab[i] = label_of(mv[i], C);
        wf[i] = kp_weight(mv[i], scale);
        fg |= mv[i] == 1 ? 1u << i : 0u;
    }
    return fg;
}

__device__ __forceinline__ long long kp_mask_at(const KpSource& K, int bi, int x, int y) {
    return load_label_rt(K.mask_dtype, K.mask, (int64_t)bi * K.ms[0] + (int64_t)y * K.ms[1] + (int64_t)x * K.ms[2]);
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
        const unsigned fg = kp_pixels8<false>(K, bi, p0, 2, lab, wf);
        if (A.vw) st8(A.vw, (int64_t)bi * A.ws[0] + p0, wf);
        if (!A.vt) return;
        const int y0 = p0 / K.w, x0 = p0 - y0 * K.w;
        const int64_t toff = (int64_t)bi * A.ts[0] + p0;
        for (int k = 0; k < K.vn; ++k) {
            float tx[HC_PPL], ty[HC_PPL];
            kp_targets8(K, hcb + 3 * k, x0, y0, fg, tx, ty);
            st8(A.vt, toff + (int64_t)(2 * k) * A.ts[1], tx);
            st8(A.vt, toff + (int64_t)(2 * k + 1) * A.ts[1], ty);
        }
    } else {
        PVNET_SPARE_VGPRS(KP_TARGETS_GENERAL_SPARE);
        const float scale = kp_scale(K, bi);
        for (int j = 0; j < HC_PPL; ++j) {
            const int p = blockIdx.x * HC_SEG + j * HC_T + (int)threadIdx.x;
            if (p >= K.npix) break;
            const int y = p / K.w, x = p - y * K.w;
            const long long m = kp_mask_at(K, bi, x, y);
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

// ---- the fused forward: head_metrics.hip's three kernels, targets and weights from kp_target / kp_weight ---------------------------
template <int VT, int NT>
__global__ __launch_bounds__(HC_T) void head_partial_kp_kernel(KpHeadArgs A, const double* __restrict__ hcoords) {
    if (VT == VT_F32) PVNET_SPARE_VGPRS(KP_HEAD_FAST_SPARE);
    else PVNET_SPARE_VGPRS(KP_HEAD_FAST16_SPARE);
    constexpr bool NT_P = NT == NT_ALL, NT_T = NT != NT_NONE;   // predictions, mask
    const KpSource& K = A.K;
    const int bi = blockIdx.y;
    const double* __restrict__ hcb = hcoords + (size_t)bi * K.vn * 3;
    const int p0 = blockIdx.x * HC_SEG + (int)threadIdx.x * HC_PPL;
    Acc acc;
    if (p0 < A.npix) {   // (npix is a multiple of 8 here: the lane's eight pixels are all inside)
        int lab[HC_PPL];
        float wf[HC_PPL];
        const unsigned fg = kp_pixels8<NT_T>(K, bi, p0, A.num_classes, lab, wf);
        // ---- class logits: maximum and arg-max in one pass, then sum exp(s - max) in a second (the planes are in cache) -------------
        const int64_t soff = (int64_t)bi * A.ss[0] + p0;
        float best[HC_PPL], sl[HC_PPL], s[HC_PPL];
        bool pfg[HC_PPL];
        load8_rt<NT_P>(A.seg_type, A.seg, soff, best);
#pragma unroll
        for (int i = 0; i < HC_PPL; ++i) {
            pfg[i] = false;
            sl[i] = best[i];   // label 0, or a bad label (not used then)
        }
        for (int c = 1; c < A.num_classes; ++c) {
            load8_rt<NT_P>(A.seg_type, A.seg, soff + (int64_t)c * A.ss[1], s);
#pragma unroll
            for (int i = 0; i < HC_PPL; ++i) {
                const bool take = takes_over(best[i], s[i]);
                best[i] = take ? s[i] : best[i];
                pfg[i] = take ? true : pfg[i];
                sl[i] = lab[i] == c ? s[i] : sl[i];
            }
        }
        double sum[HC_PPL];
#pragma unroll
        for (int i = 0; i < HC_PPL; ++i) sum[i] = 0.0;
        for (int c = 0; c < A.num_classes; ++c) {
            load8_rt<NT_P>(A.seg_type, A.seg, soff + (int64_t)c * A.ss[1], s);
#pragma unroll
            for (int i = 0; i < HC_PPL; ++i) sum[i] = sum[i] + exp((double)s[i] - (double)best[i]);
        }
#pragma unroll
        for (int i = 0; i < HC_PPL; ++i) {
            if (lab[i] >= 0) acc.ce = acc.ce + cross_entropy(sum[i], sl[i], best[i]);
            acc.packed += confusion(pfg[i], lab[i]);
        }
        // ---- the field: vn pairs of planes of prediction against the key-point's targets, under the mask's weights ------------------
        double wd[HC_PPL];
#pragma unroll
        for (int i = 0; i < HC_PPL; ++i) {
            wd[i] = (double)wf[i];
            acc.wsum = acc.wsum + wd[i];
        }
        const int y0 = p0 / K.w, x0 = p0 - y0 * K.w;
        const int64_t poff = (int64_t)bi * A.vs[0] + p0;
        for (int k = 0; k < K.vn; ++k) {
            float p[HC_PPL], tx[HC_PPL], ty[HC_PPL];
            kp_targets8(K, hcb + 3 * k, x0, y0, fg, tx, ty);
            load8<VT, NT_P>(A.vp, poff + (int64_t)(2 * k) * A.vs[1], p);
#pragma unroll
            for (int i = 0; i < HC_PPL; ++i) acc.sl1 = acc.sl1 + smooth_l1(A, wd[i], p[i], tx[i]);
            load8<VT, NT_P>(A.vp, poff + (int64_t)(2 * k + 1) * A.vs[1], p);
#pragma unroll
            for (int i = 0; i < HC_PPL; ++i) acc.sl1 = acc.sl1 + smooth_l1(A, wd[i], p[i], ty[i]);
        }
    }
    if (block_reduce<HC_T>(acc)) store_partial(A, acc);
}

__global__ __launch_bounds__(HC_T) void head_partial_kp_general_kernel(KpHeadArgs A, const double* __restrict__ hcoords) {
    PVNET_SPARE_VGPRS(KP_HEAD_GENERAL_SPARE);
    const KpSource& K = A.K;
    const int bi = blockIdx.y;
    const double* __restrict__ hcb = hcoords + (size_t)bi * K.vn * 3;
    const float scale = kp_scale(K, bi);
    Acc acc;
    for (int j = 0; j < HC_PPL; ++j) {
        const int p = blockIdx.x * HC_SEG + j * HC_T + (int)threadIdx.x;
        if (p >= A.npix) break;
        const int y = p / K.w, x = p - y * K.w;
        const long long m = kp_mask_at(K, bi, x, y);
        const int lab = label_of(m, A.num_classes);
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
        const double wd = (double)kp_weight(m, scale);
        acc.wsum = acc.wsum + wd;
        const int64_t poff = (int64_t)bi * A.vs[0] + (int64_t)y * A.vs[2] + (int64_t)x * A.vs[3];
        for (int k = 0; k < K.vn; ++k) {
            float tx = 0.0f, ty = 0.0f;
            if (m == 1) {
                const double* hc = hcb + 3 * k;
                kp_target(hc[0], hc[1], hc[2], x, y, K.motion != 0, tx, ty);
            }
            acc.sl1 = acc.sl1 + smooth_l1(A, wd, pvd::ld_elem_rt(A.vp_type, A.vp, poff + (int64_t)(2 * k) * A.vs[1]), tx);
            acc.sl1 = acc.sl1 + smooth_l1(A, wd, pvd::ld_elem_rt(A.vp_type, A.vp, poff + (int64_t)(2 * k + 1) * A.vs[1]), ty);
        }
    }
    if (block_reduce<HC_T>(acc)) store_partial(A, acc);
}

__global__ __launch_bounds__(HC_FT) void head_final_kp_kernel(KpHeadArgs A) {
    PVNET_SPARE_VGPRS(KP_HEAD_FINAL_SPARE);
    head_final_image(A);
}

// ---- the fused backward: head_grad.hip's five kernels likewise --------------------------------------------------------------------
template <bool FAST>
__global__ __launch_bounds__(HC_T) void head_grad_kp_wsum_kernel(KpGradArgs A) {
    PVNET_SPARE_VGPRS(KP_GRAD_WSUM_SPARE);
    const KpSource& K = A.K;
    const int bi = blockIdx.y;
    const float scale = kp_scale(K, bi);
    double acc = 0.0;
    if (FAST) {
        const int p0 = blockIdx.x * HC_SEG + (int)threadIdx.x * HC_PPL;
        if (p0 < A.npix) {   // (npix is a multiple of 8 here: the lane's eight pixels are all inside)
            long long mv[HC_PPL];
            load8_mask<false>(K.mask_dtype, K.mask, (int64_t)bi * K.ms[0] + p0, mv);
#pragma unroll
            for (int i = 0; i < HC_PPL; ++i) acc = acc + (double)kp_weight(mv[i], scale);
        }
    } else {
        for (int j = 0; j < HC_PPL; ++j) {
            const int p = blockIdx.x * HC_SEG + j * HC_T + (int)threadIdx.x;
            if (p >= A.npix) break;
            const int y = p / K.w, x = p - y * K.w;
            acc = acc + (double)kp_weight(kp_mask_at(K, bi, x, y), scale);
        }
    }
    acc = block_sum<HC_T>(acc);
    if (threadIdx.x == 0) A.wpart[(size_t)bi * A.nseg + blockIdx.x] = acc;
}

__global__ __launch_bounds__(HC_FT) void head_grad_kp_final_kernel(KpGradArgs A) {
    PVNET_SPARE_VGPRS(KP_GRAD_FINAL_SPARE);
    head_grad_final_image(A);
}

template <int VT, int NT>
__global__ __launch_bounds__(HC_T) void head_grad_kp_kernel(KpGradArgs A, const double* __restrict__ hcoords) {
    PVNET_SPARE_VGPRS(KP_GRAD_FAST_SPARE);
    constexpr bool NT_P = NT == NT_ALL, NT_T = NT != NT_NONE, NT_S = NT == NT_ALL;   // predictions, mask, stores
    const KpSource& K = A.K;
    const int bi = blockIdx.y;
    const double* __restrict__ hcb = hcoords + (size_t)bi * K.vn * 3;
    const int p0 = blockIdx.x * HC_SEG + (int)threadIdx.x * HC_PPL;
    const bool inside = p0 < A.npix;   // (npix is a multiple of 8 here: the lane's eight pixels are all inside)
    int bad = 0;
    int lab[HC_PPL];
    float wf[HC_PPL];
    unsigned fg = 0;
    if (inside) fg = kp_pixels8<NT_T>(K, bi, p0, A.num_classes, lab, wf);   // both halves read the mask
    if (inside && A.gs) {
        const double ks = A.coef[2 * bi];
        // ---- the maximum, then sum exp(s - max) and the share of the classes other than the label's, then the gradients: the planes
        //      are in cache after the first pass -----------------------------------------------------------------------------------
        const int64_t soff = (int64_t)bi * A.ss[0] + p0, goff = (int64_t)bi * A.gss[0] + p0;
        float best[HC_PPL], s[HC_PPL];
        load8_rt<NT_P>(A.seg_type, A.seg, soff, best);
        for (int c = 1; c < A.num_classes; ++c) {
            load8_rt<NT_P>(A.seg_type, A.seg, soff + (int64_t)c * A.ss[1], s);
#pragma unroll
            for (int i = 0; i < HC_PPL; ++i) best[i] = takes_over(best[i], s[i]) ? s[i] : best[i];
        }
        double sum[HC_PPL], rest[HC_PPL];
#pragma unroll
        for (int i = 0; i < HC_PPL; ++i) {
            sum[i] = 0.0;
            rest[i] = 0.0;
            bad |= lab[i] < 0;
        }
        for (int c = 0; c < A.num_classes; ++c) {
            load8_rt<NT_P>(A.seg_type, A.seg, soff + (int64_t)c * A.ss[1], s);
#pragma unroll
            for (int i = 0; i < HC_PPL; ++i) {
                const double e = exp((double)s[i] - (double)best[i]);
                sum[i] = sum[i] + e;
                rest[i] = rest[i] + (lab[i] == c ? 0.0 : e);
            }
        }
        for (int c = 0; c < A.num_classes; ++c) {
            load8_rt<NT_P>(A.seg_type, A.seg, soff + (int64_t)c * A.ss[1], s);
            double g[HC_PPL];
#pragma unroll
            for (int i = 0; i < HC_PPL; ++i)
                g[i] = logit_grad(lab[i], c, exp((double)s[i] - (double)best[i]), sum[i], rest[i], ks);
            store8_rt<NT_S>(A.seg_type, A.gs, goff + (int64_t)c * A.gss[1], g);
        }
    }
    if (inside && A.gv) {
        // ---- the field: vn pairs of planes of prediction against the key-point's targets, under the mask's weights ------------------
        const double kv = A.coef[2 * bi + 1];
        double wd[HC_PPL];
#pragma unroll
        for (int i = 0; i < HC_PPL; ++i) wd[i] = (double)wf[i];
        const int y0 = p0 / K.w, x0 = p0 - y0 * K.w;
        const int64_t poff = (int64_t)bi * A.vs[0] + p0, goff = (int64_t)bi * A.gvs[0] + p0;
        for (int k = 0; k < K.vn; ++k) {
            float p[HC_PPL], q[HC_PPL], tx[HC_PPL], ty[HC_PPL];
            double g[HC_PPL];
            load8<VT, NT_P>(A.vp, poff + (int64_t)(2 * k) * A.vs[1], p);
            load8<VT, NT_P>(A.vp, poff + (int64_t)(2 * k + 1) * A.vs[1], q);
            kp_targets8(K, hcb + 3 * k, x0, y0, fg, tx, ty);
#pragma unroll
            for (int i = 0; i < HC_PPL; ++i) g[i] = field_grad(A, wd[i], p[i], tx[i], kv);
            store8<VT, NT_S>(A.gv, goff + (int64_t)(2 * k) * A.gvs[1], g);
#pragma unroll
            for (int i = 0; i < HC_PPL; ++i) g[i] = field_grad(A, wd[i], q[i], ty[i], kv);
            store8<VT, NT_S>(A.gv, goff + (int64_t)(2 * k + 1) * A.gvs[1], g);
        }
    }
    if (A.gs) {   // (uniform over the grid: every lane reaches the barrier)
        const int any = __syncthreads_or(bad);
        if (threadIdx.x == 0) A.bad[(size_t)bi * A.nseg + blockIdx.x] = any ? 1 : 0;
    }
}

__global__ __launch_bounds__(HC_T) void head_grad_kp_general_kernel(KpGradArgs A, const double* __restrict__ hcoords) {
    PVNET_SPARE_VGPRS(KP_GRAD_GENERAL_SPARE);
    const KpSource& K = A.K;
    const int bi = blockIdx.y;
    const double* __restrict__ hcb = hcoords + (size_t)bi * K.vn * 3;
    const float scale = kp_scale(K, bi);
    int bad = 0;
    for (int j = 0; j < HC_PPL; ++j) {
        const int p = blockIdx.x * HC_SEG + j * HC_T + (int)threadIdx.x;
        if (p >= A.npix) break;
        const int y = p / K.w, x = p - y * K.w;
        const long long m = kp_mask_at(K, bi, x, y);
        if (A.gs) {
            const double ks = A.coef[2 * bi];
            const int lab = label_of(m, A.num_classes);
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
            const double wd = (double)kp_weight(m, scale);
            const int64_t poff = (int64_t)bi * A.vs[0] + (int64_t)y * A.vs[2] + (int64_t)x * A.vs[3];
            const int64_t goff = (int64_t)bi * A.gvs[0] + (int64_t)y * A.gvs[2] + (int64_t)x * A.gvs[3];
            for (int k = 0; k < K.vn; ++k) {
                float tx = 0.0f, ty = 0.0f;
                if (m == 1) {
                    const double* hc = hcb + 3 * k;
                    kp_target(hc[0], hc[1], hc[2], x, y, K.motion != 0, tx, ty);
                }
                store_elem_rt(A.vp_type, A.gv, goff + (int64_t)(2 * k) * A.gvs[1],
                              field_grad(A, wd, pvd::ld_elem_rt(A.vp_type, A.vp, poff + (int64_t)(2 * k) * A.vs[1]), tx, kv));
                store_elem_rt(A.vp_type, A.gv, goff + (int64_t)(2 * k + 1) * A.gvs[1],
                              field_grad(A, wd, pvd::ld_elem_rt(A.vp_type, A.vp, poff + (int64_t)(2 * k + 1) * A.vs[1]), ty, kv));
            }
        }
    }
    if (A.gs) {
        const int any = __syncthreads_or(bad);
        if (threadIdx.x == 0) A.bad[(size_t)bi * A.nseg + blockIdx.x] = any ? 1 : 0;
    }
}

__global__ __launch_bounds__(HC_FT) void head_grad_kp_status_kernel(KpGradArgs A) {
    PVNET_SPARE_VGPRS(KP_GRAD_STATUS_SPARE);
    head_grad_status_image(A);
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
constexpr uint32_t HEAD_FLAGS = PVNET_HEAD_F_VERTEX_F16 | PVNET_HEAD_F_VERTEX_BF16 | PVNET_HEAD_F_LOGITS_F16 | PVNET_HEAD_F_LOGITS_BF16 |
                                PVNET_HEAD_F_NT_NONE | PVNET_HEAD_F_NT_ALL;

// the checks of the mask, the key-points and the sizes, in the order of the two head libraries: 0 or the code to return
int check_source(const void* mask, int mask_dtype, const int64_t* mask_strides, const double* hcoords, int b, int h, int w, int vn) {
    if (!mask || !mask_strides || !hcoords) return PVNET_E_BADARG;
    if (b < 0 || h <= 0 || w <= 0 || vn <= 0) return PVNET_E_BADARG;
    if (mask_dtype == PVNET_MASK_I16 || mask_dtype == PVNET_MASK_F32 || mask_dtype == PVNET_MASK_LOGITS_F32) return PVNET_E_UNSUPPORTED;
    if (mask_dtype != PVNET_MASK_U8 && mask_dtype != PVNET_MASK_I32 && mask_dtype != PVNET_MASK_I64) return PVNET_E_BADARG;
    if (b > HC_MAX_B || (long long)h * w > HC_MAX_PIXELS || vn > (1 << 20)) return PVNET_E_UNSUPPORTED;
    return 0;
}

// the checks the two fused calls share beyond check_source
int check_head(const void* seg_pred, const int64_t* seg_strides, int num_classes, const void* vertex_pred, const int64_t* vp_strides,
               double sigma, uint32_t flags) {
    if (!seg_pred || !seg_strides || !vertex_pred || !vp_strides) return PVNET_E_BADARG;
    if (num_classes < 2 || !(sigma > 0.0) || !isfinite(sigma) || (flags & ~(HEAD_FLAGS | PVNET_TARGETS_F_MOTION)) != 0) return PVNET_E_BADARG;
    if (((flags & PVNET_HEAD_F_VERTEX_F16) && (flags & PVNET_HEAD_F_VERTEX_BF16)) ||
        ((flags & PVNET_HEAD_F_LOGITS_F16) && (flags & PVNET_HEAD_F_LOGITS_BF16)) ||
        ((flags & PVNET_HEAD_F_NT_NONE) && (flags & PVNET_HEAD_F_NT_ALL)))
        return PVNET_E_BADARG;
    return 0;
}

KpSource make_source(const void* mask, int mask_dtype, const int64_t* mask_strides, const float* weight_scale,
                     int h, int w, int vn, uint32_t flags) {
    KpSource K;
    K.mask = mask;
    K.wscale = weight_scale;
    for (int i = 0; i < 3; ++i) K.ms[i] = mask_strides[i];
    K.mask_dtype = mask_dtype;
    K.vn = vn;
    K.motion = (flags & PVNET_TARGETS_F_MOTION) ? 1 : 0;
    K.h = h;
    K.w = w;
    K.npix = h * w;
    K.nseg = (K.npix + HC_SEG - 1) / HC_SEG;
    return K;
}

template <int VT>
void launch_head_fast(int nt, dim3 grid, hipStream_t s, const KpHeadArgs& A, const double* hc) {
    if (nt == NT_NONE) hipLaunchKernelGGL((head_partial_kp_kernel<VT, NT_NONE>), grid, dim3(HC_T), 0, s, A, hc);
    else if (nt == NT_ALL) hipLaunchKernelGGL((head_partial_kp_kernel<VT, NT_ALL>), grid, dim3(HC_T), 0, s, A, hc);
    else hipLaunchKernelGGL((head_partial_kp_kernel<VT, NT_TARGETS>), grid, dim3(HC_T), 0, s, A, hc);
}

template <int VT>
void launch_grad_fast(int nt, dim3 grid, hipStream_t s, const KpGradArgs& A, const double* hc) {
    if (nt == NT_NONE) hipLaunchKernelGGL((head_grad_kp_kernel<VT, NT_NONE>), grid, dim3(HC_T), 0, s, A, hc);
    else if (nt == NT_ALL) hipLaunchKernelGGL((head_grad_kp_kernel<VT, NT_ALL>), grid, dim3(HC_T), 0, s, A, hc);
    else hipLaunchKernelGGL((head_grad_kp_kernel<VT, NT_TARGETS>), grid, dim3(HC_T), 0, s, A, hc);
}

size_t partial_bytes(int b, int h, int w) {
    const size_t nseg = ((size_t)h * w + HC_SEG - 1) / HC_SEG;
    return round256((size_t)b * nseg * sizeof(HeadPartial));
}

bool sizes_ok(int b, int h, int w) { return b > 0 && h > 0 && w > 0 && b <= HC_MAX_B && (long long)h * w <= HC_MAX_PIXELS; }

}  // namespace

extern "C" {

int pvnet_targets_abi_version(void) { return PVNET_TARGETS_ABI_VERSION; }

int pvnet_vertex_targets(const void* mask, int mask_dtype, const int64_t mask_strides[3], const double* hcoords,
                         const float* weight_scale, int b, int h, int w, int vn, uint32_t flags, float* vertex,
                         const int64_t v_strides[4], float* vertex_weights, const int64_t w_strides[3], void* stream) {
    if ((!vertex && !vertex_weights) || (vertex && !v_strides) || (vertex_weights && !w_strides)) return PVNET_E_BADARG;
    if ((flags & ~(uint32_t)PVNET_TARGETS_F_MOTION) != 0) return PVNET_E_BADARG;
    if (const int rc = check_source(mask, mask_dtype, mask_strides, hcoords, b, h, w, vn)) return rc;
    if (b == 0) return 0;
    TargetArgs A;
    A.K = make_source(mask, mask_dtype, mask_strides, weight_scale, h, w, vn, flags);
    A.vt = vertex;
    A.vw = vertex_weights;
    for (int i = 0; i < 4; ++i) A.ts[i] = vertex ? v_strides[i] : 0;
    for (int i = 0; i < 3; ++i) A.ws[i] = vertex_weights ? w_strides[i] : 0;
    const bool fast = A.K.npix % HC_PPL == 0 && plane_linear(mask, b, A.K.ms[0], 0, A.K.ms[1], A.K.ms[2], w) &&
                      (!vertex || plane_linear(vertex, b, A.ts[0], A.ts[1], A.ts[2], A.ts[3], w)) &&
                      (!vertex_weights || plane_linear(vertex_weights, b, A.ws[0], 0, A.ws[1], A.ws[2], w));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)A.K.nseg, (unsigned)b);
    if (fast) hipLaunchKernelGGL(vertex_targets_kernel<true>, grid, dim3(HC_T), 0, s, A, hcoords);
    else hipLaunchKernelGGL(vertex_targets_kernel<false>, grid, dim3(HC_T), 0, s, A, hcoords);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

size_t pvnet_head_metrics_kp_workspace_bytes(int b, int h, int w) { return sizes_ok(b, h, w) ? partial_bytes(b, h, w) : 0; }

int pvnet_head_metrics_kp(const void* seg_pred, const int64_t seg_strides[4], int num_classes, const void* vertex_pred,
                          const int64_t vp_strides[4], const double* hcoords, const float* weight_scale, const void* mask,
                          int mask_dtype, const int64_t mask_strides[3], int b, int h, int w, int vn, double sigma, uint32_t flags,
                          double* losses, int64_t* counts, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    if (!losses || !counts) return PVNET_E_BADARG;
    if (const int rc = check_head(seg_pred, seg_strides, num_classes, vertex_pred, vp_strides, sigma, flags)) return rc;
    if (const int rc = check_source(mask, mask_dtype, mask_strides, hcoords, b, h, w, vn)) return rc;
    if (b == 0) return 0;
    if (!workspace || workspace_bytes < pvnet_head_metrics_kp_workspace_bytes(b, h, w)) return PVNET_E_WORKSPACE;
    if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0) return PVNET_E_BADARG;
    KpHeadArgs A;
    A.K = make_source(mask, mask_dtype, mask_strides, weight_scale, h, w, vn, flags);
    A.seg = seg_pred;
    A.vp = vertex_pred;
    for (int i = 0; i < 4; ++i) {
        A.ss[i] = seg_strides[i];
        A.vs[i] = vp_strides[i];
    }
    A.seg_type = type_of(flags, PVNET_HEAD_F_LOGITS_F16, PVNET_HEAD_F_LOGITS_BF16);
    A.vp_type = type_of(flags, PVNET_HEAD_F_VERTEX_F16, PVNET_HEAD_F_VERTEX_BF16);
    A.num_classes = num_classes;
    A.planes = 2 * vn;
    A.npix = A.K.npix;
    A.nseg = A.K.nseg;
    const double s2 = sigma * sigma;
    A.hs = s2 / 2.0;
    A.inv = 1.0 / s2;
    A.half = 0.5 / s2;
    A.losses = losses;
    A.counts = counts;
    A.status = status;
    A.partial = static_cast<HeadPartial*>(workspace);
    const bool fast = A.npix % HC_PPL == 0 && plane_linear(seg_pred, b, A.ss[0], A.ss[1], A.ss[2], A.ss[3], w) &&
                      plane_linear(vertex_pred, b, A.vs[0], A.vs[1], A.vs[2], A.vs[3], w) &&
                      plane_linear(mask, b, A.K.ms[0], 0, A.K.ms[1], A.K.ms[2], w);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)A.nseg, (unsigned)b);
    if (fast) {
        const int nt = (flags & PVNET_HEAD_F_NT_NONE) ? NT_NONE : (flags & PVNET_HEAD_F_NT_ALL) ? NT_ALL : NT_TARGETS;
        if (A.vp_type == VT_F16) launch_head_fast<VT_F16>(nt, grid, s, A, hcoords);
        else if (A.vp_type == VT_BF16) launch_head_fast<VT_BF16>(nt, grid, s, A, hcoords);
        else launch_head_fast<VT_F32>(nt, grid, s, A, hcoords);
    } else {
        hipLaunchKernelGGL(head_partial_kp_general_kernel, grid, dim3(HC_T), 0, s, A, hcoords);
    }
    hipLaunchKernelGGL(head_final_kp_kernel, dim3((unsigned)b), dim3(HC_FT), 0, s, A);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

size_t pvnet_head_grad_kp_workspace_bytes(int b, int h, int w) {
    if (!sizes_ok(b, h, w)) return 0;
    const size_t nseg = ((size_t)h * w + HC_SEG - 1) / HC_SEG;
    return round256((size_t)b * 2 * sizeof(double)) + round256((size_t)b * nseg * sizeof(double)) + round256((size_t)b * nseg * sizeof(int32_t));
}

int pvnet_head_grad_kp(const void* seg_pred, const int64_t seg_strides[4], int num_classes, const void* vertex_pred,
                       const int64_t vp_strides[4], const double* hcoords, const float* weight_scale, const void* mask,
                       int mask_dtype, const int64_t mask_strides[3], int b, int h, int w, int vn, double sigma, uint32_t flags,
                       const double* upstream, void* grad_seg, const int64_t gs_strides[4], void* grad_vertex,
                       const int64_t gv_strides[4], int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    if (!upstream) return PVNET_E_BADARG;
    if ((!grad_seg && !grad_vertex) || (grad_seg && !gs_strides) || (grad_vertex && !gv_strides)) return PVNET_E_BADARG;
    if (const int rc = check_head(seg_pred, seg_strides, num_classes, vertex_pred, vp_strides, sigma, flags)) return rc;
    if (const int rc = check_source(mask, mask_dtype, mask_strides, hcoords, b, h, w, vn)) return rc;
    if (b == 0) return 0;
    if (!workspace || workspace_bytes < pvnet_head_grad_kp_workspace_bytes(b, h, w)) return PVNET_E_WORKSPACE;
    if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0) return PVNET_E_BADARG;
    KpGradArgs A;
    A.K = make_source(mask, mask_dtype, mask_strides, weight_scale, h, w, vn, flags);
    A.seg = seg_pred;
    A.vp = vertex_pred;
    A.gs = grad_seg;
    A.gv = grad_vertex;
    for (int i = 0; i < 4; ++i) {
        A.ss[i] = seg_strides[i];
        A.vs[i] = vp_strides[i];
        A.gss[i] = grad_seg ? gs_strides[i] : 0;
        A.gvs[i] = grad_vertex ? gv_strides[i] : 0;
    }
    A.seg_type = type_of(flags, PVNET_HEAD_F_LOGITS_F16, PVNET_HEAD_F_LOGITS_BF16);
    A.vp_type = type_of(flags, PVNET_HEAD_F_VERTEX_F16, PVNET_HEAD_F_VERTEX_BF16);
    A.num_classes = num_classes;
    A.planes = 2 * vn;
    A.npix = A.K.npix;
    A.nseg = A.K.nseg;
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
    // the mask is read by either half; each half asks the fast path's shape of its own tensors beyond it
    const bool lin_m = plane_linear(mask, b, A.K.ms[0], 0, A.K.ms[1], A.K.ms[2], w);
    const bool fast = A.npix % HC_PPL == 0 && lin_m &&
                      (!grad_seg || (plane_linear(seg_pred, b, A.ss[0], A.ss[1], A.ss[2], A.ss[3], w) &&
                                     plane_linear(grad_seg, b, A.gss[0], A.gss[1], A.gss[2], A.gss[3], w))) &&
                      (!grad_vertex || (plane_linear(vertex_pred, b, A.vs[0], A.vs[1], A.vs[2], A.vs[3], w) &&
                                        plane_linear(grad_vertex, b, A.gvs[0], A.gvs[1], A.gvs[2], A.gvs[3], w)));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)A.nseg, (unsigned)b);
    if (grad_vertex) {
        if (A.npix % HC_PPL == 0 && lin_m) hipLaunchKernelGGL(head_grad_kp_wsum_kernel<true>, grid, dim3(HC_T), 0, s, A);
        else hipLaunchKernelGGL(head_grad_kp_wsum_kernel<false>, grid, dim3(HC_T), 0, s, A);
    }
    hipLaunchKernelGGL(head_grad_kp_final_kernel, dim3((unsigned)b), dim3(HC_FT), 0, s, A);
    if (fast) {
        const int nt = (flags & PVNET_HEAD_F_NT_NONE) ? NT_NONE : (flags & PVNET_HEAD_F_NT_ALL) ? NT_ALL : NT_TARGETS;
        if (A.vp_type == VT_F16) launch_grad_fast<VT_F16>(nt, grid, s, A, hcoords);
        else if (A.vp_type == VT_BF16) launch_grad_fast<VT_BF16>(nt, grid, s, A, hcoords);
        else launch_grad_fast<VT_F32>(nt, grid, s, A, hcoords);
    } else {
        hipLaunchKernelGGL(head_grad_kp_general_kernel, grid, dim3(HC_T), 0, s, A, hcoords);
    }
    if (status) hipLaunchKernelGGL(head_grad_kp_status_kernel, dim3((unsigned)b), dim3(HC_FT), 0, s, A);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

}  // extern "C"
