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
// The load helpers restate those of head_metrics.hip: that translation unit is libpvnet_head.so's alone and is not touched.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "pvnet_train.h"
#include "vote_common.h"   // ld_elem / ld_elem_rt (VT_*), PVNET_SPARE_VGPRS

// no contraction: every product and sum rounds as the float64 restatement's separate operations do
#pragma clang fp contract(off)

namespace {

using pvd::VT_BF16;
using pvd::VT_F16;
using pvd::VT_F32;

constexpr int HG_T = 128;                // lanes of a workgroup of the per-pixel kernels
constexpr int HG_PPL = 8;                // consecutive pixels per lane (fast path)
constexpr int HG_SEG = HG_T * HG_PPL;    // pixels per workgroup
constexpr int HG_FT = 256;               // lanes of the per-image workgroups
constexpr int HG_MAX_B = 65535;
constexpr int HG_MAX_PIXELS = 1 << 30;
// the spare-VGPR granule of each kernel (PVNET_SPARE_VGPRS in vote_common.h; tools/check_kernel_resources.py holds them to it)
#define HG_FAST_SPARE 135
#define HG_GENERAL_SPARE 79
#define HG_WSUM_SPARE 31
#define HG_FINAL_SPARE 31
#define HG_STATUS_SPARE 23

enum { NT_NONE = 0, NT_TARGETS = 1, NT_ALL = 2 };

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

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef long long i64x2 __attribute__((ext_vector_type(2)));

template <bool NT, typename V>
__device__ __forceinline__ V ldv(const void* p) {
    return NT ? __builtin_nontemporal_load(reinterpret_cast<const V*>(p)) : *reinterpret_cast<const V*>(p);
}
template <bool NT, typename V>
__device__ __forceinline__ void stv(void* p, V v) {
    if (NT) __builtin_nontemporal_store(v, reinterpret_cast<V*>(p));
    else *reinterpret_cast<V*>(p) = v;
}

// eight consecutive elements at element offset `off` (a multiple of 8 from a 16-byte aligned base), widened to float32
template <int VT, bool NT>
__device__ __forceinline__ void load8(const void* base, int64_t off, float* o) {
    if (VT == VT_F32) {
        const float* p = reinterpret_cast<const float*>(base) + off;
        const f32x4 a = ldv<NT, f32x4>(p), b = ldv<NT, f32x4>(p + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            o[i] = a[i];
            o[4 + i] = b[i];
        }
    } else if (VT == VT_F16) {
        const f16x8 a = ldv<NT, f16x8>(reinterpret_cast<const _Float16*>(base) + off);
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = (float)a[i];
    } else {
        const u32x4 a = ldv<NT, u32x4>(reinterpret_cast<const uint16_t*>(base) + off);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            o[2 * i] = __uint_as_float(a[i] << 16);
            o[2 * i + 1] = __uint_as_float(a[i] & 0xFFFF0000u);
        }
    }
}
template <bool NT>
__device__ __forceinline__ void load8_rt(int vt, const void* base, int64_t off, float* o) {   // workgroup-uniform type
    if (vt == VT_F16) load8<VT_F16, NT>(base, off, o);
    else if (vt == VT_BF16) load8<VT_BF16, NT>(base, off, o);
    else load8<VT_F32, NT>(base, off, o);
}

// a float64 rounded to float32 to odd: where the conversion is inexact the result's last bit is set.  Rounding that to a narrower
// type (11 or 8 significant bits) gives what one rounding of the float64 would have given.
__device__ __forceinline__ float to_f32_odd(double x) {
    float f = (float)x;
    const double r = (double)f;
    if (r != x && x == x) {
        uint32_t u = __float_as_uint(f);
        if ((u & 1u) == 0) u += fabs(r) > fabs(x) ? 0xFFFFFFFFu : 1u;   // the other neighbour of x (sign and magnitude: +-1 steps it)
        f = __uint_as_float(u);
    }
    return f;
}
__device__ __forceinline__ uint32_t to_bf16_bits(double x) {   // round to nearest even
    const uint32_t u = __float_as_uint(to_f32_odd(x));
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (u >> 16) | 0x40u;   // NaN stays NaN
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

// eight consecutive gradient elements, each rounded once to the tensor's type
template <int VT, bool NT>
__device__ __forceinline__ void store8(void* base, int64_t off, const double* g) {
    if (VT == VT_F32) {
        float* p = reinterpret_cast<float*>(base) + off;
        f32x4 a, b;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            a[i] = (float)g[i];
            b[i] = (float)g[4 + i];
        }
        stv<NT, f32x4>(p, a);
        stv<NT, f32x4>(p + 4, b);
    } else if (VT == VT_F16) {
        f16x8 a;
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = (_Float16)to_f32_odd(g[i]);
        stv<NT, f16x8>(reinterpret_cast<_Float16*>(base) + off, a);
    } else {
        u32x4 a;
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = to_bf16_bits(g[2 * i]) | (to_bf16_bits(g[2 * i + 1]) << 16);
        stv<NT, u32x4>(reinterpret_cast<uint16_t*>(base) + off, a);
    }
}
template <bool NT>
__device__ __forceinline__ void store8_rt(int vt, void* base, int64_t off, const double* g) {   // workgroup-uniform type
    if (vt == VT_F16) store8<VT_F16, NT>(base, off, g);
    else if (vt == VT_BF16) store8<VT_BF16, NT>(base, off, g);
    else store8<VT_F32, NT>(base, off, g);
}
__device__ __forceinline__ void store_elem_rt(int vt, void* base, int64_t off, double g) {
    if (vt == VT_F16) reinterpret_cast<_Float16*>(base)[off] = (_Float16)to_f32_odd(g);
    else if (vt == VT_BF16) reinterpret_cast<uint16_t*>(base)[off] = (uint16_t)to_bf16_bits(g);
    else reinterpret_cast<float*>(base)[off] = (float)g;
}

// a label as the kernels use it: 0 .. C-1, or -1 for a value outside
__device__ __forceinline__ int label_of(long long v, int C) { return (v < 0 || v >= C) ? -1 : (int)v; }

template <bool NT>
__device__ __forceinline__ void load8_labels(int dt, const void* base, int64_t off, int C, int* lab) {
    if (dt == PVNET_MASK_U8) {
        const u32x2 a = ldv<NT, u32x2>(reinterpret_cast<const uint8_t*>(base) + off);
#pragma unroll
        for (int i = 0; i < 8; ++i) lab[i] = label_of((a[i >> 2] >> (8 * (i & 3))) & 0xFFu, C);
    } else if (dt == PVNET_MASK_I32) {
        const int32_t* p = reinterpret_cast<const int32_t*>(base) + off;
        const u32x4 a = ldv<NT, u32x4>(p), b = ldv<NT, u32x4>(p + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            lab[i] = label_of((int32_t)a[i], C);
            lab[4 + i] = label_of((int32_t)b[i], C);
        }
    } else {
        const long long* p = reinterpret_cast<const long long*>(base) + off;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const i64x2 a = ldv<NT, i64x2>(p + 2 * i);
            lab[2 * i] = label_of(a.x, C);
            lab[2 * i + 1] = label_of(a.y, C);
        }
    }
}

__device__ __forceinline__ long long load_label_rt(int dt, const void* base, int64_t off) {
    if (dt == PVNET_MASK_U8) return reinterpret_cast<const uint8_t*>(base)[off];
    if (dt == PVNET_MASK_I32) return reinterpret_cast<const int32_t*>(base)[off];
    return reinterpret_cast<const long long*>(base)[off];
}

// the running maximum of the logits as the forward keeps it: a NaN counts as the maximum and stays
__device__ __forceinline__ bool takes_over(float best, float x) { return (best == best) & !(x <= best); }

// the gradient of one field element over the image's coefficient kv = u_v / D_i: d = w (p - t); w d sigma^2 where |d| < 1 / sigma^2,
// else w sign(d).  A NaN fails the comparison, takes the second branch and stays NaN; w = 0 gives d = 0 and an exact zero.
__device__ __forceinline__ double field_grad(const GradArgs& A, double w, float p, float t, double kv) {
    const double d = w * ((double)p - (double)t);
    const double sgn = d > 0.0 ? 1.0 : d < 0.0 ? -1.0 : d;
    return (fabs(d) < A.inv ? w * (d * A.s2) : w * sgn) * kv;
}

// the gradient of one logit over ks = u_s / (h w): e / S for another class than the label's; for the label's class minus the
// others' share, rest / S -- not e / S - 1, which cancels once the label's logit leads by a margin
__device__ __forceinline__ double logit_grad(int lab, int c, double e, double sum, double rest, double ks) {
    if (lab < 0) return __builtin_nan("");
    return lab == c ? -(ks * (rest / sum)) : ks * (e / sum);
}

__device__ __forceinline__ double wave_sum(double v) {   // xor butterfly: every lane ends with the same, order-fixed sum
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

// the workgroup's sum: waves reduced by butterfly, then added in wave order; valid in lane 0
template <int T>
__device__ __forceinline__ double block_sum(double v) {
    constexpr int NW = T / 64;
    __shared__ double s_d[NW];
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s_d[threadIdx.x >> 6] = v;
    __syncthreads();
    v = s_d[0];
#pragma unroll
    for (int i = 1; i < NW; ++i) v = v + s_d[i];
    return v;
}

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
    const int bi = blockIdx.x;
    double wsum = 0.0;
    if (A.gv) {
        const double* rec = A.wpart + (size_t)bi * A.nseg;
        for (int k = threadIdx.x; k < A.nseg; k += HG_FT) wsum = wsum + rec[k];   // lane t: records t, t + 256, ... in order
        wsum = block_sum<HG_FT>(wsum);
    }
    if (threadIdx.x != 0) return;
    A.coef[2 * bi] = A.upstream[2 * bi] / (double)A.npix;
    A.coef[2 * bi + 1] = A.upstream[2 * bi + 1] / ((double)A.planes * wsum + 1e-3);   // net_utils.py:74
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
    const int bi = blockIdx.x;
    int bad = 0;
    if (A.gs) {   // (without the logits' half the mask was not read: status 0)
        const int32_t* rec = A.bad + (size_t)bi * A.nseg;
        for (int k = threadIdx.x; k < A.nseg; k += HG_FT) bad |= rec[k];
    }
    const int any = __syncthreads_or(bad);
    if (threadIdx.x == 0) A.status[bi] = any ? PVNET_HEAD_S_BAD_LABEL : 0;
}

// a tensor's planes can be accessed eight pixels at a time: pixels contiguous, base and every plane / image start on 16 bytes
bool plane_linear(const void* base, int b, int64_t sb, int64_t sc, int64_t sh, int64_t sw, int w) {
    return sw == 1 && sh == w && (b == 1 || sb % 8 == 0) && sc % 8 == 0 && (reinterpret_cast<uintptr_t>(base) & 15u) == 0;
}

int type_of(uint32_t flags, uint32_t f16, uint32_t bf16) { return (flags & f16) ? VT_F16 : (flags & bf16) ? VT_BF16 : VT_F32; }

size_t round256(size_t n) { return (n + 255) / 256 * 256; }

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
