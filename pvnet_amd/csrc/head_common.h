// head_common.h -- the network head behind the backbone, written once for its three translation units: head_metrics.hip
// (libpvnet_head.so), head_grad.hip (libpvnet_train.so) and head_targets.hip (libpvnet_targets.so).
//
//   per-pixel helpers   the 16-byte loads and stores, the label rule, torch's arg-max rule, the smooth-L1 term and its gradient, the
//                       cross-entropy and the logits' class rule, the order-fixed reductions
//   per-image bodies    head_final_image, head_grad_final_image, head_grad_status_image
//   per-pixel bodies    head_partial8 / head_partial1 (forward, fast and general path), head_grad8 / head_grad1 (backward),
//                       head_grad_wsum: ALL of the head's arithmetic, templates over a target source -- the policy that says where a
//                       pixel's label, weight and targets come from.  MemSource (here) loads them; KpSource (head_targets.hip) computes
//                       them from the mask and the image's key-points.  The fused forms equal the head on materialised targets bit
//                       for bit because both instantiate the same body; the sources differ in where (t, w) come from and in the
//                       order they walk the field's planes, nothing else.
//   arguments           HeadArgs<SRC> for the forward, GradArgs<SRC> for the backward: one layout each, the source a member
//   host side           the argument checks and their order, the size limits, the workspaces, the arguments' filling, the VT x NT
//                       dispatch: what the five entry points do before they launch
//
// The __global__ kernels stay in their translation units, as thin wrappers with their spare-VGPR constants.  Every function here is
// inlined into the kernel that calls it: the three libraries share source, not symbols.  namespace pvh.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "pvnet_head.h"
#include "vote_common.h"   // ld_elem / ld_elem_rt (VT_*), PVNET_SPARE_VGPRS

// no contraction: every product and sum rounds as the float64 restatements' separate operations do
#pragma clang fp contract(off)

namespace pvh {

using pvd::VT_BF16;
using pvd::VT_F16;
using pvd::VT_F32;

constexpr int HC_T = 128;                // lanes of a workgroup of the per-pixel kernels
constexpr int HC_PPL = 8;                // consecutive pixels per lane (fast paths)
constexpr int HC_SEG = HC_T * HC_PPL;    // pixels per workgroup = per partial record
constexpr int HC_FT = 256;               // lanes of the per-image workgroups
constexpr int HC_MAX_B = 65535;
constexpr int HC_MAX_PIXELS = 1 << 30;

enum { NT_NONE = 0, NT_TARGETS = 1, NT_ALL = 2 };

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

// a label as the kernels use it: 0 .. C-1, or -1 for a value outside (which is still "not background")
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

// the same eight mask elements as stored, for the callers that need the VALUE (the weight of a pixel is its mask value)
template <bool NT>
__device__ __forceinline__ void load8_mask(int dt, const void* base, int64_t off, long long* v) {
    if (dt == PVNET_MASK_U8) {
        const u32x2 a = ldv<NT, u32x2>(reinterpret_cast<const uint8_t*>(base) + off);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (a[i >> 2] >> (8 * (i & 3))) & 0xFFu;
    } else if (dt == PVNET_MASK_I32) {
        const int32_t* p = reinterpret_cast<const int32_t*>(base) + off;
        const u32x4 a = ldv<NT, u32x4>(p), b = ldv<NT, u32x4>(p + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[i] = (int32_t)a[i];
            v[4 + i] = (int32_t)b[i];
        }
    } else {
        const long long* p = reinterpret_cast<const long long*>(base) + off;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const i64x2 a = ldv<NT, i64x2>(p + 2 * i);
            v[2 * i] = a.x;
            v[2 * i + 1] = a.y;
        }
    }
}

__device__ __forceinline__ long long load_label_rt(int dt, const void* base, int64_t off) {
    if (dt == PVNET_MASK_U8) return reinterpret_cast<const uint8_t*>(base)[off];
    if (dt == PVNET_MASK_I32) return reinterpret_cast<const int32_t*>(base)[off];
    return reinterpret_cast<const long long*>(base)[off];
}

// torch.argmax's rule (k1_mask.hip:69-80): the first maximum wins and a NaN counts as the maximum -- a NaN replaces a number, a
// later NaN never an earlier one
__device__ __forceinline__ bool takes_over(float best, float x) { return (best == best) & !(x <= best); }

// one smooth-L1 term (net_utils.py:66-71): d = w (p - t); d^2 sigma^2 / 2 where |d| < 1 / sigma^2, else |d| - 0.5 / sigma^2.  A NaN
// fails the comparison, takes the second branch and stays NaN.  A: hs = sigma^2 / 2, inv = 1 / sigma^2, half = 0.5 / sigma^2.
template <typename ARGS>
__device__ __forceinline__ double smooth_l1(const ARGS& A, double w, float p, float t) {
    const double d = w * ((double)p - (double)t);
    const double a = fabs(d);
    return a < A.inv ? d * d * A.hs : a - A.half;
}

// log(sum_c exp(s_c - m)) - (s_label - m): the cross-entropy of one pixel with the maximum m subtracted first, as log_softmax does
__device__ __forceinline__ double cross_entropy(double sum, float s_label, float m) {
    return log(sum) - ((double)s_label - (double)m);
}

// the gradient of one field element over the image's coefficient kv = u_v / D_i: d = w (p - t); w d sigma^2 where |d| < 1 / sigma^2,
// else w sign(d).  A NaN fails the comparison, takes the second branch and stays NaN; w = 0 gives d = 0 and an exact zero.
// A: s2 = sigma^2, inv = 1 / sigma^2.
template <typename ARGS>
__device__ __forceinline__ double field_grad(const ARGS& A, double w, float p, float t, double kv) {
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
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
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

// ---- the forward's records ------------------------------------------------------------------------------------------------------
struct HeadPartial {   // 32 bytes
    double ce, sl1, wsum;
    unsigned long long packed;   // tp | fp << 16 | fn << 32 | bad << 48: each at most HC_SEG
};
static_assert(sizeof(HeadPartial) == 32 && HC_SEG < (1 << 16), "a record's four counts share one 64-bit word");

struct Acc {
    double ce = 0.0, sl1 = 0.0, wsum = 0.0;
    unsigned long long packed = 0;
};
constexpr unsigned long long ONE_TP = 1ull, ONE_FP = 1ull << 16, ONE_FN = 1ull << 32, ONE_BAD = 1ull << 48;

__device__ __forceinline__ unsigned long long confusion(bool pred_fg, int lab) {
    const bool fg = lab != 0;
    return (pred_fg && fg ? ONE_TP : 0) | (pred_fg && !fg ? ONE_FP : 0) | (!pred_fg && fg ? ONE_FN : 0) | (lab < 0 ? ONE_BAD : 0);
}

// the workgroup's record: waves reduced by butterfly, then added in wave order by lane 0
template <int T>
__device__ __forceinline__ bool block_reduce(Acc& a) {
    constexpr int NW = T / 64;
    __shared__ double s_d[NW][3];
    __shared__ unsigned long long s_p[NW];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double ce = wave_sum(a.ce), sl1 = wave_sum(a.sl1), wsum = wave_sum(a.wsum);
    const unsigned long long packed = wave_sum(a.packed);
    if (lane == 0) {
        s_d[wave][0] = ce;
        s_d[wave][1] = sl1;
        s_d[wave][2] = wsum;
        s_p[wave] = packed;
    }
    __syncthreads();
    if (threadIdx.x != 0) return false;
    a.ce = s_d[0][0];
    a.sl1 = s_d[0][1];
    a.wsum = s_d[0][2];
    a.packed = s_p[0];
#pragma unroll
    for (int i = 1; i < NW; ++i) {
        a.ce = a.ce + s_d[i][0];
        a.sl1 = a.sl1 + s_d[i][1];
        a.wsum = a.wsum + s_d[i][2];
        a.packed = a.packed + s_p[i];
    }
    return true;
}

// A: partial, nseg
template <typename ARGS>
__device__ __forceinline__ void store_partial(const ARGS& A, const Acc& a) {
    HeadPartial* r = A.partial + (size_t)blockIdx.y * A.nseg + blockIdx.x;
    r->ce = a.ce;
    r->sl1 = a.sl1;
    r->wsum = a.wsum;
    r->packed = a.packed;
}

// the forward's per-image kernel, a workgroup of HC_FT lanes per image: sums the image's records in a fixed order, finalises, writes
// the outputs.  A: partial, nseg, npix, planes, losses, counts, status.
template <typename ARGS>
__device__ __forceinline__ void head_final_image(const ARGS& A) {
    const int bi = blockIdx.x;
    Acc acc;
    long long tp = 0, fp = 0, fn = 0, bad = 0;   // a record's packed counts are unpacked before they are added: no field overflows
    const HeadPartial* rec = A.partial + (size_t)bi * A.nseg;
    for (int k = threadIdx.x; k < A.nseg; k += HC_FT) {   // lane t: records t, t + 256, ... in order
        acc.ce = acc.ce + rec[k].ce;
        acc.sl1 = acc.sl1 + rec[k].sl1;
        acc.wsum = acc.wsum + rec[k].wsum;
        const unsigned long long q = rec[k].packed;
        tp += (long long)(q & 0xFFFFu);
        fp += (long long)((q >> 16) & 0xFFFFu);
        fn += (long long)((q >> 32) & 0xFFFFu);
        bad += (long long)(q >> 48);
    }
    __shared__ long long s_cnt[HC_FT / 64][4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    tp = (long long)wave_sum((unsigned long long)tp);
    fp = (long long)wave_sum((unsigned long long)fp);
    fn = (long long)wave_sum((unsigned long long)fn);
    bad = (long long)wave_sum((unsigned long long)bad);
    if (lane == 0) {
        s_cnt[wave][0] = tp;
        s_cnt[wave][1] = fp;
        s_cnt[wave][2] = fn;
        s_cnt[wave][3] = bad;
    }
    if (!block_reduce<HC_FT>(acc)) return;   // (its barrier also orders s_cnt)
    tp = fp = fn = bad = 0;
#pragma unroll
    for (int i = 0; i < HC_FT / 64; ++i) {
        tp += s_cnt[i][0];
        fp += s_cnt[i][1];
        fn += s_cnt[i][2];
        bad += s_cnt[i][3];
    }
    double* out = A.losses + (size_t)bi * 4;
    out[0] = bad ? __builtin_nan("") : acc.ce / (double)A.npix;
    out[1] = acc.sl1 / ((double)A.planes * acc.wsum + 1e-3);   // net_utils.py:74
    out[2] = ((double)tp + 1.0) / ((double)tp + (double)fp + 1.0);
    out[3] = ((double)tp + 1.0) / ((double)tp + (double)fn + 1.0);
    int64_t* cnt = A.counts + (size_t)bi * 3;
    cnt[0] = tp;
    cnt[1] = fp;
    cnt[2] = fn;
    if (A.status) A.status[bi] = bad ? PVNET_HEAD_S_BAD_LABEL : 0;
}

// the backward's two per-image kernels, a workgroup of HC_FT lanes per image.  A: gv, gs, wpart, bad, nseg, npix, planes, upstream,
// coef, status.
template <typename ARGS>
__device__ __forceinline__ void head_grad_final_image(const ARGS& A) {
    const int bi = blockIdx.x;
    double wsum = 0.0;
    if (A.gv) {
        const double* rec = A.wpart + (size_t)bi * A.nseg;
        for (int k = threadIdx.x; k < A.nseg; k += HC_FT) wsum = wsum + rec[k];   // lane t: records t, t + 256, ... in order
        wsum = block_sum<HC_FT>(wsum);
    }
    if (threadIdx.x != 0) return;
    A.coef[2 * bi] = A.upstream[2 * bi] / (double)A.npix;
    A.coef[2 * bi + 1] = A.upstream[2 * bi + 1] / ((double)A.planes * wsum + 1e-3);   // net_utils.py:74
}
template <typename ARGS>
__device__ __forceinline__ void head_grad_status_image(const ARGS& A) {
    const int bi = blockIdx.x;
    int bad = 0;
    if (A.gs) {   // (without the logits' half the mask's labels were not judged: status 0)
        const int32_t* rec = A.bad + (size_t)bi * A.nseg;
        for (int k = threadIdx.x; k < A.nseg; k += HC_FT) bad |= rec[k];
    }
    const int any = __syncthreads_or(bad);
    if (threadIdx.x == 0) A.status[bi] = any ? PVNET_HEAD_S_BAD_LABEL : 0;
}

// ---- the memory source: a pixel's target and weight are loaded ------------------------------------------------------------------
// A target source is the policy of the four per-pixel bodies below: it says where the label, the weight and the 2 vn targets of a
// pixel come from, and in which order the field's planes are walked.  This one loads them (head_metrics.hip, head_grad.hip); the
// other, KpSource of head_targets.hip, computes them from the mask and the image's key-points.  What a source provides:
//   Lane8 / Pixel, Image     what it keeps of a lane's eight pixels / of one pixel between the two halves, and of an image
//   pixels8                  opens a lane's eight pixels and gives their labels (the mask is read for them alone here: not at all
//                            where `labels` is false)
//   pixel1, label1           the same for one pixel, the label on demand
//   weights8 / weight1       the weights as float64
//   planes8 / planes1        the field loop: load(k, p) fetches plane k of the prediction, use(k, p, t) takes it with its targets
struct MemSource {
    const float* vt;
    const float* vw;
    const void* mask;
    int64_t ts[4], ws[3], ms[3];
    int mask_dtype;

    struct Lane8 {};
    struct Image {};
    struct Pixel {};

    template <bool NT>
    __device__ __forceinline__ void pixels8(int bi, int p0, int C, bool labels, int* lab, Lane8&) const {
        if (labels) load8_labels<NT>(mask_dtype, mask, (int64_t)bi * ms[0] + p0, C, lab);
    }
    template <bool NT>
    __device__ __forceinline__ void weights8(int bi, int p0, const Lane8&, double* wd) const {
        float wf[HC_PPL];
        load8<VT_F32, NT>(vw, (int64_t)bi * ws[0] + p0, wf);
#pragma unroll
        for (int i = 0; i < HC_PPL; ++i) wd[i] = (double)wf[i];
    }
    // prediction, then target, plane by plane (BOTH is the key-point source's: see there)
    template <bool NT, bool BOTH, typename LOAD, typename USE>
    __device__ __forceinline__ void planes8(const double*, int bi, int p0, int planes, const Lane8&, LOAD load, USE use) const {
        const int64_t toff = (int64_t)bi * ts[0] + p0;
#pragma unroll 2
        for (int k = 0; k < planes; ++k) {
            float p[HC_PPL], t[HC_PPL];
            load(k, p);
            load8<VT_F32, NT>(vt, toff + (int64_t)k * ts[1], t);
            use(k, p, t);
        }
    }

    __device__ __forceinline__ Image image(int) const { return Image(); }
    __device__ __forceinline__ Pixel pixel1(int, int, int) const { return Pixel(); }
    __device__ __forceinline__ int label1(int bi, int x, int y, int C, const Pixel&) const {
        return label_of(load_label_rt(mask_dtype, mask, (int64_t)bi * ms[0] + (int64_t)y * ms[1] + (int64_t)x * ms[2]), C);
    }
    __device__ __forceinline__ double weight1(const Image&, int bi, int x, int y, const Pixel&) const {
        return (double)vw[(int64_t)bi * ws[0] + (int64_t)y * ws[1] + (int64_t)x * ws[2]];
    }
    template <typename USE>
    __device__ __forceinline__ void planes1(const double*, int bi, int x, int y, int planes, const Pixel&, USE use) const {
        const int64_t toff = (int64_t)bi * ts[0] + (int64_t)y * ts[2] + (int64_t)x * ts[3];
        for (int k = 0; k < planes; ++k) use(k, vt[toff + (int64_t)k * ts[1]]);
    }

    // host: the fast path's shape of what the field's half loads
    bool targets_linear(int b, int w) const;
};

// ---- the kernels' arguments: one layout for the forward, one for the backward, the source a member -------------------------------
template <typename SRC>
struct HeadInputs {   // what both read.  Pointers, then the source, then the strides: the kernels hold most of this in SGPRs, and with
                      // the source's pointers away from the others head_grad_general_kernel no longer keeps its scalars in registers
    const void* seg;
    const void* vp;
    SRC T;            // where a pixel's label, weight and targets come from
    int64_t ss[4], vs[4];
    int seg_type, vp_type, num_classes, planes;
    int w, npix, nseg;
    double s2, hs, inv, half;   // sigma^2, sigma^2 / 2, 1 / sigma^2, 0.5 / sigma^2
};
template <typename SRC>
struct HeadArgs : HeadInputs<SRC> {
    double* losses;
    int64_t* counts;
    int32_t* status;
    HeadPartial* partial;
};
template <typename SRC>
struct GradArgs : HeadInputs<SRC> {
    void* gs;   // NULL: the logits' half is skipped
    void* gv;   // NULL: the field's half is skipped
    int64_t gss[4], gvs[4];
    const double* upstream;
    double* coef;     // [b][2]: u_s / (h w), u_v / D_i
    double* wpart;    // [b][nseg]: a segment's sum of the weights
    int32_t* bad;     // [b][nseg]: the segment holds a label outside 0 .. C-1
    int32_t* status;
};

// ---- the four per-pixel bodies, each written once for both sources.  grid (segments of HC_SEG pixels, images), HC_T lanes; hcb: the
//      image's key-points (the key-point source's; NULL otherwise) -- a kernel argument of its own, see head_targets.hip ------------
// forward, fast path: eight consecutive pixels per lane (npix a multiple of 8: a lane's eight pixels are all inside or all outside)
template <int VT, int NT, typename SRC>
__device__ __forceinline__ void head_partial8(const HeadArgs<SRC>& A, const double* __restrict__ hcb) {
    constexpr bool NT_P = NT == NT_ALL, NT_T = NT != NT_NONE;   // predictions, what the source loads
    const int bi = blockIdx.y;
    const int p0 = blockIdx.x * HC_SEG + (int)threadIdx.x * HC_PPL;
    Acc acc;
    if (p0 < A.npix) {
        int lab[HC_PPL];
        typename SRC::Lane8 L;
        A.T.template pixels8<NT_T>(bi, p0, A.num_classes, true, lab, L);
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
        // ---- the field: 2 vn planes of prediction against their targets under one plane of weights; a plane's prediction is loaded
        //      when its targets are there -------------------------------------------------------------------------------------------
        double wd[HC_PPL];
        A.T.template weights8<NT_T>(bi, p0, L, wd);
#pragma unroll
        for (int i = 0; i < HC_PPL; ++i) acc.wsum = acc.wsum + wd[i];
        const int64_t poff = (int64_t)bi * A.vs[0] + p0;
        A.T.template planes8<NT_T, false>(
            hcb, bi, p0, A.planes, L, [&](int k, float* p) { load8<VT, NT_P>(A.vp, poff + (int64_t)k * A.vs[1], p); },
            [&](int, const float* p, const float* t) {
#pragma unroll
                for (int i = 0; i < HC_PPL; ++i) acc.sl1 = acc.sl1 + smooth_l1(A, wd[i], p[i], t[i]);
            });
    }
    if (block_reduce<HC_T>(acc)) store_partial(A, acc);
}

// forward, general path: the same record from any element strides, any alignment, any h * w -- a pixel per lane and load
template <typename SRC>
__device__ __forceinline__ void head_partial1(const HeadArgs<SRC>& A, const double* __restrict__ hcb) {
    const int bi = blockIdx.y;
    const typename SRC::Image I = A.T.image(bi);
    Acc acc;
    for (int j = 0; j < HC_PPL; ++j) {
        const int p = blockIdx.x * HC_SEG + j * HC_T + (int)threadIdx.x;
        if (p >= A.npix) break;
        const int y = p / A.w, x = p - y * A.w;
        const typename SRC::Pixel P = A.T.pixel1(bi, x, y);
        const int lab = A.T.label1(bi, x, y, A.num_classes, P);
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
        const double wd = A.T.weight1(I, bi, x, y, P);
        acc.wsum = acc.wsum + wd;
        const int64_t poff = (int64_t)bi * A.vs[0] + (int64_t)y * A.vs[2] + (int64_t)x * A.vs[3];
        A.T.planes1(hcb, bi, x, y, A.planes, P, [&](int k, float t) {
            acc.sl1 = acc.sl1 + smooth_l1(A, wd, pvd::ld_elem_rt(A.vp_type, A.vp, poff + (int64_t)k * A.vs[1]), t);
        });
    }
    if (block_reduce<HC_T>(acc)) store_partial(A, acc);
}

// the segment's bad-label flag, for head_grad_status_image (A.gs is uniform over the grid: every lane reaches the barrier)
template <typename SRC>
__device__ __forceinline__ void store_bad(const GradArgs<SRC>& A, int bad) {
    if (!A.gs) return;
    const int any = __syncthreads_or(bad);
    if (threadIdx.x == 0) A.bad[(size_t)blockIdx.y * A.nseg + blockIdx.x] = any ? 1 : 0;
}

// backward, fast path: reads every input byte once, writes every gradient byte once; a half that is not asked for is skipped, its
// loads included
template <int VT, int NT, typename SRC>
__device__ __forceinline__ void head_grad8(const GradArgs<SRC>& A, const double* __restrict__ hcb) {
    constexpr bool NT_P = NT == NT_ALL, NT_T = NT != NT_NONE, NT_S = NT == NT_ALL;   // predictions, what the source loads, stores
    const int bi = blockIdx.y;
    const int p0 = blockIdx.x * HC_SEG + (int)threadIdx.x * HC_PPL;
    const bool inside = p0 < A.npix;
    int bad = 0;
    int lab[HC_PPL];
    typename SRC::Lane8 L;
    if (inside) A.T.template pixels8<NT_T>(bi, p0, A.num_classes, A.gs != nullptr, lab, L);
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
        // ---- the field: 2 vn planes of prediction against their targets under one plane of weights; the predictions are in flight
        //      while the targets are made --------------------------------------------------------------------------------------------
        const double kv = A.coef[2 * bi + 1];
        double wd[HC_PPL];
        A.T.template weights8<NT_T>(bi, p0, L, wd);
        const int64_t poff = (int64_t)bi * A.vs[0] + p0, goff = (int64_t)bi * A.gvs[0] + p0;
        A.T.template planes8<NT_T, true>(
            hcb, bi, p0, A.planes, L, [&](int k, float* p) { load8<VT, NT_P>(A.vp, poff + (int64_t)k * A.vs[1], p); },
            [&](int k, const float* p, const float* t) {
                double g[HC_PPL];
#pragma unroll
                for (int i = 0; i < HC_PPL; ++i) g[i] = field_grad(A, wd[i], p[i], t[i], kv);
                store8<VT, NT_S>(A.gv, goff + (int64_t)k * A.gvs[1], g);
            });
    }
    store_bad(A, bad);
}

// backward, general path: a pixel per lane and access
template <typename SRC>
__device__ __forceinline__ void head_grad1(const GradArgs<SRC>& A, const double* __restrict__ hcb) {
    const int bi = blockIdx.y;
    const typename SRC::Image I = A.T.image(bi);
    int bad = 0;
    for (int j = 0; j < HC_PPL; ++j) {
        const int p = blockIdx.x * HC_SEG + j * HC_T + (int)threadIdx.x;
        if (p >= A.npix) break;
        const int y = p / A.w, x = p - y * A.w;
        const typename SRC::Pixel P = A.T.pixel1(bi, x, y);
        if (A.gs) {
            const double ks = A.coef[2 * bi];
            const int lab = A.T.label1(bi, x, y, A.num_classes, P);
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
            const double wd = A.T.weight1(I, bi, x, y, P);
            const int64_t poff = (int64_t)bi * A.vs[0] + (int64_t)y * A.vs[2] + (int64_t)x * A.vs[3];
            const int64_t goff = (int64_t)bi * A.gvs[0] + (int64_t)y * A.gvs[2] + (int64_t)x * A.gvs[3];
            A.T.planes1(hcb, bi, x, y, A.planes, P, [&](int k, float t) {
                store_elem_rt(A.vp_type, A.gv, goff + (int64_t)k * A.gvs[1],
                              field_grad(A, wd, pvd::ld_elem_rt(A.vp_type, A.vp, poff + (int64_t)k * A.vs[1]), t, kv));
            });
        }
    }
    store_bad(A, bad);
}

// the segment's sum of the weights, in the forward's order (so D_i = 2vn sum w + 1e-3 is the forward's denominator bit for bit).  What
// it reads is loaded plainly: the gradient kernel reads it again.
template <bool FAST, typename SRC>
__device__ __forceinline__ void head_grad_wsum(const GradArgs<SRC>& A) {
    const int bi = blockIdx.y;
    double acc = 0.0;
    if (FAST) {
        const int p0 = blockIdx.x * HC_SEG + (int)threadIdx.x * HC_PPL;
        if (p0 < A.npix) {   // (npix is a multiple of 8 here: the lane's eight pixels are all inside)
            int lab[HC_PPL];
            typename SRC::Lane8 L;
            double wd[HC_PPL];
            A.T.template pixels8<false>(bi, p0, A.num_classes, false, lab, L);
            A.T.template weights8<false>(bi, p0, L, wd);
#pragma unroll
            for (int i = 0; i < HC_PPL; ++i) acc = acc + wd[i];
        }
    } else {
        const typename SRC::Image I = A.T.image(bi);
        for (int j = 0; j < HC_PPL; ++j) {
            const int p = blockIdx.x * HC_SEG + j * HC_T + (int)threadIdx.x;
            if (p >= A.npix) break;
            const int y = p / A.w, x = p - y * A.w;
            acc = acc + A.T.weight1(I, bi, x, y, A.T.pixel1(bi, x, y));
        }
    }
    acc = block_sum<HC_T>(acc);
    if (threadIdx.x == 0) A.wpart[(size_t)bi * A.nseg + blockIdx.x] = acc;
}

// ---- host side: what the five entry points of the three libraries do before they launch ------------------------------------------
// a tensor's planes can be accessed eight pixels at a time: pixels contiguous, base and every plane / image start on 16 bytes
inline bool plane_linear(const void* base, int b, int64_t sb, int64_t sc, int64_t sh, int64_t sw, int w) {
    return sw == 1 && sh == w && (b == 1 || sb % 8 == 0) && sc % 8 == 0 && (reinterpret_cast<uintptr_t>(base) & 15u) == 0;
}
inline bool linear4(const void* base, int b, const int64_t* s, int w) { return plane_linear(base, b, s[0], s[1], s[2], s[3], w); }
inline bool linear3(const void* base, int b, const int64_t* s, int w) { return plane_linear(base, b, s[0], 0, s[1], s[2], w); }
inline bool MemSource::targets_linear(int b, int w) const { return linear4(vt, b, ts, w) && linear3(vw, b, ws, w); }

inline int type_of(uint32_t flags, uint32_t f16, uint32_t bf16) { return (flags & f16) ? VT_F16 : (flags & bf16) ? VT_BF16 : VT_F32; }

inline size_t round256(size_t n) { return (n + 255) / 256 * 256; }

constexpr uint32_t HEAD_FLAGS = PVNET_HEAD_F_VERTEX_F16 | PVNET_HEAD_F_VERTEX_BF16 | PVNET_HEAD_F_LOGITS_F16 | PVNET_HEAD_F_LOGITS_BF16 |
                                PVNET_HEAD_F_NT_NONE | PVNET_HEAD_F_NT_ALL;

// the argument checks, in the order every entry point makes them: 0 or the code to return.  pointers: none of the call's required
// pointers is NULL; known: the flags the call takes.  (The targets alone have no classes and no sigma: they pass 2 and 1.)
inline int check_args(bool pointers, int mask_dtype, int b, int h, int w, int vn, int num_classes, double sigma, uint32_t flags,
                      uint32_t known) {
    if (!pointers) return PVNET_E_BADARG;
    if (b < 0 || h <= 0 || w <= 0 || vn <= 0 || num_classes < 2 || !(sigma > 0.0) || !isfinite(sigma) || (flags & ~known) != 0)
        return PVNET_E_BADARG;
    if (((flags & PVNET_HEAD_F_VERTEX_F16) && (flags & PVNET_HEAD_F_VERTEX_BF16)) ||
        ((flags & PVNET_HEAD_F_LOGITS_F16) && (flags & PVNET_HEAD_F_LOGITS_BF16)) ||
        ((flags & PVNET_HEAD_F_NT_NONE) && (flags & PVNET_HEAD_F_NT_ALL)))
        return PVNET_E_BADARG;
    if (mask_dtype == PVNET_MASK_I16 || mask_dtype == PVNET_MASK_F32 || mask_dtype == PVNET_MASK_LOGITS_F32) return PVNET_E_UNSUPPORTED;
    if (mask_dtype != PVNET_MASK_U8 && mask_dtype != PVNET_MASK_I32 && mask_dtype != PVNET_MASK_I64) return PVNET_E_BADARG;
    if (b > HC_MAX_B || (long long)h * w > HC_MAX_PIXELS || vn > (1 << 20)) return PVNET_E_UNSUPPORTED;
    return 0;
}

// the workspaces: the forward's records; the backward's coefficients, weight sums and bad-label flags.  0 for sizes out of range.
inline size_t segments(size_t npix) { return (npix + HC_SEG - 1) / HC_SEG; }
inline bool sizes_ok(int b, int h, int w) { return b > 0 && h > 0 && w > 0 && b <= HC_MAX_B && (long long)h * w <= HC_MAX_PIXELS; }
inline size_t head_workspace_bytes(int b, int h, int w) {
    return sizes_ok(b, h, w) ? round256((size_t)b * segments((size_t)h * w) * sizeof(HeadPartial)) : 0;
}
inline size_t grad_workspace_bytes(int b, int h, int w) {
    if (!sizes_ok(b, h, w)) return 0;
    const size_t nseg = segments((size_t)h * w);
    return round256((size_t)b * 2 * sizeof(double)) + round256((size_t)b * nseg * sizeof(double)) + round256((size_t)b * nseg * sizeof(int32_t));
}
inline int check_workspace(const void* workspace, size_t have, size_t need) {
    if (!workspace || have < need) return PVNET_E_WORKSPACE;
    return (reinterpret_cast<uintptr_t>(workspace) & 7u) != 0 ? PVNET_E_BADARG : 0;
}

// what the forward's and the backward's arguments share, from a checked call (A.T is the caller's)
template <typename SRC>
void fill_inputs(HeadInputs<SRC>& A, const void* seg_pred, const int64_t* seg_strides, int num_classes, const void* vertex_pred,
                 const int64_t* vp_strides, int h, int w, int vn, double sigma, uint32_t flags) {
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
    A.w = w;
    A.npix = h * w;
    A.nseg = (int)segments((size_t)A.npix);
    A.s2 = sigma * sigma;
    A.hs = A.s2 / 2.0;
    A.inv = 1.0 / A.s2;
    A.half = 0.5 / A.s2;
}
inline MemSource make_mem_source(const float* vertex_target, const int64_t* vt_strides, const float* vertex_weights, const int64_t* w_strides,
                                 const void* mask, int mask_dtype, const int64_t* mask_strides) {
    MemSource T;
    T.vt = vertex_target;
    T.vw = vertex_weights;
    T.mask = mask;
    for (int i = 0; i < 4; ++i) T.ts[i] = vt_strides[i];
    for (int i = 0; i < 3; ++i) {
        T.ws[i] = w_strides[i];
        T.ms[i] = mask_strides[i];
    }
    T.mask_dtype = mask_dtype;
    return T;
}
template <typename SRC>
void fill_head(HeadArgs<SRC>& A, double* losses, int64_t* counts, int32_t* status, void* workspace) {
    A.losses = losses;
    A.counts = counts;
    A.status = status;
    A.partial = static_cast<HeadPartial*>(workspace);
}
template <typename SRC>
void fill_grad(GradArgs<SRC>& A, int b, const double* upstream, void* grad_seg, const int64_t* gs_strides, void* grad_vertex,
               const int64_t* gv_strides, int32_t* status, void* workspace) {
    A.gs = grad_seg;
    A.gv = grad_vertex;
    for (int i = 0; i < 4; ++i) {
        A.gss[i] = grad_seg ? gs_strides[i] : 0;
        A.gvs[i] = grad_vertex ? gv_strides[i] : 0;
    }
    A.upstream = upstream;
    char* ws = static_cast<char*>(workspace);
    A.coef = reinterpret_cast<double*>(ws);
    ws += round256((size_t)b * 2 * sizeof(double));
    A.wpart = reinterpret_cast<double*>(ws);
    ws += round256((size_t)b * A.nseg * sizeof(double));
    A.bad = reinterpret_cast<int32_t*>(ws);
    A.status = status;
}

// the fast kernels' dispatch over the field's element type and the non-temporal policy: launch(VT, NT) gets two integral constants
template <int V>
using ic = std::integral_constant<int, V>;
template <typename F>
void launch_fast(int vt, uint32_t flags, F launch) {
    const auto with = [&](auto v) {
        if (flags & PVNET_HEAD_F_NT_NONE) launch(v, ic<NT_NONE>());
        else if (flags & PVNET_HEAD_F_NT_ALL) launch(v, ic<NT_ALL>());
        else launch(v, ic<NT_TARGETS>());
    };
    if (vt == VT_F16) with(ic<VT_F16>());
    else if (vt == VT_BF16) with(ic<VT_BF16>());
    else with(ic<VT_F32>());
}

inline int launched() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

}  // namespace pvh
