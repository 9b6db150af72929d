// head_common.h -- what the translation units of the network head share: head_metrics.hip (libpvnet_head.so), head_grad.hip
// (libpvnet_train.so) and head_targets.hip (libpvnet_targets.so).  Per-pixel helpers only -- the 16-byte loads and stores, the label
// rule, torch's arg-max rule, the smooth-L1 term and its gradient, the cross-entropy and the logits' class rule, the order-fixed
// reductions -- and the bodies of the per-image kernels, which are the same whether the targets come from memory or from key-points.
// Every function is inlined into the kernel that calls it: the three libraries share source, not symbols.  namespace pvh.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

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

// ---- host side --------------------------------------------------------------------------------------------------------------------
// a tensor's planes can be accessed eight pixels at a time: pixels contiguous, base and every plane / image start on 16 bytes
inline bool plane_linear(const void* base, int b, int64_t sb, int64_t sc, int64_t sh, int64_t sw, int w) {
    return sw == 1 && sh == w && (b == 1 || sb % 8 == 0) && sc % 8 == 0 && (reinterpret_cast<uintptr_t>(base) & 15u) == 0;
}

inline int type_of(uint32_t flags, uint32_t f16, uint32_t bf16) { return (flags & f16) ? VT_F16 : (flags & bf16) ? VT_BF16 : VT_F32; }

inline size_t round256(size_t n) { return (n + 255) / 256 * 256; }

}  // namespace pvh
